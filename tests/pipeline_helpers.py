"""The mirror's batch pipeline (retriever.iter_batched_retrieve) restated per batch over option_helpers.expected_outputs.

A call over N queries on an engine of max_batch = b is cut into the batches [lo, hi) of batch_cuts.  What batch j must
return is expected_outputs(R_j, spec_j, ctx_j): R_j the score rows of a DIRECT retrieve_converged(k=1, want_all_scores=True)
on that batch's rows under the batch's scoring configuration (kept facts, scope with its filter rows, lexical blend, sweep
budget: anchor_kw) and nothing else; spec_j the call's CallSpec with k = want_of(...) -- the docstring of
iter_batched_retrieve -- and the per-query ids cut to [lo, hi); ctx_j["allowed"] = allowed[lo:hi]; ctx_j["boost"] compiled
from the batch's OWN term lists (never through BoostProgram.select, which is the code under test).  expected_outputs takes
any k <= n, so the same restatement holds the host forms behind num_to_retrieve > max_topk.
numpy and host code only: nothing here needs a device (tests/test_pipeline_options_host.py holds it to a naive loop)."""

import dataclasses

import numpy as np

from tests import option_helpers as oh

FIELDS = ("doc_idx", "doc_score", "group_idx", "hit_idx", "hit_score", "mmr_value")
TOGGLES = ("filter", "seeds", "group_agg", "group_hits", "mmr", "lexical", "boost")
# (kind, per query) of the doc filter by subset number: the pipeline takes packed words, one row [W] or [N, W]
FILTERS = (("half", True), ("payload", True), ("few", False), ("sparse", True), ("payload", False), ("half", False))
# under filter_scope="seeds" the facts come from the allowed passages: only filters broad enough to leave every batch a
# seeded row (PAYLOAD_FILTERS 3 and 4 allow a handful of passages and none; per query they go with the "ranking" scope)
SCOPED_FILTERS = (("half", True), ("payload", False), ("half", False))
ONE_ROW_PAYLOAD = (0, 1, 2, 6)            # the PAYLOAD_FILTERS a one-row filter takes (None is a per-query entry)
FILTER_MODES = 5                          # fact_filter's behaviours, by query number


def batch_cuts(n_queries: int, b: int):
    """[(lo, hi)]: the batches of n_queries on an engine of max_batch b, the last one ragged; none for no query."""
    return [(lo, min(lo + b, n_queries)) for lo in range(0, n_queries, b)]


def want_of(num_to_retrieve: int, n_passages: int, groups=None) -> int:
    """Entries per query as the docstring of iter_batched_retrieve defines them: num_to_retrieve, at least 1 and at most
    the passages there are; a grouped call counts groups, so also at most the groups there are."""
    want = max(1, min(int(num_to_retrieve), int(n_passages)))
    if groups is not None:
        want = max(1, min(want, int(np.max(groups)) + 1))
    return want


def pool_of(mmr_candidates, want: int, n_passages: int, groups=None):
    """mmr_candidates as the engine is asked: None stays None (the call then ranks `want`); else max(mmr_candidates, want),
    at most the passages (groups) there are -- but never below want."""
    if mmr_candidates is None:
        return None
    available = n_passages if groups is None else min(n_passages, int(np.max(groups)) + 1)
    return max(want, min(int(mmr_candidates), available))


def base_iters(ppr_iters: int, ppr_tol: float, narrow, rows: int, damping: float) -> int:
    """The sweeps a batch of `rows` queries is asked for (RetrievalConfig.ppr_base_iters_narrow): under a tolerance, with
    damping <= 0.5 and at most 64 rows, max(11, min(narrow, ppr_iters)); ppr_iters otherwise."""
    if narrow and ppr_tol > 0 and rows <= 64 and damping <= 0.5:
        return max(11, min(int(narrow), int(ppr_iters)))
    return int(ppr_iters)


def csr_rows(csr, ids):
    """The sparse queries `ids` (in that order) of a (q_ptr, q_term, q_weight) triple, as a triple of their own."""
    qp, qt, qw = csr
    ptr, terms, weights = [0], [], []
    for i in ids:
        terms.extend(qt[qp[i]: qp[i + 1]].tolist())
        weights.extend(qw[qp[i]: qp[i + 1]].tolist())
        ptr.append(len(terms))
    return np.asarray(ptr, np.int32), np.asarray(terms, np.int32), np.asarray(weights, np.float32)


def query_number(q: str) -> int:
    """The number of the query string "q<i>" or "q<i> <words>"."""
    return int(q.split()[0][1:])


def fact_filter(k_f: int):
    """A recognition-memory filter that is a function of the query string alone ("q<i>"); by i % FILTER_MODES it keeps every
    candidate; every second one; none (a DPR-fallback row); raises (the same); answers an id twice, an id that was no
    candidate, and more than k_f ids."""
    def flt(query, items, indices, len_after_rerank=None):
        mode = query_number(query) % FILTER_MODES
        ids, its = list(indices), list(items)
        if mode == 0:
            return ids, its, {}
        if mode == 1:
            return ids[::2], its[::2], {}
        if mode == 2:
            return [], [], {}
        if mode == 3:
            raise RuntimeError("filter failed")
        pick = [p for p in (1, 1, None, 0, 2, 3, 4, 0) if p is None or p < len(ids)]
        return ([10 ** 6 if p is None else ids[p] for p in pick],
                [("no", "such", "fact") if p is None else its[p] for p in pick], {})
    return flt


def kept_facts(cand_idx, cand_score, queries, facts, rerank_filter, k_f: int):
    """(kept_idx int32 [b, max(k_f, 1)], kept_score fp32, kept_count int32 [b], kept fact lists): the filter's answer per
    query as phase B takes it (HippoRAG.py:1659-1707) -- the answered ids that were candidates, in the filter's order, at
    most k_f, each with the score phase A gave it; a filter that raises keeps nothing."""
    b = len(queries)
    kept_idx = np.full((b, max(k_f, 1)), -1, np.int32)
    kept_sc = np.zeros((b, max(k_f, 1)), np.float32)
    kept_cnt = np.zeros(b, np.int32)
    seeds = []
    for i, q in enumerate(queries):
        cand = [int(j) for j in cand_idx[i] if j >= 0]
        try:
            ids, kfacts, _ = rerank_filter(q, [facts[j] for j in cand], cand, len_after_rerank=k_f)
        except Exception:                                       # noqa: BLE001 (the reference swallows it, :1705-1707)
            ids, kfacts = [], []
        n = 0
        for j in ids:
            if n < k_f and int(j) in cand:
                kept_idx[i, n] = int(j)
                kept_sc[i, n] = cand_score[i][list(cand_idx[i]).index(int(j))]
                n += 1
        kept_cnt[i] = n
        seeds.append(list(kfacts))
    return kept_idx, kept_sc, kept_cnt, seeds


# ------------------------------------------------------------------------------------------ the calls
def pipeline_spec(on, i: int, n_queries: int, want: int) -> "oh.CallSpec":
    """The whole call of one subset of TOGGLES over n_queries, k = want: the option values rotate with the subset's number i
    as in tests/test_gpu_option_matrix.py::_spec; payload ids (i + r) % 7 and boost programs (i + 3 r) % 10 over the rows."""
    s = oh.CallSpec(entry="retrieve_converged", k=want)
    if "filter" in on:
        table = SCOPED_FILTERS if "seeds" in on else FILTERS
        s.filter_kind, s.filter_per_query = table[i % len(table)]
        s.filter_form, s.filter_seed = "words", 100 + i
        s.payload_ids = [(i + r) % 7 for r in range(n_queries)] if s.filter_per_query else [ONE_ROW_PAYLOAD[i % 4]]
    if "seeds" in on:
        s.filter_scope = "seeds"
    if "group_agg" in on:
        s.group_agg = ("max", "sum")[i % 2]
    if "group_hits" in on:
        s.group_hits = (2, 1, 5)[i % 3]
    if "mmr" in on:
        s.mmr_lambda, s.mmr_candidates = (0.5, 0.0, 1.0, 0.3)[i % 4], (40, None, 10, 200)[(i // 2) % 4]
    if "lexical" in on:
        s.lexical_weight = (0.3, 1.0, 0.5)[i % 3]
    if "boost" in on:
        s.boost_kind, s.boost_form = oh.BOOST_KINDS[i % 2], "program"
        s.boost_ids = [(i + 3 * r) % len(oh.BOOST_PROGRAMS) for r in range(n_queries if s.boost_kind == "per_query" else 1)]
        if s.boost_kind == "one" and oh.BOOST_PROGRAMS[s.boost_ids[0]] is None:       # (None is a per-query entry)
            s.boost_ids[0] = 7
    return s


def call_allowed(spec, n_passages: int, n_queries: int, payload_allowed=None):
    """allowed bool [n_queries, n] of the whole call (None without a filter)."""
    return oh.make_allowed(spec, n_passages, n_queries, payload_allowed)


def offsets_differ(values, b: int) -> bool:
    """Row r differs from row r - b for every r >= b: what makes a wrong batch offset visible."""
    v = list(values)
    return all(not np.array_equal(v[r], v[r - b]) for r in range(b, len(v)))


def batch_spec(spec, lo: int, hi: int, n_passages: int, groups=None):
    """The CallSpec of batch [lo, hi): the per-query ids cut to the batch, mmr_candidates as the engine is asked."""
    s = dataclasses.replace(spec)
    if spec.filter_kind == "payload" and spec.filter_per_query:
        s.payload_ids = list(spec.payload_ids[lo:hi])
    if spec.boost_kind == "per_query":
        s.boost_ids = list(spec.boost_ids[lo:hi])
    if spec.mmr_lambda is not None:
        s.mmr_candidates = pool_of(spec.mmr_candidates, spec.k, n_passages, groups if spec.group_agg is not None else None)
    return s


def batch_ctx(ctx, spec_j, allowed, lo: int, hi: int, columns=None):
    """ctx_j: the call's ctx with allowed[lo:hi] and the boost compiled from the batch's own term lists."""
    c = dict(ctx, allowed=None if allowed is None else np.ascontiguousarray(allowed[lo:hi]))
    c["boost"] = oh.boost_ctx(spec_j, columns, hi - lo) if spec_j.boost_kind is not None else None
    return c


def expected_batch(R_j, spec, ctx, allowed, lo: int, hi: int, columns=None, rows=None, hit_rows=None):
    """expected_outputs of batch [lo, hi) of the call `spec` (k = want) over its anchor rows R_j."""
    groups = ctx.get("groups")
    s = batch_spec(spec, lo, hi, ctx["n_passages"], groups)
    return oh.expected_outputs(R_j, s, batch_ctx(ctx, s, allowed, lo, hi, columns), rows=rows, hit_rows=hit_rows)


def batch_loop_rows(spec, n_rows: int, fallback_rows, rng):
    """(rows, hit_rows) one batch's outputs are checked on, as option_helpers.loop_rows: every row for the rankings; the
    Python-loop restatements (the hit arrays always, every field of an MMR call) on the first and the last row of the
    batch, every DPR-fallback row among its first 16, and rows drawn from rng up to LOOP_ROWS."""
    must = sorted({0, n_rows - 1} | {int(r) for r in fallback_rows if r < min(16, n_rows)})
    rest = [int(r) for r in rng.permutation(n_rows) if r not in must]
    sel = np.sort(np.asarray(must + rest[:max(0, oh.LOOP_ROWS - len(must))], np.int64))
    return (np.arange(n_rows) if spec.mmr_lambda is None else sel), sel


def anchor_kw(spec, allowed_words_j, lexical_j, base: int, ppr_tol: float, ppr_max_iters: int):
    """The scoring configuration of a batch's anchor call: the sweep budget, the scope with the batch's filter rows, the
    lexical blend of the batch's own queries; no boost, group, hits or MMR."""
    kw = dict(k=1, want_all_scores=True, ppr_iters=base, ppr_tol=ppr_tol, ppr_max_iters=ppr_max_iters)
    if spec.filter_scope == "seeds":
        kw.update(filter_scope="seeds", doc_filter=allowed_words_j)
    if spec.lexical_weight is not None and spec.lexical_weight > 0:
        kw.update(lexical=lexical_j, lexical_weight=spec.lexical_weight)
    return kw
