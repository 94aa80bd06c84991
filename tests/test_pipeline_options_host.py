"""The mirror's batch pipeline one layer above the engine, without a device: what retriever.iter_batched_retrieve and
HippoRAG.retrieve_fused hand to the engine per batch (a recording double), the host forms behind num_to_retrieve > max_topk
against option_helpers.expected_outputs, and tests/pipeline_helpers.py itself against a naive per-query loop."""

import dataclasses
import itertools

import numpy as np
import pytest

from tests import option_helpers as oh
from tests import pipeline_helpers as ph
from tests.group_helpers import random_groups, same_bits
from tests.lex_helpers import make_queries

N_PASS, K_F = 150, 5
KEYS = ["year", "user", "score", "flag", "mixed"]


@pytest.fixture(scope="module")
def world():
    from hipporag_amd.payload import encode_columns
    from tests.payload_helpers import columns_of, random_metadata
    rng = np.random.default_rng(612)
    columns = encode_columns(columns_of(random_metadata(rng, N_PASS), KEYS), N_PASS)
    emb = rng.standard_normal((N_PASS, 16)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    groups = random_groups(rng, N_PASS, "shuffled")
    rows = (rng.random((200, N_PASS)) - 0.5).astype(np.float32)    # (the zeros rank in the middle)
    rows[:, 10:40] = np.round(rows[:, 10:40] * 4) / 4               # exact ties
    rows[::3, 50:60] = np.float32(0.0)
    rows[::3, 55:58] = np.float32(-0.0)                             # the two zeros
    rows[1::4, 70:73] = np.float32(np.nan)

    def gram(ids):
        e = emb[np.maximum(ids, 0)]
        return np.einsum("rcd,red->rce", e, e).astype(np.float32)
    return dict(columns=columns, groups=groups, rows=rows, gram=gram, payload_allowed=oh.payload_allowed_fn(columns),
                lex=make_queries(np.random.default_rng(7), 200))


def _ctx(world, max_topk=N_PASS):
    return dict(n_passages=N_PASS, groups=world["groups"], gram=world["gram"], max_topk=max_topk)


# ------------------------------------------------------------------------------------------ the helper itself
def test_the_clamps_are_the_documented_ones():
    g = np.array([0, 1, 1, 2, 0, 2, 1], np.int32)
    assert [ph.want_of(v, 7) for v in (0, 1, 5, 7, 12)] == [1, 1, 5, 7, 7]
    assert [ph.want_of(v, 7, g) for v in (0, 2, 3, 5, 12)] == [1, 2, 3, 3, 3]
    assert ph.batch_cuts(0, 4) == [] and ph.batch_cuts(3, 4) == [(0, 3)] and ph.batch_cuts(4, 4) == [(0, 4)]
    assert ph.batch_cuts(11, 4) == [(0, 4), (4, 8), (8, 11)]
    assert ph.pool_of(None, 5, 7) is None
    assert [ph.pool_of(c, 5, 7) for c in (1, 5, 6, 7, 40)] == [5, 5, 6, 7, 7]
    assert [ph.pool_of(c, 2, 7, g) for c in (1, 2, 3, 40)] == [2, 2, 3, 3]
    assert ph.base_iters(20, 1.5e-6, 12, 64, 0.5) == 12 and ph.base_iters(20, 1.5e-6, 12, 65, 0.5) == 20
    assert ph.base_iters(20, 0.0, 12, 4, 0.5) == 20 and ph.base_iters(20, 1e-6, None, 4, 0.5) == 20
    assert ph.base_iters(20, 1e-6, 3, 4, 0.5) == 11 and ph.base_iters(11, 1e-6, 30, 4, 0.5) == 11
    assert ph.base_iters(20, 1e-6, 12, 4, 0.85) == 20


def test_the_rotations_move_every_per_query_value_between_batches(world):
    """(i + r) % 7 and (i + 3 r) % 10 at b = 4, 16, 65: row r never carries the value of row r - b -- payload id, filter row,
    boost program, lexical query -- so a batch served with another batch's rows cannot pass."""
    lex = world["lex"]
    for b in (4, 16, 65):
        n = 2 * b + 3
        assert ph.offsets_differ([ph.csr_rows(lex, [r])[1].tolist() + ph.csr_rows(lex, [r])[2].tolist() for r in range(n)], b)
        for i in range(64):
            s = ph.pipeline_spec(ph.TOGGLES, i, n, 10)
            if s.filter_per_query:
                assert ph.offsets_differ(s.payload_ids, b), (b, i)
                assert ph.offsets_differ(ph.call_allowed(s, N_PASS, n, world["payload_allowed"]), b), (b, i, s.filter_kind)
            if s.boost_kind == "per_query":
                assert ph.offsets_differ(s.boost_ids, b), (b, i)
                assert ph.offsets_differ([oh.BOOST_PROGRAMS[j] for j in s.boost_ids], b), (b, i)


def test_the_fact_filter_and_the_kept_facts(world):
    facts = [("s", "p", str(j)) for j in range(100)]
    flt = ph.fact_filter(K_F)
    cand = np.array([[10, 11, 12, 13, 14]] * 5 + [[20, 21, -1, -1, -1]], np.int32)
    sc = np.linspace(1, 0.5, 30, dtype=np.float32).reshape(6, 5)
    qs = [f"q{i}" for i in (0, 1, 2, 3, 4, 9)]
    idx, ksc, cnt, seeds = ph.kept_facts(cand, sc, qs, facts, flt, K_F)
    assert cnt.tolist() == [5, 3, 0, 0, 5, 4]
    assert idx[1].tolist() == [10, 12, 14, -1, -1] and ksc[1].tolist()[:3] == [sc[1, 0], sc[1, 2], sc[1, 4]]
    assert idx[4].tolist() == [11, 11, 10, 12, 13]                  # twice, the foreign id dropped, cut at k_f
    assert idx[5].tolist() == [21, 21, 20, 20, -1]                  # two candidates: what there is
    assert seeds[2] == [] and seeds[3] == [] and len(seeds[4]) == 8 and ("no", "such", "fact") in seeds[4]
    assert ph.csr_rows(world["lex"], [3, 1])[0].tolist()[0] == 0


@pytest.mark.parametrize("b", [4, 65])
def test_the_batch_restatement_is_the_per_query_restatement(world, b):
    """expected_batch over [lo, hi) equals, row by row, expected_outputs of that ONE query with its own filter row, payload
    id and boost list: the helper cuts nothing at the wrong offset."""
    n = 2 * b + 3
    R = world["rows"][:n]
    subsets = [on for r in range(len(ph.TOGGLES) + 1) for on in itertools.combinations(ph.TOGGLES, r)]
    checked = 0
    for i, on in enumerate(subsets):
        if "lexical" in on:                  # (scoring options do not enter the restatement)
            continue
        spec = ph.pipeline_spec(on, i, n, 10)
        if oh.servable(spec, dict(max_topk=N_PASS)) is not None:
            continue
        allowed = ph.call_allowed(spec, N_PASS, n, world["payload_allowed"])
        for lo, hi in ph.batch_cuts(n, b):
            sel = np.array(sorted({0, hi - lo - 1, (hi - lo) // 2}))
            got = ph.expected_batch(R[lo:hi], spec, _ctx(world), allowed, lo, hi, world["columns"], rows=sel, hit_rows=sel)
            for at, r in enumerate(sel + lo):
                one = dataclasses.replace(spec)
                if spec.filter_kind == "payload" and spec.filter_per_query:
                    one.payload_ids = [spec.payload_ids[r]]
                if spec.boost_kind == "per_query":
                    one.boost_ids = [spec.boost_ids[r]]
                one.mmr_candidates = ph.pool_of(spec.mmr_candidates, 10, N_PASS, world["groups"] if spec.group_agg else None)
                ctx = dict(_ctx(world), allowed=None if allowed is None else allowed[r:r + 1],
                           boost=oh.boost_ctx(one, world["columns"], 1) if one.boost_kind else None)
                want = oh.expected_outputs(R[r:r + 1], one, ctx)
                for name in ph.FIELDS:
                    assert (got[name] is None) == (want[name] is None), (on, name)
                    if want[name] is not None:
                        g, w = got[name][at], want[name][0]
                        assert same_bits(g, w) if w.dtype == np.float32 else np.array_equal(g, w), (on, lo, r, name)
                checked += 1
    assert checked == 9 * 30             # the 30 servable subsets without lexical x 3 batches x 3 rows


# ------------------------------------------------------------------------------------------ what the engine is handed
class _Recorder:
    """An engine double that records every call.  Queries are tagged by their number (column 0 of the query tensor).  Phase
    A answers facts 10 * tag + slot; phase B answers doc_idx = tag in every slot and, when asked for all scores, the rows
    of `table` of its tags -- so the host forms can be held to the restatement over those rows."""
    has_fact_sources = True

    def __init__(self, max_batch, max_topk, table, groups, two_halves=False):
        import torch
        if two_halves:
            self.retrieve_converged_start = self._start
        self.max_batch, self.max_topk, self.table, self.groups = max_batch, max_topk, table, groups
        self.device, self.emb_dtype = torch.device("cpu"), torch.float32
        self.a, self.b, self.fused = [], [], []

    def last_doc_scores(self, batch):          # (its presence is what lets the pipeline rank beyond max_topk)
        raise AssertionError("the pipeline reads all_scores, not the handle")

    def score_facts(self, q, k, scope_filter=None):
        import torch
        tags = q[:, 0].int()
        self.a.append(dict(tags=tags.tolist(), k=k, scope_filter=None if scope_filter is None else scope_filter.numpy().copy()))
        idx = (tags[:, None] * 10 + torch.arange(k, dtype=torch.int32)[None, :]).to(torch.int32)
        return idx, torch.linspace(1.0, 0.5, k).repeat(q.shape[0], 1)

    def retrieve_converged(self, q, kept_idx, kept_score, kept_count, **kw):
        import torch
        from hipporag_amd.engine import RetrieveOutput
        tags = q[:, 0].int()
        rec = dict(kw, tags=tags.tolist(), kept_idx=kept_idx.numpy().copy(), kept_count=kept_count.numpy().copy())
        if "doc_filter" in kw:
            rec["doc_filter"] = kw["doc_filter"].numpy().copy()
        self.b.append(rec)
        b, k = len(tags), kw["k"]
        ids = tags[:, None].repeat(1, k).to(torch.int32)
        out = RetrieveOutput(ids, ids.float(), torch.where(kept_count == 0, 1, 0).to(torch.int32), torch.zeros(b),
                             torch.full((b,), 20, dtype=torch.int32))
        if kw.get("group_agg") is not None:
            out.group_idx = ids.clone()
        if kw.get("group_hits") is not None:
            out.hit_idx = ids[:, :, None].repeat(1, 1, kw["group_hits"])
            out.hit_score = out.hit_idx.float()
        if kw.get("mmr_lambda") is not None:
            out.mmr_value = ids.float()
        if kw.get("want_all_scores"):
            out.all_scores = torch.from_numpy(self.table[tags.numpy()])
        return out

    def _start(self, *a, **kw):
        out = self.retrieve_converged(*a, **kw)

        class Pending:
            repeated, flags = False, out.flags.numpy()

            def finish(self):
                return out
        p = Pending()
        p.out = out
        return p

    def last_fused(self, mp, **kw):
        import torch
        from hipporag_amd.engine import RetrieveOutput
        self.fused.append(dict(kw, mp=np.asarray(mp).tolist(),
                               doc_filter=None if kw.get("doc_filter") is None else kw["doc_filter"].numpy().copy()))
        nq, k = len(mp) - 1, kw["k"]
        ids = torch.zeros((nq, k), dtype=torch.int32)
        out = RetrieveOutput(ids, ids.float(), torch.zeros(nq, dtype=torch.int32))
        out.group_idx = ids if kw.get("group_agg") else None
        return out


def _q_tensor(qs, kind):
    import torch
    return torch.tensor([[float(ph.query_number(q))] for q in qs])


def _drive(eng, world, spec, n, num, *, ppr_tol=1.5e-6, keep_all=False, encoded=None):
    """iter_batched_retrieve over n queries with the options of `spec` -> [(lo, rows)], allowed, words, the BoostProgram"""
    from hipporag_amd.boost import compile_boosts
    from hipporag_amd.engine import pack_mask
    from hipporag_amd.retriever import iter_batched_retrieve
    queries = [f"q{i}" for i in range(n)]
    facts = [("s", "p", str(j)) for j in range(10 * n + 10)]
    allowed = ph.call_allowed(spec, N_PASS, max(n, 1), world["payload_allowed"])      # (n = 0: a filter without rows)
    kw = dict(linking_top_k=K_F, damping=0.5, passage_node_weight=0.05, ppr_iters=20, num_to_retrieve=num,
              n_passages=N_PASS, ppr_tol=ppr_tol, ppr_max_iters=60, ppr_base_iters_narrow=12, keep_all_scores=keep_all)
    words = None
    if allowed is not None:
        words = pack_mask(allowed if spec.filter_per_query else allowed[0])
        words = words[:n] if spec.filter_per_query else words
        kw.update(doc_filter=words, filter_scope=spec.filter_scope)
    if spec.group_agg is not None:
        kw.update(group_agg=spec.group_agg, group_of=world["groups"], group_hits=spec.group_hits)
    if spec.mmr_lambda is not None:
        kw.update(mmr_lambda=spec.mmr_lambda, mmr_candidates=spec.mmr_candidates)
    if spec.lexical_weight is not None:
        def encode(qs):
            encoded.append(list(qs))
            return ph.csr_rows(world["lex"], [ph.query_number(q) for q in qs])
        kw.update(lexical_encode=encode, lexical_weight=spec.lexical_weight)
    prog = None
    if spec.boost_kind is not None:
        prog = compile_boosts(world["columns"], oh.boost_arg(spec, max(n, 1)), max(n, 1))
        kw["boost"] = prog
    got = list(iter_batched_retrieve(eng, queries, _q_tensor, facts, ph.fact_filter(K_F), **kw))
    return got, allowed, words, prog


def _same_arrays(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f")
                                    for x, y in zip(a, b))


@pytest.mark.parametrize("b,n", [(4, 11), (4, 3), (4, 4), (4, 0), (65, 133), (65, 64)])
def test_every_batch_hands_the_engine_its_own_rows_and_the_documented_clamps(world, b, n):
    """Per batch [lo, hi): the filter rows in both scopes and in score_facts(scope_filter=), the boost rows, the strings
    given to lexical_encode, k, mmr_candidates, group_hits, want_all_scores and ppr_iters -- over the servable subsets of
    the options, with the ragged last batch, N < b, N = b and N = 0."""
    from hipporag_amd.boost import compile_boosts
    max_topk = 60
    subsets = [on for r in range(len(ph.TOGGLES) + 1) for on in itertools.combinations(ph.TOGGLES, r)]
    served = 0
    for i, on in enumerate(subsets):
        num = (10, 25, max_topk + 7)[i % 3] if "mmr" not in on else 10
        groups = world["groups"] if "group_agg" in on else None
        want = ph.want_of(num, N_PASS, groups)
        spec = ph.pipeline_spec(on, i, max(n, 1), want)
        if oh.servable(spec, dict(max_topk=max_topk)) is not None:
            continue
        served += 1
        eng, encoded = _Recorder(b, max_topk, world["rows"], world["groups"]), []
        keep_all = bool(i % 2)
        got, allowed, words, prog = _drive(eng, world, spec, n, num, keep_all=keep_all, encoded=encoded)
        cuts = ph.batch_cuts(n, b)
        assert [lo for lo, _ in got] == [lo for lo, _ in cuts] and len(eng.b) == len(cuts) == len(eng.a)
        beyond = want > max_topk
        scoped = spec.filter_scope == "seeds"
        if spec.lexical_weight is not None:
            assert encoded == [[f"q{r}" for r in range(lo, hi)] for lo, hi in cuts]
        for (lo, hi), a, rec, (_, rows) in zip(cuts, eng.a, eng.b, got):
            tags = list(range(lo, hi))
            assert a["tags"] == tags and rec["tags"] == tags and a["k"] == K_F
            rows_w = None if words is None else (words if words.ndim == 1 else words[lo:hi])
            if scoped:
                assert np.array_equal(a["scope_filter"].view(np.uint32), rows_w) and rec["filter_scope"] == "seeds"
            else:
                assert a["scope_filter"] is None and "filter_scope" not in rec
            if words is None:
                assert "doc_filter" not in rec
            else:
                assert rec["doc_filter"].dtype == np.int32 and np.array_equal(rec["doc_filter"].view(np.uint32), rows_w)
            if prog is None:
                assert "boost" not in rec
            else:
                own = compile_boosts(world["columns"], oh.boost_arg(ph.batch_spec(spec, lo, hi, N_PASS, groups), hi - lo), hi - lo)
                assert rec["boost"].broadcast == own.broadcast == (spec.boost_kind == "one")
                assert rec["boost"].batch == own.batch and _same_arrays(rec["boost"].arrays(), own.arrays()), (on, lo)
            if spec.lexical_weight is not None:
                assert _same_arrays(rec["lexical"], ph.csr_rows(world["lex"], tags)) and rec["lexical_weight"] == spec.lexical_weight
            else:
                assert "lexical" not in rec and "lexical_weight" not in rec
            assert rec["k"] == min(want, max_topk), (on, num)
            if spec.mmr_lambda is None:
                assert "mmr_lambda" not in rec and "mmr_candidates" not in rec
            else:
                c = ph.pool_of(spec.mmr_candidates, want, N_PASS, groups)
                assert rec["mmr_lambda"] == spec.mmr_lambda and rec["mmr_candidates"] == (want if c is None else c)
            assert rec.get("group_agg") == spec.group_agg
            assert rec.get("group_hits") == (None if beyond else spec.group_hits)          # withheld: the host form serves them
            assert bool(rec.get("want_all_scores")) == (beyond or keep_all)
            assert rec["ppr_iters"] == ph.base_iters(20, 1.5e-6, 12, hi - lo, 0.5) == (12 if hi - lo <= 64 else 20)
            assert (rec["link_top_k"], rec["damping"], rec["ppr_tol"], rec["ppr_max_iters"]) == (K_F, 0.5, 1.5e-6, 60)
            # the kept facts of every query are the filter's answer over ITS candidates
            cand = np.array([[10 * t + s for s in range(K_F)] for t in tags], np.int32)
            k_idx, _, k_cnt, seeds = ph.kept_facts(cand, np.tile(np.linspace(1.0, 0.5, K_F, dtype=np.float32), (hi - lo, 1)),
                                                   [f"q{t}" for t in tags], [("s", "p", str(j)) for j in range(10 * n + 10)],
                                                   ph.fact_filter(K_F), K_F)
            assert np.array_equal(rec["kept_idx"], k_idx) and np.array_equal(rec["kept_count"], k_cnt)
            assert [r[2] for r in rows] == seeds and len(rows) == hi - lo
            assert (k_cnt == 0).any() or hi - lo < 3
            if keep_all:
                assert rows.repeated is True and np.array_equal(rows.all_scores.numpy(), world["rows"][lo:hi], equal_nan=True)
            if not beyond:
                assert rows.doc_idx.shape == (hi - lo, min(want, max_topk)) and (rows.doc_idx == np.array(tags)[:, None]).all()
                assert (rows.group_idx is None) == (spec.group_agg is None) and (rows.hit_idx is None) == (spec.group_hits is None)
                assert (rows.mmr_value is None) == (spec.mmr_lambda is None)
                continue
            # the host forms: the restatement over the rows the double answered, k = want > max_topk
            exp = ph.expected_batch(world["rows"][lo:hi], dataclasses.replace(spec, boost_kind=None), _ctx(world, max_topk),
                                    allowed, lo, hi, world["columns"])
            for name in ph.FIELDS[:5]:
                g, w = getattr(rows, name), exp[name]
                assert (g is None) == (w is None), (on, name)
                if w is not None:
                    assert g.shape == w.shape and g.dtype == w.dtype, (on, name, g.shape, w.shape)
                    assert same_bits(g, w) if w.dtype == np.float32 else np.array_equal(g, w), (on, lo, name)
    assert served == 51, served          # 60 of the 128 subsets are servable; 9 of them ask MMR for 200 > max_topk candidates


@pytest.mark.parametrize("num", [61, N_PASS, N_PASS + 5])
def test_the_host_forms_beyond_max_topk_are_the_restatement(world, num):
    """num_to_retrieve in {max_topk + 1, n, n + 5} over rows with exact ties, both zeros and NaN: the bare argsort, rank_allowed
    (a "few" filter leaves fewer than want: the -1 / 0 padding), group_rank_rows and group_hits_rows, max and sum."""
    S = lambda **kw: oh.CallSpec(entry="retrieve_converged", filter_form="words", **kw)
    calls = [S(), S(filter_kind="half", filter_per_query=True, filter_seed=3), S(filter_kind="few", filter_seed=4),
             S(group_agg="max"), S(group_agg="sum", group_hits=2), S(group_agg="max", group_hits=3, filter_kind="sparse", filter_seed=5),
             S(group_agg="sum", group_hits=1, filter_kind="payload", filter_per_query=True, payload_ids=[r % 7 for r in range(11)])]
    assert int(world["groups"].max()) + 1 > 20
    for spec in calls:
        spec.k = ph.want_of(num, N_PASS, world["groups"] if spec.group_agg else None)
        eng = _Recorder(4, 20, world["rows"], world["groups"])
        got, allowed, _, _ = _drive(eng, world, spec, 11, num)
        assert all(rec["k"] == 20 and rec["want_all_scores"] and "group_hits" not in rec for rec in eng.b)
        for (lo, hi), (_, rows) in zip(ph.batch_cuts(11, 4), got):
            exp = ph.expected_batch(world["rows"][lo:hi], spec, _ctx(world, 20), allowed, lo, hi, world["columns"])
            for name in ph.FIELDS[:5]:
                g, w = getattr(rows, name), exp[name]
                assert (g is None) == (w is None), (spec, name)
                if w is not None:
                    assert g.shape == w.shape and g.dtype == w.dtype, (spec, name, g.shape, w.shape)
                    assert same_bits(g, w) if w.dtype == np.float32 else np.array_equal(g, w), (spec, lo, name)


def test_a_tolerance_of_zero_and_no_narrow_budget_keep_the_sweep_count(world):
    for tol, narrow, want_iters in ((0.0, 12, 20), (1.5e-6, None, 20), (1.5e-6, 40, 20), (1.5e-6, 5, 11)):
        from hipporag_amd.retriever import iter_batched_retrieve
        eng = _Recorder(4, 60, world["rows"], world["groups"])
        list(iter_batched_retrieve(eng, ["q0", "q1"], _q_tensor, [], ph.fact_filter(K_F), linking_top_k=K_F, damping=0.5,
                                   passage_node_weight=0.05, ppr_iters=20, num_to_retrieve=5, n_passages=N_PASS, ppr_tol=tol,
                                   ppr_base_iters_narrow=narrow))
        assert [r["ppr_iters"] for r in eng.b] == [want_iters]


def test_the_refusals_of_this_layer_come_before_anything_is_enqueued(world):
    eng = _Recorder(4, 60, world["rows"], world["groups"])
    base = oh.CallSpec(entry="retrieve_converged", k=10)
    cases = [(dataclasses.replace(base, mmr_lambda=0.5, mmr_candidates=61), ValueError, "mmr_candidates"),
             (dataclasses.replace(base, filter_kind="half", filter_scope="seeds", lexical_weight=0.3), NotImplementedError,
              "filter_scope")]
    for spec, exc, name in cases:
        with pytest.raises(exc, match=name):
            _drive(eng, world, spec, 11, 10, encoded=[])
    eng.has_fact_sources = False
    with pytest.raises(ValueError, match="set_fact_sources"):
        _drive(eng, world, dataclasses.replace(base, filter_kind="half", filter_scope="seeds"), 11, 10)
    from hipporag_amd.retriever import iter_batched_retrieve
    with pytest.raises(ValueError, match="group_of"):
        list(iter_batched_retrieve(eng, ["q0"], _q_tensor, [], ph.fact_filter(K_F), linking_top_k=K_F, damping=0.5,
                                   passage_node_weight=0.05, ppr_iters=20, num_to_retrieve=5, n_passages=N_PASS, group_agg="max"))
    assert not eng.a and not eng.b


# ------------------------------------------------------------------------------------------ retrieve_fused's chunks
def _fused_mirror(world, max_batch, max_topk):
    from hipporag_amd.retriever import HippoRAG, RetrievalConfig
    rag = HippoRAG(RetrievalConfig(max_batch=max_batch, retrieval_top_k=max_topk))
    rag.passage_texts = [f"passage {i}" for i in range(N_PASS)]
    rag.passage_node_keys = [f"chunk-{i}" for i in range(N_PASS)]
    rag.chunk_metadata = {f"chunk-{i}": {"src": int(world["groups"][i])} for i in range(N_PASS)}
    rag.engine = _Recorder(max_batch, max_topk, world["rows"], world["groups"], two_halves=True)
    rag.engine.set_passage_groups = lambda g: None
    rag.ready_to_retrieve = True
    rag.get_query_embeddings = lambda qs: None
    rag._q_tensor = _q_tensor
    return rag


@pytest.mark.parametrize("num", [5, 70])
def test_fused_chunks_hold_whole_questions_under_their_own_filter_rows(world, num):
    """retrieve_fused cuts the questions into device chunks of at most max_batch sub-queries: no question straddles two
    chunks, every member run gets its QUESTION's filter row, the fusion gets the chunk's member_ptr and question rows --
    on the device form and on the host form (num_to_retrieve > max_topk)."""
    sizes = [3, 1, 2, 4, 1, 1, 3, 2, 4, 2]
    rag = _fused_mirror(world, 4, 60)
    start = np.concatenate([[0], np.cumsum(sizes)])
    questions = [[f"q{m}" for m in range(start[j], start[j + 1])] for j in range(len(sizes))]
    allowed = np.random.default_rng(5).random((len(sizes), N_PASS)) < 0.5
    assert ph.offsets_differ(allowed, 1)
    got = rag.retrieve_fused(questions, fuse="sum", num_to_retrieve=num, doc_filter=[a for a in allowed], filter_scope="seeds")
    from hipporag_amd.engine import pack_mask
    words = pack_mask(allowed)
    eng = rag.engine
    chunks = [r["tags"] for r in eng.b]
    assert [m for c in chunks for m in c] == list(range(start[-1])) and all(len(c) <= 4 for c in chunks)
    q_of = np.repeat(np.arange(len(sizes)), sizes)
    seen = 0
    for c, a, rec in zip(chunks, eng.a if eng.a else [None] * len(chunks), eng.b):
        qs = sorted(set(q_of[c].tolist()))
        assert c == list(range(start[qs[0]], start[qs[-1] + 1]))                        # whole questions
        assert np.array_equal(rec["doc_filter"].view(np.uint32), words[q_of[c]]) and rec["filter_scope"] == "seeds"
        assert rec["k"] == 1 and rec["want_all_scores"] is True
        seen += len(qs)
    assert seen == len(sizes) and len(chunks) >= 3 and len(got) == len(sizes)
    if num <= 60:
        assert len(eng.fused) == len(chunks)
        for c, f in zip(chunks, eng.fused):
            qs = sorted(set(q_of[c].tolist()))
            assert f["mp"] == (start[qs[0]: qs[-1] + 2] - start[qs[0]]).tolist()
            assert np.array_equal(f["doc_filter"].view(np.uint32), words[qs]) and f["k"] == num
    else:                                   # the host form: fuse_rows_host + rank_allowed per chunk, under the questions' rows
        assert not eng.fused
        from tests.fuse_helpers import fuse_np
        for j, sol in enumerate(got):
            F = fuse_np(world["rows"][start[j]: start[j + 1]], [0, sizes[j]], "sum", None, 60, None, allowed[j: j + 1])
            idx, sc = oh.rank_rows(F, num, allowed[j: j + 1])
            keep = idx[0] >= 0
            assert sol.docs == [f"passage {p}" for p in idx[0][keep]] and same_bits(np.asarray(sol.doc_scores), sc[0][keep])
    with pytest.raises(ValueError, match="exceeds max_batch=4"):
        rag.retrieve_fused([["q0", "q1", "q2", "q3", "q4"]], fuse="sum", num_to_retrieve=5)
