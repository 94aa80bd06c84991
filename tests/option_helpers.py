"""The composed retrieve call restated in numpy: every option of HippoRAGEngine.retrieve / retrieve_scored / dense_retrieve /
retrieve_converged / last_fused (doc filter, filter_scope="seeds", group_agg, group_hits, fusion, mmr_*, lexical, boost) is a
pure function of the fp32 score rows R the UNBOOSTED call leaves on the handle (last_doc_scores), the filter bits, the group
table, the passage embeddings, the payload columns and the option values.  expected_outputs composes the per-feature
restatements of tests/*_helpers.py in the order engine.py documents; servable is the refusal table of engine.py's
docstrings; random_spec / plan generate calls.
numpy only: nothing here needs a device (tests/test_option_helpers_host.py holds this file to a naive loop)."""

import dataclasses
import json
from typing import List, Optional

import numpy as np

from tests.fuse_helpers import fuse_np, partitions
from tests.group_helpers import canonical, group_rank_np
from tests.group_hits_helpers import group_hits_np
from tests.mmr_helpers import mmr_batch_np

ENTRIES = ("retrieve", "retrieve_scored", "dense_retrieve", "retrieve_converged", "last_fused")
FILTER_KINDS = ("none", "all", "empty", "one", "few", "half", "sparse", "payload")
FILTER_FORMS = ("bool", "words", "payload")
OPTIONS = ("filter", "seeds", "group_agg", "group_hits", "fusion", "mmr", "lexical", "boost")
GROUP_KINDS = ("one", "singletons", "two", "contiguous", "shuffled", "sorted")
BATCHES = (1, 8, 9, 64, 65, 130, 257)      # the last small-batch kernel; both ends of the fp16 state; one e4m3 slab; a slab
#                                            pair; a pair plus an odd slab
MMR_MAX_CANDIDATES = 1024
LOOP_ROWS = 8                              # rows per call the Python-loop restatements (MMR, hits) check
PLAN_SEED, PLAN_CASES, PLAN_CALLS = 60612, 84, 6     # the plan the three GPU slices of tests/test_gpu_soak_slices.py run between
#                                                      them; tests/test_option_helpers_host.py asserts what it covers

# filter dicts over the keys of payload_helpers.random_metadata: a broad one, a conjunction, $any, a set that holds a
# handful of passages, nothing, no filter for this query, a range with a negation
PAYLOAD_FILTERS = [{"year": {"$gte": 2020}}, {"user": ["alice", "bob"], "$not": {"year": 2021}},
                   {"$any": {"score": {"$lt": 1.0}, "user": "carol"}, "year": {"$exists": True}},
                   {"user": "dave", "year": 2018, "score": 3.5, "flag": True}, {"user": "nobody"}, None,
                   {"score": {"$gt": 0.5, "$lte": 2.5}, "$not": {"flag": {"$exists": False}}}]

# term lists of hipporag_amd/boost.py's grammar over the same keys (BOOST_PROGRAMS[i] is one query's boost):
#  0  a constant MUL under $any, a constant ADD under $not of an IN-list
#  1  FIELD terms: sqrt with a `missing` value on a column with holes, the plain value with and without one
#  2  NaN entries: the metadata holds no negative number, so no sqrt is NaN; year * 1e306 is +inf in fp64 and two such ADDs
#     of opposite sign sum to NaN wherever the condition holds and the passage has a year
#  3 / 4 / 5  the linear / exp / gauss decays (MUL with missing, MUL without: no hit where the value is absent, ADD)
#  6  mul 0.0 under a condition (and a negative MUL on top: M = -0.0): exact ties at zero over most of a row
#  7  an ADD far above every score on a handful of passages: they lead the second ranking whatever the first one was
#  8 / 9  [] and None: a query without terms (None only as an entry of a per-query program)
BOOST_PROGRAMS = [
    [{"if": {"$any": {"user": "alice", "year": 2022}}, "mul": 1.5}, {"if": {"$not": {"user": ["bob", "carol"]}}, "add": -1e-3}],
    [{"field": "score", "modifier": "sqrt", "add": 1e-4, "missing": 0.0}, {"field": "mixed", "mul": 0.5, "missing": 2.0},
     {"field": "score", "add": -2e-5}],
    [{"if": {"flag": True}, "field": "year", "add": 1e306}, {"if": {"flag": True}, "field": "year", "add": -1e306},
     {"field": "mixed", "modifier": "sqrt", "mul": 1.25}],
    [{"decay": {"field": "year", "origin": 2023, "scale": 3, "kind": "linear"}, "mul": 1.0, "missing": 0.25}],
    [{"decay": {"field": "score", "origin": 0.0, "scale": 1.5, "offset": 0.5, "kind": "exp"}, "mul": 2.0}],
    [{"decay": {"field": "mixed", "origin": 2.5, "scale": 0.7, "decay": 0.3, "kind": "gauss"}, "add": 1e-3, "missing": -1.0}],
    [{"if": {"year": {"$lte": 2021}}, "mul": 0.0}, {"if": {"user": "dave"}, "mul": -1.0}],
    [{"if": {"user": "dave", "year": 2018}, "add": 10.0}],
    [], None]
BOOST_KINDS = ("one", "per_query")
BOOST_FORMS = ("grammar", "program")


@dataclasses.dataclass
class CallSpec:
    """One call.  filter_kind "none": no doc filter; "payload": the rows of PAYLOAD_FILTERS named by payload_ids, in any
    form; the other kinds in the forms "bool" / "words".  filter_per_query: [rows, n] (one row for the batch otherwise),
    rows = the questions of a last_fused, else the batch.  entry "last_fused": a retrieve (carrying the scope, its filter
    and the lexical blend) followed by last_fused (carrying the filter, the groups, the hits, MMR and the boost).
    boost_kind None: no boost; "one": BOOST_PROGRAMS[boost_ids[0]] for every row (BoostProgram.broadcast); "per_query": row r
    takes BOOST_PROGRAMS[boost_ids[r]]; boost_form: the grammar itself handed to the call, or compile_boosts' program."""
    entry: str = "retrieve"
    k: int = 10
    filter_kind: str = "none"
    filter_form: str = "bool"
    filter_per_query: bool = False
    filter_seed: int = 0
    payload_ids: Optional[List[int]] = None
    filter_scope: str = "ranking"
    group_agg: Optional[str] = None
    group_hits: Optional[int] = None
    mmr_lambda: Optional[float] = None
    mmr_candidates: Optional[int] = None
    lexical_weight: Optional[float] = None       # None: no lexical
    lexical_empty: bool = False                  # every query without terms
    fuse: Optional[str] = None                   # last_fused only: "sum" / "max" / "rrf"
    member_ptr: Optional[List[int]] = None
    weights: Optional[List[float]] = None
    rrf_c: int = 60
    rrf_depth: Optional[int] = None
    workspace: bool = False
    boost_kind: Optional[str] = None
    boost_ids: Optional[List[int]] = None
    boost_form: str = "grammar"

    def to_json(self) -> str:
        return json.dumps(dataclasses.asdict(self))

    @classmethod
    def from_dict(cls, d) -> "CallSpec":
        return cls(**d)

    def options(self):
        """The options that are on."""
        on = []
        if self.filter_kind != "none":
            on.append("filter")
        if self.filter_scope == "seeds":
            on.append("seeds")
        for name, v in (("group_agg", self.group_agg), ("group_hits", self.group_hits)):
            if v is not None:
                on.append(name)
        if self.entry == "last_fused":
            on.append("fusion")
        if self.mmr_lambda is not None or self.mmr_candidates is not None:
            on.append("mmr")
        if self.lexical_weight is not None:
            on.append("lexical")
        if self.boost_kind is not None:
            on.append("boost")
        return on

    def rows(self, batch: int) -> int:
        """Rows of the call's outputs: the questions of a fusion, else the batch."""
        return len(self.member_ptr) - 1 if self.entry == "last_fused" else batch

    def candidates(self) -> int:
        """Entries the call ranks: c = max(mmr_candidates, k) under MMR, else k."""
        if self.mmr_lambda is None:
            return self.k
        return max(self.k if self.mmr_candidates is None else self.mmr_candidates, self.k)


def servable(spec: CallSpec, limits=None):
    """None, or (exception type, the argument the message names) of the FIRST refusal the call meets -- the table of
    engine.py's docstrings, in the order the calls check:
      - filter_scope="seeds" without a doc filter: ValueError (filter_scope);
      - lexical with filter_scope="seeds": NotImplementedError (filter_scope); dense_retrieve(lexical=): ValueError;
      - dense_retrieve(lexical=) with group_agg / group_hits / mmr_lambda / mmr_candidates: ValueError naming it;
      - mmr_candidates without mmr_lambda, c > 1024, c > max_topk: ValueError (mmr_candidates);
      - group_hits without group_agg: ValueError (group_hits);
      - the "seeds" scope takes its kept facts from score_facts(scope_filter=), which without fact sources raises
        RuntimeError (HragError) naming set_fact_sources;
      - dense_retrieve(boost=) with group_agg / group_hits / mmr_lambda / mmr_candidates / lexical: ValueError naming it, then
        with filter_scope="seeds": ValueError (filter_scope) -- all before dense_retrieve's lexical refusals.  On every
        other entry boost adds no refusal: retrieve / retrieve_scored / retrieve_converged / last_fused compile it after
        their own checks and serve it with every option they serve.
    limits: dict(max_topk=, fact_sources=); what is missing is not checked."""
    lim = limits or {}
    seeds, lex = spec.filter_scope == "seeds", spec.lexical_weight is not None
    scope_err = (ValueError, "filter_scope") if seeds and spec.filter_kind == "none" else None
    lex_scope = (NotImplementedError, "filter_scope") if seeds and lex else None
    mmr_err = None
    if spec.mmr_lambda is None:
        if spec.mmr_candidates is not None:
            mmr_err = (ValueError, "mmr_candidates")
    elif spec.candidates() > min(lim.get("max_topk", MMR_MAX_CANDIDATES), MMR_MAX_CANDIDATES):
        mmr_err = (ValueError, "mmr_candidates")
    hits_err = (ValueError, "group_hits") if spec.group_hits is not None and spec.group_agg is None else None
    src_err = (RuntimeError, "fact_sources") if seeds and not lim.get("fact_sources", True) else None
    if spec.entry == "dense_retrieve" and spec.boost_kind is not None:
        for name in ("group_agg", "group_hits", "mmr_lambda", "mmr_candidates"):
            if getattr(spec, name) is not None:
                return ValueError, name
        if lex:
            return ValueError, "lexical"
        return (ValueError, "filter_scope") if seeds else None
    if spec.entry == "dense_retrieve" and lex:
        for name in ("group_agg", "group_hits", "mmr_lambda", "mmr_candidates"):
            if getattr(spec, name) is not None:
                return ValueError, name
        return (ValueError, "filter_scope") if seeds else None
    if spec.entry != "last_fused":
        order = (mmr_err, scope_err, lex_scope, hits_err, src_err)    # MMR's arguments are checked before any work
    else:                                                             # the retrieve behind it refuses first
        order = (scope_err, lex_scope, mmr_err, hits_err, src_err)
    for err in order:
        if err is not None:
            return err
    return None


# ------------------------------------------------------------------------------------------ the filter bits
def make_allowed(spec: CallSpec, n: int, rows: int, payload_allowed=None):
    """allowed bool [rows, n] of the spec's doc filter (None without one); a one-row filter is repeated.  A function of the
    spec alone.  payload_allowed(filters) -> bool [len(filters), n]: the restatement of a list of filter dicts."""
    if spec.filter_kind == "none":
        return None
    m = rows if spec.filter_per_query else 1
    rng = np.random.default_rng(spec.filter_seed)
    kind = spec.filter_kind
    if kind == "payload":
        a = np.asarray(payload_allowed([PAYLOAD_FILTERS[i] for i in spec.payload_ids[:m]]), bool)
    elif kind == "all":
        a = np.ones((m, n), bool)
    elif kind == "empty":
        a = np.zeros((m, n), bool)
    elif kind in ("one", "few"):
        a = np.zeros((m, n), bool)
        for r in range(m):
            cnt = 1 if kind == "one" else (int(rng.integers(1, spec.k)) if spec.k > 1 else 0)      # fewer than k
            a[r, rng.choice(n, min(cnt, n), replace=False)] = True
    else:
        a = rng.random((m, n)) < (0.5 if kind == "half" else 0.01)
    return np.ascontiguousarray(np.broadcast_to(a, (rows, n)) if m == 1 else a)


def payload_allowed_fn(host_columns):
    """payload_allowed for make_allowed from a PayloadColumns (host side: no device)."""
    from hipporag_amd.payload import compile_filters
    from tests.payload_helpers import cols_for_restatement, payload_filter_np
    cols = cols_for_restatement(host_columns)

    def fn(filters):
        pf = compile_filters(host_columns, list(filters))
        return payload_filter_np(host_columns.n_passages, cols, pf.arrays(), pf.batch)
    return fn


# ------------------------------------------------------------------------------------------ the boost
def boost_arg(spec: CallSpec, rows: int):
    """The grammar the spec's call takes as boost=: one term list, or one list (or None) per output row."""
    if spec.boost_kind is None:
        return None
    if spec.boost_kind == "one":
        return BOOST_PROGRAMS[spec.boost_ids[0]]
    return [BOOST_PROGRAMS[i] for i in spec.boost_ids[:rows]]


def boost_ctx(spec: CallSpec, host_columns, rows: int):
    """ctx["boost"] of expected_outputs (None without a boost): the program arrays of compile_boosts over a PayloadColumns
    (host code: no device) and the columns as boost_helpers.boost_rows_np takes them."""
    if spec.boost_kind is None:
        return None
    from hipporag_amd.boost import compile_boosts
    from tests.payload_helpers import cols_for_restatement
    prog = compile_boosts(host_columns, boost_arg(spec, rows), rows)
    assert prog.broadcast == (spec.boost_kind == "one") and (prog.broadcast or prog.batch == rows)
    return dict(cols=cols_for_restatement(host_columns), prog=prog.arrays(), broadcast=prog.broadcast, n_terms=prog.n_terms)


def boosted_rows(X, n: int, boost, mn=None, mx=None, naive=False):
    """X fp32 [r, >= n] boosted row by row (row r by query r of the program): boost_helpers.boost_rows_np, or its
    element-by-element loop."""
    from tests.boost_helpers import boost_rows_naive, boost_rows_np
    fn = boost_rows_naive if naive else boost_rows_np
    return fn(np.asarray(X, np.float32)[:, :n], n, boost["cols"], boost["prog"], boost["broadcast"], mn=mn, mx=mx)


def boost_score_rows(X, spec: CallSpec, ctx, naive=False):
    """The rows a boosted call ranks and leaves behind (None: the call has no boost, or a program without any term on
    dense_retrieve, which is the plain call).  X: the fused rows on last_fused, else R.  The ungrouped dense_retrieve -- the
    only dense call that serves a boost -- boosts the min-max of its RAW rows ctx["rank_rows"] (numpy's min / max of each
    row), a query without terms keeping its raw scores; every other entry boosts X as it stands."""
    boost = ctx.get("boost") if spec.boost_kind is not None else None
    if boost is None:
        return None
    n = ctx["n_passages"]
    if spec.entry != "dense_retrieve":
        return boosted_rows(X, n, boost, naive=naive)
    if not boost["n_terms"]:
        return None
    raw = np.asarray(ctx["rank_rows"], np.float32)[:, :n]
    return boosted_rows(raw, n, boost, mn=raw.min(axis=1), mx=raw.max(axis=1), naive=naive)


# ------------------------------------------------------------------------------------------ the restatement
def rank_rows(x, k: int, allowed=None):
    """(idx int32 [B, k], score fp32 [B, k]): every row ranked by the project rule (score descending, ties to the larger
    index, NaN first, the two zeros tie) under allowed bool [B, n]; -1 / 0 beyond the allowed passages; scores as every
    ranking returns them.  fuse_helpers.rank_np without the loop over rows."""
    x = np.asarray(x, np.float32)
    b, n = x.shape
    order = np.argsort(x + np.float32(0), axis=1, kind="stable")[:, ::-1]
    cnt = np.full(b, n)
    if allowed is not None:
        a = np.take_along_axis(np.asarray(allowed, bool), order, axis=1)
        order = np.take_along_axis(order, np.argsort(~a, axis=1, kind="stable"), axis=1)      # the allowed ones first, in order
        cnt = a.sum(axis=1)
    idx = np.full((b, k), -1, np.int32)
    sc = np.zeros((b, k), np.float32)
    kk = min(k, n)
    live = np.arange(kk)[None, :] < cnt[:, None]
    idx[:, :kk] = np.where(live, order[:, :kk], -1)
    sc[:, :kk] = np.where(live, canonical(np.take_along_axis(x, order[:, :kk], axis=1)), np.float32(0))
    return idx, sc


def expected_outputs(R, spec: CallSpec, ctx, rows=None, hit_rows=None):
    """Every output field of the call from the score rows R fp32 [B, n] alone, for the output rows `rows` (ascending; None:
    all), the hit arrays for hit_rows (a subset of rows; None: rows).
    ctx: dict(n_passages, groups int [n] or None, allowed bool [rows of the call, n] or None, gram(ids int [r, c]) -> fp32
    [r, c, c], max_topk; boost: boost_ctx's dict (read when the spec has a boost); rank_rows: the raw rows fp32 [B, n] an
    UNGROUPED dense_retrieve ranks -- hrag_sim_scores, or the
    blended rows -- while its scores are their min-max, R: two raw scores one ulp apart can round to one normalised score,
    so that call's ids are a function of the raw rows, not of R; every other call ranks R itself, the ungrouped dense call
    in the "seeds" scope included: there the rows are normalised over the allowed passages BEFORE the ranking).  -> dict(doc_idx, doc_score, group_idx, hit_idx, hit_score, mmr_value: arrays over `rows` or
    None; fused: F fp32 [Q, n] of a fusion (every question), else None; rows: the boosted rows fp32 [rows of the call, n]
    (every row) the call ranks and leaves on the handle, None without a boost).  The order engine.py documents: fuse; boost
    (boost_score_rows: R on every entry but last_fused, where the fused rows are boosted); rank under the filter (grouped:
    group_rank_np); MMR picks k of the c ranked entries, group_idx following the slots; the hits of the final group_idx
    under the same filter, over the same -- boosted -- rows."""
    n = ctx["n_passages"]
    X = np.asarray(R, np.float32)[:, :n]
    allowed = ctx.get("allowed")
    k, c = spec.k, spec.candidates()
    fused = None
    if spec.entry == "last_fused":
        depth = None
        if spec.fuse == "rrf":
            depth = min(c, ctx["max_topk"], n) if spec.rrf_depth is None else spec.rrf_depth
        fused = fuse_np(X, spec.member_ptr, spec.fuse, spec.weights, spec.rrf_c, depth, allowed)
        X = fused
    XB = boost_score_rows(X, spec, ctx)
    if XB is not None:
        X = XB
    rows = np.arange(X.shape[0]) if rows is None else np.asarray(rows, np.int64)
    a = None if allowed is None else np.asarray(allowed, bool)[rows]
    out = dict(doc_idx=None, doc_score=None, group_idx=None, hit_idx=None, hit_score=None, mmr_value=None, fused=fused,
               rows=XB)
    if spec.group_agg is None:
        raw = ctx.get("rank_rows") if spec.entry == "dense_retrieve" and spec.filter_scope != "seeds" else None
        if XB is not None:          # (the boosted dense call ranks the boosted rows themselves)
            raw = None
        if raw is None:
            idx, sc = rank_rows(X[rows], c, a)
        else:       # the ungrouped dense call ranks the RAW rows and returns the normalised scores of what it ranked
            idx, _ = rank_rows(np.asarray(raw, np.float32)[rows][:, :n], c, a)
            sc = np.where(idx >= 0, canonical(np.take_along_axis(X[rows], np.maximum(idx, 0).astype(np.int64), axis=1)),
                          np.float32(0)).astype(np.float32)
        gi = None
    else:
        g = ctx["groups"]
        per = [group_rank_np(X[r], g, None if a is None else a[i], c, spec.group_agg) for i, r in enumerate(rows)]
        gi, sc, idx = (np.stack([p[j] for p in per]) if per else np.zeros((0, c), t)
                       for j, t in ((0, np.int32), (1, np.float32), (2, np.int32)))
    if spec.mmr_lambda is not None:
        G = ctx["gram"](idx)
        sel, idx, sc, val = mmr_batch_np(sc, idx, G, k, spec.mmr_lambda, normalize=True, n_ids=n)
        out["mmr_value"] = val
        if gi is not None:
            gi = np.where(sel >= 0, np.take_along_axis(gi, np.maximum(sel, 0).astype(np.int64), axis=1), -1).astype(np.int32)
    out["doc_idx"], out["doc_score"], out["group_idx"] = idx, sc, gi
    if spec.group_hits is not None:      # over hit_rows only (rows among `rows`; None: all of them)
        m = spec.group_hits
        at = np.arange(len(rows)) if hit_rows is None else np.searchsorted(rows, np.asarray(hit_rows, np.int64))
        assert np.array_equal(rows[at], rows if hit_rows is None else np.asarray(hit_rows, np.int64))
        hits = [group_hits_np(X[rows[i]], ctx["groups"], None if a is None else a[i], gi[i], m) for i in at]
        out["hit_idx"] = np.stack([h[0] for h in hits]) if hits else np.zeros((0, k, m), np.int32)
        out["hit_score"] = np.stack([h[1] for h in hits]) if hits else np.zeros((0, k, m), np.float32)
    return out


def loop_rows(spec: CallSpec, n_rows: int, fallback_rows, rng):
    """(rows, hit_rows) a call's outputs are checked on.  The rankings -- plain, filtered, grouped -- are checked on every
    row.  The Python-loop restatements check at most LOOP_ROWS rows: row 0, the last row, every DPR-fallback row among the
    first 16, the rest from rng -- the hit arrays always (hit_rows), every field of an MMR call (rows = hit_rows)."""
    pick = [0, n_rows - 1] + [int(r) for r in fallback_rows if r < min(16, n_rows)]
    pick = list(dict.fromkeys(pick))[:LOOP_ROWS]
    rest = [int(r) for r in rng.permutation(n_rows) if r not in pick]
    sel = np.sort(np.asarray(pick + rest[:LOOP_ROWS - len(pick)], np.int64))
    return (np.arange(n_rows) if spec.mmr_lambda is None else sel), sel


# ------------------------------------------------------------------------------------------ the generator
def n_passages_of(v: int, pfrac: float) -> int:
    return max(1, int(round(v * pfrac)))          # synth.make_kg


def random_spec(rng, limits) -> CallSpec:
    """A servable spec.  limits: dict(batch, n_passages, max_topk, fact_sources=True)."""
    b, n, top = limits["batch"], limits["n_passages"], limits["max_topk"]
    s = CallSpec()
    s.entry = str(rng.choice(ENTRIES, p=[0.25, 0.15, 0.15, 0.15, 0.30]))
    s.workspace = bool(rng.random() < 0.25)
    cmax = min(top, MMR_MAX_CANDIDATES)
    kmax = top
    s.k = int(min(kmax, rng.choice([1, int(rng.integers(2, 21)), int(rng.integers(21, 201)), kmax])))
    if rng.random() < 0.75:
        s.filter_kind = str(rng.choice(FILTER_KINDS[1:]))
        s.filter_form = "payload" if s.filter_kind == "payload" and rng.random() < 0.6 else str(rng.choice(FILTER_FORMS[:2]))
        s.filter_per_query = bool(rng.random() < 0.6)
        s.filter_seed = int(rng.integers(1, 1 << 30))
        if s.filter_kind == "payload":
            s.payload_ids = [int(i) for i in rng.integers(0, len(PAYLOAD_FILTERS), b if s.filter_per_query else 1)]
            if not s.filter_per_query:                # one dict for the batch (None is a per-query entry only)
                s.payload_ids[0] = int(rng.choice([0, 1, 2, 3, 4, 6]))
        if rng.random() < 0.45 and limits.get("fact_sources", True):
            s.filter_scope = "seeds"
    if s.filter_scope != "seeds" and rng.random() < 0.5:
        s.lexical_weight = float(rng.choice([0.0, 0.3, 0.5, 1.0], p=[0.1, 0.4, 0.3, 0.2]))
        s.lexical_empty = bool(rng.random() < 0.15)
    if not (s.entry == "dense_retrieve" and s.lexical_weight is not None):
        if rng.random() < 0.5:
            s.group_agg = str(rng.choice(["max", "sum"]))
            if rng.random() < 0.65:
                s.group_hits = int(rng.choice([1, 2, 3, 8, 64] if s.k <= 20 else [1, 2, 3, 8]))
        if rng.random() < 0.42:
            s.k = min(s.k, cmax)
            s.mmr_lambda = float(rng.choice([0.0, 0.3, 0.5, 1.0]))
            cand = [None, s.k, min(2 * s.k, cmax), min(max(s.k, 50), cmax), cmax if rng.random() < 0.2 else None, 1]
            v = cand[int(rng.integers(0, len(cand)))]
            s.mmr_candidates = None if v is None else int(v)
    plain_dense = s.entry == "dense_retrieve" and (s.group_agg, s.mmr_lambda, s.lexical_weight) == (None, None, None) \
        and s.filter_scope != "seeds"           # the dense call serves a boost with nothing but the ranking filter
    if rng.random() < (0.38 if s.entry != "dense_retrieve" else 0.75) and (s.entry != "dense_retrieve" or plain_dense):
        s.boost_kind = str(rng.choice(BOOST_KINDS, p=[0.35, 0.65]))
        s.boost_form = str(rng.choice(BOOST_FORMS))
        s.boost_ids = [int(i) for i in rng.integers(0, len(BOOST_PROGRAMS), b if s.boost_kind == "per_query" else 1)]
        if s.boost_kind == "one" and BOOST_PROGRAMS[s.boost_ids[0]] is None:      # (None is a per-query entry only)
            s.boost_ids[0] = int(rng.integers(0, len(BOOST_PROGRAMS) - 1))
    if s.entry == "last_fused":
        s.fuse = str(rng.choice(["sum", "max", "rrf"]))
        cuts = partitions(rng, b)
        s.member_ptr = [int(v) for v in cuts[str(rng.choice(sorted(cuts)))]]
        if s.fuse != "max" and rng.random() < 0.5:
            w = rng.integers(0, 9, b) / 4.0
            s.weights = [float(v) for v in w]
        if s.fuse == "rrf":
            s.rrf_c = int(rng.choice([0, 1, 60]))
            dmax = min(top, n)
            d = [None, 1, min(dmax, int(rng.integers(1, 41))), dmax if rng.random() < 0.2 else None]
            v = d[int(rng.integers(0, len(d)))]
            s.rrf_depth = None if v is None else int(v)
    assert servable(s, limits) is None, s
    return s


def case_limits(case) -> dict:
    n = n_passages_of(case["v"], case["pfrac"])
    top = n if case["max_topk"] == "n" else min(int(case["max_topk"]), n)
    return dict(batch=case["b"], n_passages=n, max_topk=top, fact_sources=True)


def case_specs(case, calls: int):
    """The specs of one case: a function of the case's own seed."""
    rng = np.random.default_rng(case["seed"] ^ 0x0B7104)
    lim = case_limits(case)
    return [random_spec(rng, lim) for _ in range(calls)]


def iter_plan(seed: int, calls_per_case: int, batches=BATCHES):
    """The seeded stream of (case parameters, specs): no GPU is touched.  The batch sizes rotate through `batches`; the
    index size, the engine's max_topk and the group table's kind are drawn."""
    rng = np.random.default_rng(seed)
    i = 0
    while True:
        v = int(rng.choice([600, 1500, 4000, 9000]))
        case = dict(v=v, e=int(v * rng.choice([3, 6, 10])), dim=int(rng.choice([32, 64])),
                    pfrac=float(rng.choice([0.125, 0.3])), b=int(batches[i % len(batches)]),
                    max_topk=[10, 200, "n"][int(rng.integers(0, 3))], groups=str(rng.choice(GROUP_KINDS)),
                    seed=int(rng.integers(1, 1 << 30)))
        yield case, case_specs(case, calls_per_case)
        i += 1


def plan(seed: int, n_cases: int, calls_per_case: int, batches=BATCHES):
    """The first n_cases of iter_plan as a list."""
    import itertools
    return list(itertools.islice(iter_plan(seed, calls_per_case, batches), n_cases))
