"""tests/option_helpers.py without a GPU: the composed restatement (the reference of tools/soak_options.py and of
tests/test_gpu_option_matrix.py) against a deliberately naive per-row Python loop, the refusal table against itself, and
the coverage of the seeded plan the GPU slices of tests/test_gpu_soak_slices.py run."""

import functools
import itertools

import numpy as np
import pytest

from tests.fuse_helpers import partitions, rank_np
from tests.group_helpers import random_groups, same_bits
from tests.group_hits_helpers import group_hits_loop
from tests.mmr_helpers import gram_np, mmr_np
from tests.option_helpers import (BATCHES, BOOST_FORMS, BOOST_KINDS, BOOST_PROGRAMS, ENTRIES, FILTER_FORMS, FILTER_KINDS,
                                  GROUP_KINDS, OPTIONS, PAYLOAD_FILTERS, PLAN_CALLS, PLAN_CASES, PLAN_SEED, CallSpec, boost_arg,
                                  boost_ctx, boost_score_rows, case_limits, expected_outputs, loop_rows, make_allowed,
                                  n_passages_of, payload_allowed_fn, plan, random_spec, rank_rows, servable)


# ------------------------------------------------------------------------------------------ the naive loop
def _before(s, a, b):
    """is position a ranked before position b?  (score descending, NaN above everything, ties to the larger position)"""
    na, nb = s[a] != s[a], s[b] != s[b]
    if na or nb:
        return (na and not nb) or (na and nb and a > b)
    return s[a] > s[b] or (s[a] == s[b] and a > b)             # -0.0 == 0.0


def _sorted(s, positions):
    return sorted(positions, key=functools.cmp_to_key(lambda a, b: -1 if _before(s, a, b) else 1))


def _canon(v):
    return np.float32(np.nan) if v != v else np.float32(v) + np.float32(0)


def _naive_fuse(R, spec, allowed, depth):
    mp, n = spec.member_ptr, R.shape[1]
    F = np.zeros((len(mp) - 1, n), np.float32)
    for q in range(len(mp) - 1):
        members = range(mp[q], mp[q + 1])
        w = [1.0 if spec.weights is None else float(np.float32(spec.weights[i])) for i in range(len(R))]
        if spec.fuse == "sum":
            for p in range(n):
                acc = 0.0
                for i in members:
                    acc = acc + w[i] * float(R[i, p])                   # Python floats are doubles
                F[q, p] = np.float32(acc)
        elif spec.fuse == "max":
            for p in range(n):
                col = [float(R[i, p]) for i in members]
                best = col[0]
                for v in col[1:]:
                    if v != v or (best == best and v > best):
                        best = v
                F[q, p] = _canon(best)
        else:
            for i in members:
                s = [float(v) for v in R[i]]
                order = [p for p in _sorted(s, range(n)) if allowed is None or allowed[q][p]][:depth]
                for rank, p in enumerate(order, start=1):
                    F[q, p] = F[q, p] + np.float32(w[i] / (float(spec.rrf_c) + rank))
    return F


def naive_outputs(R, spec, ctx):
    """expected_outputs by plain loops: the boost element by element with Python floats (boost_helpers.boost_rows_naive),
    sort by the ranking rule, walk, keep the allowed, take the first passage per group, greedy MMR element by element
    (mmr_helpers.mmr_np), hits by repeated selection (group_hits_loop)."""
    n = ctx["n_passages"]
    X = np.asarray(R, np.float32)[:, :n]
    allowed, g = ctx.get("allowed"), ctx.get("groups")
    k, c = spec.k, spec.candidates()
    fused = None
    if spec.entry == "last_fused":
        depth = (min(c, ctx["max_topk"], n) if spec.rrf_depth is None else spec.rrf_depth) if spec.fuse == "rrf" else None
        fused = X = _naive_fuse(X, spec, allowed, depth)
    XB = boost_score_rows(X, spec, ctx, naive=True)      # (which rows are boosted is the rule; the loop is the boost's)
    if XB is not None:
        X = XB
    rows = X.shape[0]
    out = dict(doc_idx=np.full((rows, k), -1, np.int32), doc_score=np.zeros((rows, k), np.float32), group_idx=None,
               hit_idx=None, hit_score=None, mmr_value=None, fused=fused, rows=XB)
    if spec.group_agg is not None:
        out["group_idx"] = np.full((rows, k), -1, np.int32)
    if spec.mmr_lambda is not None:
        out["mmr_value"] = np.zeros((rows, k), np.float32)
    if spec.group_hits is not None:
        out["hit_idx"] = np.full((rows, k, spec.group_hits), -1, np.int32)
        out["hit_score"] = np.zeros((rows, k, spec.group_hits), np.float32)
    for r in range(rows):
        s = [float(v) for v in X[r]]
        ok = [p for p in range(n) if allowed is None or allowed[r][p]]
        if spec.group_agg is None:
            raw = ctx.get("rank_rows") if spec.entry == "dense_retrieve" and spec.filter_scope != "seeds" else None
            if XB is not None:
                raw = None                                              # (a boosted dense call ranks its boosted rows)
            ids = _sorted(s if raw is None else [float(v) for v in raw[r]], ok)[:c]       # (the dense call ranks the raw row)
            sc = [s[p] for p in ids]
            gids = None
        else:
            best, total = {}, {}
            for p in _sorted(s, ok):
                best.setdefault(int(g[p]), p)                           # the first passage of each group
            for p in ok:                                                # SUM: doubles, in passage order, rounded once
                total[int(g[p])] = total.get(int(g[p]), 0.0) + s[p]
            gscore = {gid: (s[p] if spec.group_agg == "max" else float(np.float32(total[gid]))) for gid, p in best.items()}
            keys = sorted(gscore)
            gs = [gscore[gid] for gid in keys]
            order = _sorted(gs, range(len(keys)))[:c]                    # ties between groups: the larger group id first
            gids = [keys[j] for j in order]
            ids = [best[gid] for gid in gids]
            sc = [gs[j] for j in order]
        pad = c - len(ids)
        ids_c = np.asarray(ids + [-1] * pad, np.int32)
        sc_c = np.asarray([_canon(v) for v in sc] + [np.float32(0)] * pad, np.float32)
        gid_c = None if gids is None else np.asarray(gids + [-1] * pad, np.int32)
        if spec.mmr_lambda is not None:
            G = ctx["gram"](ids_c[None])[0]
            sel, ids_c, sc_c, val = mmr_np(sc_c, ids_c, G, k, spec.mmr_lambda, normalize=True, n_ids=n)
            out["mmr_value"][r] = val
            if gid_c is not None:
                gid_c = np.asarray([gid_c[j] if j >= 0 else -1 for j in sel], np.int32)
        out["doc_idx"][r], out["doc_score"][r] = ids_c[:k], sc_c[:k]
        if gid_c is not None:
            out["group_idx"][r] = gid_c[:k]
        if spec.group_hits is not None:
            out["hit_idx"][r], out["hit_score"][r] = group_hits_loop(X[r], g, None if allowed is None else allowed[r],
                                                                     out["group_idx"][r], spec.group_hits)
    return out


# ------------------------------------------------------------------------------------------ inputs
def _rows(rng, b, n, kind):
    """score rows with heavy ties, both zeros, and rows that are all equal"""
    if kind == "ties":
        x = rng.integers(-3, 4, (b, n)).astype(np.float32) / 4
    elif kind == "zeros":
        x = np.where(rng.random((b, n)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        x[rng.random((b, n)) < 0.2] = 0.5
    elif kind == "equal":
        x = np.full((b, n), 0.25, np.float32)
        x[0] = rng.random(n).astype(np.float32)
    else:
        x = rng.random((b, n)).astype(np.float32)
        x[rng.random((b, n)) < 0.3] = 0.5                                # a tie class in every row
        x[rng.random((b, n)) < 0.05] = -0.0
    return x


def _ctx(rng, n, group_kind, allowed):
    emb = rng.integers(-2, 3, (n, 8)).astype(np.float64) / 2             # coarse rows: duplicates and tied similarities
    emb[rng.integers(0, n, n // 4)] = emb[0]
    return dict(n_passages=n, groups=random_groups(rng, n, group_kind), allowed=allowed, max_topk=n,
                gram=lambda ids: np.stack([gram_np(emb, r) for r in np.asarray(ids)]).astype(np.float32))


def _same(got, want, what):
    for name, w in want.items():
        gv = got[name]
        assert (gv is None) == (w is None), (what, name)
        if w is None:
            continue
        if w.dtype == np.float32:
            assert same_bits(gv, w), (what, name, gv, w)
        else:
            np.testing.assert_array_equal(gv, w, err_msg=f"{what} {name}")


FILTERS = list(FILTER_KINDS) + ["no group allowed"]


@pytest.mark.parametrize("seed", range(8))
def test_the_composition_matches_the_naive_loop(seed):
    """Random composed calls on rows of 50 .. 400 passages: every row kind, filter kind ("fewer than k" and "no group has
    an allowed member" included), group table kind, k in {1, middle, n}, c in {k, 2k, n}, lambda in {0, 0.3, 1} and fusion
    mode x partition comes up over the eight seeds (asserted by test_the_naive_grid_covers_what_it_claims)."""
    for params in _grid(seed):
        R, spec, ctx = _build(params)
        _same(expected_outputs(R, spec, ctx), naive_outputs(R, spec, ctx), params)


def _grid(seed):
    rng = np.random.default_rng(7000 + seed)
    out = []
    for t in range(14):
        n = int(rng.integers(50, 401))
        b = int(rng.integers(3, 7))
        fuse = [None, "sum", "max", "rrf"][(seed + t) % 4]
        cuts = partitions(np.random.default_rng(1000 * seed + t), b)
        names = sorted(cuts)
        mmr = (t + seed) % 2 == 1
        if mmr and ((t // 2) % 3 == 2 or t % 3 == 2):                      # c = n or k = n under MMR: the element-by-element
            n = int(rng.integers(50, 121))                                 # loop is O(k c) per row, so the shorter rows
        kk = [1, int(rng.integers(2, n)), n][t % 3]
        if mmr and t % 3 == 1:
            kk = min(kk, 30)
        out.append(dict(seed=1000 * seed + t, n=n, b=b, rows=["ties", "zeros", "equal", "plain"][(t + seed // 2) % 4],
                        filter=FILTERS[(3 * seed + t) % len(FILTERS)], per_query=bool((t + seed) % 3),
                        groups=GROUP_KINDS[(seed + 2 * t) % len(GROUP_KINDS)], k=kk,
                        agg=[None, "max", "sum"][(t + seed) % 3], hits=[None, 1, 3][(t // 3 + seed) % 3],
                        lam=[0.0, 0.3, 1.0][(t // 2 + seed) % 3] if mmr else None, c=["k", "2k", "n"][(t // 2) % 3],
                        fuse=fuse, cut=names[(t // 4 + seed) % len(names)], weights=bool(t % 2),
                        boost=[None, "one", "per_query"][(t // 2 + 2 * seed) % 3], boost_at=(5 * seed + 3 * t) % len(BOOST_PROGRAMS)))
    return out


def _metadata_columns(seed, n):
    from hipporag_amd.payload import encode_columns
    from tests.payload_helpers import columns_of, random_metadata
    meta = random_metadata(np.random.default_rng(seed + 2), n)
    return encode_columns(columns_of(meta, ["year", "user", "score", "flag", "mixed"]), n), meta


def test_a_payload_filter_kind_maps_its_rows_to_the_queries():
    """make_allowed(kind "payload"): row r is the restatement of PAYLOAD_FILTERS[payload_ids[r]] over the metadata -- held
    here to a plain predicate per dict -- and a one-row filter is payload_ids[0] repeated."""
    n, rows = 90, 7
    host, meta = _metadata_columns(3, n)
    preds = [lambda m: m.get("year", 0) >= 2020,
             lambda m: m.get("user") in ("alice", "bob") and m.get("year") != 2021,
             lambda m: "year" in m and (("score" in m and m["score"] < 1.0) or m.get("user") == "carol"),
             lambda m: m.get("user") == "dave" and m.get("year") == 2018 and m.get("score") == 3.5 and m.get("flag") is True,
             lambda m: False, lambda m: True,
             lambda m: "score" in m and 0.5 < m["score"] <= 2.5 and "flag" in m]
    spec = CallSpec(filter_kind="payload", filter_per_query=True, payload_ids=[3, 0, 5, 6, 1, 2, 4])
    got = make_allowed(spec, n, rows, payload_allowed_fn(host))
    for r, i in enumerate(spec.payload_ids):
        np.testing.assert_array_equal(got[r], [bool(preds[i](m)) for m in meta], err_msg=str(PAYLOAD_FILTERS[i]))
    assert got[2].all() and not got[6].any() and 0 < got[1].sum() < n
    spec.filter_per_query = False
    one = make_allowed(spec, n, rows, payload_allowed_fn(host))
    assert one.shape == (rows, n) and (one == got[0]).all()


def _build(p):
    rng = np.random.default_rng(p["seed"])
    n, b = p["n"], p["b"]
    R = _rows(rng, b, n, p["rows"])
    spec = CallSpec(entry="last_fused" if p["fuse"] else "retrieve", k=p["k"], group_agg=p["agg"],
                    group_hits=p["hits"] if p["agg"] else None, filter_seed=p["seed"], filter_per_query=p["per_query"])
    if p["fuse"]:
        spec.fuse = p["fuse"]
        spec.member_ptr = [int(v) for v in partitions(np.random.default_rng(p["seed"]), b)[p["cut"]]]
        if p["weights"] and p["fuse"] != "max":
            spec.weights = [float(v) for v in rng.integers(0, 9, b) / 4.0]
        if p["fuse"] == "rrf":
            spec.rrf_c, spec.rrf_depth = int(rng.choice([0, 60])), [None, 1, int(rng.integers(1, n + 1))][p["seed"] % 3]
    if p["lam"] is not None:
        spec.mmr_lambda = p["lam"]
        spec.mmr_candidates = {"k": spec.k, "2k": min(2 * spec.k, n), "n": n}[p["c"]]
    rows = spec.rows(b)
    if p["boost"]:          # the programs rotate from boost_at on: every one comes up as the batch's and as a query's
        spec.boost_kind = p["boost"]
        spec.boost_ids = [(p["boost_at"] + 3 * r) % len(BOOST_PROGRAMS) for r in range(rows)]
        if p["boost"] == "one" and BOOST_PROGRAMS[spec.boost_ids[0]] is None:
            spec.boost_ids[0] = 2
    groups = random_groups(np.random.default_rng(p["seed"] + 1), n, p["groups"])
    if p["filter"] == "no group allowed":
        allowed = np.zeros((rows, n), bool)                              # row 0: nothing; the others: one whole group
        for r in range(1, rows):
            allowed[r] = groups == groups[r]
    else:
        spec.filter_kind = p["filter"]
        fn = None
        if p["filter"] == "payload":                                     # rows of PAYLOAD_FILTERS over random metadata
            spec.payload_ids = [int(i) for i in rng.integers(0, len(PAYLOAD_FILTERS), rows)]
            if not p["per_query"] and spec.payload_ids[0] == 5:
                spec.payload_ids[0] = 0
            fn = payload_allowed_fn(_metadata_columns(p["seed"], n)[0])
        allowed = make_allowed(spec, n, rows, fn)
    ctx = _ctx(rng, n, p["groups"], allowed)
    ctx["groups"] = groups
    ctx["boost"] = boost_ctx(spec, _metadata_columns(p["seed"], n)[0], rows)
    return R, spec, ctx


def test_the_ungrouped_dense_call_ranks_the_raw_rows_not_their_min_max():
    """Found by tools/soak_options.py: dense_retrieve without group_agg ranks the raw similarity rows and returns the
    min-max of what it ranked.  Raw scores a few ulps apart round to ONE normalised score, whose tie the raw ranking breaks
    by value and a ranking of the normalised row R by position: the ids are a function of the raw rows (ctx["rank_rows"]).
    In the "seeds" scope the same call normalises over the allowed passages first and ranks THOSE rows (csrc/engine.hip,
    dense_impl): there, as behind a grouped call, the ids are a function of R."""
    from tests.lex_helpers import minmax_np, row_minmax_np
    rng = np.random.default_rng(5)
    n, b = 120, 4
    raw = rng.random((b, n)).astype(np.float32)
    raw[:, 0], raw[:, 1] = -100.0, 1.0
    near = np.float32(0.99)
    for j in range(2, 40):                               # 38 distinct values within a few ulps of 0.99: x - mn rounds them together
        raw[:, j] = near
        near = np.nextafter(near, np.float32(1))
    raw = raw[:, rng.permutation(n)]
    R = np.stack([minmax_np(r, *[v[0] for v in row_minmax_np(r[None])]) for r in raw])
    assert all(len(np.unique(R[r])) < len(np.unique(raw[r])) - 20 for r in range(b))
    for allowed in (None, rng.random((b, n)) < 0.6):
        for kw in (dict(k=n), dict(k=30, mmr_lambda=0.3, mmr_candidates=60)):
            spec = CallSpec(entry="dense_retrieve", **kw)
            ctx = _ctx(rng, n, "two", allowed)
            ctx["rank_rows"] = raw
            want = naive_outputs(R, spec, ctx)
            _same(expected_outputs(R, spec, ctx), want, kw)
            ctx.pop("rank_rows")
            assert not np.array_equal(expected_outputs(R, spec, ctx)["doc_idx"], want["doc_idx"])       # R alone: other ids
            # a grouped dense call, like every other entry, ranks R itself: the raw rows change nothing there
            spec_g = CallSpec(entry="dense_retrieve", group_agg="max", **kw)
            got = expected_outputs(R, spec_g, dict(ctx, rank_rows=raw))
            _same(got, naive_outputs(R, spec_g, dict(ctx, rank_rows=raw)), ("grouped", kw))
            _same(got, expected_outputs(R, spec_g, ctx), ("grouped, no raw rows", kw))
            # ... and so does the ungrouped call in the "seeds" scope: its rows are normalised over the allowed passages first
            if allowed is not None:
                spec_s = CallSpec(entry="dense_retrieve", filter_kind="half", filter_scope="seeds", **kw)
                got = expected_outputs(R, spec_s, dict(ctx, rank_rows=raw))
                _same(got, naive_outputs(R, spec_s, dict(ctx, rank_rows=raw)), ("seeds", kw))
                _same(got, expected_outputs(R, spec_s, ctx), ("seeds, no raw rows", kw))


def test_the_naive_grid_covers_what_it_claims():
    ps = [p for seed in range(8) for p in _grid(seed)]
    for key, values in (("rows", ["ties", "zeros", "equal", "plain"]), ("filter", FILTERS), ("groups", list(GROUP_KINDS)),
                        ("agg", [None, "max", "sum"]), ("lam", [None, 0.0, 0.3, 1.0]), ("fuse", [None, "sum", "max", "rrf"]),
                        ("c", ["k", "2k", "n"]), ("cut", ["singletons", "one", "random", "one_then_big"])):
        assert {p[key] for p in ps} >= set(values), key
    assert any(p["k"] == 1 for p in ps) and any(p["k"] == p["n"] for p in ps) and any(1 < p["k"] < p["n"] for p in ps)
    built = [_build(p)[1] for p in ps]
    mmr = [(s, p["n"]) for s, p in zip(built, ps) if s.mmr_lambda is not None]
    assert any(s.candidates() == n and s.k < n for s, n in mmr) and any(s.k == s.candidates() == n for s, n in mmr)
    assert any(s.k == 1 for s, n in mmr) and any(s.candidates() == 2 * s.k for s, n in mmr)
    assert any(s.k == n and s.mmr_lambda is None for s, n in zip(built, (p["n"] for p in ps)) if n > 120)
    assert any(p["agg"] and p["hits"] and p["lam"] is not None and p["filter"] != "none" for p in ps)
    assert any(p["fuse"] and p["agg"] and p["lam"] is not None for p in ps)
    for fuse in ("sum", "max", "rrf"):
        assert {p["cut"] for p in ps if p["fuse"] == fuse} >= {"singletons", "one", "random", "one_then_big"}, fuse
    # the boost: both kinds; with the groups, the hits, MMR and a filter at once; behind every fusion mode; every program as
    # the batch's and as one query's; NaN entries and rows of exact zeros in the boosted rows of grouped SUM and of MMR calls
    assert {p["boost"] for p in ps} == {None, "one", "per_query"}
    assert any(p["boost"] and p["agg"] and p["hits"] and p["lam"] is not None and p["filter"] != "none" for p in ps)
    assert {p["fuse"] for p in ps if p["boost"]} == {None, "sum", "max", "rrf"}
    one = {s.boost_ids[0] for s in built if s.boost_kind == "one"}
    per = {i for s, p in zip(built, ps) if s.boost_kind == "per_query" for i in s.boost_ids}
    assert one == set(range(len(BOOST_PROGRAMS) - 1)) and per == set(range(len(BOOST_PROGRAMS)))
    nan_in, zeros_in = set(), set()
    for p, s in zip(ps, built):
        if s.boost_kind is not None:
            R, _, ctx = _build(p)
            XB = expected_outputs(R, s, ctx)["rows"]
            what = (s.group_agg, s.mmr_lambda is not None)
            if np.isnan(XB).any():
                nan_in.add(what)
            if ((XB == 0).sum(axis=1) > XB.shape[1] // 3).any() and (XB != 0).any():
                zeros_in.add(what)
    for got in (nan_in, zeros_in):
        assert {a for a, _ in got} >= {None, "max", "sum"} and {m for _, m in got} == {False, True}, got


def test_the_boosted_dense_call_boosts_the_min_max_of_the_raw_rows():
    """dense_retrieve(boost=) is its own rule (engine.py): numpy's min-max of the raw rows, the boost over the normalised
    entries, the plain ranking of the result under the filter -- no normalisation behind the boost.  In a per-query
    program a query without terms keeps its RAW scores, and a program without any term is the plain call: the raw rows
    ranked, their min-max returned.  Both forms against the naive loop, and against each other where they must differ."""
    from tests.lex_helpers import minmax_np, row_minmax_np
    rng = np.random.default_rng(9)
    n, b = 150, 6
    raw = (rng.random((b, n)).astype(np.float32) - np.float32(0.3)) * np.float32(0.7)
    raw[:, rng.integers(0, n, 20)] = np.float32(0.25)                      # a tie class in every row
    R = np.stack([minmax_np(r, *[v[0] for v in row_minmax_np(r[None])]) for r in raw])
    host = _metadata_columns(9, n)[0]
    for allowed in (None, rng.random((b, n)) < 0.5, np.zeros((b, n), bool)):
        for kind, ids in (("one", [1]), ("one", [8]), ("per_query", [0, 9, 2, 8, 7, 6]), ("per_query", [8, 9, 9, 8, 8, 9])):
            spec = CallSpec(entry="dense_retrieve", k=40, boost_kind=kind, boost_ids=ids)
            ctx = dict(_ctx(rng, n, "two", allowed), rank_rows=raw, boost=boost_ctx(spec, host, b))
            got, want = expected_outputs(R, spec, ctx), naive_outputs(R, spec, ctx)
            _same(got, want, (kind, ids))
            plain = expected_outputs(R, CallSpec(entry="dense_retrieve", k=40), ctx)
            if all(not BOOST_PROGRAMS[i] for i in ids):                    # no term at all: the plain call
                assert got["rows"] is None
                _same(got, plain, ("no terms", ids))
                continue
            XB = got["rows"]
            for q in range(b):
                terms = BOOST_PROGRAMS[ids[q if kind == "per_query" else 0]]
                if not terms:                                              # its raw scores, bit for bit: not their min-max
                    assert same_bits(XB[q], raw[q]) and not same_bits(XB[q], R[q])
                    np.testing.assert_array_equal(got["doc_idx"][q], plain["doc_idx"][q])
                else:
                    assert not same_bits(XB[q], raw[q])
            wi, ws = rank_np(XB, 40, allowed)                              # ... and the ranking is the plain one of XB
            np.testing.assert_array_equal(got["doc_idx"], wi)
            assert same_bits(got["doc_score"], ws)


def test_rank_rows_is_the_loop_of_fuse_helpers():
    rng = np.random.default_rng(3)
    for kind in ("ties", "zeros", "equal", "plain"):
        x = _rows(rng, 5, 97, kind)
        x[1, 7] = np.nan
        for allowed in (None, rng.random((5, 97)) < 0.5, np.zeros((5, 97), bool)):
            for k in (1, 40, 97, 120):
                gi, gs = rank_rows(x, k, allowed)
                wi, ws = rank_np(x, k, allowed)
                np.testing.assert_array_equal(gi, wi)
                assert same_bits(gs, ws)


def test_the_checked_rows_hold_the_ends_and_the_fallbacks():
    """Every ranking -- grouped ones included -- is checked on every row; only the hit arrays, and every field of an MMR
    call, on at most 8: the two ends, the fallback rows among the first 16, the rest drawn."""
    rng = np.random.default_rng(1)
    for spec in (CallSpec(), CallSpec(group_agg="max"), CallSpec(group_agg="sum", group_hits=2)):
        rows, hit_rows = loop_rows(spec, 130, [3, 11, 40], rng)
        np.testing.assert_array_equal(rows, np.arange(130))
        assert len(hit_rows) == 8 and {0, 129, 3, 11} <= set(hit_rows.tolist())
    for spec in (CallSpec(mmr_lambda=0.5), CallSpec(group_agg="max", group_hits=2, mmr_lambda=0.5)):
        rows, hit_rows = loop_rows(spec, 130, [3, 11, 40], rng)
        np.testing.assert_array_equal(rows, hit_rows)
        assert len(rows) == 8 and {0, 129, 3, 11} <= set(rows.tolist()) and (np.diff(rows) > 0).all()
    for n in (1, 5):
        rows, hit_rows = loop_rows(CallSpec(group_agg="max", mmr_lambda=0.5), n, [0], rng)
        np.testing.assert_array_equal(rows, np.arange(n))
        np.testing.assert_array_equal(hit_rows, np.arange(n))
    # the hit arrays of a subset of rows are those rows of the full computation
    R = _rows(rng, 12, 60, "ties")
    spec = CallSpec(group_agg="max", group_hits=3, k=7, filter_kind="half", filter_per_query=True, filter_seed=4)
    ctx = _ctx(rng, 60, "shuffled", make_allowed(spec, 60, 12))
    full, part = expected_outputs(R, spec, ctx), expected_outputs(R, spec, ctx, hit_rows=[2, 5, 11])
    np.testing.assert_array_equal(part["hit_idx"], full["hit_idx"][[2, 5, 11]])
    assert same_bits(part["hit_score"], full["hit_score"][[2, 5, 11]])
    np.testing.assert_array_equal(part["group_idx"], full["group_idx"])


# ------------------------------------------------------------------------------------------ the refusal table
def test_the_refusal_table():
    lim = dict(max_topk=50, fact_sources=True)
    f = dict(filter_kind="half")
    for kw, want in ((dict(), None), (dict(filter_scope="seeds"), (ValueError, "filter_scope")),
                     (dict(filter_scope="seeds", **f), None),
                     (dict(filter_scope="seeds", lexical_weight=0.3, **f), (NotImplementedError, "filter_scope")),
                     (dict(group_hits=2), (ValueError, "group_hits")), (dict(group_hits=2, group_agg="sum"), None),
                     (dict(mmr_candidates=20), (ValueError, "mmr_candidates")), (dict(mmr_lambda=0.5, mmr_candidates=50), None),
                     (dict(mmr_lambda=0.5, mmr_candidates=51), (ValueError, "mmr_candidates")),
                     (dict(mmr_lambda=0.5, k=51), (ValueError, "mmr_candidates")),
                     (dict(entry="dense_retrieve", lexical_weight=0.3, group_agg="max", group_hits=2), (ValueError, "group_agg")),
                     (dict(entry="dense_retrieve", lexical_weight=0.3, group_hits=2), (ValueError, "group_hits")),
                     (dict(entry="dense_retrieve", lexical_weight=0.3, mmr_lambda=0.5), (ValueError, "mmr_lambda")),
                     (dict(entry="dense_retrieve", lexical_weight=0.3, mmr_candidates=5), (ValueError, "mmr_candidates")),
                     (dict(entry="dense_retrieve", lexical_weight=0.3, filter_scope="seeds", **f), (ValueError, "filter_scope")),
                     (dict(entry="dense_retrieve", lexical_weight=0.3, **f), None)):
        assert servable(CallSpec(**kw), lim) == want, kw
    # the boost: dense_retrieve serves it with the ranking filter alone and names what it refuses -- in its own order, and
    # before the lexical refusals; every other entry refuses exactly what it refuses without the boost
    bst, d = dict(boost_kind="one", boost_ids=[0]), dict(entry="dense_retrieve")
    for kw, want in ((dict(), None), (f, None), (dict(group_agg="max"), (ValueError, "group_agg")),
                     (dict(group_agg="max", group_hits=2, mmr_lambda=0.5, lexical_weight=0.3), (ValueError, "group_agg")),
                     (dict(group_hits=2, mmr_lambda=0.5), (ValueError, "group_hits")),
                     (dict(mmr_lambda=0.5, mmr_candidates=5, lexical_weight=0.3), (ValueError, "mmr_lambda")),
                     (dict(mmr_lambda=0.5, k=51), (ValueError, "mmr_lambda")),
                     (dict(mmr_candidates=5, lexical_weight=0.3), (ValueError, "mmr_candidates")),
                     (dict(lexical_weight=0.3, **f), (ValueError, "lexical")),
                     (dict(lexical_weight=0.3, filter_scope="seeds", **f), (ValueError, "lexical")),
                     (dict(filter_scope="seeds", **f), (ValueError, "filter_scope")),
                     (dict(filter_scope="seeds"), (ValueError, "filter_scope"))):
        assert servable(CallSpec(**d, **bst, **kw), lim) == want, kw
        assert servable(CallSpec(**d, boost_kind="per_query", boost_ids=[9, 8], boost_form="program", **kw), lim) == want, kw
    for entry in ENTRIES:
        if entry != "dense_retrieve":
            for kw in (dict(), f, dict(filter_scope="seeds"), dict(filter_scope="seeds", **f), dict(group_hits=2),
                       dict(filter_scope="seeds", lexical_weight=0.3, **f), dict(mmr_candidates=20), dict(mmr_lambda=0.5, k=51),
                       dict(group_agg="sum", group_hits=2, mmr_lambda=0.5, mmr_candidates=50, lexical_weight=0.3, **f)):
                assert servable(CallSpec(entry=entry, **bst, **kw), lim) == servable(CallSpec(entry=entry, **kw), lim), (entry, kw)
    assert servable(CallSpec(mmr_lambda=0.5, mmr_candidates=1025), None) == (ValueError, "mmr_candidates")
    assert servable(CallSpec(filter_scope="seeds", **f), dict(fact_sources=False)) == (RuntimeError, "fact_sources")


def test_a_spec_without_the_boost_fields_still_loads():
    """A replay JSON written before the boost fields existed is a call without a boost."""
    import json
    d = json.loads(CallSpec(entry="last_fused", fuse="rrf", member_ptr=[0, 2, 3], group_agg="max").to_json())
    for name in ("boost_kind", "boost_ids", "boost_form"):
        d.pop(name)
    s = CallSpec.from_dict(d)
    assert s.boost_kind is None and "boost" not in s.options() and boost_arg(s, 2) is None and boost_ctx(s, None, 2) is None
    assert "boost" in CallSpec(boost_kind="one", boost_ids=[0]).options()


def test_the_boost_programs_hold_what_they_claim():
    """BOOST_PROGRAMS compiles over random_metadata's columns, and over them: a constant MUL and ADD under $any / $not / an
    IN-list, FIELD with and without sqrt, `missing` on a column with holes, the three decays, NaN entries, a row of exact
    zeros, and an ADD that puts a handful of passages above everything else."""
    from hipporag_amd._lib import (BOOST_ADD, BOOST_CONST, BOOST_DECAY, BOOST_EXP, BOOST_FIELD, BOOST_GAUSS, BOOST_HAS_MISSING,
                                   BOOST_LINEAR, BOOST_MUL, BOOST_NONE, BOOST_SQRT)
    from hipporag_amd.boost import compile_boosts
    from tests.payload_helpers import cols_for_restatement
    n = 400
    host = _metadata_columns(21, n)[0]
    prog = compile_boosts(host, BOOST_PROGRAMS)
    assert not prog.broadcast and prog.batch == len(BOOST_PROGRAMS)
    assert compile_boosts(host, []).broadcast and compile_boosts(host, []).n_terms == 0
    ops = [(int(o) & 0xFF, (int(o) >> 8) & 0xFF, (int(o) >> 16) & 0xFF, bool(int(o) & BOOST_HAS_MISSING)) for o in prog.t_op]
    assert {(k_, m) for k_, m, _, _ in ops} >= {(BOOST_CONST, BOOST_MUL), (BOOST_CONST, BOOST_ADD)}
    assert {sub for k_, _, sub, _ in ops if k_ == BOOST_FIELD} == {BOOST_NONE, BOOST_SQRT}
    assert {sub for k_, _, sub, _ in ops if k_ == BOOST_DECAY} == {BOOST_LINEAR, BOOST_EXP, BOOST_GAUSS}
    cols = cols_for_restatement(host)
    assert any(has and cols[int(c)][2] is not None and not cols[int(c)][2].all() for (_, _, _, has), c in zip(ops, prog.t_col))
    text = repr(BOOST_PROGRAMS)
    assert "$any" in text and "$not" in text and "['bob', 'carol']" in text and "'mul': 0.0" in text
    assert BOOST_PROGRAMS[-2:] == [[], None]
    rng = np.random.default_rng(2)
    R = rng.random((len(BOOST_PROGRAMS), n)).astype(np.float32)
    spec = CallSpec(k=10, boost_kind="per_query", boost_ids=list(range(len(BOOST_PROGRAMS))))
    ctx = dict(n_passages=n, allowed=None, boost=boost_ctx(spec, host, len(BOOST_PROGRAMS)))
    out = expected_outputs(R, spec, ctx)
    XB, first = out["rows"], rank_rows(R, 10)[0]
    assert 0 < np.isnan(XB[2]).sum() < n and np.isnan(out["doc_score"][2]).all()       # NaN ranks first
    assert not np.isnan(np.delete(XB, 2, axis=0)).any()
    assert (XB[6] == 0).sum() > n // 3 and (XB[6] != 0).any()
    top = np.flatnonzero(XB[7] > 5)
    assert 2 <= len(top) <= 10 and set(out["doc_idx"][7][:len(top)]) == set(top) and not set(top) <= set(first[7])
    assert same_bits(XB[8:], R[8:]) and np.array_equal(out["doc_idx"][8:], first[8:])   # no terms: the row, the plain ranking
    for q in range(8):
        assert not same_bits(XB[q], R[q]), q


def test_random_spec_draws_only_servable_specs():
    rng = np.random.default_rng(11)
    for b, n, top in itertools.product((1, 9, 257), (75, 2700), (10, 200, 2700)):
        lim = dict(batch=b, n_passages=n, max_topk=min(top, n), fact_sources=True)
        for _ in range(60):
            s = random_spec(rng, lim)
            assert servable(s, lim) is None and 1 <= s.k <= lim["max_topk"]
            assert CallSpec.from_dict(__import__("json").loads(s.to_json())) == s          # JSON round trip
            if s.boost_kind is not None:
                assert s.boost_kind in BOOST_KINDS and s.boost_form in BOOST_FORMS
                assert len(s.boost_ids) == (b if s.boost_kind == "per_query" else 1)
                assert s.boost_kind == "per_query" or BOOST_PROGRAMS[s.boost_ids[0]] is not None
                arg = boost_arg(s, s.rows(b))
                assert len(arg) == s.rows(b) if s.boost_kind == "per_query" else all(isinstance(t, dict) for t in arg)
        lim["fact_sources"] = False
        assert all(random_spec(rng, lim).filter_scope != "seeds" for _ in range(60))


# ------------------------------------------------------------------------------------------ the plan of the GPU slices
def _pair_is_servable(a, b):
    """can options a and b be on together in some call?  (each with what it needs: seeds a filter, hits an aggregate)"""
    for entry in ENTRIES:
        if ("fusion" in (a, b)) != (entry == "last_fused"):
            continue
        s = CallSpec(entry=entry)
        for o in (a, b):
            if o in ("filter", "seeds"):
                s.filter_kind = "half"
            if o == "seeds":
                s.filter_scope = "seeds"
            if o in ("group_agg", "group_hits"):
                s.group_agg = "max"
            if o == "group_hits":
                s.group_hits = 2
            if o == "mmr":
                s.mmr_lambda = 0.5
            if o == "lexical":
                s.lexical_weight = 0.3
            if o == "fusion":
                s.fuse, s.member_ptr = "sum", [0, 1]
            if o == "boost":
                s.boost_kind, s.boost_ids = "one", [0]
        if servable(s, dict(max_topk=100)) is None:
            return True
    return False


def test_the_plan_of_the_gpu_slices_covers_every_condition():
    cases = plan(PLAN_SEED, PLAN_CASES, PLAN_CALLS)
    assert cases == plan(PLAN_SEED, PLAN_CASES, PLAN_CALLS)                      # seeded: the same list every time
    specs = [s for _, ss in cases for s in ss]
    assert len(specs) == PLAN_CASES * PLAN_CALLS
    for o in OPTIONS:                                                            # every option in a quarter of the calls
        assert sum(o in s.options() for s in specs) * 4 >= len(specs), o
    pairs = [(a, b) for a, b in itertools.combinations(OPTIONS, 2) if _pair_is_servable(a, b)]
    # seeds x lexical is served nowhere; the boost composes with each of the other seven on some entry: 20 + 7 pairs
    assert ("seeds", "lexical") not in pairs and len(pairs) == 27
    assert len([p for p in pairs if "boost" in p]) == len(OPTIONS) - 1
    for a, b in pairs:
        assert any(a in s.options() and b in s.options() for s in specs), (a, b)
    assert {s.filter_kind for s in specs} == set(FILTER_KINDS) and {s.filter_form for s in specs} == set(FILTER_FORMS)
    assert any(s.filter_per_query for s in specs) and any(not s.filter_per_query and s.filter_kind != "none" for s in specs)
    assert {s.entry for s in specs} == set(ENTRIES)
    assert {c["b"] for c, _ in cases} == set(BATCHES)
    assert any(n_passages_of(c["v"], c["pfrac"]) > 2048 for c, _ in cases)       # two lexical tiles
    assert any(s.k == case_limits(c)["n_passages"] for c, ss in cases for s in ss)
    assert any(s.workspace for s in specs) and any(s.lexical_empty for s in specs)
    assert {s.fuse for s in specs} >= {"sum", "max", "rrf"}
    for fam in ((1, 8), (9, 64), (65, 130, 257)):                                # each slice: a grouped MMR call with c > k and hits
        assert any(s.group_agg and s.group_hits and s.mmr_lambda is not None and s.candidates() > s.k
                   for c, ss in cases if c["b"] in fam for s in ss), fam
        # ... and a boosted one under a per-query filter; a boosted call on every entry
        mine = [s for c, ss in cases if c["b"] in fam for s in ss if s.boost_kind is not None]
        assert any(s.group_agg and s.group_hits and s.mmr_lambda is not None and s.candidates() > s.k
                   and s.filter_kind != "none" and s.filter_per_query for s in mine), fam
        assert {s.entry for s in mine} == set(ENTRIES), fam
    boosted = [s for s in specs if s.boost_kind is not None]
    assert {s.boost_kind for s in boosted} == set(BOOST_KINDS) and {s.boost_form for s in boosted} == set(BOOST_FORMS)
    assert {(s.boost_kind, s.boost_form) for s in boosted} == set(itertools.product(BOOST_KINDS, BOOST_FORMS))
    assert any(s.filter_kind in ("few", "one") for s in boosted)                 # fewer than k allowed: the -1 / 0 padding
    assert any(s.filter_kind == "empty" for s in boosted)
    assert any(s.filter_scope == "seeds" for s in boosted)
    assert any(s.workspace for s in boosted) and any(s.lexical_weight is not None for s in boosted)
    assert {i for s in boosted for i in s.boost_ids} == set(range(len(BOOST_PROGRAMS)))
    assert any(s.k == case_limits(c)["max_topk"] == case_limits(c)["n_passages"] for c, ss in cases for s in ss
               if s.boost_kind is not None)                                      # k = max_topk = n
    assert any(case_limits(c)["max_topk"] == 10 for c, ss in cases for s in ss if s.boost_kind is not None)
    for c, ss in cases:                                                          # servable under the case's own limits
        assert all(servable(s, case_limits(c)) is None for s in ss)
