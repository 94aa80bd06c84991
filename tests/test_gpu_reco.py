"""Recommend by example on the device (include/hrag.h, "recommend by example"; csrc/reco.hip): the fused kernel held to
the numpy restatement bit for bit on exact inputs and to gather + hrag_sim_gemm + hrag_reco_rows on realistic ones, the
reduce, the average_vector query and the exclusion held to their restatements, Engine.recommend to the seams chained by
hand, retrieve(feedback=) to retrieve_scored over the hand-made blend, and the planted corpus.

Shapes follow the kernel's constants: passages around HRAG_RECO_TILE, dims with and without a k tail, batches of one, of
less than and of more than one column tile of queries, the example counts around the 16-column MFMA block."""

import numpy as np
import pytest

from tests.helpers import rounded_score_bound, sim_reference, split_f32_np, split_score_bound
from tests.reco_helpers import (COUNTS, RECO_TILE, all_bits, effective_sign, exclude_np, make_examples, ordered_sum_case,
                                query_bits, reco_query_np, reco_rows_np, same_bits, tree_sum_rows_np)
from tests.test_gpu_mmr import _realistic_rows, _row_engine
from tests.test_gpu_sim_exact import _exact_inputs, _operands, _sim_gemm, _unit

pytestmark = pytest.mark.gpu

KINDS = ["bf16", "fp16", "split"]
MODES = {"best_score": 0, "sum_scores": 1}
GUARD = -7.25
NS = [1, RECO_TILE - 1, RECO_TILE, RECO_TILE + 1, 300 + 2 * RECO_TILE]
DIMS = [64, 200, 768]
BATCHES = [1, 3, 70]


def _L():
    from hipporag_amd import _lib
    return _lib, _lib.load()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _np(t):
    return t.cpu().numpy()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _batches(b):
    """the count lists of every launch at batch b: each of the issue's counts at every batch"""
    if b == 1:
        return [[c] for c in COUNTS]
    if b == 3:
        return [[COUNTS[(i + j) % 8] for j in range(3)] for i in (0, 3, 5)]
    return [[COUNTS[(3 * i) % 8] if i % 5 else COUNTS[i % 8] for i in range(b)]]


def _fused(emb, n, kdim, dt, split, ex, mode, ld=None, pad=0):
    """hrag_reco_scores_rows -> (the [B, n] view, the whole guard-filled buffer with a guard in front and behind)"""
    import torch
    L, lib = _L()
    ptr, idx, sign = ex
    b = len(ptr) - 1
    ld = n if ld is None else ld
    buf = torch.full((pad + b * ld + pad,), GUARD, dtype=torch.float32, device="cuda")
    need = int(lib.hrag_reco_workspace_bytes(b))
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    d_ptr, d_idx, d_sign = _dev(ptr), _dev(idx), _dev(sign)          # (held until the call has run)
    L.check(lib.hrag_reco_scores_rows(emb.data_ptr(), n, kdim, dt, 1 if split else 0, ptr.ctypes.data, d_ptr.data_ptr(),
                                      d_idx.data_ptr(), d_sign.data_ptr(), b, MODES[mode],
                                      buf.data_ptr() + 4 * pad, ld, ws.data_ptr(), need, _stream()))
    torch.cuda.synchronize()
    return buf[pad:pad + b * ld].view(b, ld), buf


def _reco_rows(s, ptr, sign, n, mode, ld_out=None):
    import torch
    L, lib = _L()
    b = len(ptr) - 1
    ld_out = n if ld_out is None else ld_out
    out = torch.full((b, ld_out), GUARD, dtype=torch.float32, device="cuda")
    d_ptr, d_sign = _dev(np.asarray(ptr, np.int32)), _dev(np.asarray(sign, np.int32))      # (held until the call has run)
    L.check(lib.hrag_reco_rows(s.data_ptr(), s.stride(0), d_ptr.data_ptr(), d_sign.data_ptr(), b, n, MODES[mode],
                               out.data_ptr(), ld_out, _stream()))
    torch.cuda.synchronize()
    return out


def _three_step_matrix(emb, kind, kdim, dt, n, idx):
    """The [E, n] matrix the fused kernel never writes: the example rows gathered (an empty id: a zero row), as queries
    ([hi | hi | lo] on split), through hrag_sim_gemm.  At least three queries: one or two take hrag_sim_gemm's dot-product
    kernel, whose summation order is another one (include/hrag.h)."""
    import torch
    ok = (idx >= 0) & (idx < n)
    sel = _dev(np.where(ok, idx, 0).astype(np.int64))
    eg = (emb[sel] * _dev(ok)[:, None]).contiguous()
    if kind == "split":
        d = kdim // 3
        eg = torch.cat([eg[:, :d], eg[:, 2 * d:], eg[:, d:2 * d]], dim=1).contiguous()
    e = eg.shape[0]
    if e < 3:
        eg = torch.cat([eg, torch.zeros((3 - e, kdim), dtype=eg.dtype, device="cuda")]).contiguous()
    ld = n + (-n) % 4
    out = torch.empty((eg.shape[0], ld), device="cuda")
    _sim_gemm(emb, eg, kdim, dt, out)
    torch.cuda.synchronize()
    return out[:e]


# ---------------------------------------------------------------------------------- 1. exact inputs
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", DIMS)
def test_fused_exact_inputs_equal_the_restatement(gpu_device, kind, dim):
    for n in NS:
        x, _, _ = _exact_inputs(kind, n, dim, 1, seed=n * 7 + dim)
        emb, _, kdim, dt, _, _ = _operands(kind, x, x[:1])
        if kind == "split":
            hi, lo = split_f32_np(_np(x))
            rows, lo = hi.astype(np.float64), lo.astype(np.float64)
        else:
            rows, lo = _np(emb.float()).astype(np.float64), None
        for b in BATCHES:
            for li, counts in enumerate(_batches(b)):
                rng = np.random.default_rng(n * 31 + dim + b + li)
                ptr, idx, sign = make_examples(rng, n, counts)
                if b == 70:
                    idx[ptr[5]] = -1                                  # ... and one query whose first example is empty
                eff = effective_sign(idx, sign, n)
                safe = np.where(eff != 0, idx, 0)
                q = rows[safe]
                s = q @ rows.T                                        # [E, n]: exact, whatever the order
                if lo is not None:
                    s = s + q @ lo.T + lo[safe] @ rows.T              # hi.qhi + lo.qhi + hi.qlo
                s32 = s.astype(np.float32)
                assert np.array_equal(s32.astype(np.float64), s)
                for mode in MODES:
                    ld = n + 3
                    got, buf = _fused(emb, n, kdim, dt, kind == "split", (ptr, idx, sign), mode, ld=ld, pad=64)
                    want = reco_rows_np(s32, ptr, eff, mode)
                    assert same_bits(_np(got)[:, :n], want), (kind, dim, n, b, li, mode)
                    assert bool((got[:, n:] == GUARD).all()) and bool((buf[:64] == GUARD).all())
                    assert bool((buf[64 + b * ld:] == GUARD).all())


# ---------------------------------------------------------------------------------- 2. realistic rows
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", DIMS)
def test_fused_realistic_rows_equal_gather_gemm_reduce(gpu_device, kind, dim):
    import torch
    n = NS[-1]
    x = _realistic_rows(n, dim, seed=dim + 1)
    emb, _, kdim, dt, x_ref, _ = _operands(kind, x, x[:1])
    for b in BATCHES:
        for li, counts in enumerate(_batches(b)[:3]):
            rng = np.random.default_rng(dim + 13 * b + li)
            ptr, idx, sign = make_examples(rng, n, counts)
            eff = effective_sign(idx, sign, n)
            s = _three_step_matrix(emb, kind, kdim, dt, n, idx)
            # every s within the derived bound of the fp64 product
            ok = _dev(eff != 0)
            qr = x_ref[_dev(np.where(eff != 0, idx, 0).astype(np.int64))] * ok[:, None]
            want = sim_reference(x_ref, qr)
            bound = split_score_bound(x_ref, qr) if kind == "split" else rounded_score_bound(x_ref, qr, kdim)
            err = (s[:, :n].double() - want).abs()
            assert bool((err <= bound).all()), (kind, dim, b, float((err / bound.clamp_min(1e-300)).max()))
            for mode in MODES:
                got, _ = _fused(emb, n, kdim, dt, kind == "split", (ptr, idx, sign), mode)
                three = _reco_rows(s, ptr, eff, n, mode)
                assert torch.equal(got.view(torch.int32), three.view(torch.int32)), (kind, dim, b, li, mode)
                assert same_bits(_np(three), reco_rows_np(_np(s)[:, :n], ptr, eff, mode)), (kind, dim, b, li, mode)


def test_reco_rows_alone_with_special_values(gpu_device):
    """NaN, infinities and signed zeros through the reduce; guard columns beyond n"""
    rng = np.random.default_rng(3)
    n = 300
    ptr, _, sign = make_examples(rng, n, COUNTS + [(2, 2), (3, 0)])
    e = int(ptr[-1])
    s = rng.standard_normal((e, n)).astype(np.float32)
    for v in (np.nan, np.inf, -np.inf, -0.0, 0.0):
        s[rng.integers(0, e, 40), rng.integers(0, n, 40)] = v
    s[:, 7] = -0.0
    s[:, 8] = np.nan
    sign[rng.random(e) < 0.1] = 0
    for mode in MODES:
        out = _reco_rows(_dev(s), ptr, sign, n - 5, mode, ld_out=n)
        assert same_bits(_np(out)[:, :n - 5], reco_rows_np(s[:, :n - 5], ptr, sign, mode)), mode
        assert bool((out[:, n - 5:] == GUARD).all())


# ---------------------------------------------------------------------------------- 3. all-negative scores
@pytest.mark.parametrize("kind", KINDS)
def test_best_score_of_all_negative_scores_is_the_negative_maximum(gpu_device, kind):
    """examples antipodal to the scored half of the corpus: every real score is negative, and a +0.0 from one of the 13
    padding columns of the query's block (or from the empty example) must not win"""
    import torch
    n, dim = 2 * RECO_TILE + 10, 64
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    d = _unit(torch.randn((1, dim), generator=g, device="cuda", dtype=torch.float64))
    x = _unit(d + 0.3 * _unit(torch.randn((n, dim), generator=g, device="cuda", dtype=torch.float64)))
    x[n // 2:] = -x[n // 2:]
    emb, _, kdim, dt, _, _ = _operands(kind, x.float().contiguous(), x[:1].float())
    ptr = np.array([0, 4, 6], np.int32)
    idx = np.array([n - 1, n - 2, -1, n - 3, n - 4, n - 5], np.int32)
    sign = np.array([1, 1, 1, 1, 1, 1], np.int32)
    got, _ = _fused(emb, n, kdim, dt, kind == "split", (ptr, idx, sign), "best_score")
    head = _np(got)[:, :n // 2]
    assert (head < 0).all() and np.isfinite(head).all(), kind
    s = _three_step_matrix(emb, kind, kdim, dt, n, idx)
    eff = effective_sign(idx, sign, n)
    assert same_bits(_np(got), reco_rows_np(_np(s)[:, :n], ptr, eff, "best_score"))
    assert same_bits(head[0], _np(s)[[0, 1, 3], :n // 2].max(0))


# ---------------------------------------------------------------------------------- 4. the ordered sum
def test_sum_scores_adds_in_list_order(gpu_device):
    import torch
    sc, in_order, tree = ordered_sum_case()
    n, dim = 6, 64
    x = np.zeros((n, dim), np.float32)
    x[0, 0] = 1.0                                  # the scored passage
    x[1:5, 0] = sc                                 # the examples: s(0, e) = sc[e], exactly
    emb = _dev(x).to(torch.bfloat16)
    assert torch.equal(emb.float(), _dev(x))
    ptr, idx, sign = np.array([0, 4], np.int32), np.array([1, 2, 3, 4], np.int32), np.ones(4, np.int32)
    got, _ = _fused(emb, n, dim, 0, False, (ptr, idx, sign), "sum_scores")
    assert _np(got)[0, 0] == in_order != tree
    rows = np.zeros((4, 8), np.float32)
    rows[:, 0] = sc
    assert _np(_reco_rows(_dev(rows), ptr, sign, 8, "sum_scores"))[0, 0] == in_order
    assert tree_sum_rows_np(rows, ptr, sign)[0, 0] == tree and reco_rows_np(rows, ptr, sign, "sum_scores")[0, 0] == in_order


# ---------------------------------------------------------------------------------- 5. the average_vector query
def _examples(ex, device="cuda"):
    from hipporag_amd.reco import Examples
    return Examples(*ex, device=device)


@pytest.mark.parametrize("kind", KINDS)
def test_reco_query_bits_and_the_average_vector_call(gpu_device, kind):
    import torch
    n, dim, k = 300, 200, 20
    x = _realistic_rows(n, dim, seed=9)
    emb, _, kdim, dt, _, _ = _operands(kind, x, x[:1])
    xs = x if kind == "split" else x.to(emb.dtype)
    if kind == "split":
        hi, lo = split_f32_np(_np(x))
        values = hi.astype(np.float64) + lo.astype(np.float64)
    else:
        values = _np(emb.float()).astype(np.float64)
    rng = np.random.default_rng(12)
    ex = make_examples(rng, n, COUNTS)
    with _row_engine(kind, xs, len(COUNTS), max_topk=k) as eng:
        e = _examples(ex)
        q16, v, flags = eng.recommend_query(e, return_bits=True)
        want_v, want_flags = reco_query_np(values, *ex)
        assert np.array_equal(_np(flags), want_flags) and want_flags[1] == 1 and want_flags[0] == 0
        assert same_bits(_np(v), want_v)
        assert np.array_equal(_np(q16).view(np.uint16), query_bits(kind, want_v)), kind
        assert not _np(q16)[1].any()                                    # no positive: the all-zero query
        q, _ = eng.recommend_query(e)
        filt = eng.recommend_filter(e)
        want = eng.dense_retrieve(q, k=k, doc_filter=filt)
        got = eng.recommend(e, k=k, strategy="average_vector")
        assert torch.equal(got[0], want[0]) and same_bits(_np(got[1]), _np(want[1]))
        got = eng.recommend(e, k=k, strategy="average_vector", exclude_examples=False, mmr_lambda=0.5)
        want = eng.dense_retrieve(q, k=k, mmr_lambda=0.5)
        assert all(torch.equal(a.view(torch.int32), w.view(torch.int32)) for a, w in zip(got, want)) and len(got) == 3


# ---------------------------------------------------------------------------------- 6. the exclusion
def test_exclude_clears_exactly_the_example_bits(gpu_device):
    import torch
    L, lib = _L()
    n = 32 * 5 + 7                                     # a last partial word
    ptr = np.array([0, 5, 9, 10, 12], np.int32)
    idx = np.array([0, 31, 32, n - 1, 31,              # word 0, bit 31 / 32, the last partial word, a repeated id
                    5, -1, n + 5, 2 ** 31 - 1,         # empty ids clear nothing
                    64,
                    3, 100], np.int32)
    sign = np.array([1, -1, 1, 1, 1, 1, 1, 1, 1, -1, 0, 1], np.int32)      # (sign 0: empty, bit 3 stays)
    rng = np.random.default_rng(1)
    words = rng.integers(0, 2 ** 32, (4, 8), dtype=np.uint64).astype(np.uint32)      # ld 8 > 6 words: the tail is untouched
    w = _dev(words.view(np.int32))
    d_ptr, d_idx, d_sign = _dev(ptr), _dev(idx), _dev(sign)
    L.check(lib.hrag_reco_exclude(w.data_ptr(), 8, n, d_ptr.data_ptr(), d_idx.data_ptr(), d_sign.data_ptr(), 4, _stream()))
    torch.cuda.synchronize()
    want = exclude_np(words, ptr, idx, sign, n)
    assert np.array_equal(_np(w).view(np.uint32), want)
    assert (want[2] != words[2]).sum() <= 1 and np.array_equal(want[:, 6:], words[:, 6:])
    assert want[3, 0] & 8 == words[3, 0] & 8
    # ex_sign NULL: every id in range
    w = _dev(words.view(np.int32))
    L.check(lib.hrag_reco_exclude(w.data_ptr(), 8, n, d_ptr.data_ptr(), d_idx.data_ptr(), None, 4, _stream()))
    assert np.array_equal(_np(w).view(np.uint32), exclude_np(words, ptr, idx, np.ones_like(sign), n))
    assert lib.hrag_reco_exclude(w.data_ptr(), 5, n, d_ptr.data_ptr(), d_idx.data_ptr(), None, 4, _stream()) == L.HRAG_EINVAL


def test_recommend_filter_and_exclusion_in_the_ranking(gpu_device):
    import torch
    from hipporag_amd.engine import pack_mask
    n, dim, k = 2 * RECO_TILE + 37, 64, 30
    x = _realistic_rows(n, dim, seed=2)
    x[3::4] = _unit(torch.randn((len(x[3::4]), dim), device="cuda", dtype=torch.float64,
                                generator=torch.Generator(device="cuda").manual_seed(1))).float()      # no near-duplicates
    xs = x.to(torch.bfloat16)
    rng = np.random.default_rng(4)
    pos = [rng.choice(n, 6, replace=False).tolist() for _ in range(5)]
    neg = [[int(rng.integers(0, n))] for _ in range(5)]
    from hipporag_amd.reco import Examples
    with _row_engine("bf16", xs, 5, max_topk=k) as eng:
        e = Examples.from_lists(pos, neg)
        ex = (e.ex_ptr, e.ex_idx_host, e.ex_sign_host)
        # no filter: all n bits, minus the examples
        assert np.array_equal(_np(eng.recommend_filter(e)).view(np.uint32), exclude_np(all_bits(5, n), *ex, n))
        # a shared row is expanded, in a tensor of its own: the caller's row is left as it is
        allowed = rng.random(n) < 0.7
        shared = _dev(pack_mask(allowed).view(np.int32))
        keep = shared.clone()
        got = eng.recommend_filter(e, shared)
        assert torch.equal(shared, keep) and got.shape[0] == 5
        assert np.array_equal(_np(got).view(np.uint32), exclude_np(np.tile(pack_mask(allowed), (5, 1)), *ex, n))
        got = eng.recommend_filter(e, _dev(allowed))                     # the bool form
        assert np.array_equal(_np(got).view(np.uint32), exclude_np(np.tile(pack_mask(allowed), (5, 1)), *ex, n))
        for strategy in ("best_score", "sum_scores", "average_vector"):
            idx, _ = eng.recommend(e, k=k, strategy=strategy, doc_filter=shared)
            for q in range(5):
                ids = _np(idx)[q]
                assert not set(ids.tolist()) & set(pos[q] + neg[q]) and allowed[ids].all(), (strategy, q)
        # not excluded: on unit rows every positive scores ~1 against itself and ranks first
        idx, sc = eng.recommend(e, k=k, exclude_examples=False)
        for q in range(5):
            assert set(_np(idx)[q, :6].tolist()) == set(pos[q]), q


# ---------------------------------------------------------------------------------- 7. the planted corpus
def test_planted_clusters(gpu_device):
    """Two tight clusters A and B far apart with one positive in each, a third cluster C with the negative in it, passages
    M between A and B, fillers.  best_score ranks the members of A and B above everything else and C's last;
    average_vector does not: its mean lies between the clusters, where M is."""
    import torch
    from hipporag_amd.reco import Examples
    rng = np.random.default_rng(7)
    dim, m = 128, 6

    def unit(v):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)

    base = np.linalg.qr(rng.standard_normal((dim, dim)))[0][:4]          # orthonormal centres
    ca, cb, cc = base[0], base[1], base[2]

    def cluster(c, count):
        return unit(c + 0.03 * unit(rng.standard_normal((count, dim))))
    a, b_, c_ = cluster(ca, m), cluster(cb, m), cluster(cc, m)
    mid = cluster(unit(ca + cb), 3)
    fill = unit(base[3] + 0.8 * unit(rng.standard_normal((40, dim))))
    x = np.concatenate([a, b_, c_, mid, fill]).astype(np.float32)
    n = x.shape[0]
    ia, ib, ic, im = range(0, m), range(m, 2 * m), range(2 * m, 3 * m), range(3 * m, 3 * m + 3)
    e = Examples.from_lists([[0, m]], [[2 * m]])
    with _row_engine("bf16", _dev(x).to(torch.bfloat16), 1, max_topk=n) as eng:
        idx, sc = eng.recommend(e, k=n - 3, strategy="best_score")
        ids = _np(idx)[0].tolist()
        members = (set(ia) | set(ib)) - {0, m}
        assert set(ids[:len(members)]) == members
        assert set(ids[-(m - 1):]) == set(ic) - {2 * m}                  # the negative's neighbours rank last
        idx, _ = eng.recommend(e, k=n - 3, strategy="average_vector")
        ids = _np(idx)[0].tolist()
        assert set(ids[:3]) == set(im) and set(ids[:len(members)]) != members


# ---------------------------------------------------------------------------------- 8. the engine calls
@pytest.fixture(scope="module")
def case(gpu_device):
    from hipporag_amd.engine import HippoRAGEngine
    from hipporag_amd.late import TokenIndex
    from oracle.checks import make_case
    from tests.late_helpers import exact_tokens
    kg, pass_bits, fact_bits, _ = make_case(3000, 24000, 64, seed=4242)
    n_p = kg.n_passages
    rng = np.random.default_rng(8)
    eng = HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                         max_batch=70, max_topk=min(200, n_p))
    tix = TokenIndex.from_ragged(exact_tokens(rng, rng.integers(1, 20, n_p), 32), "bf16")
    eng.set_token_index(tix)
    yield gpu_device, kg, pass_bits, fact_bits, eng
    eng.close()
    tix.close()


def _bf16(bits, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)


def _same(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_recommend_is_its_seams_chained_by_hand(case):
    import torch
    from hipporag_amd.late import LateQueries
    from tests.late_helpers import exact_tokens
    dev, kg, pass_bits, fact_bits, eng = case
    n_p, b, k, c = kg.n_passages, 70, 10, 40
    rng = np.random.default_rng(21)
    ex = make_examples(rng, n_p, [COUNTS[i % 8] for i in range(b)], shuffle=False)
    e = _examples(ex)
    allowed = _dev(np.arange(n_p) % 3 != 0)
    lq = LateQueries.from_ragged(exact_tokens(rng, [1 + q % 9 for q in range(b)], 32), "bf16")
    pass_dev = _bf16(pass_bits, dev).contiguous()
    wk = eng.workspace()
    for strategy in MODES:
        rows = eng.recommend_scores(e, strategy)
        # the engine call equals the engine-free one on the same rows, on both handles
        free, _ = _fused(pass_dev, n_p, pass_bits.shape[1], 0, False, ex, strategy)
        assert _same(rows, free) and _same(wk.recommend_scores(e, strategy), rows)
        filt = eng.recommend_filter(e, allowed)
        want = eng._rank_rows(rows, k, False, filt)
        got = eng.recommend(e, k=k, strategy=strategy, doc_filter=allowed)
        assert len(got) == 2 and _same(got[0], want[0]) and _same(got[1], want[1]), strategy
        assert all(_same(x, y) for x, y in zip(wk.recommend(e, k=k, strategy=strategy, doc_filter=allowed), got))
        # MMR over c ranked entries
        ci, cs = eng._rank_rows(rows, c, False, filt)
        want = eng.mmr(ci, cs, k, 0.5)
        got = eng.recommend(e, k=k, strategy=strategy, doc_filter=allowed, mmr_lambda=0.5, mmr_candidates=c)
        assert len(got) == 3 and all(_same(x, y) for x, y in zip(got, want)), strategy
        # late reranking of c ranked entries
        li, ls, sel = eng.late_rerank(ci, lq, k, return_sel=True)
        got = eng.recommend(e, k=k, strategy=strategy, doc_filter=allowed, late=lq, late_candidates=c)
        first = torch.gather(cs, 1, sel.clamp_min(0).long())
        assert len(got) == 3 and _same(got[0], li) and _same(got[1], ls) and _same(got[2], first), strategy
        # ... then MMR among all c rescored entries, the late scores as relevance; the first-stage scores follow the picks
        lc, lsc, selc = eng.late_rerank(ci, lq, c, return_sel=True)
        firstc = torch.gather(cs, 1, selc.clamp_min(0).long())
        mi, ms, mv, msel = eng.mmr(lc, lsc, k, 0.5, return_sel=True)
        got = eng.recommend(e, k=k, strategy=strategy, doc_filter=allowed, late=lq, late_candidates=c, mmr_lambda=0.5)
        assert len(got) == 4 and _same(got[0], mi) and _same(got[1], ms) and _same(got[2], mv), strategy
        assert _same(got[3], torch.gather(firstc, 1, msel.clamp_min(0).long())), strategy
        # batch 1 equals row q of batch 70, at any position
        for q in (0, 5, 37, 69):
            one = eng.recommend_scores(e.select([q]), strategy)
            assert _same(one[0], rows[q]), (strategy, q)
    wk.close()
    for kw, name in ((dict(group_agg="max"), "group_agg"), (dict(group_hits=2), "group_hits"), (dict(boost=[{"mul": 2.0}]), "boost"),
                     (dict(lexical=(np.zeros(b + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))), "lexical")):
        with pytest.raises(ValueError, match=f"does not serve {name}: .*retrieve_scored"):
            eng.recommend(e, k=k, **kw)
    with pytest.raises(ValueError, match="strategy='cosine'"):
        eng.recommend(e, k=k, strategy="cosine")
    with pytest.raises(ValueError, match="produces a query"):
        eng.recommend_scores(e, "average_vector")


def test_retrieve_with_feedback_is_retrieve_scored_over_the_blend(case):
    import torch
    from hipporag_amd import synth
    from hipporag_amd.engine import row_minmax
    L, lib = _L()
    dev, kg, pass_bits, fact_bits, eng = case
    n_p, b, k = kg.n_passages, 9, 20
    qf = _bf16(synth.make_queries_np(fact_bits, b, seed=5)[0], dev)
    qp = _bf16(synth.make_queries_np(pass_bits, b, seed=6)[0], dev)
    idx, sc = eng.score_facts(qf, k=5)
    cnt = torch.full((b,), 5, dtype=torch.int32, device=dev)
    cnt[::4] = 0
    rng = np.random.default_rng(2)
    e = _examples(make_examples(rng, n_p, [COUNTS[(i + 2) % 8] for i in range(b)]))
    plain = eng.retrieve(qp, idx, sc, cnt, k=k)
    for strategy, w in (("best_score", 0.3), ("sum_scores", 0.75)):
        dense = eng.sim_scores("passages", qp)
        rec = eng.recommend_scores(e, strategy)
        mn_d, mx_d = row_minmax(dense, n_p)
        mn_r, mx_r = row_minmax(rec, n_p)
        blend = torch.empty_like(dense)
        L.check(lib.hrag_lex_blend_rows(dense.data_ptr(), dense.stride(0), rec.data_ptr(), rec.stride(0), b, n_p,
                                        mn_d.data_ptr(), mx_d.data_ptr(), mn_r.data_ptr(), mx_r.data_ptr(), w,
                                        blend.data_ptr(), blend.stride(0), _stream()))
        want = eng.retrieve_scored(blend, idx, sc, cnt, k=k)
        got = eng.retrieve(qp, idx, sc, cnt, k=k, feedback=e, feedback_weight=w, feedback_strategy=strategy)
        assert _same(got.doc_idx, want.doc_idx) and _same(got.doc_score, want.doc_score) and _same(got.flags, want.flags)
        assert not _same(got.doc_idx, plain.doc_idx)                               # (the feedback does something)
        conv = eng.retrieve_converged(qp, idx, sc, cnt, k=k, ppr_tol=0.0, feedback=e, feedback_weight=w,
                                      feedback_strategy=strategy)
        assert _same(conv.doc_idx, want.doc_idx) and _same(conv.doc_score, want.doc_score)
    zero = eng.retrieve(qp, idx, sc, cnt, k=k, feedback=e, feedback_weight=0)
    assert _same(zero.doc_idx, plain.doc_idx) and _same(zero.doc_score, plain.doc_score) and _same(zero.flags, plain.flags)
    with pytest.raises(ValueError, match="feedback together with lexical"):
        eng.retrieve(qp, idx, sc, cnt, k=k, feedback=e, lexical=(np.zeros(b + 1, np.int32), np.zeros(0, np.int32),
                                                                 np.zeros(0, np.float32)))
    with pytest.raises(ValueError, match="feedback: it holds 9 queries, the call 4"):
        eng.retrieve(qp[:4], idx[:4], sc[:4], cnt[:4], k=k, feedback=e)
    with pytest.raises(ValueError, match="feedback_weight=1.5"):
        eng.retrieve(qp, idx, sc, cnt, k=k, feedback=e, feedback_weight=1.5)


def test_the_c_calls_refuse_bad_arguments_before_anything_is_enqueued(case):
    import torch
    L, lib = _L()
    dev, kg, pass_bits, fact_bits, eng = case
    n_p = kg.n_passages
    e = _examples(make_examples(np.random.default_rng(0), n_p, COUNTS[:3]))
    out = torch.full((3, n_p), GUARD, device="cuda")
    need = int(lib.hrag_reco_workspace_bytes(3))
    ws = torch.empty((need + 16,), dtype=torch.uint8, device="cuda")
    ptr = e.ex_ptr

    def call(h=eng._handle, p=ptr, b=3, mode=0, o=out.data_ptr(), w=ws.data_ptr(), wb=need, pd=e.ex_ptr_dev.data_ptr()):
        return lib.hrag_reco_scores(h, p.ctypes.data if p is not None else None, pd, e.ex_idx.data_ptr(),
                                    e.ex_sign.data_ptr(), b, mode, o, n_p, w, wb, _stream())
    assert lib.hrag_reco_workspace_bytes(0) < 0 and need == 3 * 32 * 8 + 16
    for kw, what in ((dict(h=None), "engine is NULL"), (dict(b=0), "batch 0"), (dict(b=71), "batch 71"), (dict(mode=2), "mode=2"),
                     (dict(mode=-1), "mode=-1"), (dict(o=None), "output"), (dict(w=None), "workspace"), (dict(wb=need - 1), "workspace"),
                     (dict(w=ws.data_ptr() + 4), "16-byte aligned"), (dict(p=None), "ex_ptr"), (dict(pd=None), "ex_ptr"),
                     (dict(p=np.array([0, 5, 3, 6], np.int32)), "ex_ptr decreases"), (dict(p=np.array([1, 2, 3, 4], np.int32)), "ex_ptr\\[0\\]")):
        assert call(**kw) == L.HRAG_EINVAL, kw
        import re
        assert re.search(what, lib.hrag_last_error().decode()), (kw, lib.hrag_last_error())
    q16 = torch.zeros((3, 64), dtype=torch.int16, device="cuda")
    fl = torch.zeros(3, dtype=torch.int32, device="cuda")
    assert lib.hrag_reco_query(eng._handle, ptr.ctypes.data, e.ex_ptr_dev.data_ptr(), e.ex_idx.data_ptr(), e.ex_sign.data_ptr(), 3,
                               None, None, fl.data_ptr(), _stream()) == L.HRAG_EINVAL
    assert lib.hrag_reco_rows(None, n_p, e.ex_ptr_dev.data_ptr(), e.ex_sign.data_ptr(), 3, n_p, 0, out.data_ptr(), n_p,
                              _stream()) == L.HRAG_EINVAL
    assert lib.hrag_reco_rows(out.data_ptr(), n_p, e.ex_ptr_dev.data_ptr(), e.ex_sign.data_ptr(), 3, n_p, 2, out.data_ptr(), n_p,
                              _stream()) == L.HRAG_EINVAL
    torch.cuda.synchronize()
    assert bool((out == GUARD).all()) and not q16.any()
    assert call() == L.HRAG_OK
    torch.cuda.synchronize()
    assert not bool((out == GUARD).any())


# ---------------------------------------------------------------------------------- 9. the mirror
def test_the_mirror_recommends_and_feeds_back(gpu_device):
    from hipporag_amd.reco import Examples
    from hipporag_amd.retriever import HippoRAG, RetrievalConfig
    from tests.late_helpers import PlantedEmbedder, planted_late_corpus, planted_texts
    corpus = planted_late_corpus(5)
    docs, triples, queries = planted_texts(corpus)
    rag = HippoRAG(RetrievalConfig(max_batch=2), embedding_model=PlantedEmbedder(corpus))
    rag.index_from_openie(docs, triples)
    rag.prepare_retrieval_objects() if not rag.ready_to_retrieve else None
    eng, keys, docs = rag.engine, rag.passage_node_keys, list(rag.passage_texts)      # (position i: docs[i], keys[i])
    pos = [[docs[0], keys[3]], [docs[5]], [docs[2], docs[7], docs[1]]]
    neg = [[docs[4]], [], [keys[6]]]
    ids_p, ids_n = [[0, 3], [5], [2, 7, 1]], [[4], [], [6]]
    for strategy in ("best_score", "sum_scores", "average_vector"):
        sols = rag.recommend(pos, neg, num_to_retrieve=5, strategy=strategy)
        assert len(sols) == 3
        for q, s_ in enumerate(sols):                                   # batches of two queries: each equals the engine call
            idx, sc = eng.recommend(Examples.from_lists([ids_p[q]], [ids_n[q]]), k=5, strategy=strategy)
            assert s_.question is None and s_.docs == [docs[i] for i in _np(idx)[0] if i >= 0], (strategy, q)
            assert same_bits(np.asarray(s_.doc_scores, np.float32), _np(sc)[0][:len(s_.docs)])
            assert all(d["recommended"] == strategy for d in s_.doc_metadata)
            assert not set(s_.docs) & {docs[i] for i in ids_p[q] + ids_n[q]}
    with pytest.raises(ValueError, match="recommend: unknown document 'no such passage'"):
        rag.recommend([["no such passage"]])
    # retrieve(like=, unlike=): each batch of the pipeline gets its own rows of the examples
    plain = rag.retrieve(queries[:3], num_to_retrieve=4)
    fed = rag.retrieve(queries[:3], num_to_retrieve=4, like=pos, unlike=neg, feedback_weight=0.6)
    serial = [s_ for lo in (0, 2) for s_ in rag.retrieve(queries[lo:lo + 2][:3 - lo], num_to_retrieve=4, like=pos[lo:lo + 2],
                                                         unlike=neg[lo:lo + 2], feedback_weight=0.6)]
    for a, b_ in zip(fed, serial):
        assert a.docs == b_.docs and same_bits(np.asarray(a.doc_scores, np.float32), np.asarray(b_.doc_scores, np.float32))
        assert all(d["feedback_weight"] == 0.6 for d in a.doc_metadata)
    assert any(a.docs != p.docs or not same_bits(np.asarray(a.doc_scores, np.float32), np.asarray(p.doc_scores, np.float32))
               for a, p in zip(fed, plain))
    zero = rag.retrieve(queries[:3], num_to_retrieve=4, like=pos, unlike=neg, feedback_weight=0.0)
    for a, p in zip(zero, plain):
        assert a.docs == p.docs and same_bits(np.asarray(a.doc_scores, np.float32), np.asarray(p.doc_scores, np.float32))
        assert all("feedback_weight" not in d for d in a.doc_metadata)
