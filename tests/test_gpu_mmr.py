"""Diversified retrieval on the device (include/hrag.h, "diversified retrieval"; csrc/mmr.hip): the gathered Gram kernel
held to fp64 and to hrag_sim_gemm, the selection kernel held to the numpy restatement bit for bit, the engine call to the
composition of the two, Engine.retrieve(mmr_lambda=) to the restatement over the plain call's own ranking, and the
planted-duplicate corpus."""

import numpy as np
import pytest

from hipporag_amd import synth
from hipporag_amd.engine import pack_mask
from oracle.checks import make_case
from tests.helpers import rounded_score_bound, sim_reference, split_f32_np, split_score_bound
from tests.mmr_helpers import bf16_round, gram_np, mmr_batch_np, mmr_np, planted_corpus, same_bits
from tests.test_gpu_sim_exact import _exact_inputs, _operands, _sim_gemm, _unit

pytestmark = pytest.mark.gpu

KINDS = ["bf16", "fp16", "split"]
GUARD = -7.25


def _L():
    from hipporag_amd import _lib
    return _lib, _lib.load()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _np(t):
    return t.cpu().numpy()


def _gram(emb, kdim, dt, split, ids, ld=None, pad=0):
    """hrag_gram_rows -> (the [B, c, ld] view, the whole guard-filled buffer)"""
    import torch
    L, lib = _L()
    b, c = ids.shape
    ld = c if ld is None else ld
    buf = torch.full((b * c * ld + pad,), GUARD, dtype=torch.float32, device="cuda")
    L.check(lib.hrag_gram_rows(emb.data_ptr(), emb.shape[0], kdim, dt, 1 if split else 0, ids.data_ptr(), b, c,
                               buf.data_ptr(), ld, _stream()))
    return buf[:b * c * ld].view(b, c, ld), buf


def _mmr_rows(score, ids, sim, k, lam, normalize):
    import torch
    L, lib = _L()
    b, c = ids.shape
    sel, idx = (torch.full((b, k), 77, dtype=torch.int32, device="cuda") for _ in range(2))
    sc, val = (torch.full((b, k), GUARD, dtype=torch.float32, device="cuda") for _ in range(2))
    L.check(lib.hrag_mmr_rows(score.data_ptr(), ids.data_ptr(), sim.data_ptr(), sim.shape[2], b, c, k, lam,
                              1 if normalize else 0, sel.data_ptr(), idx.data_ptr(), sc.data_ptr(), val.data_ptr(), _stream()))
    return sel, idx, sc, val


def _ids(rng, b, c, n):
    """candidate ids with repeats, -1 slots and ids outside [0, n)"""
    ids = rng.integers(0, n, (b, c)).astype(np.int32)
    if c >= 2:
        ids[:, 1] = ids[:, 0]                              # a repeated id
    m = rng.random((b, c))
    ids[m < 0.08] = -1
    ids[(m >= 0.08) & (m < 0.12)] = n + 5
    ids[(m >= 0.12) & (m < 0.14)] = 2 ** 31 - 1
    return ids


# (B, c, dim): every c, dim and B of the issue's lists; 200 exercises every k tail; c > 64 more than one tile
GRAM_SHAPES = [(1, 1, 64), (3, 2, 200), (1, 15, 768), (3, 16, 64), (70, 17, 200), (3, 63, 768), (1, 65, 200), (70, 65, 64),
               (3, 200, 768), (1, 200, 200), (3, 1024, 64), (1, 1024, 200)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("b,c,dim", GRAM_SHAPES)
def test_gram_exact_inputs_are_exact(gpu_device, kind, b, c, dim):
    import torch
    n = 300
    x, _, _ = _exact_inputs(kind, n, dim, 1, seed=c * 7 + dim + b)
    emb, _, kdim, dt, _, _ = _operands(kind, x, x[:1])
    rng = np.random.default_rng(c * 31 + dim + b)
    ids = _ids(rng, b, c, n)
    ld = c + 3
    g, buf = _gram(emb, kdim, dt, kind == "split", torch.from_numpy(ids).cuda(), ld=ld, pad=64)
    torch.cuda.synchronize()
    got = _np(g)
    if kind == "split":
        hi, lo = split_f32_np(_np(x))
        rows, lo = hi.astype(np.float64), lo.astype(np.float64)
    else:
        rows, lo = _np(emb.float()).astype(np.float64), None
    for q in range(b):
        want = gram_np(rows, ids[q], lo)
        assert np.array_equal(got[q, :, :c].astype(np.float64), want), (kind, b, c, dim, q)
    assert (got[:, :, c:] == GUARD).all() and bool((buf[b * c * ld:] == GUARD).all())
    empty = (ids < 0) | (ids >= n)
    assert not got[:, :, :c][empty].any() and not np.swapaxes(got[:, :, :c], 1, 2)[empty].any()


def _realistic_rows(n, dim, seed):
    """unit Gaussian rows, every fourth a near-duplicate (cos ~ 0.999) of the row before it"""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = _unit(torch.randn((n, dim), generator=g, device="cuda", dtype=torch.float64))
    dup = torch.arange(3, n, 4, device="cuda")
    x[dup] = _unit(x[dup - 1] + 0.045 * _unit(torch.randn((len(dup), dim), generator=g, device="cuda", dtype=torch.float64)))
    return x.float().contiguous()


# (c, dim): c >= 3 (the GEMV serves fewer queries); 16- / 64- / 128-query tiles of sim_gemm_kernel and, at (300, 64), the
# 256-row kernel
REAL_SHAPES = [(3, 64), (16, 200), (17, 768), (64, 200), (70, 768), (200, 200), (200, 768), (300, 64), (1024, 64)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c,dim", REAL_SHAPES)
def test_gram_realistic_within_the_bound_and_bit_identical_to_sim_gemm(gpu_device, kind, c, dim):
    import torch
    n = 1500
    x = _realistic_rows(n, dim, seed=c + dim)
    emb, _, kdim, dt, x_ref, _ = _operands(kind, x, x[:1])
    rng = np.random.default_rng(c + 3 * dim)
    ids = np.stack([rng.permutation(n)[:c], rng.integers(0, n, c)]).astype(np.int32)       # distinct ids; with repeats
    ids[1, c // 2] = -1
    ids_d = torch.from_numpy(ids).cuda()
    g, _ = _gram(emb, kdim, dt, kind == "split", ids_d, ld=c + (-c) % 4)
    g = g[:, :, :c]
    torch.cuda.synchronize()
    assert torch.equal(g, g.transpose(1, 2)), "the mirror is bit-symmetric"
    iu = torch.triu(torch.ones((c, c), dtype=torch.bool, device="cuda"))
    for q in range(2):
        ok = torch.from_numpy(ids[q] >= 0).cuda()
        sel = ids_d[q].clamp_min(0).long()
        rows = x_ref[sel] * ok[:, None]
        want = sim_reference(rows, rows)                                 # [query j][row i]
        bound = split_score_bound(rows, rows) if kind == "split" else rounded_score_bound(rows, rows, kdim)
        err = (g[q].double() - want).abs()
        assert bool((err <= bound).all()), (kind, c, dim, q, float((err / bound.clamp_min(1e-300)).max()))
        # hrag_sim_gemm on the gathered rows with the gathered rows as queries: out[j][i] = row i against query j
        eg = (emb[sel] * ok[:, None]).contiguous()
        if kind == "split":
            d = dim
            qq = torch.cat([eg[:, :d], eg[:, 2 * d:], eg[:, d:2 * d]], dim=1).contiguous()      # [hi | hi | lo]
        else:
            qq = eg
        out = torch.empty((c, c + (-c) % 4), device="cuda")
        _sim_gemm(eg, qq, kdim, dt, out)
        torch.cuda.synchronize()
        assert torch.equal(g[q][iu], out[:, :c].T[iu]), (kind, c, dim, q)


# ---------------------------------------------------------------------------------- selection
def _scores(rng, b, n):
    x = (rng.integers(-40, 40, (b, n)).astype(np.float32) / 8 * rng.random((b, n)).astype(np.float32)).astype(np.float32)
    if n >= 6:
        for i in range(b):
            at = rng.integers(0, n, 6)
            x[i, at[0]] = np.nan
            x[i, at[1]] = np.inf
            x[i, at[2]] = -np.inf
            x[i, at[3]] = -0.0
            x[i, at[4]] = x[i, at[5]]
    return x


LAMBDAS = (0.0, 0.3, 0.5, 1.0)
# every c with every B; each runs every k in {1, c // 2, c}, every lambda and both normalize values on the device.  At B = 256
# beyond c = 65 the batch shares ONE similarity matrix (256 matrices of 1024 x 1024 are a gigabyte to restate on the host;
# scores, ids and empty slots still differ per query) and the host restates a sample of the queries, first and last included
SELECT = [(b, c) for c in (1, 2, 63, 64, 65, 255, 257, 1024) for b in (1, 9, 256)]
SAMPLE = [0, 1, 2, 63, 64, 127, 128, 200, 254, 255]


@pytest.mark.parametrize("b,c", SELECT)
def test_selection_matches_the_restatement_bit_for_bit(gpu_device, b, c):
    import torch
    rng = np.random.default_rng(b * 2000 + c)
    shared = b == 256 and c > 65
    rows = np.asarray(SAMPLE) if shared else np.arange(b)
    ks = sorted({1, max(1, c // 2), c})
    ld = c + 2
    for normalize in (True, False):
        s = _scores(rng, b, c)
        ids = np.stack([rng.permutation(4 * c)[:c] for _ in range(b)]).astype(np.int32)
        ids[rng.random((b, c)) < 0.05] = -1
        if b > 1:
            ids[1, :] = -1                                                        # a query without candidates
        g = rng.standard_normal((1 if shared else b, c, c)).astype(np.float32)
        g = np.triu(g) + np.swapaxes(np.triu(g, 1), 1, 2)
        if c >= 3:
            g[:, 1, 2] = g[:, 2, 1] = np.nan
        gd = torch.full((b, c, ld), GUARD, device="cuda")
        gd[:, :, :c] = torch.from_numpy(g).cuda()                                 # (broadcast over the batch when shared)
        sd, idd = torch.from_numpy(s).cuda(), torch.from_numpy(ids).cuda()
        for k in ks:
            for lam in LAMBDAS:
                got = [_np(t)[rows] for t in _mmr_rows(sd, idd, gd, k, lam, normalize)]
                want = mmr_batch_np(s[rows], ids[rows], g, k, lam, normalize)
                msg = (b, c, k, lam, normalize)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), msg
                assert same_bits(got[2], want[2]) and same_bits(got[3], want[3]), msg
    if c <= 65:       # the element-by-element restatement itself, on the last inputs
        for q in range(min(b, 3)):
            w = mmr_np(s[q], ids[q], g[q], ks[-1], 0.5, normalize)
            got = [_np(t)[q] for t in _mmr_rows(sd, idd, gd, ks[-1], 0.5, normalize)]
            assert np.array_equal(got[0], w[0]) and same_bits(got[3], w[3]), (b, c, q)


@pytest.mark.parametrize("c", [1, 2, 63, 64, 65, 255, 257, 1024])
def test_lambda_one_on_finite_rows_returns_the_first_k(gpu_device, c):
    import torch
    rng = np.random.default_rng(c)
    b = 5
    s = -np.sort(-rng.random((b, c)).astype(np.float32), axis=1)                 # a ranking's order; ties stay in slot order
    s[:, c // 2:c // 2 + 2] = s[:, c // 2:c // 2 + 1]
    ids = np.stack([rng.permutation(3 * c)[:c] for _ in range(b)]).astype(np.int32)
    g = torch.from_numpy(rng.standard_normal((b, c, c)).astype(np.float32)).cuda()
    for k in sorted({1, max(1, c // 2), c}):
        for normalize in (True, False):
            sel, idx, sc, _ = _mmr_rows(torch.from_numpy(s).cuda(), torch.from_numpy(ids).cuda(), g, k, 1.0, normalize)
            assert np.array_equal(_np(idx), ids[:, :k]) and np.array_equal(_np(sel), np.tile(np.arange(k), (b, 1)))
            assert same_bits(_np(sc), s[:, :k])


# ---------------------------------------------------------------------------------- the engine call
def _row_engine(kind, x, max_batch, max_topk=16):
    from hipporag_amd.engine import HippoRAGEngine
    from hipporag_amd.graph import build_csr
    rows = x.shape[0]
    g = build_csr(rows + 4, [0, 1], [1, 2], [1.0, 1.0])
    zeros = np.zeros(rows, np.int32)
    emb = x.cpu().numpy() if kind == "split" else x
    return HippoRAGEngine(g, np.arange(4, rows + 4, dtype=np.int32), emb, emb, zeros, zeros, np.zeros(rows + 4, np.int32),
                          max_batch=max_batch, max_topk=max_topk)


@pytest.mark.parametrize("kind", KINDS)
def test_engine_mmr_is_the_composition_of_the_two_seams(gpu_device, kind):
    import torch
    n, dim, b, c, k = 900, 200, 7, 130, 40
    x = _realistic_rows(n, dim, seed=11)
    emb, _, kdim, dt, _, _ = _operands(kind, x, x[:1])
    xs = x if kind == "split" else x.to(emb.dtype)
    rng = np.random.default_rng(5)
    ids = np.stack([rng.permutation(n)[:c] for _ in range(b)]).astype(np.int32)
    ids[rng.random((b, c)) < 0.05] = -1
    s = -np.sort(-rng.random((b, c)).astype(np.float32), axis=1)
    idd, sd = torch.from_numpy(ids).cuda(), torch.from_numpy(s).cuda()
    g, _ = _gram(emb, kdim, dt, kind == "split", idd, ld=c + (-c) % 4)
    with _row_engine(kind, xs, b) as eng:
        wk = eng.workspace()
        for lam, normalize in ((0.5, True), (0.2, False)):
            want = _mmr_rows(sd, idd, g, k, lam, normalize)
            for handle in (eng, wk):
                got = handle.mmr(idd, sd, k, lam, normalize)
                torch.cuda.synchronize()
                assert torch.equal(got[0], want[1]), (kind, lam)
                assert same_bits(_np(got[1]), _np(want[2])) and same_bits(_np(got[2]), _np(want[3])), (kind, lam)
        # an id >= n_passages is an empty slot of the engine call
        ids2 = ids.copy()
        ids2[:, 3] = n + 1
        got = eng.mmr(torch.from_numpy(ids2).cuda(), sd, k, 0.5)
        w = mmr_batch_np(s, ids2, _np(_gram(emb, kdim, dt, kind == "split", torch.from_numpy(ids2).cuda())[0]), k, 0.5, True, n)
        assert np.array_equal(_np(got[0]), w[1]) and same_bits(_np(got[2]), w[3])
        # more queries than max_batch: slices
        big = eng.mmr(idd.repeat(3, 1), sd.repeat(3, 1), k, 0.5)
        one = eng.mmr(idd, sd, k, 0.5, return_sel=True)
        assert torch.equal(big[0], one[0].repeat(3, 1)) and same_bits(_np(big[2]), _np(one[2].repeat(3, 1)))
        # the slots of the picks (hrag_mmr_sel) are the selection seam's
        assert torch.equal(one[3], _mmr_rows(sd, idd, g, k, 0.5, True)[0]) and torch.equal(one[0], eng.mmr(idd, sd, k, 0.5)[0])


@pytest.fixture(scope="module")
def case(gpu_device):
    from hipporag_amd.engine import HippoRAGEngine
    from tests.group_helpers import random_groups
    kg, pass_bits, fact_bits, _ = make_case(3000, 24000, 64, seed=4141)
    grp = random_groups(np.random.default_rng(2), kg.n_passages, "shuffled")
    eng = HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                         max_batch=130, max_topk=min(200, kg.n_passages))
    eng.set_passage_groups(grp)
    yield gpu_device, kg, pass_bits, fact_bits, eng, grp
    eng.close()


def _bf16(bits, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)


def _inputs(dev, eng, fact_bits, pass_bits, b, seed):
    import torch
    qf = _bf16(synth.make_queries_np(fact_bits, b, seed=seed)[0], dev)
    qp = _bf16(synth.make_queries_np(pass_bits, b, seed=seed + 1)[0], dev)
    idx, sc = eng.score_facts(qf, k=5)
    cnt = torch.full((b,), 5, dtype=torch.int32, device=dev)
    cnt[::4] = 0
    return qp, idx, sc, cnt


def _want_from_plain(pass_dev, dim, plain_idx, plain_score, k, lam, n_p):
    """mmr over a plain call's own top-c ids and scores and the device Gram -> (sel, idx, score, value)"""
    g, _ = _gram(pass_dev, dim, 0, False, plain_idx.contiguous())
    return mmr_batch_np(_np(plain_score), _np(plain_idx), _np(g), k, lam, True, n_p)


@pytest.mark.parametrize("b,want_state", [(4, 4), (40, 2), (130, 8)])
def test_retrieve_with_mmr_is_the_restatement_over_its_own_ranking(case, b, want_state):
    import torch
    dev, kg, pass_bits, fact_bits, eng, grp = case
    n_p, dim = kg.n_passages, pass_bits.shape[1]
    c, k = min(50, n_p), 10
    pass_dev = _bf16(pass_bits, dev).contiguous()
    qp, idx, sc, cnt = _inputs(dev, eng, fact_bits, pass_bits, b, 70 + b)
    before = eng.retrieve(qp, idx, sc, cnt, k=k)
    plain = eng.retrieve(qp, idx, sc, cnt, k=c)
    assert eng.stats()["last_ppr_state"] == want_state
    out = eng.retrieve(qp, idx, sc, cnt, k=k, mmr_lambda=0.5, mmr_candidates=c)
    torch.cuda.synchronize()
    w = _want_from_plain(pass_dev, dim, plain.doc_idx, plain.doc_score, k, 0.5, n_p)
    assert np.array_equal(_np(out.doc_idx), w[1]), b
    assert same_bits(_np(out.doc_score), w[2]) and same_bits(_np(out.mmr_value), w[3]), b
    assert torch.equal(out.flags, plain.flags)
    # without mmr_lambda: the call that never heard of it
    after = eng.retrieve(qp, idx, sc, cnt, k=k)
    assert after.mmr_value is None and torch.equal(after.doc_idx, before.doc_idx)
    assert same_bits(_np(after.doc_score), _np(before.doc_score)) and torch.equal(after.flags, before.flags)
    assert torch.equal(after.doc_idx, plain.doc_idx[:, :k])


def test_mmr_composes_with_filter_groups_fusion_and_dense(case):
    import torch
    dev, kg, pass_bits, fact_bits, eng, grp = case
    n_p, dim, b, c, k = kg.n_passages, pass_bits.shape[1], 12, 40, 8
    pass_dev = _bf16(pass_bits, dev).contiguous()
    qp, idx, sc, cnt = _inputs(dev, eng, fact_bits, pass_bits, b, 9)
    allowed = torch.from_numpy(np.arange(n_p) % 3 != 0).to(dev)
    # doc filter
    plain = eng.retrieve(qp, idx, sc, cnt, k=c, doc_filter=allowed)
    out = eng.retrieve(qp, idx, sc, cnt, k=k, doc_filter=allowed, mmr_lambda=0.3, mmr_candidates=c)
    w = _want_from_plain(pass_dev, dim, plain.doc_idx, plain.doc_score, k, 0.3, n_p)
    assert np.array_equal(_np(out.doc_idx), w[1]) and same_bits(_np(out.mmr_value), w[3])
    assert bool(allowed[out.doc_idx.long().clamp_min(0)].all())
    # groups: the candidates are the groups' best passages with the group scores; group_idx and the hits follow the picks
    plain = eng.retrieve(qp, idx, sc, cnt, k=c, group_agg="max")
    out = eng.retrieve(qp, idx, sc, cnt, k=k, group_agg="max", group_hits=2, mmr_lambda=0.5, mmr_candidates=c)
    w = _want_from_plain(pass_dev, dim, plain.doc_idx, plain.doc_score, k, 0.5, n_p)
    assert np.array_equal(_np(out.doc_idx), w[1]) and same_bits(_np(out.doc_score), w[2])
    want_groups = np.take_along_axis(_np(plain.group_idx), np.maximum(w[0], 0).astype(np.int64), axis=1)
    assert np.array_equal(_np(out.group_idx), np.where(w[0] >= 0, want_groups, -1))
    assert np.array_equal(_np(out.hit_idx)[:, :, 0], _np(out.doc_idx)) and out.hit_idx.shape == (b, k, 2)
    # fusion
    mp = [0, 3, 4, 12]
    eng.retrieve(qp, idx, sc, cnt, k=1)
    plain = eng.last_fused(mp, fuse="sum", k=c)
    eng.retrieve(qp, idx, sc, cnt, k=1)
    out = eng.last_fused(mp, fuse="sum", k=k, mmr_lambda=0.5, mmr_candidates=c)
    w = _want_from_plain(pass_dev, dim, plain.doc_idx, plain.doc_score, k, 0.5, n_p)
    assert np.array_equal(_np(out.doc_idx), w[1]) and same_bits(_np(out.mmr_value), w[3])
    # dense
    di, ds = eng.dense_retrieve(qp, k=c)
    gi, gs, gv = eng.dense_retrieve(qp, k=k, mmr_lambda=0.7, mmr_candidates=c)
    w = _want_from_plain(pass_dev, dim, di, ds, k, 0.7, n_p)
    assert np.array_equal(_np(gi), w[1]) and same_bits(_np(gs), w[2]) and same_bits(_np(gv), w[3])
    # more candidates than the engine ranks, and the python-side checks
    with pytest.raises(ValueError, match="mmr_candidates"):       # (named on the host, before anything is enqueued)
        eng.retrieve(qp, idx, sc, cnt, k=k, mmr_lambda=0.5, mmr_candidates=eng.max_topk + 1)
    with pytest.raises(ValueError, match="mmr_candidates"):
        eng.last_fused(mp, fuse="sum", k=k, mmr_lambda=0.5, mmr_candidates=eng.max_topk + 1)
    for kw in (dict(mmr_lambda=1.5), dict(mmr_lambda=float("nan")), dict(mmr_candidates=20), dict(mmr_lambda=0.5, mmr_candidates=2000)):
        with pytest.raises(ValueError):
            eng.retrieve(qp, idx, sc, cnt, k=k, **kw)
    from hipporag_amd.engine import CapturedPipeline
    with pytest.raises(ValueError, match="mmr_lambda"):
        CapturedPipeline(eng, 4, mmr_lambda=0.5)


def test_einval_cases_leave_the_outputs_untouched(case):
    import torch
    from hipporag_amd import dist
    L, lib = _L()
    dev, kg, pass_bits, fact_bits, eng, grp = case
    b, c, k = 4, 20, 5
    ids = torch.arange(b * c, dtype=torch.int32, device=dev).view(b, c) % kg.n_passages
    s = torch.rand((b, c), device=dev)
    need = int(lib.hrag_mmr_workspace_bytes(b, c))
    ws = torch.empty((need + 16,), dtype=torch.uint8, device=dev)
    oi = torch.full((b, k), 7, dtype=torch.int32, device=dev)
    os_, ov = (torch.full((b, k), 7.0, device=dev) for _ in range(2))

    def call(e=eng, ci=ids.data_ptr(), cs=s.data_ptr(), batch=b, c_=c, k_=k, lam=0.5, oi_=oi.data_ptr(), os__=os_.data_ptr(),
             ov_=ov.data_ptr(), wp=ws.data_ptr(), wb=need):
        return lib.hrag_mmr(e._handle, ci, cs, batch, c_, k_, lam, 1, oi_, os__, ov_, wp, wb, _stream())

    bad = [dict(c_=0), dict(c_=1025), dict(k_=0), dict(k_=c + 1), dict(lam=-0.01), dict(lam=1.01), dict(lam=float("nan")),
           dict(batch=0), dict(batch=eng.max_batch + 1), dict(ci=None), dict(cs=None), dict(oi_=None), dict(os__=None),
           dict(ov_=None), dict(wp=None), dict(wb=need - 1), dict(wp=ws.data_ptr() + 4)]
    for kw in bad:
        assert call(**kw) == L.HRAG_EINVAL, kw
        torch.cuda.synchronize()
        assert bool((oi == 7).all()) and bool((os_ == 7.0).all()) and bool((ov == 7.0).all()), kw
    sidx = dist.shard_index(kg.csr, kg.passage_vertex, 2, kg.subj_vertex, kg.obj_vertex, kg.num_chunks)
    sh = dist.build_shard_engine(sidx, pass_bits, fact_bits, 1, max_batch=8, max_topk=10)
    try:
        assert call(e=sh) == L.HRAG_EINVAL and b"row-shard" in lib.hrag_last_error()
    finally:
        sh.close()
    assert bool((oi == 7).all())
    assert call() == L.HRAG_OK                                                   # the good call still works
    torch.cuda.synchronize()
    assert bool((oi >= 0).all())
    # the engine-free seams
    g = torch.zeros((b, c, c), device=dev)
    e16 = _bf16(pass_bits, dev).contiguous()
    st = _stream()
    for args in ((None, 10, 64, 0, 0, ids.data_ptr(), b, c, g.data_ptr(), c), (e16.data_ptr(), 10, 60, 0, 0, ids.data_ptr(), b, c, g.data_ptr(), c),
                 (e16.data_ptr(), 10, 64, 2, 0, ids.data_ptr(), b, c, g.data_ptr(), c), (e16.data_ptr(), 10, 64, 1, 1, ids.data_ptr(), b, c, g.data_ptr(), c),
                 (e16.data_ptr(), 10, 64, 0, 0, ids.data_ptr(), b, 1025, g.data_ptr(), 1025), (e16.data_ptr(), 10, 64, 0, 0, ids.data_ptr(), b, c, g.data_ptr(), c - 1),
                 (e16.data_ptr(), 10, 64, 0, 0, ids.data_ptr(), 0, c, g.data_ptr(), c)):
        assert lib.hrag_gram_rows(*args, st) == L.HRAG_EINVAL, args
    for args in ((s.data_ptr(), ids.data_ptr(), g.data_ptr(), c, b, c, 0, 0.5), (s.data_ptr(), ids.data_ptr(), g.data_ptr(), c - 1, b, c, k, 0.5),
                 (s.data_ptr(), ids.data_ptr(), g.data_ptr(), c, b, c, k, 2.0), (s.data_ptr(), ids.data_ptr(), None, c, b, c, k, 0.5)):
        assert lib.hrag_mmr_rows(*args, 1, oi.data_ptr(), oi.data_ptr(), os_.data_ptr(), ov.data_ptr(), st) == L.HRAG_EINVAL, args
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------- planted duplicates
@pytest.mark.parametrize("kind", KINDS)
def test_planted_duplicates_one_pick_per_cluster(gpu_device, kind):
    import torch
    seeds = list(range(16))
    cases = [planted_corpus(s) for s in seeds]
    emb = np.concatenate([cs[0] for cs in cases])
    n1 = len(cases[0][0])
    x = torch.from_numpy(emb).cuda()
    xs = x if kind == "split" else x.to(torch.bfloat16 if kind == "bf16" else torch.float16)
    ids = torch.stack([torch.arange(n1, dtype=torch.int32) + i * n1 for i in range(len(seeds))]).cuda()
    score = torch.from_numpy(np.stack([cs[2] for cs in cases])).cuda()
    with _row_engine(kind, xs, len(seeds)) as eng:
        idx, sc, val = eng.mmr(ids, score, 8, 0.5)
        torch.cuda.synchronize()
    idx = _np(idx)
    for i, (_, cluster, _) in enumerate(cases):
        picks = cluster[idx[i] - i * n1]
        assert sorted(picks.tolist()) == list(range(8)), (kind, i, picks)
        assert len(set(cluster[:8].tolist())) == 2


def test_mirror_returns_no_two_copies_among_the_first_qa_top_k(gpu_device):
    """The toy corpus with four documents indexed twice (same words, same triples: cosine ~ 0.99, the same PPR mass).  The
    plain ranking puts the two copies side by side; with mmr_lambda = 0.5 a copy's value is 0.5 * (rel - 0.99) once its twin
    is picked, against 0.5 * (rel_o - cos_o) of an unrelated document with cos_o <= ~0.35 (one shared word of three): the
    copy comes after every document whose relevance is above rel - 0.64.  That holds for the copies of documents 0, 2, 4
    and 8, whose relevance stays below 0.6 for every query.  It does NOT hold for a copy of a query's single dominant hit on
    this corpus (relevance 0.99 against 0.05 for the rest): MMR at lambda 0.5 then returns the copy third, by its
    definition -- such a copy needs a smaller lambda."""
    from tests.golden.make_golden import DOCS, QUERIES, TRIPLES, MockEmbeddingModel
    from hipporag_amd import HippoRAG, RetrievalConfig
    dup = [0, 2, 4, 8]
    docs = list(DOCS) + [DOCS[i] + " ." for i in dup]                              # the same words: cosine ~ 0.99
    triples = list(TRIPLES) + [TRIPLES[i] for i in dup]
    origin = {d: (i if i < len(DOCS) else dup[i - len(DOCS)]) for i, d in enumerate(docs)}
    cfg = RetrievalConfig(embedding_precision="bf16", max_batch=4, ppr_iters=40, ppr_tol=0.0)
    rag = HippoRAG(cfg, embedding_model=MockEmbeddingModel())
    rag.index_from_openie(docs, triples)
    n, top = len(docs), cfg.qa_top_k
    plain = rag.retrieve(QUERIES, num_to_retrieve=n)
    mmr = rag.retrieve(QUERIES, num_to_retrieve=n, mmr_lambda=0.5)
    twice = 0
    for p, m in zip(plain, mmr):
        twice += len({origin[d] for d in p.docs[:top]}) < top
        assert len({origin[d] for d in m.docs[:top]}) == top, [origin[d] for d in m.docs[:top]]
        assert sorted(m.docs) == sorted(p.docs) and m.docs[0] == p.docs[0]
        score_of = dict(zip(p.docs, np.asarray(p.doc_scores, np.float32).view(np.uint32).tolist()))
        assert [score_of[d] for d in m.docs] == np.asarray(m.doc_scores, np.float32).view(np.uint32).tolist()
        assert all("mmr_value" in md for md in m.doc_metadata) and all("mmr_value" not in md for md in p.doc_metadata)
    assert twice == len(QUERIES), "the plain ranking puts two copies among its first qa_top_k of every query"
    # fewer documents than candidates, mmr_candidates not given: the candidates are retrieval_top_k entries (here: every
    # passage), so the reader's qa_top_k documents are the first picks of the full call, not a permutation of the plain top 5
    few = rag.retrieve(QUERIES, num_to_retrieve=top, mmr_lambda=0.5)
    for f, m in zip(few, mmr):
        assert f.docs == m.docs[:top] and len({origin[x] for x in f.docs}) == top
        assert [md["mmr_value"] for md in f.doc_metadata] == [md["mmr_value"] for md in m.doc_metadata[:top]]
    three = rag.retrieve(QUERIES, num_to_retrieve=top, mmr_lambda=0.5, mmr_candidates=3)     # below num_to_retrieve: top
    for t3, p in zip(three, plain):
        assert sorted(t3.docs) == sorted(p.docs[:top])
    for m, f in zip(rag.retrieve_dpr(QUERIES, num_to_retrieve=5, mmr_lambda=0.5), rag.retrieve_dpr(QUERIES, num_to_retrieve=n, mmr_lambda=0.5)):
        assert len({origin[x] for x in m.docs}) == 5 and "mmr_value" in m.doc_metadata[0] and m.docs == f.docs[:5]
    cfg_on = HippoRAG(RetrievalConfig(embedding_precision="bf16", max_batch=4, ppr_iters=40, ppr_tol=0.0, mmr_lambda=0.5),
                      embedding_model=MockEmbeddingModel())
    cfg_on.index_from_openie(docs, triples)
    for a, b in zip(cfg_on.retrieve(QUERIES, num_to_retrieve=top), mmr):
        assert a.docs == b.docs[:top]
    for call in (lambda: rag.retrieve_fused([[QUERIES[0]]], mmr_lambda=0.5), lambda: rag.retrieve_ircot(QUERIES[:1], 1, mmr_lambda=0.5),
                 lambda: cfg_on.retrieve_fused([[QUERIES[0]]]), lambda: rag.retrieve(QUERIES, mmr_candidates=5),
                 lambda: rag.retrieve(QUERIES, num_to_retrieve=3, mmr_lambda=0.5, mmr_candidates="all"),
                 lambda: rag.retrieve_dpr(QUERIES, num_to_retrieve=3, mmr_lambda=1.5)):
        with pytest.raises(ValueError, match="mmr_"):
            call()
