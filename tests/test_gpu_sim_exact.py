"""Every similarity path, in every embedding type, held to an fp64 dot product (tests/helpers.py sim_reference): bf16 and
fp16 rows compared with the fp64 product of the rounded vectors, the split engine (HRAG_F32_SPLIT, retrieve_knn's
"f32": fp16 halves in the layout [hi | lo | hi] x [qhi | qhi | qlo], kdim = 3 * dim) with the fp64 product of the
ORIGINAL fp32 vectors.

Two kinds of input:
  exact      dyadic values whose every product and partial sum is exact in fp32, whatever the summation order.  Split:
             hi = h 2^-3 (h in {-1, 0, 1}, at most 1024 non-zeros per row), lo = +-2^-16 where h != 0 -- halves known
             exactly -- and queries of the same kind, half of them with lo = 0 (fp16-exact: the dropped lo . qlo is 0,
             so the split chain IS x . q).  The only correct answer is the exact one: bit equality.  Catches a dropped or
             repeated k-chunk, a wrong tail, a swapped third of the layout, a wrong lane mapping.
  realistic  unit Gaussian rows, near-duplicate queries (cos ~ 0.999), rows of norm 1e-3 and 1e3, components spanning
             1e-8 ... 0.5.  Every pair within the derived bound (rounded_score_bound / split_score_bound); the split
             paths also pass the aggregate check (split_aggregate_check, RMS of the error in units of its modelled
             spread) on the unit-scale pairs.

Which kernel a shape reaches (csrc/sim_gemm.hip launch_sim_gemm; kdim = dim, or 3 * dim for the split):
  GEMV sim_gemv_kernel            B <= 2 and kdim <= 4096: chunks 1 / 2 / 4 / 8 for kdim <= 512 / 1024 / 2048 / 4096
                                  (split: dims 64 / 200 / 512 / 768); kdim > 4096 falls through to the 16-query tile
  sim_gemm_kernel<16>             B <= 16 (B <= 2 beyond kdim 4096), and every accumulate=1 call
  sim_gemm_kernel<64>             17 <= B <= 64
  sim_gemm_kernel<128>            B > 64 with kdim % 64 != 0 or rows < 256
  sim_gemm256_kernel<4 | 8>       B > 64, kdim % 64 == 0, rows >= 256 (BN 128 up to B = 128, 256 beyond)
The fused top-k (hrag_sim_topk; hrag_score_facts at B > 16, k <= 16): pass 1 on sim_gemm_kernel<64> (B <= 64),
sim_gemm_kernel<128> or sim_gemm256_kernel (tile maxima), tile_select_kernel in registers (<= 8192 tiles) or re-reading
memory, pass 3 per (tile, query) (tile_rescore_kernel) or grouped by tile (tile_rescore_grouped_kernel: tiles >= 64 and
B k >= 4 tiles).  The prefix first pass of hrag_sim_topk_min_score runs here on bf16 (the fp16 split one:
tests/test_gpu_knn.py).  The engine paths (sim_scores, score_facts, dense_retrieve) and a split engine at dim 4096 end to
end run the same kernels behind the C ABI."""

import numpy as np
import pytest

from tests.helpers import (
    assert_topk_equal, expected_topk, rounded_score_bound, sim_reference, split_aggregate_check, split_error_sigma,
    split_score_bound, tie_aware_equal, write_test_report,
)

pytestmark = pytest.mark.gpu

KINDS = ["bf16", "fp16", "split"]

# (rows, dim, B): every branch of launch_sim_gemm in every type (module docstring)
SHAPES = [
    (1000, 64, 1), (1000, 64, 2), (777, 200, 2), (600, 512, 1), (517, 768, 2), (300, 1536, 1), (257, 4096, 2),
    (333, 4608, 1),                                                           # GEMV chunks / beyond 4096
    (1029, 200, 3), (515, 768, 8), (300, 4096, 16),                           # 16-query tile
    (2000, 200, 17), (700, 1536, 64),                                         # 64-query tile
    (1000, 200, 70), (200, 768, 130),                                         # 128-query tile
    (256, 64, 65), (257, 768, 128), (4097, 128, 129), (1500, 64, 256), (700, 4096, 257),   # 256-row kernel
]


def _lib():
    from hipporag_amd import _lib as L
    return L, L.load()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _split(x, as_query):
    """hrag_split_f32(normalize = 0): fp32 [n, dim] -> fp16 [n, 3 dim]"""
    import torch
    L, lib = _lib()
    out = torch.empty((x.shape[0], 3 * x.shape[1]), dtype=torch.float16, device=x.device)
    L.check(lib.hrag_split_f32(x.data_ptr(), x.shape[0], x.shape[1], 1 if as_query else 0, 0, out.data_ptr(), _stream()))
    return out


def _operands(kind, x, q):
    """fp32 device vectors -> (emb, qq, kdim, dtype code, what the scores are compared with: x_ref, q_ref)"""
    import torch
    if kind == "split":
        return _split(x, False), _split(q, True), 3 * x.shape[1], 1, x, q
    t = torch.bfloat16 if kind == "bf16" else torch.float16
    e, qq = x.to(t).contiguous(), q.to(t).contiguous()
    return e, qq, x.shape[1], 0 if kind == "bf16" else 1, e.float(), qq.float()


def _sim_gemm(emb, qq, kdim, dtype, out, accumulate=0):
    L, lib = _lib()
    rows, b = emb.shape[0], qq.shape[0]
    L.check(lib.hrag_sim_gemm(emb.data_ptr(), rows, kdim, qq.data_ptr(), b, out.data_ptr(), out.shape[1], accumulate,
                              dtype, _stream()))
    return out


def _exact_inputs(kind, rows, dim, b, seed):
    """-> (x, q, want): want = the exact scores (fp64), equal to the fp64 product of the original vectors when the
    query's lo is zero and, for the split queries with lo, to the split chain hi.qhi + lo.qhi + hi.qlo"""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    if kind != "split":
        x = torch.randint(-3, 4, (rows, dim), generator=g, device="cuda").float() * 2.0 ** -3
        q = torch.randint(-3, 4, (b, dim), generator=g, device="cuda").float() * 2.0 ** -3
        return x, q, sim_reference(x, q)

    def halves(n, with_lo):
        nnz = min(dim // 2, 1024)
        keep = torch.rand((n, dim), generator=g, device="cuda").argsort(1) < nnz      # nnz random positions per row
        h = (torch.randint(0, 2, (n, dim), generator=g, device="cuda") * 2 - 1).float() * keep
        lo = (torch.randint(0, 2, (n, dim), generator=g, device="cuda") * 2 - 1).float() * keep * 2.0 ** -16
        lo = lo * with_lo[:, None]
        return h * 2.0 ** -3, lo

    hi, lo = halves(rows, torch.ones(rows, device="cuda"))
    qhi, qlo = halves(b, (torch.arange(b, device="cuda") % 2).float())            # odd queries carry a lo half
    want = sim_reference(hi, qhi) + sim_reference(lo, qhi) + sim_reference(hi, qlo)
    x, q = hi + lo, qhi + qlo
    assert torch.equal(want[::2], sim_reference(x, q)[::2])                     # qlo = 0: the chain is x . q
    return x, q, want


def _unit(x):
    return x / x.norm(dim=1, keepdim=True)


def _realistic_inputs(rows, dim, b, seed):
    """-> (x, q, unit_rows, unit_queries): unit Gaussian rows, then (at least 1/8 each) rows of norm 1e-3, 1e3 and rows
    whose components span 1e-8 ... 0.5; queries: near-duplicates of rows (cos ~ 0.999), unrelated unit vectors, and
    one query of each odd kind.  unit_rows / unit_queries: how many leading rows / queries are unit-scale."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = _unit(torch.randn((rows, dim), generator=g, device="cuda", dtype=torch.float64))
    n_odd = rows // 8
    nu = rows - 3 * n_odd
    if n_odd:
        x[nu:nu + n_odd] *= 1e-3
        x[nu + n_odd:nu + 2 * n_odd] *= 1e3
        span = torch.exp(torch.empty((n_odd, dim), device="cuda", dtype=torch.float64).uniform_(np.log(1e-8), np.log(0.5), generator=g))
        x[nu + 2 * n_odd:] = span * torch.sign(torch.randn((n_odd, dim), generator=g, device="cuda", dtype=torch.float64))
    n_dup = max(1, b // 2)
    src = torch.randint(0, nu, (n_dup,), generator=g, device="cuda")
    qd = _unit(x[src] + 0.045 * _unit(torch.randn((n_dup, dim), generator=g, device="cuda", dtype=torch.float64)))
    qs = [qd, _unit(torch.randn((b - n_dup, dim), generator=g, device="cuda", dtype=torch.float64))]
    q = torch.cat(qs)
    nq = b
    if b >= 8 and n_odd:
        q[-3:] = x[nu:nu + 3 * n_odd:n_odd]                                      # one small, one large, one wide-range
        nq = b - 3
    return x.float().contiguous(), q.float().contiguous(), nu, nq


def _bound(kind, x_ref, q_ref, kdim):
    return split_score_bound(x_ref, q_ref) if kind == "split" else rounded_score_bound(x_ref, q_ref, kdim)


def _check_realistic(kind, got, x_ref, q_ref, kdim, nu, nq, label):
    """every pair within the bound; split: the aggregate check on the unit-scale pairs (at most 64 x 1024 of them)"""
    want = sim_reference(x_ref, q_ref)
    err = got.double() - want
    bound = _bound(kind, x_ref, q_ref, kdim)
    ratio = float((err.abs() / bound).max())
    assert ratio <= 1.0, (label, ratio, float(err.abs().max()))
    rec = {"max_err": float(err.abs().max()), "max_err_over_bound": ratio}
    if kind == "split":
        bq, br = min(nq, 64), min(nu, 1024)
        sigma = split_error_sigma(x_ref[:br], q_ref[:bq])
        ok, stats = split_aggregate_check(err[:bq, :br].cpu().numpy(), sigma.cpu().numpy())
        rec.update(stats)
        assert ok, (label, stats)
    return rec


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,dim,b", SHAPES)
def test_sim_gemm_exact_inputs_are_exact(gpu_device, kind, rows, dim, b):
    """hrag_sim_gemm, plain and accumulate=1 (into dyadic values already in the buffer, NaN padding beyond `rows`)"""
    import torch
    x, q, want = _exact_inputs(kind, rows, dim, b, seed=rows * 7 + dim + b)
    emb, qq, kdim, dt, _, _ = _operands(kind, x, q)
    ld = rows + 3
    out = torch.full((b, ld), float("nan"), device="cuda")
    _sim_gemm(emb, qq, kdim, dt, out)
    g = torch.Generator(device="cuda")
    g.manual_seed(rows)
    pre = torch.full((b, ld), float("nan"), device="cuda")
    pre[:, :rows] = torch.randint(-64, 65, (b, rows), generator=g, device="cuda").float() * 2.0 ** -10
    pre0 = pre.clone()
    _sim_gemm(emb, qq, kdim, dt, pre, accumulate=1)
    torch.cuda.synchronize()
    assert torch.equal(out[:, :rows].double(), want), (kind, float((out[:, :rows].double() - want).abs().max()))
    assert torch.isnan(out[:, rows:]).all()
    assert torch.equal(pre[:, :rows].double(), want + pre0[:, :rows].double())
    assert torch.isnan(pre[:, rows:]).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,dim,b", SHAPES)
def test_sim_gemm_realistic_inputs_within_the_bound(gpu_device, kind, rows, dim, b):
    import torch
    x, q, nu, nq = _realistic_inputs(rows, dim, b, seed=rows + 13 * dim + b)
    emb, qq, kdim, dt, x_ref, q_ref = _operands(kind, x, q)
    out = torch.empty((b, rows + (-rows) % 4), device="cuda")
    _sim_gemm(emb, qq, kdim, dt, out)
    torch.cuda.synchronize()
    rec = _check_realistic(kind, out[:, :rows], x_ref, q_ref, kdim, nu, nq, (kind, rows, dim, b))
    if kind == "split":
        write_test_report(f"sim_exact_split_{rows}_{dim}_{b}", rec)


# ----------------------------------------------------------------------------- the fused top-k (hrag_sim_topk)
def _sim_topk(emb, qq, kdim, dt, k, approx_dim=None, min_score=0.0, margin=0.0):
    import torch
    L, lib = _lib()
    rows, b = emb.shape[0], qq.shape[0]
    nbytes = int(lib.hrag_sim_topk_workspace_bytes(rows, b))
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device="cuda")
    idx = torch.empty((b, k), dtype=torch.int32, device="cuda")
    val = torch.empty((b, k), dtype=torch.float32, device="cuda")
    if approx_dim is None:
        L.check(lib.hrag_sim_topk(emb.data_ptr(), rows, kdim, qq.data_ptr(), b, k, dt, ws.data_ptr(), nbytes,
                                  idx.data_ptr(), val.data_ptr(), _stream()))
        return idx, val
    over = torch.empty((b,), dtype=torch.int32, device="cuda")
    L.check(lib.hrag_sim_topk_min_score(emb.data_ptr(), rows, kdim, qq.data_ptr(), b, k, dt, approx_dim, min_score,
                                        margin, ws.data_ptr(), nbytes, idx.data_ptr(), val.data_ptr(), over.data_ptr(),
                                        _stream()))
    return idx, val, over


def _expected_topk_dev(s, k):
    """expected_topk's ranking (score desc, ties: larger index first) on the device, for rows without NaN"""
    import torch
    n = s.shape[1]
    v, j = torch.sort(s.flip(1), dim=1, descending=True, stable=True)
    return (n - 1 - j[:, :k]).int(), v[:, :k]


# (rows, dim, b, k): pass 1 on the 64-query tile + per-pair rescore; 256-row kernel + grouped; 128-query tile + per-pair;
# 128-query tile + grouped; > 8192 tiles (selection re-reads memory)
FUSED = [(5000, 768, 40, 16), (9000, 64, 300, 16), (6000, 200, 70, 5), (20000, 200, 300, 16), (1_100_000, 32, 66, 5)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,dim,b,k", FUSED)
def test_sim_topk_exact_inputs_match_the_exact_ranking(gpu_device, kind, rows, dim, b, k):
    import torch
    x, q, want = _exact_inputs(kind, rows, dim, b, seed=rows + dim + b + k)
    emb, qq, kdim, dt, _, _ = _operands(kind, x, q)
    del x
    idx, val = _sim_topk(emb, qq, kdim, dt, k)
    w_idx, w_val = _expected_topk_dev(want.float(), k)
    torch.cuda.synchronize()
    assert torch.equal(idx, w_idx), (kind, int((idx != w_idx).sum()))
    assert torch.equal(val, w_val)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,dim,b,k", FUSED[:4])
def test_sim_topk_realistic_inputs(gpu_device, kind, rows, dim, b, k):
    """returned scores within the bound of fp64; nothing clearly better than the k-th returned row is missing"""
    import torch
    x, q, nu, nq = _realistic_inputs(rows, dim, b, seed=rows + dim + b + k + 1)
    emb, qq, kdim, dt, x_ref, q_ref = _operands(kind, x, q)
    idx, val = _sim_topk(emb, qq, kdim, dt, k)
    want = sim_reference(x_ref, q_ref)
    bound = _bound(kind, x_ref, q_ref, kdim)
    il = idx.long()
    assert (idx >= 0).all()
    got64 = torch.gather(want, 1, il)
    assert bool(((val.double() - got64).abs() <= torch.gather(bound, 1, il)).all()), kind
    # a row outside the result whose fp64 score beats a returned one by both their bounds is a miss
    strict = (want - bound) > torch.gather(want + bound, 1, il).min(1).values[:, None]
    strict.scatter_(1, il, False)
    assert not bool(strict.any()), (kind, int(strict.sum()))


def test_sim_topk_min_score_prefix_pass_bf16(gpu_device):
    """hrag_sim_topk_min_score with a prefix first pass on bf16 rows (256-row kernel over the first half of every row,
    row stride = dim): the queries are zero in the second half, so the prefix IS the product and the result must equal
    the plain fused top-k wherever it reaches the threshold"""
    import torch
    rows, dim, b, k = 9000, 128, 300, 16
    x, q, _ = _exact_inputs("bf16", rows, dim, b, seed=3)
    q[:, dim // 2:] = 0
    emb, qq = x.bfloat16().contiguous(), q.bfloat16().contiguous()
    want = sim_reference(emb.float(), qq.float()).float()
    thr = float(torch.topk(want, 8, dim=1).values[:, 7].median()) + 2.0 ** -7      # about half the queries: < 8 rows above
    idx, val, over = _sim_topk(emb, qq, dim, 0, k, approx_dim=dim // 2, min_score=thr, margin=2.0 ** -20)
    w_idx, w_val = _expected_topk_dev(want, k)
    torch.cuda.synchronize()
    for r in range(b):
        n = int((w_val[r] >= thr).sum())
        if over[r] == 0 and (n < k):
            assert torch.equal(idx[r, :n], w_idx[r, :n]) and torch.equal(val[r, :n], w_val[r, :n]), r
            assert (val[r, n:][idx[r, n:] >= 0] < thr).all()
    assert int((over == 0).sum()) > b // 4


# ----------------------------------------------------------------------------- engine entry points
def _engine(kind, x, rows_f):
    """an engine whose facts AND passages are x (bf16 / fp16 device tensors, or fp32 numpy for the split)"""
    from hipporag_amd.engine import HippoRAGEngine
    from hipporag_amd.graph import build_csr
    rows = x.shape[0]
    g = build_csr(rows + 4, [0, 1], [1, 2], [1.0, 1.0])
    zeros = np.zeros(rows, np.int32)
    emb = x.cpu().numpy() if kind == "split" else x
    return HippoRAGEngine(g, np.arange(4, rows + 4, dtype=np.int32), emb, emb, zeros, zeros, np.zeros(rows + 4, np.int32),
                          max_batch=rows_f, max_topk=16)


ENGINE_SHAPES = [(1000, 64, 1), (517, 768, 2), (257, 4096, 2), (515, 768, 8), (2000, 200, 17), (1000, 200, 70),
                 (9000, 64, 300), (700, 1536, 64)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,dim,b", ENGINE_SHAPES)
def test_engine_paths_exact(gpu_device, kind, rows, dim, b):
    """sim_scores (facts, passages), score_facts (fused at B > 16) and dense_retrieve: exact scores, and ids and min-max
    normalised scores identical to expected_topk of the exact scores"""
    import torch
    x, q, want = _exact_inputs(kind, rows, dim, b, seed=rows + dim * 3 + b)
    xs = x if kind == "split" else x.to(torch.bfloat16 if kind == "bf16" else torch.float16)
    qs = q if kind == "split" else q.to(xs.dtype)
    with _engine(kind, xs, b) as eng:
        for which in ("facts", "passages"):
            s = eng.sim_scores(which, qs)
            torch.cuda.synchronize()
            assert torch.equal(s.double(), want), (kind, which)
        w = expected_topk(want.float().cpu().numpy(), 16)
        for fn in (eng.score_facts, eng.dense_retrieve):
            idx, sc = fn(qs, k=16)
            torch.cuda.synchronize()
            assert_topk_equal((idx.cpu().numpy(), sc.cpu().numpy(), None, None), (w[0], w[2], None, None),
                              f"{kind} {fn.__name__}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,dim,b", ENGINE_SHAPES)
def test_engine_paths_realistic(gpu_device, kind, rows, dim, b):
    import torch
    x, q, nu, nq = _realistic_inputs(rows, dim, b, seed=rows + dim * 5 + b)
    xs = x if kind == "split" else x.to(torch.bfloat16 if kind == "bf16" else torch.float16)
    qs = q if kind == "split" else q.to(xs.dtype)
    x_ref, q_ref = xs.float(), qs.float()
    kdim = 3 * dim if kind == "split" else dim
    want = sim_reference(x_ref, q_ref)
    bound = _bound(kind, x_ref, q_ref, kdim)
    with _engine(kind, xs, b) as eng:
        s = eng.sim_scores("passages", qs)
        torch.cuda.synchronize()
        _check_realistic(kind, s, x_ref, q_ref, kdim, nu, nq, (kind, rows, dim, b))
        idx, _ = eng.score_facts(qs, k=16)
        idx = idx.cpu().numpy()
    want_h, bound_h = want.cpu().numpy(), bound.cpu().numpy()
    for r in range(b):
        order = np.argsort(want_h[r], kind="stable")[::-1][:16]
        gap = 2 * float(bound_h[r][order].max())
        assert tie_aware_equal(idx[r], order, want_h[r][order], rel_gap=0, abs_gap=gap), (kind, r)


# ----------------------------------------------------------------------------- a split engine at dim 4096, end to end
@pytest.mark.parametrize("b", [2, 40, 130])
def test_split_engine_dim_4096_end_to_end(gpu_device, b):
    """The default engine (embedding_precision "f32") at the reference's default model width (NV-Embed-v2: 4096, kdim
    12288): raw fact scores within the split bound of the fp64 product of the fp32 vectors, phase A + B against the
    oracle run on those fp32 vectors, with the assertions of test_gpu_parity.py test_fp16_embeddings_end_to_end"""
    import torch
    import oracle
    from hipporag_amd.engine import HippoRAGEngine
    from tests.helpers import make_case
    dim = 4096
    kg, pass_bits, fact_bits, index = make_case(2000, 16000, 64, seed=77)
    rng = np.random.default_rng(b)

    def vecs(n):
        v = rng.standard_normal((n, dim)).astype(np.float32)
        return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)

    pas, fac = vecs(pass_bits.shape[0]), vecs(fact_bits.shape[0])
    index.passage_emb, index.fact_emb = pas, fac

    def near(m, n):
        v = m[rng.integers(0, len(m), n)] + 0.05 * vecs(n)
        return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)

    qf, qp = near(fac, b), near(pas, b)
    with HippoRAGEngine(kg.csr, kg.passage_vertex, pas, fac, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                        max_batch=b, max_topk=50) as eng:
        tq = torch.from_numpy(qf).to(gpu_device)
        raw = eng.sim_scores("facts", tq)
        idx, sc = eng.score_facts(tq, k=5)
        cnt = torch.full((b,), 5, dtype=torch.int32, device=gpu_device)
        out = eng.retrieve(torch.from_numpy(qp).to(gpu_device), idx, sc, cnt, ppr_iters=20, k=50)
        got_idx, got_sc = out.doc_idx.cpu().numpy(), out.doc_score.cpu().numpy()
        idx_h = idx.cpu().numpy()
    xf, qt = torch.from_numpy(fac).to(gpu_device), tq
    err = (raw.double() - sim_reference(xf, qt)).abs()
    assert bool((err <= split_score_bound(xf, qt)).all()), float(err.max())
    for q in range(b):
        ref = oracle.retrieve_one(index, qf[q], qp[q])
        assert tie_aware_equal(idx_h[q], np.array(ref.fact_candidates), ref.fact_candidate_scores, abs_gap=2e-6), q
        assert tie_aware_equal(got_idx[q], ref.sorted_doc_ids[:50], ref.sorted_doc_scores[:50], rel_gap=2e-5), q
        w = ref.x[kg.passage_vertex][got_idx[q]]
        assert (np.abs(got_sc[q] - w) / w).max() < 1e-5, q
