"""Every device path of the row ranking held to one numpy reference (tests/helpers.py expected_topk:
np.argsort(x, kind="stable")[::-1], every NaN first, ties by the larger index): indices, raw and min-max normalised
scores, row min / max, exactly.

  path 1  row_topk_kernel, one workgroup per row (hrag_topk_rows), its overflow refinement included;
  path 2  the same kernel split over several workgroups + topk_merge_kernel (engines at batch < 64 on rows >= 32768:
          hrag_score_facts, hrag_dense_retrieve);
  path 4  the fused tile-max / tile-select / rescore top-k (hrag_score_facts at batch > 16 with k <= 16, hrag_sim_topk);
  path 5  the KNN's dense path (k = 2047 through path 1's overflow refinement).

Paths 2 and 4 get their scores fully controlled: a bf16 engine and one-hot queries q = e_c make every score exactly
emb[:, c] (the other products are exact zeros), and a NaN anywhere in an embedding row makes that row's score NaN for
every query -- checked against hrag_sim_scores before anything is ranked."""

import numpy as np
import pytest

from tests.helpers import assert_topk_equal, expected_topk

pytestmark = pytest.mark.gpu

# NaNs of both signs, quiet and signalling, several payloads
_NANS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FC12345, 0xFF812345],
                 np.uint32).view(np.float32)
_SUB = np.array([1, 2, 0x7FFFFF, 0x400000], np.uint32).view(np.float32)
_FI = np.finfo(np.float32)
_SPECIAL = np.concatenate([np.array([0.0, -0.0], np.float32), _SUB, -_SUB,
                           np.array([_FI.tiny, -_FI.tiny, _FI.max, -_FI.max, np.inf, -np.inf, 1.0, -1.0], np.float32),
                           _NANS])


def _put(x, at, values):
    x[at] = values[np.arange(len(at)) % len(values)]


def _rows(n, seed):
    """8 rows of length n: random, all equal, few distinct values, every float class, a few NaNs, more NaNs than 2048
    (mixed signs and payloads) with +-inf, ascending with NaNs, all NaN"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((8, n)).astype(np.float32)
    if n == 0:
        return x
    x[1] = np.float32(0.25)
    x[2] = rng.choice(np.array([-1.5, 0.0, -0.0, 0.5, 3.0], np.float32), n)
    _put(x[3], np.flatnonzero(rng.random(n) < 0.6), _SPECIAL[rng.permutation(len(_SPECIAL))])
    _put(x[4], rng.choice(n, min(n, 5), replace=False), _NANS)
    _put(x[5], rng.choice(n, n // 50, replace=False), np.array([np.inf, -np.inf], np.float32))
    _put(x[5], rng.choice(n, max(1, n // 40), replace=False), _NANS)
    x[6] = np.sort(x[6])
    _put(x[6], rng.choice(n, max(1, n // 100), replace=False), _NANS[::-1])
    _put(x[7], np.arange(n), _NANS)
    return x


def _on_device(x, ld, misalign, fill):
    """x [b, n] in a device buffer with row stride ld (ld - n floats of padding after every row), the first row starting
    `misalign` floats in; padding and the misalignment gap hold `fill`, so a read past n shows up in the ranking"""
    import torch
    b, n = x.shape
    buf = torch.full((misalign + b * ld + 4,), fill, dtype=torch.float32, device="cuda")
    buf[misalign:misalign + b * ld].view(b, ld)[:, :n].copy_(torch.from_numpy(x))
    return buf, buf.data_ptr() + 4 * misalign


def _topk_rows(ptr, b, n, ld, k, idx_offset, normalize):
    import torch
    from hipporag_amd import _lib
    lib = _lib.load()
    idx = torch.empty((b, k), dtype=torch.int32, device="cuda")
    val = torch.empty((b, k), dtype=torch.float32, device="cuda")
    mn = torch.empty((b,), dtype=torch.float32, device="cuda")
    mx = torch.empty((b,), dtype=torch.float32, device="cuda")
    _lib.check(lib.hrag_topk_rows(ptr, b, n, ld, k, idx_offset, normalize, idx.data_ptr(), val.data_ptr(),
                                  mn.data_ptr(), mx.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return idx.cpu().numpy(), val.cpu().numpy(), mn.cpu().numpy(), mx.cpu().numpy()


def _check_path1(x, ks, *, pad, misalign, fill, idx_offset):
    b, n = x.shape
    buf, ptr = _on_device(x, n + pad, misalign, fill)
    for k in ks:
        want = expected_topk(x, k, idx_offset)
        for normalize in (0, 1):
            got = _topk_rows(ptr, b, n, n + pad, k, idx_offset, normalize)
            assert_topk_equal(got, (want[0], want[2 if normalize else 1], want[3], want[4]),
                              f"n={n} k={k} norm={normalize} pad={pad} misalign={misalign} fill={fill}")
    del buf


# (pad, misalign, fill, idx_offset): the row stride padding and the gap before row 0 hold NaN or +inf
_LAYOUTS = [(0, 0, float("nan"), 0), (3, 1, float("nan"), 1000), (1, 2, float("inf"), 7), (5, 3, float("inf"), 0)]
_KS = [1, 2, 16, 200, 512, 513, 2047, 2048]


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4096, 4097, 32767])
def test_path1_topk_rows_short_rows(gpu_device, n):
    x = _rows(n, seed=n)
    for pad, misalign, fill, off in _LAYOUTS:
        _check_path1(x, _KS, pad=pad, misalign=misalign, fill=fill, idx_offset=off)


@pytest.mark.parametrize("layout", [0, 3])
def test_path1_topk_rows_300001(gpu_device, layout):
    """k near 2048 on 300 001 keys overflows the candidate buffer on every row: the refinement, NaN rows included"""
    pad, misalign, fill, off = _LAYOUTS[layout]
    _check_path1(_rows(300_001, seed=5 + layout), _KS, pad=pad, misalign=misalign, fill=fill, idx_offset=off)


@pytest.mark.parametrize("misalign", [0, 3])
def test_path1_overflow_placement_with_nans(gpu_device, misalign):
    """test_gpu_parity.py test_topk_rows_adversarial_overflow_path's placement -- every large value in the slice that
    one thread's float4 stride scans, so the thread-local maxima give a useless bound -- with NaNs planted in the same
    slice (row 0), spread over the row (row 1), and outnumbering k (row 2)"""
    n = 1 << 18
    rng = np.random.default_rng(misalign)
    x = rng.random((3, n)).astype(np.float32)
    hot = np.arange(0, n, 4096)
    for r in range(3):
        x[r, hot] += 10.0
        x[r, hot + 1] += 10.0
    _put(x[0], hot[::7] + 2, _NANS)
    _put(x[1], rng.choice(n, 40, replace=False), _NANS)
    _put(x[2], np.concatenate([hot + 2, hot + 3, rng.choice(n, 2100, replace=False)]), _NANS)
    _check_path1(x, [1, 200, 513, 2047, 2048], pad=0, misalign=misalign, fill=float("nan"), idx_offset=0)
    _check_path1(x[:, :n - 7], [200, 2047], pad=4, misalign=misalign, fill=float("inf"), idx_offset=3)


# ----------------------------------------------------------------------------- one-hot engines (paths 2 and 4)
_DIM = 64
_BF16_NANS = np.array([0x7FC0, 0xFFC0, 0x7F81, 0xFF81, 0x7FFF, 0xFFFF], np.uint16)


def _bf16_bits(x):
    """float32 values that are exact in bf16 -> their bf16 bit patterns"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    assert np.all(u & 0xFFFF == 0)
    return (u >> 16).astype(np.uint16)


def _bf16_round(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + 0x8000) & 0xFFFF0000).view(np.float32)


def _one_hot_matrix(rows, cols, nan_rows):
    """[rows, _DIM] bf16 bits: column c holds cols[c] (float32 values exact in bf16), the others zero; the rows in
    nan_rows carry a NaN in the last column, which makes every score of that row NaN"""
    e = np.zeros((rows, _DIM), np.uint16)
    for c, v in enumerate(cols):
        e[:, c] = _bf16_bits(v)
    _put(e[:, _DIM - 1], np.asarray(nan_rows), _BF16_NANS)
    return e


def _queries(cols_of_queries):
    import torch
    q = np.zeros((len(cols_of_queries), _DIM), np.uint16)
    q[np.arange(len(cols_of_queries)), cols_of_queries] = 0x3F80          # bf16 1.0
    return torch.from_numpy(q.view(np.int16)).cuda().view(torch.bfloat16)


def _expected_scores(cols, nan_rows, cols_of_queries):
    s = np.stack([cols[c] for c in cols_of_queries]).astype(np.float32)
    s[:, np.asarray(nan_rows)] = np.float32(np.nan)
    return s


def _check_scores_assumption(eng, which, cols, nan_rows, cols_of_queries):
    """hrag_sim_scores of the one-hot queries IS the constructed matrix (NaN where planted, the values bit for bit)"""
    got = eng.sim_scores(which, _queries(cols_of_queries)).cpu().numpy()
    want = _expected_scores(cols, nan_rows, cols_of_queries)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(got[ok].view(np.uint32), (want[ok] + np.float32(0)).view(np.uint32), err_msg=which)
    return want


def _split_cols(n, seed):
    """score columns for the split path (exact in bf16): heavy ties, all equal, few distinct, hot entries packed into
    the first part, hot entries packed into the last (short) part, ascending"""
    rng = np.random.default_rng(seed)
    base = _bf16_round(rng.random(n).astype(np.float32) * 0.5)
    hot_first = np.full(n, np.float32(0.125))
    hot_first[100:100 + 3000] = _bf16_round(0.75 + 0.1 * rng.random(3000).astype(np.float32))
    hot_last = np.full(n, np.float32(-0.5))
    hot_last[n - 2500:] = _bf16_round(0.5 + 0.2 * rng.random(2500).astype(np.float32))
    return [base,
            np.full(n, np.float32(0.5)),
            rng.choice(np.array([-1.0, 0.0, 0.25, 2.0], np.float32), n),
            hot_first,
            hot_last,
            _bf16_round(np.linspace(-1, 1, n).astype(np.float32))]


def _empty_graph(v):
    from hipporag_amd.graph import build_csr
    return build_csr(v, [0, 1], [1, 2], [1.0, 1.0])


@pytest.fixture(scope="module", params=[(65537, 98307), (32770, 32769)], ids=["F65537-P98307", "F32770-P32769"])
def split_engine(request, gpu_device):
    from hipporag_amd.engine import HippoRAGEngine
    F, P = request.param
    fcols, pcols = _split_cols(F, 1), _split_cols(P, 2)
    # NaN rows: a few in the first part, a run of 40 (more than small k, fewer than large k) in the last, short part
    fnan = np.concatenate([[0, 1, 7, 9000], np.arange(F - 40, F)])
    pnan = np.concatenate([[3, 4, 20000], np.arange(P - 43, P - 3)])
    fe, pe = _one_hot_matrix(F, fcols, fnan), _one_hot_matrix(P, pcols, pnan)
    zeros = np.zeros(F, np.int32)
    eng = HippoRAGEngine(_empty_graph(P), np.arange(P, dtype=np.int32), pe, fe, zeros, zeros, np.zeros(P, np.int32),
                         max_batch=63, max_topk=2048)
    yield dict(eng=eng, fcols=fcols, pcols=pcols, fnan=fnan, pnan=pnan)
    eng.close()


def _cols_for(b, ncols):
    return [i % ncols for i in range(b)]


@pytest.mark.parametrize("b,ks", [(1, [1, 5, 200, 512, 513, 2048]), (16, [1, 16, 200, 512, 513, 2048]),
                                  (17, [17, 512, 513, 2047]), (63, [17, 200, 2048])])
def test_path2_score_facts_split(split_engine, b, ks):
    import torch
    e = split_engine
    cq = _cols_for(b, len(e["fcols"]))
    s = _check_scores_assumption(e["eng"], "facts", e["fcols"], e["fnan"], cq)
    q = _queries(cq)
    for k in ks:
        idx, sc = e["eng"].score_facts(q, k=k)
        torch.cuda.synchronize()
        want = expected_topk(s, k)
        assert_topk_equal((idx.cpu().numpy(), sc.cpu().numpy(), None, None), (want[0], want[2], None, None),
                          f"b={b} k={k}")


@pytest.mark.parametrize("b,ks", [(1, [1, 200, 512, 513, 2048]), (3, [5, 512, 513]), (40, [16, 513, 2047]),
                                  (63, [200, 2048])])
def test_path2_dense_retrieve_split(split_engine, b, ks):
    import torch
    e = split_engine
    cq = _cols_for(b, len(e["pcols"]))
    s = _check_scores_assumption(e["eng"], "passages", e["pcols"], e["pnan"], cq)
    q = _queries(cq)
    for k in ks:
        idx, sc = e["eng"].dense_retrieve(q, k=k)
        torch.cuda.synchronize()
        want = expected_topk(s, k)
        assert_topk_equal((idx.cpu().numpy(), sc.cpu().numpy(), None, None), (want[0], want[2], None, None),
                          f"b={b} k={k}")


# ----------------------------------------------------------------------------- path 4: the fused tile top-k
_F4 = 64 * 128 + 45           # 64 full 128-row tiles + 45 rows: pass 3 grouped by tile at wide batches, per pair below


def _fused_cols(n, seed):
    """score columns for the fused path: NaN rows sit in tiles whose other entries are LOW in every column but the last
    one (a tile max that skips NaN never selects them); exact ties across the tile boundary at 128 and at the last
    full tile / partial tile boundary; all equal; random"""
    rng = np.random.default_rng(seed)
    low_tiles = np.zeros(n, bool)
    for t in (7, 20, n // 128):                              # the tiles of the NaN rows below
        low_tiles[t * 128:(t + 1) * 128] = True
    mid = _bf16_round(0.25 + 0.5 * rng.random(n).astype(np.float32))
    mid[low_tiles] = np.float32(-0.75)
    ties = mid.copy()
    ties[120:136] = np.float32(0.875)                        # 16 exact ties spanning tiles 0 and 1
    last = n // 128 * 128
    ties[last - 6:last + 6] = np.float32(0.875)              # ... and the last full tile / the partial tile
    equal = np.full(n, np.float32(0.5))
    equal[low_tiles] = np.float32(-0.75)
    rand = _bf16_round(rng.standard_normal(n).astype(np.float32))
    return [mid, ties, equal, rand]


_F4_NAN = np.array([7 * 128 + 5, 20 * 128 + 127, 20 * 128 + 0, _F4 - 2])


@pytest.fixture(scope="module")
def fused_engine(gpu_device):
    from hipporag_amd.engine import HippoRAGEngine
    cols = _fused_cols(_F4, 3)
    fe = _one_hot_matrix(_F4, cols, _F4_NAN)
    zeros = np.zeros(_F4, np.int32)
    eng = HippoRAGEngine(_empty_graph(4), np.array([3], np.int32), fe[:1], fe, zeros, zeros, np.zeros(4, np.int32),
                         max_batch=200, max_topk=16)
    yield dict(eng=eng, cols=cols, fe=fe)
    eng.close()


@pytest.mark.parametrize("b", [17, 64, 65, 130, 200])   # 64-query tiles, the 256-row kernel (NJ 4 and 8)
def test_path4_score_facts_fused(fused_engine, b):
    import torch
    e = fused_engine
    cq = _cols_for(b, len(e["cols"]))
    s = _check_scores_assumption(e["eng"], "facts", e["cols"], _F4_NAN, cq)
    q = _queries(cq)
    for k in (1, 3, 4, 5, 16):                              # k <= 4: fewer selected tiles than NaN tiles
        idx, sc = e["eng"].score_facts(q, k=k)
        torch.cuda.synchronize()
        want = expected_topk(s, k)
        assert_topk_equal((idx.cpu().numpy(), sc.cpu().numpy(), None, None), (want[0], want[2], None, None),
                          f"b={b} k={k}")


@pytest.mark.parametrize("b", [1, 17, 65, 130])
def test_path4_sim_topk(fused_engine, b):
    import torch
    from hipporag_amd import _lib
    lib = _lib.load()
    e = fused_engine
    cq = _cols_for(b, len(e["cols"]))
    s = _expected_scores(e["cols"], _F4_NAN, cq)
    emb = torch.from_numpy(e["fe"].view(np.int16)).cuda()
    q = _queries(cq)
    need = int(lib.hrag_sim_topk_workspace_bytes(_F4, b))
    ws = torch.zeros((need,), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for k in (1, 4, 5, 16):
        idx = torch.empty((b, k), dtype=torch.int32, device="cuda")
        val = torch.empty((b, k), dtype=torch.float32, device="cuda")
        _lib.check(lib.hrag_sim_topk(emb.data_ptr(), _F4, _DIM, q.data_ptr(), b, k, 0, ws.data_ptr(), need,
                                     idx.data_ptr(), val.data_ptr(), stream))
        torch.cuda.synchronize()
        want = expected_topk(s, k)
        assert_topk_equal((idx.cpu().numpy(), val.cpu().numpy(), None, None), (want[0], want[1], None, None),
                          f"b={b} k={k}")


# ----------------------------------------------------------------------------- path 5: the KNN's dense path
def test_path5_knn_nan_key_comes_first(gpu_device):
    """k = 2047 over 300 001 keys, the last one a NaN vector: it heads every row (score NaN), and the rest of the row
    is the same call's row without it"""
    from hipporag_amd.knn import retrieve_knn
    rng = np.random.default_rng(9)
    n, dim = 300_000, 32
    keys = rng.standard_normal((n + 1, dim)).astype(np.float32)
    keys[n] = np.float32(np.nan)
    qv = rng.standard_normal((4, dim)).astype(np.float32)
    kid = [str(i) for i in range(n + 1)]
    idx, sc = retrieve_knn(["q"] * 4, kid, qv, keys, k=2047, return_arrays=True)
    idx0, sc0 = retrieve_knn(["q"] * 4, kid[:n], qv, keys[:n], k=2047, return_arrays=True)
    assert np.all(idx[:, 0] == n) and np.all(np.isnan(sc[:, 0]))
    np.testing.assert_array_equal(idx[:, 1:], idx0[:, :2046])
    np.testing.assert_array_equal(sc[:, 1:].view(np.uint32), sc0[:, :2046].view(np.uint32))
    assert not np.isnan(sc0).any()
