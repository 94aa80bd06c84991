"""hrag_topk_rows_ws (K4', csrc/topk.hip): the row ranking at ANY k equals np.argsort(x, kind="stable")[::-1][:k] exactly
-- indices, raw and min-max normalised scores, row min / max -- on rows of every shape the engine and the KNN produce,
and its prefix is hrag_topk_rows' bit for bit."""

import numpy as np
import pytest

from tests.helpers import expected_topk

pytestmark = pytest.mark.gpu


_NANS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FC12345, 0xFF812345],
                 np.uint32).view(np.float32)


def _rows(batch, n, seed):
    """Row r of the batch takes distribution r % 7: random, all equal, few distinct values, ascending, descending,
    random with +-inf, random with NaNs of both signs and mixed payloads (quiet and signalling)."""
    rng = np.random.default_rng(seed)
    x = np.empty((batch, n), np.float32)
    for r in range(batch):
        kind = r % 7
        if kind == 0:
            x[r] = rng.random(n, dtype=np.float32)
        elif kind == 1:
            x[r] = np.float32(0.25)
        elif kind == 2:
            x[r] = rng.choice(np.array([-1.5, 0.0, 0.5, 3.0], np.float32), n)
        elif kind == 3:
            x[r] = np.sort(rng.standard_normal(n).astype(np.float32))
        elif kind == 4:
            x[r] = np.sort(rng.standard_normal(n).astype(np.float32))[::-1]
        elif kind == 5:
            x[r] = rng.standard_normal(n).astype(np.float32)
            x[r, rng.integers(0, n, max(1, n // 100))] = np.inf
            x[r, rng.integers(0, n, max(1, n // 100))] = -np.inf
        else:
            x[r] = rng.standard_normal(n).astype(np.float32)
            at = rng.integers(0, n, max(1, n // 50))
            x[r, at] = _NANS[np.arange(len(at)) % len(_NANS)]
    return x


def _expected(x, k, idx_offset):
    return expected_topk(x, k, idx_offset)


def _on_device(x, ld, misalign):
    """x [b, n] copied into a device buffer with row stride ld, the first row starting `misalign` floats in."""
    import torch
    b, n = x.shape
    buf = torch.full((misalign + b * ld,), float("nan"), dtype=torch.float32, device="cuda")
    buf[misalign:].view(b, ld)[:, :n].copy_(torch.from_numpy(x))
    return buf, buf.data_ptr() + 4 * misalign


def _call(ptr, b, n, ld, k, idx_offset, normalize, large=True):
    import torch
    from hipporag_amd import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    idx = torch.empty((b, k), dtype=torch.int32, device="cuda")
    val = torch.empty((b, k), dtype=torch.float32, device="cuda")
    mn = torch.empty((b,), dtype=torch.float32, device="cuda")
    mx = torch.empty((b,), dtype=torch.float32, device="cuda")
    if large:
        need = int(lib.hrag_topk_rows_workspace_bytes(b, n, k))
        ws = torch.empty((max(need, 1),), dtype=torch.uint8, device="cuda")
        _lib.check(lib.hrag_topk_rows_ws(ptr, b, n, ld, k, idx_offset, normalize, idx.data_ptr(), val.data_ptr(),
                                         mn.data_ptr(), mx.data_ptr(), ws.data_ptr() if need else None, need, stream))
    else:
        _lib.check(lib.hrag_topk_rows(ptr, b, n, ld, k, idx_offset, normalize, idx.data_ptr(), val.data_ptr(),
                                      mn.data_ptr(), mx.data_ptr(), stream))
    torch.cuda.synchronize()
    return idx.cpu().numpy(), val.cpu().numpy(), mn.cpu().numpy(), mx.cpu().numpy()


def _check(x, ks, *, ld=None, misalign=0, idx_offset=0):
    b, n = x.shape
    ld = n if ld is None else ld
    buf, ptr = _on_device(x, ld, misalign)
    for k in ks:
        want = _expected(x, k, idx_offset)
        for normalize in (0, 1):
            idx, val, mn, mx = _call(ptr, b, n, ld, k, idx_offset, normalize)
            np.testing.assert_array_equal(idx, want[0], err_msg=f"k={k} norm={normalize}")
            np.testing.assert_array_equal(val, want[2 if normalize else 1], err_msg=f"k={k} norm={normalize}")
            np.testing.assert_array_equal(mn, want[3])
            np.testing.assert_array_equal(mx, want[4])
    del buf


@pytest.mark.parametrize("ld_pad,misalign,idx_offset", [(0, 0, 0), (5, 1, 1000)])
def test_short_rows_every_distribution(gpu_device, ld_pad, misalign, idx_offset):
    x = _rows(7, 4099, seed=1)
    _check(x, [2049, 4096, 4099, 4099 + 7, 16384, 50000], ld=4099 + ld_pad, misalign=misalign, idx_offset=idx_offset)


@pytest.mark.parametrize("ld_pad,misalign,idx_offset", [(0, 0, 0), (3, 3, 7)])
def test_long_rows_every_distribution(gpu_device, ld_pad, misalign, idx_offset):
    """125 000 keys: k <= 16384 sorts in LDS, k > 16384 tile-sorts and merges in the workspace (n + 7: the tail
    beyond n)."""
    x = _rows(7, 125000, seed=2)
    _check(x, [2049, 16384, 16385, 50000, 125000, 125007], ld=125000 + ld_pad, misalign=misalign, idx_offset=idx_offset)


def test_one_knn_row_of_875k(gpu_device):
    x = _rows(1, 875000, seed=3)
    _check(x, [2049, 4096, 16384, 50000, 875000])
    x = _rows(7, 875000, seed=4)[6:7]         # the NaN row
    _check(x, [4096, 50000])


def test_wide_batch(gpu_device):
    x = _rows(256, 125000, seed=5)
    _check(x, [4096, 16385, 125000])


def test_prefix_and_small_k_are_hrag_topk_rows_bit_for_bit(gpu_device):
    x = _rows(14, 125000, seed=6)
    b, n = x.shape
    rows = np.arange(b)     # the NaN rows included: hrag_topk_rows' overflow refinement counts NaN keys too
    buf, ptr = _on_device(x, n, 0)
    for normalize in (0, 1):
        base = _call(ptr, b, n, n, 2048, 0, normalize, large=False)
        for k in (2049, 16384, 16385, n):
            got = _call(ptr, b, n, n, k, 0, normalize)
            np.testing.assert_array_equal(got[0][rows, :2048], base[0][rows])
            np.testing.assert_array_equal(got[1][rows, :2048].view(np.int32), base[1][rows].view(np.int32))
            np.testing.assert_array_equal(got[2].view(np.int32), base[2].view(np.int32))
            np.testing.assert_array_equal(got[3].view(np.int32), base[3].view(np.int32))
        for k in (1, 200, 2047, 2048):      # k <= 2048 through the new entry point IS hrag_topk_rows
            a = _call(ptr, b, n, n, k, 0, normalize, large=False)
            c = _call(ptr, b, n, n, k, 0, normalize)
            for u, v in zip(a, c):
                np.testing.assert_array_equal(u[rows].view(np.int32), v[rows].view(np.int32))
    del buf


def test_workspace_is_checked(gpu_device):
    import torch
    from hipporag_amd import _lib
    lib = _lib.load()
    x = torch.rand((2, 40000), device="cuda")
    idx = torch.empty((2, 20000), dtype=torch.int32, device="cuda")
    val = torch.empty((2, 20000), dtype=torch.float32, device="cuda")
    need = int(lib.hrag_topk_rows_workspace_bytes(2, 40000, 20000))
    assert need > 0
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    st = lib.hrag_topk_rows_ws(x.data_ptr(), 2, 40000, 40000, 20000, 0, 0, idx.data_ptr(), val.data_ptr(), None, None,
                               ws.data_ptr(), need - 8, torch.cuda.current_stream().cuda_stream)
    assert st == _lib.HRAG_EINVAL
    _lib.check(lib.hrag_topk_rows_ws(x.data_ptr(), 2, 40000, 40000, 20000, 0, 0, idx.data_ptr(), val.data_ptr(), None,
                                     None, ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    want = np.argsort(x.cpu().numpy(), axis=1, kind="stable")[:, ::-1][:, :20000]
    np.testing.assert_array_equal(idx.cpu().numpy(), want)


def test_engine_topk_rows_helper(gpu_device):
    import torch
    from hipporag_amd.engine import topk_rows
    x = _rows(3, 30000, seed=7)
    t = torch.from_numpy(x).cuda()
    idx, val, mn, mx = topk_rows(t, 30000, normalize=True, want_minmax=True)
    want = _expected(x, 30000, 0)
    np.testing.assert_array_equal(idx.cpu().numpy(), want[0])
    np.testing.assert_array_equal(val.cpu().numpy(), want[2])
