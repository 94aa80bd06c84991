"""The small kernels around the similarity GEMM, called directly: hrag_split_f32 (csrc/knn.hip split3_kernel) and
hrag_normalize_split_bf16 (normalize_split_kernel) against numpy -- bit for bit without normalisation, within the stated
precision of F.normalize with it -- and hrag_row_minmax (the passage prior's min / max in every hrag_retrieve) against the
rule of include/hrag.h: fminf / fmaxf, NaN skipped, a row without a number gives +inf / -inf."""

import numpy as np
import pytest

from tests.helpers import expected_topk, split_f32_np
from tests.test_gpu_topk_exact import _on_device, _rows

pytestmark = pytest.mark.gpu


def _bf16_np(x):
    """fp32 -> bf16 bits, round to nearest even (NaN stays NaN with its quiet bit set, as the kernel does)"""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def _bits_to_f32(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def _inputs(rows, dim, seed):
    """Gaussian rows at scales 1e-6 ... 1e4 per row, plus: a zero row, fp32 subnormals, +-0, components near the fp16
    limits (65504, 2^-14, 2^-24) and very large ones (1e30 overflow fp16: hi = inf, lo = -inf on both sides)"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, dim)) * 10.0 ** rng.uniform(-6, 4, (rows, 1))).astype(np.float32)
    x[0] = 0
    x[1, ::2] = np.array([1, 2, 0x7FFFFF, 0x400000], np.uint32).view(np.float32)[np.arange(dim // 2) % 4]
    x[1, 1::2] = -x[1, ::2]
    x[2, :4] = np.array([0.0, -0.0, 65504.0, -65519.0], np.float32)
    x[2, 4:8] = np.array([2.0 ** -14, 2.0 ** -24, 3 * 2.0 ** -26, 1e30], np.float32)
    x[3] = np.float32(1e30) * rng.standard_normal(dim).astype(np.float32)
    return x


def _dev(x):
    import torch
    return torch.from_numpy(x).to("cuda")


@pytest.mark.parametrize("rows,dim", [(7, 8), (130, 64), (33, 200), (5, 4096)])
def test_split_f32_is_bit_exact(gpu_device, rows, dim):
    import torch
    from hipporag_amd import _lib
    lib = _lib.load()
    x = _inputs(rows, dim, seed=rows + dim)
    hi, lo = split_f32_np(x)
    hi, lo = hi.view(np.uint16), lo.view(np.uint16)
    for as_query, layout in ((0, (hi, lo, hi)), (1, (hi, hi, lo))):
        out = torch.full((rows, 3 * dim), -1, dtype=torch.int16, device="cuda")
        _lib.check(lib.hrag_split_f32(_dev(x).data_ptr(), rows, dim, as_query, 0, out.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint16), np.concatenate(layout, axis=1), err_msg=str(as_query))


@pytest.mark.parametrize("rows,dim", [(7, 8), (130, 64), (33, 200), (5, 4096)])
def test_normalize_split_bf16_is_bit_exact(gpu_device, rows, dim):
    import torch
    from hipporag_amd import _lib
    lib = _lib.load()
    x = _inputs(rows, dim, seed=rows * dim)
    hi = _bf16_np(x)
    lo = _bf16_np(x - _bits_to_f32(hi))
    out_hi = torch.full((rows, dim), -1, dtype=torch.int16, device="cuda")
    out_lo = torch.full((rows, dim), -1, dtype=torch.int16, device="cuda")
    _lib.check(lib.hrag_normalize_split_bf16(_dev(x).data_ptr(), rows, dim, 0, out_hi.data_ptr(), out_lo.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream))
    only_hi = torch.full((rows, dim), -1, dtype=torch.int16, device="cuda")
    _lib.check(lib.hrag_normalize_split_bf16(_dev(x).data_ptr(), rows, dim, 0, only_hi.data_ptr(), None,
                                             torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out_hi.cpu().numpy().view(np.uint16), hi)
    np.testing.assert_array_equal(out_lo.cpu().numpy().view(np.uint16), lo)
    np.testing.assert_array_equal(only_hi.cpu().numpy().view(np.uint16), hi)


@pytest.mark.parametrize("rows,dim", [(130, 64), (33, 200), (5, 4096)])
def test_normalizing_splits_match_f_normalize(gpu_device, rows, dim):
    """normalize = 1: hi + lo = F.normalize(x) (x / max(|x|, 1e-12)) up to the halves' precision -- fp16:
    max(2^-22 |v|, 2^-25) per component, bf16 (8 significant bits per half): 2^-16 |v| -- plus the kernel's own fp32 normalisation (1 / norm and the
    product, rounded: 2^-22 |v|).  Zero rows give zeros; fp32 subnormals, +-0 and rows with components of 1e30 are
    normalised without overflow (the norm is summed in fp64)"""
    import torch
    import torch.nn.functional as F
    from hipporag_amd import _lib
    lib = _lib.load()
    x = _inputs(rows, dim, seed=rows + 3 * dim)
    x[2, 6:8] = 1.0                                   # no overflow of fp16 after normalisation anyway
    want = F.normalize(torch.from_numpy(x).double(), dim=1).numpy()
    assert np.isfinite(want).all()
    stream = torch.cuda.current_stream().cuda_stream
    for as_query in (0, 1):
        out = torch.empty((rows, 3 * dim), dtype=torch.float16, device="cuda")
        _lib.check(lib.hrag_split_f32(_dev(x).data_ptr(), rows, dim, as_query, 1, out.data_ptr(), stream))
        torch.cuda.synchronize()
        o = out.cpu().numpy().astype(np.float64)
        hi, lo = o[:, :dim], (o[:, dim:2 * dim] if not as_query else o[:, 2 * dim:])
        err = np.abs(hi + lo - want)
        tol = np.maximum(2.0 ** -22 * np.abs(want), 2.0 ** -25) + 2.0 ** -22 * np.abs(want)
        assert np.all(err <= tol), float((err / tol).max())
        assert np.all(o[0] == 0)
    out_hi = torch.empty((rows, dim), dtype=torch.int16, device="cuda")
    out_lo = torch.empty((rows, dim), dtype=torch.int16, device="cuda")
    _lib.check(lib.hrag_normalize_split_bf16(_dev(x).data_ptr(), rows, dim, 1, out_hi.data_ptr(), out_lo.data_ptr(), stream))
    torch.cuda.synchronize()
    v = _bits_to_f32(out_hi.cpu().numpy().view(np.uint16)).astype(np.float64) + \
        _bits_to_f32(out_lo.cpu().numpy().view(np.uint16)).astype(np.float64)
    err = np.abs(v - want)
    tol = (2.0 ** -16 + 2.0 ** -22) * np.abs(want) + 2.0 ** -126
    assert np.all(err <= tol), float((err / tol).max())
    assert np.all(v[0] == 0)


def _row_minmax(ptr, b, n, ld):
    import torch
    from hipporag_amd import _lib
    lib = _lib.load()
    mn = torch.empty((b,), dtype=torch.float32, device="cuda")
    mx = torch.empty((b,), dtype=torch.float32, device="cuda")
    _lib.check(lib.hrag_row_minmax(ptr, b, n, ld, mn.data_ptr(), mx.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return mn.cpu().numpy(), mx.cpu().numpy()


@pytest.mark.parametrize("n", [1, 2, 3, 1023, 1024, 1025, 300_001])
@pytest.mark.parametrize("pad,misalign,fill", [(0, 0, float("nan")), (3, 1, float("-inf")), (5, 3, float("inf"))])
def test_row_minmax_follows_the_rule(gpu_device, n, pad, misalign, fill):
    """every float class (NaNs of both signs and any payload, +-inf, +-0, +-max, subnormals), rows that are all NaN
    (+inf / -inf), padding beyond n and a gap before row 0 holding NaN or +-inf (a read past n would show)"""
    x = _rows(n, seed=n + pad)
    buf, ptr = _on_device(x, n + pad, misalign, fill)
    mn, mx = _row_minmax(ptr, x.shape[0], n, n + pad)
    _, _, _, w_mn, w_mx = expected_topk(x, 1)
    np.testing.assert_array_equal(mn, w_mn)
    np.testing.assert_array_equal(mx, w_mx)
    assert mn[7] == np.inf and mx[7] == -np.inf                  # row 7: NaN only
    del buf
