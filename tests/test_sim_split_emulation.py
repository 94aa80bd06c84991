"""The split engine's error checks (tests/helpers.py split_score_bound, split_aggregate_check) on a numpy emulation of
the kernels, no GPU: fp32 vectors as fp16 halves in the layout [hi | lo | hi] x [qhi | qhi | qlo] (csrc/knn.hip
split3_kernel), the 3 * dim products summed 32 at a time into an fp32 accumulator (one v_mfma_f32_16x16x32_f16 step
each).  The correct layout must pass both checks; two mutants on the same inputs must fail the aggregate one: lo
dropped (hi . qhi alone) and bf16 halves (what csrc/knn.hip tried first)."""

import numpy as np
import pytest
import torch

from tests.helpers import AGGREGATE_Z_LIMIT, split_aggregate_check, split_error_sigma, split_f32_np, split_score_bound


def _bf16(x):
    """fp32 -> bf16 (round to nearest even) -> fp32"""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
    return u.astype(np.uint32).view(np.float32)


def _halves(x, how):
    if how == "bf16":
        hi = _bf16(x)
        return hi.astype(np.float64), _bf16(x - hi).astype(np.float64)
    hi, lo = split_f32_np(x)
    lo = np.zeros_like(lo) if how == "no_lo" else lo
    return hi.astype(np.float64), lo.astype(np.float64)


def _emulate(x, q, how):
    """scores [B, rows] as the MFMA chain computes them: 32-element partial sums (exact in fp64 here) added to an fp32
    accumulator in ascending k"""
    hi, lo = _halves(x, how)
    qhi, qlo = _halves(q, how)
    rows3 = np.concatenate([hi, lo, hi], axis=1)
    q3 = np.concatenate([qhi, qhi, qlo], axis=1)
    acc = np.zeros((q.shape[0], x.shape[0]), np.float32)
    for c in range(0, rows3.shape[1], 32):
        acc = (acc.astype(np.float64) + q3[:, c:c + 32] @ rows3[:, c:c + 32].T).astype(np.float32)
    return acc.astype(np.float64)


def _unit(x):
    x = np.asarray(x, np.float64)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _inputs(dim, seed):
    """rows: unit Gaussian; queries: near-duplicates of the first rows (cos ~ 0.999) and unrelated unit vectors;
    -> (rows, queries, near-duplicate mask [B, rows])"""
    rng = np.random.default_rng(seed)
    x = _unit(rng.standard_normal((256, dim)))
    n_dup = 48
    q = np.concatenate([_unit(x[:n_dup] + 0.045 * _unit(rng.standard_normal((n_dup, dim)))),
                        _unit(rng.standard_normal((16, dim)))])
    near = np.zeros((q.shape[0], x.shape[0]), bool)
    near[np.arange(n_dup), np.arange(n_dup)] = True
    return x, q, near


@pytest.mark.parametrize("dim", [64, 200, 768, 4096])
def test_aggregate_check_passes_the_split_layout_and_fails_its_mutants(dim):
    x, q, near = _inputs(dim, seed=dim)
    q = np.concatenate([q, x[:16]])                  # self pairs: where a dropped lo . qlo is systematic
    want = q.astype(np.float64) @ x.astype(np.float64).T
    assert np.all(np.abs(want[:near.shape[0]][near] - 0.999) < 2e-3)
    sigma = split_error_sigma(torch.from_numpy(x), torch.from_numpy(q)).numpy()
    stats = {}
    for how in ("split", "no_lo", "bf16"):
        err = _emulate(x, q, how) - want
        ok, stats[how] = split_aggregate_check(err, sigma)
        if how == "split":
            assert ok, stats
            bound = split_score_bound(torch.from_numpy(x), torch.from_numpy(q)).numpy()
            assert np.all(np.abs(err) <= bound), float((np.abs(err) / bound).max())
        else:
            assert not ok, (how, stats)
    assert stats["no_lo"]["rms_z"] > 50 * AGGREGATE_Z_LIMIT, stats
    assert stats["bf16"]["rms_z"] > 1.5 * AGGREGATE_Z_LIMIT, stats


def test_split_bound_holds_on_small_large_and_wide_range_vectors():
    """The per-pair bound carries the 2^-25 floor of fp16 subnormals: vectors of norm 1e-3, 1e3 and components spanning
    1e-8 ... 0.5 stay inside it (a purely relative 2^-21 |x| |q| does not hold for the small ones)"""
    rng = np.random.default_rng(1)
    dim = 1024
    base = _unit(rng.standard_normal((96, dim)))
    wide = base * np.exp(rng.uniform(np.log(1e-8), np.log(0.5), (96, dim))).astype(np.float32)
    x = np.concatenate([base * np.float32(1e-3), base * np.float32(1e3), wide]).astype(np.float32)
    q = np.concatenate([x[::7], _unit(rng.standard_normal((16, dim)))]).astype(np.float32)
    want = q.astype(np.float64) @ x.astype(np.float64).T
    err = np.abs(_emulate(x, q, "split") - want)
    bound = split_score_bound(torch.from_numpy(x), torch.from_numpy(q)).numpy()
    assert np.all(err <= bound), float((err / bound).max())
    rel = err / (np.linalg.norm(q, axis=1)[:, None] * np.linalg.norm(x, axis=1)[None])
    assert rel[:, :96].max() > 2.0 ** -21      # norm 1e-3 rows: the relative claim alone would fail here
