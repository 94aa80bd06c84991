"""Shared test scaffolding: small synthetic indexes in both the oracle's and the engine's form."""

from __future__ import annotations

import numpy as np

import oracle
from hipporag_amd import synth
from hipporag_amd.graph import bf16_bits_to_float


from oracle.checks import (  # noqa: E402,F401  (the checkers live with the oracle: bench.py and smoke() use them too)
    ID_GAP_FLOOR, make_case, prior_noise_allowance, ranked_parity, tie_aware_equal, tie_aware_report, ulp4_report,
)


def write_test_report(name: str, record: dict) -> None:
    """Leave a small JSON record of a GPU test's parity figures under gpurun_out/test_reports/ (merged back from the
    GPU box) and on stdout (pytest -s); never fails the test."""
    import json
    import os
    print(f"[{name}] {json.dumps(record)}")
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        d = os.path.join(root, "gpurun_out", "test_reports")
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, name + ".json"), "w") as f:
            json.dump(record, f)
    except OSError:
        pass


def expected_topk(x, k, idx_offset=0):
    """The library's row ranking restated in numpy -- np.argsort(..., kind="stable")[::-1][:k] per row (every NaN first,
    ties by the larger index), -1 / 0 beyond n -- with the raw and min-max normalised scores in float32 and the row
    min / max as fminf / fmaxf from +-inf give them (NaN skipped; a row without a number gives +inf / -inf).
    -> (idx, raw, normalised, mn, mx)."""
    x = np.asarray(x, np.float32)
    b, n = x.shape
    kk = min(k, n)
    order = np.argsort(x, axis=1, kind="stable")[:, ::-1][:, :kk]
    raw = np.take_along_axis(x, order, axis=1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        # (not np.fmin / np.fmax: on a signalling NaN they may return NaN, where fminf / fmaxf skip every NaN)
        nan = np.isnan(x)
        mn = np.where(nan, np.float32(np.inf), x).min(axis=1, initial=np.inf)
        mx = np.where(nan, np.float32(-np.inf), x).max(axis=1, initial=-np.inf)
        rng_ = (mx - mn)[:, None]
        norm = np.where(rng_ == 0, np.float32(1), (raw - mn[:, None]) / rng_).astype(np.float32)
    idx = np.full((b, k), -1, np.int32)
    idx[:, :kk] = order + idx_offset
    val_raw, val_norm = np.zeros((b, k), np.float32), np.zeros((b, k), np.float32)
    val_raw[:, :kk], val_norm[:, :kk] = raw, norm
    return idx, val_raw, val_norm, mn.astype(np.float32), mx.astype(np.float32)


def assert_topk_equal(got, want, msg=""):
    """got (idx, val, mn, mx) against one of expected_topk's score columns: indices exactly, scores and min / max
    exactly (a NaN where numpy has one, +0 == -0)"""
    idx, val, mn, mx = got
    w_idx, w_val, w_mn, w_mx = want
    np.testing.assert_array_equal(idx, w_idx, err_msg=f"indices {msg}")
    np.testing.assert_array_equal(val, w_val, err_msg=f"scores {msg}")
    if mn is not None:
        np.testing.assert_array_equal(mn, w_mn, err_msg=f"row min {msg}")
        np.testing.assert_array_equal(mx, w_mx, err_msg=f"row max {msg}")


# ----------------------------------------------------------------------------- similarity scores against fp64
# A similarity kernel computes S[b][m] = sum_k q[b][k] * e[m][k] over kdim 16-bit elements: bf16 / fp16 rows as the
# engine stores them, or -- an HRAG_F32_SPLIT engine / retrieve_knn(precision="f32") -- fp32 vectors stored as fp16
# halves x = hi + lo in the layout [hi | lo | hi] x [qhi | qhi | qlo] (kdim = 3 * dim, csrc/knn.hip split3_kernel).
# The reference below is the fp64 dot product of what the engine claims to compute: the rounded 16-bit vectors, or the
# ORIGINAL fp32 vectors of a split engine.  The helpers take torch tensors (device or host) and return fp64 tensors.

U32 = 2.0 ** -23          # fp32 unit roundoff of ANY faithful rounding (2^-24 for round-to-nearest; truncation included)
HALF_TINY = 2.0 ** -25    # half the fp16 subnormal spacing: the absolute error of an fp16 rounding below 2^-14


def sim_reference(x, q):
    """fp64 [B, rows] = q . x^T of the given vectors (exact for fp16 / bf16 / fp32 inputs up to fp64 rounding)"""
    return q.double() @ x.double().T


def accumulation_depth(kdim: int) -> int:
    """An upper bound on the number of fp32 roundings along any score's chain, over every similarity kernel:
      - MFMA kernels (16 / 64 / 128-query tiles, the 256-row kernel, the fused top-k's rescore): ceil(kdim / 32)
        v_mfma_f32_16x16x32 steps into one accumulator, each adding 32 exact products; however the unit orders the 32
        (a binary tree at worst: 5 levels) and the accumulator add, that is <= ceil(kdim / 32) + 5 roundings deep;
      - the GEMV (B <= 2, kdim <= 4096): per lane 4 * ceil(kdim / 512) v_dot2c steps of <= 2 roundings each, then a
        64-lane butterfly (6 levels): <= 8 * ceil(kdim / 512) + 6."""
    return max(-(-kdim // 32) + 5, 8 * (-(-kdim // 512)) + 6)


def gamma(n: int) -> float:
    """Higham's gamma_n = n u / (1 - n u) for the fp32 unit roundoff U32: |fl(sum of n + 1 terms) - sum| <=
    gamma_n * sum |terms| for any evaluation order of depth n"""
    return n * U32 / (1 - n * U32)


def rounded_score_bound(x, q, kdim: int):
    """Per-pair bound [B, rows] on |kernel score - fp64 dot| for vectors that ARE 16-bit values (bf16 / fp16 engines):
    every product of two bf16 / fp16 values is exact in fp32 (8 + 8 or 11 + 11 significant bits, exponents far inside
    fp32's range), so the only error is the fp32 accumulation: gamma(depth) * |q| . |x|^T, plus fp64 rounding of the
    reference itself (2^-50 of the same sum covers it)."""
    a = q.double().abs() @ x.double().abs().T
    return (gamma(accumulation_depth(kdim)) + 2.0 ** -50) * a


def split_score_bound(x, q):
    """Per-pair bound [B, rows] on |split-engine score - fp64 dot of the fp32 vectors x (rows), q (queries)|.

    Layout term.  hi = fp16(v) (round to nearest), lo = fp16(v - hi); v - hi is exact in fp32 (hi is within a factor 2
    of v, or 0).  For |v| < 65504 (fp16 overflow otherwise):
      |v - hi - lo| <= e(v) = max(2^-22 |v|, 2^-25)   (2^-11 relative twice while lo is a normal fp16, i.e. |v| >= 2^-3;
                                                       below, lo -- or hi itself under 2^-14 -- is subnormal: 2^-25 absolute)
      |lo| <= l(v) = 2^-11 |v| + 2^-25
    The kernel computes hi.qhi + lo.qhi + hi.qlo = x'.q' - lo.qlo with x' = hi + lo, q' = qhi + qlo, so
      |x.q - score| <= e(x).|q| + |x|.e(q) + e(x).e(q) + l(x).l(q)
    (component-wise products summed: the bound tightens where components are small, and carries the 2^-25 floor of
    every component: 2^-25 (|x|_1 + |q|_1) in all -- 3.8e-6 at dim 4096 in the worst case, not 2^-21 |x| |q|).
    Accumulation term: gamma(depth of kdim = 3 * dim) times the sum of the absolute products, which is at most
    (|x| + 2 l(x)) . (|q| + 2 l(q))."""
    xa, qa = x.double().abs(), q.double().abs()
    ex, eq = (xa * 2.0 ** -22).clamp_min(HALF_TINY), (qa * 2.0 ** -22).clamp_min(HALF_TINY)
    lx, lq = xa * 2.0 ** -11 + HALF_TINY, qa * 2.0 ** -11 + HALF_TINY
    layout = eq @ xa.T + qa @ ex.T + eq @ ex.T + lq @ lx.T
    kdim = 3 * x.shape[1]
    acc = (gamma(accumulation_depth(kdim)) + 2.0 ** -50) * ((qa + 2 * lq) @ (xa + 2 * lx).T)
    return layout + acc


def split_error_sigma(x, q):
    """Per-pair model [B, rows] of the standard deviation of a CORRECT split score's error: each rounding error taken as
    independent and uniform over its interval (variance = half-width^2 / 3), every half-width the largest the analysis
    of split_score_bound allows:
      - layout: component i of x is off by at most e = max(2^-22 |x_i|, 2^-25) and enters the score weighted by q_i (and
        symmetrically): var = sum_i (e(x_i)^2 q_i^2 + x_i^2 e(q_i)^2) / 3 (the dropped lo.qlo, <= 2^-22 |x_i q_i| per
        component, is of the same size and rides in this budget);
      - accumulation, MFMA chain (the deepest one): the fp32 accumulator is rounded once per 32 elements, within 2^-24
        of the running sum.  Over the first third of the layout (hi.qhi) that sum is S_j, the partial dot product of x
        and q over their first 32 j components; over the other two thirds (lo.qhi, hi.qlo: 2^-11 of it) it stays at the
        score s: var = (2^-24)^2 / 3 * (sum_j S_j^2 + (2 dim / 32) s^2).  The roundings inside one MFMA step (at most 5
        levels over 32 products) add 5 (2^-24)^2 / 3 * sum_j C_j^2, C_j the sum of |x_i q_i| over chunk j.
    Memory: B * rows * dim / 32 doubles."""
    xd, qd = x.double(), q.double()
    xa, qa = xd.abs(), qd.abs()
    ex, eq = (xa * 2.0 ** -22).clamp_min(HALF_TINY), (qa * 2.0 ** -22).clamp_min(HALF_TINY)
    layout = ((eq * eq) @ (xa * xa).T + (qa * qa) @ (ex * ex).T) / 3
    b, dim = qd.shape
    nch = -(-dim // 32)
    pad = nch * 32 - dim
    if pad:
        xd = _torch_pad(xd, pad)
        qd = _torch_pad(qd, pad)
    xc, qc = xd.reshape(-1, nch, 32), qd.reshape(b, nch, 32)
    part = (qc[:, None] * xc[None]).sum(-1)                          # [B, rows, nch] chunk sums of x_i q_i
    cabs = (qc.abs()[:, None] * xc.abs()[None]).sum(-1)
    run = part.cumsum(-1)
    s = run[..., -1]
    acc = (2.0 ** -48 / 3) * ((run * run).sum(-1) + 2 * nch * s * s + 5 * (cabs * cabs).sum(-1))
    return (layout + acc).sqrt()


def _torch_pad(t, n):
    import torch
    return torch.cat([t, t.new_zeros((t.shape[0], n))], dim=1)


AGGREGATE_Z_LIMIT = 1.5


def split_aggregate_check(err, sigma):
    """The aggregate check of a split kernel over many pairs: RMS(err / split_error_sigma) <= AGGREGATE_Z_LIMIT.  The
    model's variance is an upper bound of each pair's, so a correct kernel has E[z^2] <= 1; where the fp16 subnormal
    floor dominates (unit vectors at dim 4096: every lo is subnormal) the bound is attained, and a numpy emulation of
    the MFMA chain measures RMS(z) 0.6 - 0.96 at dims 64 - 4096.  The limit leaves 1.5x for the sampling spread of pairs
    that share their rows' rounding errors.  fp16 halves without lo (2^-11 per component) measure 175 - 775 and bf16
    halves (8 + 8 significant bits: up to 2^-16 per component) 2.6 - 11.5 (tests/test_sim_split_emulation.py).
    -> (ok, stats dict)."""
    z = np.asarray(err, np.float64).ravel() / np.asarray(sigma, np.float64).ravel()
    stats = {"rms_z": float(np.sqrt(np.mean(z * z))), "p999_z": float(np.quantile(np.abs(z), 0.999)),
             "max_z": float(np.abs(z).max()), "pairs": int(z.size)}
    return stats["rms_z"] <= AGGREGATE_Z_LIMIT, stats


def split_f32_np(x):
    """numpy restatement of hrag_split_f32's halves: hi = fp16(x) (round to nearest even), lo = fp16(x - hi) with
    x - hi in fp32 -> (hi, lo) as float16 arrays"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        hi = x.astype(np.float16)
        lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


# ----------------------------------------------------------------------------- the reset vector restated
def seeds_np(kept_idx, kept_score, kept_count, link_top_k, subj, obj, num_chunks):
    """hrag_stage_seeds restated in numpy (include/hrag.h; HippoRAG.py:1574-1623, :1505-1542):
      - the entries of a query are (fact r, subject) then (fact r, object) for r < clamp(kept_count, 0, kf); a fact id
        or vertex outside its table is skipped;
      - w = fp32 score / fp32 num_chunks[v] where num_chunks[v] > 0, the score itself otherwise;
      - per phrase an fp64 sum and count in entry order, mean = sum / count;
      - stable descending selection by the fp64 mean, every NaN mean above every number, ties (NaN included) in
        first-occurrence order; the first min(link_top_k, m) when 0 < link_top_k < m, else all m phrases;
      - seed_w = fp32(mean) sanitised: NaN, negative or zero -> +0;
      - flags bit 0: kept_count <= 0 (DPR fallback); bit 2: a kept phrase's mean is exactly +-0 before sanitising.
    -> (seed_vtx int32 [B, 32] (-1 beyond seed_cnt), seed_w float32 [B, 32] (0 beyond), seed_cnt int32 [B],
        flags int32 [B], means: list of the kept fp64 means per query)."""
    kept_idx = np.asarray(kept_idx, np.int64)
    kept_score = np.asarray(kept_score, np.float32)
    kept_count = np.asarray(kept_count, np.int64)
    subj, obj, num_chunks = (np.asarray(a, np.int64) for a in (subj, obj, num_chunks))
    b, kf = kept_idx.shape
    n_facts, n_v = subj.shape[0], num_chunks.shape[0]
    vtx = np.full((b, 32), -1, np.int32)
    wts = np.zeros((b, 32), np.float32)
    cnt = np.zeros(b, np.int32)
    flags = np.zeros(b, np.int32)
    means = []
    for q in range(b):
        c = int(min(max(kept_count[q], 0), kf))
        total, occ, order = {}, {}, []
        for r in range(c):
            f = int(kept_idx[q, r])
            s = kept_score[q, r]
            for side in (subj, obj):
                if not 0 <= f < n_facts:
                    continue
                v = int(side[f])
                if not 0 <= v < n_v:
                    continue
                nc = int(num_chunks[v])
                with np.errstate(all="ignore"):
                    w = np.float32(s / np.float32(nc)) if nc > 0 else s
                if v not in total:
                    total[v], occ[v] = 0.0, 0
                    order.append(v)
                total[v] += float(w)
                occ[v] += 1
        mean = {v: total[v] / occ[v] for v in order}
        ranked = sorted(order, key=lambda v: (0, 0.0) if np.isnan(mean[v]) else (1, -mean[v]))
        m = len(ranked)
        keep = link_top_k if 0 < link_top_k < m else m
        kept = ranked[:keep]
        for j, v in enumerate(kept):
            w32 = np.float32(mean[v])
            vtx[q, j] = v
            wts[q, j] = w32 if w32 > 0 else np.float32(0)
        cnt[q] = keep
        flags[q] = (1 if c == 0 else 0) | (4 if any(mean[v] == 0.0 for v in kept) else 0)
        means.append([mean[v] for v in kept])
    return vtx, wts, cnt, flags, means


def prior_np(scores, weight, mn=None, mx=None):
    """The passage prior every phase-B path forms, restated in fp32 (include/hrag.h): minmax(s) * weight with the row
    min / max over the numbers of the row (NaN skipped, expected_topk's rule) unless given, a zero range giving 1,
    then sanitised -- NaN, negative or zero -> +0.  -> float32 [B, n]."""
    s = np.asarray(scores, np.float32)
    if mn is None:
        _, _, _, mn, mx = expected_topk(s, 1)
    mn = np.asarray(mn, np.float32)[:, None]
    mx = np.asarray(mx, np.float32)[:, None]
    with np.errstate(all="ignore"):
        rng_ = mx - mn
        nrm = np.where(rng_ == 0, np.float32(1), (s - mn) / rng_).astype(np.float32)
        v = (nrm * np.float32(weight)).astype(np.float32)
    return np.where(v > 0, v, np.float32(0)).astype(np.float32)
