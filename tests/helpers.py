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
