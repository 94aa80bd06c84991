"""The numpy restatement of facets (include/hrag.h, "facets") and builders of columns and specs.  The bin function is stated
once, in facet_bins_np; counts are np.bincount over it.  Everything is an integer: every comparison of this feature is
assert_array_equal, there is no tolerance anywhere."""

from collections import namedtuple

import numpy as np

from hipporag_amd._lib import FACET_CODES, FACET_EDGES, FACET_WINDOW, PAY_F64, PAY_I64
from tests.payload_helpers import I64_MAX, I64_MIN, bits, make_columns

WINDOW = FACET_WINDOW
LDS_EDGES = 1024          # kFacetLdsEdges of csrc/facet_bin.h: an edge list up to this length is searched in LDS
# col: the column; kind: FACET_CODES / FACET_EDGES; lo: CODES' first value; edges: EDGES' int64 words (doubles as their bits)
Spec = namedtuple("Spec", "col kind n_bins lo edges")


def codes(col, lo, n_bins):
    return Spec(col, FACET_CODES, int(n_bins), int(lo), None)


def edges_i64(col, values):
    e = np.asarray(values, np.int64).reshape(-1)
    return Spec(col, FACET_EDGES, len(e) + 1, 0, e)


def edges_f64(col, values):
    e = bits(np.asarray(values, np.float64).reshape(-1))
    return Spec(col, FACET_EDGES, len(e) + 1, 0, e)


def facet_bins_np(n, cols, spec):
    """int64 [n]: per passage its bin in [0, n_bins), n_bins for "other" (present, the value maps to no bin) or n_bins + 1
    for "missing" (not present).  cols: (type, int64 values [n], present bool [n] or None) per column."""
    typ, values, present = cols[spec.col]
    nb = spec.n_bins
    x = np.asarray(values, np.int64)
    if spec.kind == FACET_CODES:
        assert typ == PAY_I64
        d = x.view(np.uint64) - np.uint64(spec.lo % (1 << 64))              # wraps modulo 2^64, as the definition's cast
        ok = (x >= spec.lo) & (d < np.uint64(nb))
        out = np.where(ok, d, np.uint64(nb)).astype(np.int64)
    elif typ == PAY_F64:
        xf, e = x.view(np.float64), np.asarray(spec.edges, np.int64).view(np.float64)
        nan = np.isnan(xf)
        out = np.searchsorted(e, np.where(nan, 0.0, xf), side="right").astype(np.int64)     # the edges <= x; -0.0 == 0.0
        out[nan] = nb
    else:
        out = np.searchsorted(np.asarray(spec.edges, np.int64), x, side="right").astype(np.int64)
    if present is not None:
        out[~np.asarray(present, bool)] = nb + 1
    return out


def facet_bins_naive(n, cols, spec):
    """The definition of include/hrag.h read passage by passage, in Python's integers and floats."""
    typ, values, present = cols[spec.col]
    nb = spec.n_bins
    out = np.empty(n, np.int64)
    for p in range(n):
        if present is not None and not present[p]:
            out[p] = nb + 1
            continue
        x = int(values[p])
        if spec.kind == FACET_CODES:
            out[p] = x - spec.lo if x >= spec.lo and (x - spec.lo) % (1 << 64) < nb else nb
        elif typ == PAY_F64:
            xf = float(np.int64(x).view(np.float64))
            out[p] = nb if xf != xf else sum(1 for e in np.asarray(spec.edges, np.int64).view(np.float64) if float(e) <= xf)
        else:
            out[p] = sum(1 for e in spec.edges if int(e) <= x)
    return out


def facet_counts_np(n, cols, spec, allowed, bins=None):
    """int32 [B, n_bins + 2] from allowed bool [B, n] (or [n]: one row): the counts, then "other", then "missing"."""
    bins = facet_bins_np(n, cols, spec) if bins is None else bins
    allowed = np.atleast_2d(np.asarray(allowed, bool))
    return np.stack([np.bincount(bins[a], minlength=spec.n_bins + 2) for a in allowed]).astype(np.int32)


def facet_ids_np(n, cols, spec, ids, bins=None):
    """The same over id lists int [B, k]: an id outside [0, n) is skipped, a repeated id counts each time."""
    bins = facet_bins_np(n, cols, spec) if bins is None else bins
    ids = np.atleast_2d(np.asarray(ids, np.int64))
    return np.stack([np.bincount(bins[r[(r >= 0) & (r < n)]], minlength=spec.n_bins + 2) for r in ids]).astype(np.int32)


# ---------------------------------------------------------------------------------- builders
SKEW_COL, WIDE_COL, GONE_COL = 4, 5, 6
SKEW_CODE, SKEW_VALUES = 7, 300


def facet_columns(rng, n):
    """payload_helpers.make_columns' four -- 0: I64 with INT64_MIN / INT64_MAX and holes; 1: F64 with NaN, both infinities,
    both zeros, denormals and holes; 2: I64 codes 0 .. 999, every passage present; 3: F64, every passage present -- then
    4: a skewed keyword-like column, one code holds a third of the passages; 5: codes -3 .. 2 * WINDOW + 9 with holes, for
    specs of several windows; 6: a column no passage has a value in."""
    cols = make_columns(rng, n)
    skew = rng.integers(0, SKEW_VALUES, n).astype(np.int64)
    skew[rng.random(n) < 1 / 3] = SKEW_CODE
    wide = rng.integers(-3, 2 * WINDOW + 10, n).astype(np.int64)
    return cols + [(PAY_I64, skew, None), (PAY_I64, wide, rng.random(n) < 0.9), (PAY_I64, np.zeros(n, np.int64), np.zeros(n, bool))]


def special_specs():
    """name -> Spec: every case the header's definition names, over facet_columns' columns."""
    return {
        "1 bin": codes(2, 5, 1),
        "lo = INT64_MAX": codes(0, I64_MAX, 4),                   # INT64_MIN - INT64_MAX wraps to 1: other, not bin 1
        "lo = INT64_MIN": codes(0, I64_MIN, 3),
        "around zero": codes(0, -5, 11),
        "m = 0": edges_f64(1, []),
        "m = 0, i64": edges_i64(0, []),
        "equal neighbouring edges": edges_f64(1, [-0.5, 0.0, 0.0, 1.5]),
        "edges at the infinities": edges_f64(1, [-np.inf, 0.0, np.inf]),
        "an edge at -0.0": edges_f64(1, [-0.0]),
        "denormal edges": edges_f64(1, [-5e-324, 5e-324]),
        "i64 edges at the extremes": edges_i64(0, [I64_MIN, -2, 3, 3, I64_MAX]),
        "12 edges": edges_f64(3, np.linspace(-1.5, 1.5, 12)),
        "LDS_EDGES edges": edges_i64(WIDE_COL, 8 * np.arange(LDS_EDGES) - 3),
        "LDS_EDGES + 1 edges": edges_i64(WIDE_COL, 8 * np.arange(LDS_EDGES + 1) - 3),
        "1000 codes": codes(2, 0, 1000),
        "skewed": codes(SKEW_COL, 0, SKEW_VALUES),
        "all missing": codes(GONE_COL, 0, 10),
        "all missing, edges": edges_i64(GONE_COL, [0]),
        "WINDOW - 1": codes(WIDE_COL, 0, WINDOW - 1),
        "WINDOW": codes(WIDE_COL, 0, WINDOW),
        "WINDOW + 1": codes(WIDE_COL, 0, WINDOW + 1),
        "2 * WINDOW + 5": codes(WIDE_COL, 0, 2 * WINDOW + 5),
        "the second window only": codes(WIDE_COL, -WINDOW, 2 * WINDOW),      # bins 0 .. WINDOW - 4 stay empty
    }


def random_spec(rng):
    kind = int(rng.integers(0, 4))
    if kind == 0:
        col = [0, 2, SKEW_COL, WIDE_COL][int(rng.integers(0, 4))]
        return codes(col, int(rng.integers(-6, 40)), int(rng.integers(1, 2 * WINDOW + 40 if col == WIDE_COL else 1200)))
    if kind == 1:
        return edges_f64([1, 3][int(rng.integers(0, 2))], np.sort(rng.integers(-8, 9, int(rng.integers(0, 9))) / 4.0))
    if kind == 2:
        return edges_i64([0, 2, WIDE_COL][int(rng.integers(0, 3))], np.sort(rng.integers(-6, 1100, int(rng.integers(0, 40)))))
    return edges_i64(WIDE_COL, np.sort(rng.integers(-3, 2 * WINDOW + 10, int(rng.integers(WINDOW, WINDOW + 300)))))
