"""numpy restatement of recommend by example (include/hrag.h, "recommend by example"): the two row strategies over the
matrix of s(p, e), the average_vector query and the exclusion.  Written from the definitions, not from csrc/reco.hip: the
sequential fp64 sums are explicit loops over the examples in list order (np.sum is pairwise and is not the definition), the
`>` maximum is written out.  tests/test_reco_host.py holds it to a brute-force fp64 statement of Qdrant's formulas."""

import numpy as np

from hipporag_amd.graph import float_to_bf16_bits
from tests.helpers import split_f32_np
from tests.mmr_helpers import bf16_round, same_bits  # noqa: F401  (re-exported for the tests)

RECO_MAX_EXAMPLES = 32        # HRAG_RECO_MAX_EXAMPLES
RECO_TILE = 128               # HRAG_RECO_TILE
QNAN = np.array([0x7fc00000], np.uint32).view(np.float32)[0]
EMPTY_IDS = (-1, None, 2 ** 31 - 1)      # None: n + 5


def effective_sign(ex_idx, ex_sign, n):
    """The sign of every example as the device reads it: 0 for an empty example (id outside [0, n) or sign 0)."""
    idx, sg = np.asarray(ex_idx, np.int64), np.sign(np.asarray(ex_sign, np.int64))
    return np.where((idx >= 0) & (idx < n), sg, 0).astype(np.int32)


def reco_rows_np(s, ex_ptr, sign, mode):
    """s fp32 [E, n] (row ex_ptr[b] + e: s(., e) of query b's example e), sign int [E] (0: empty) -> fp32 [B, n]"""
    s = np.asarray(s, np.float32)
    ptr = np.asarray(ex_ptr, np.int64)
    b, n = ptr.shape[0] - 1, s.shape[1]
    out = np.empty((b, n), np.float32)
    with np.errstate(all="ignore"):
        for q in range(b):
            lo, hi = int(ptr[q]), int(min(ptr[q + 1], ptr[q] + RECO_MAX_EXAMPLES))
            if mode == "best_score":
                bp = np.full(n, -np.inf, np.float32)
                bn = np.full(n, -np.inf, np.float32)
                for e in range(lo, hi):
                    if sign[e] > 0:
                        bp = np.where(s[e] > bp, s[e], bp)
                    elif sign[e] < 0:
                        bn = np.where(s[e] > bn, s[e], bn)
                out[q] = np.where(bp > bn, bp, -(bn * bn).astype(np.float32))
            elif mode == "sum_scores":
                acc = np.zeros(n, np.float64)
                for e in range(lo, hi):
                    if sign[e] > 0:
                        acc = acc + s[e].astype(np.float64)
                for e in range(lo, hi):
                    if sign[e] < 0:
                        acc = acc - s[e].astype(np.float64)
                o = acc.astype(np.float32)
                out[q] = np.where(np.isnan(o), QNAN, o)
            else:
                raise ValueError(mode)
    return out


def tree_sum_rows_np(s, ex_ptr, sign):
    """sum_scores with a pairwise tree over the signed fp64 terms instead of the list order: what the definition is NOT"""
    s = np.asarray(s, np.float32)
    ptr = np.asarray(ex_ptr, np.int64)
    out = np.empty((ptr.shape[0] - 1, s.shape[1]), np.float32)
    for q in range(ptr.shape[0] - 1):
        terms = [s[e].astype(np.float64) * float(sign[e]) for e in range(int(ptr[q]), int(ptr[q + 1])) if sign[e]]
        while len(terms) > 1:
            terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
        out[q] = (terms[0] if terms else np.zeros(s.shape[1])).astype(np.float32)
    return out


def reco_query_np(values, ex_ptr, ex_idx, ex_sign):
    """values fp64 [n, dim] (the stored 16-bit values, or hi + lo of a split engine) -> (v fp32 [B, dim], flags int32 [B])"""
    values = np.asarray(values, np.float64)
    n, dim = values.shape
    ptr = np.asarray(ex_ptr, np.int64)
    sign = effective_sign(ex_idx, ex_sign, n)
    b = ptr.shape[0] - 1
    v, flags = np.zeros((b, dim), np.float32), np.zeros(b, np.int32)
    for q in range(b):
        sp, sn, n_pos, n_neg = np.zeros(dim, np.float64), np.zeros(dim, np.float64), 0, 0
        for e in range(int(ptr[q]), int(min(ptr[q + 1], ptr[q] + RECO_MAX_EXAMPLES))):
            if sign[e] > 0:
                sp, n_pos = sp + values[ex_idx[e]], n_pos + 1
            elif sign[e] < 0:
                sn, n_neg = sn + values[ex_idx[e]], n_neg + 1
        if n_pos == 0:
            flags[q] = 1
            continue
        a = sp / np.float64(n_pos)
        if n_neg:
            g = sn / np.float64(n_neg)
            a = a + (a - g)
        v[q] = a.astype(np.float32)
    return v, flags


def query_bits(kind, v):
    """The 16-bit query of an fp32 vector as the similarity kernels read it: uint16 [B, dim] (bf16 / fp16, round to nearest
    even) or [B, 3 dim] = [qhi | qhi | qlo] (hrag_split_f32, as_query = 1)"""
    v = np.asarray(v, np.float32)
    if kind == "bf16":
        return float_to_bf16_bits(v)
    if kind == "fp16":
        return v.astype(np.float16).view(np.uint16)
    hi, lo = split_f32_np(v)
    return np.concatenate([hi, hi, lo], axis=1).view(np.uint16)


def exclude_np(words, ex_ptr, ex_idx, ex_sign, n):
    """words uint32 [B, W] -> a copy with the bits of every query's non-empty examples cleared"""
    w = np.array(words, np.uint32, copy=True)
    ptr = np.asarray(ex_ptr, np.int64)
    sign = effective_sign(ex_idx, ex_sign, n)
    for q in range(ptr.shape[0] - 1):
        for e in range(int(ptr[q]), int(min(ptr[q + 1], ptr[q] + RECO_MAX_EXAMPLES))):
            if sign[e]:
                w[q, ex_idx[e] >> 5] &= np.uint32(~(1 << (int(ex_idx[e]) & 31)) & 0xffffffff)
    return w


def all_bits(b, n):
    w = np.full((b, (n + 31) // 32), 0xffffffff, np.uint32)
    if n % 32:
        w[:, -1] = (1 << (n % 32)) - 1
    return w


# the issue's per-query example counts (positives, negatives)
COUNTS = [(1, 0), (0, 1), (15, 1), (16, 0), (16, 1), (17, 15), (32, 0), (1, 31)]


def make_examples(rng, n, counts, shuffle=True):
    """A ragged batch in CSR form: query i holds counts[i] = (positives, negatives) ids in [0, n); every query of three or
    more examples carries a repeated id and an empty id (-1, n + 5, 2^31 - 1 in turn); the signs of every other query are
    interleaved (a list need not hold its positives first).  -> (ex_ptr int32, ex_idx int32, ex_sign int32)"""
    ptr, idx, sign = [0], [], []
    for i, (n_pos, n_neg) in enumerate(counts):
        tot = n_pos + n_neg
        ids = rng.integers(0, n, tot).astype(np.int64)
        sg = np.array([1] * n_pos + [-1] * n_neg, np.int64)
        if shuffle and i % 2:
            sg = sg[rng.permutation(tot)]
        if tot >= 3:
            ids[1] = ids[0]
            empty = EMPTY_IDS[i % 3]
            ids[2 + int(rng.integers(0, tot - 2))] = n + 5 if empty is None else empty
        idx.append(ids)
        sign.append(sg)
        ptr.append(ptr[-1] + tot)
    return np.asarray(ptr, np.int32), np.concatenate(idx).astype(np.int32), np.concatenate(sign).astype(np.int32)


def ordered_sum_case():
    """Four example scores whose list-order fp64 sum and pairwise-tree sum differ in the last fp32 bit: 1 + 2^-24 is an
    fp32 rounding tie (to even: 1.0); in list order each 2^-53 is half an fp64 ulp of the running sum and is rounded away
    (ties to even), the tree adds 2^-53 + 2^-53 = 2^-52 first and the sum lands above the tie: 1 + 2^-23.  Every value is a
    power of two, so bf16 holds it.  -> (scores fp32 [4], list-order result, tree result)"""
    s = np.array([1.0, 2.0 ** -24, 2.0 ** -53, 2.0 ** -53], np.float32)
    return s, np.float32(1.0), np.float32(1.0 + 2.0 ** -23)
