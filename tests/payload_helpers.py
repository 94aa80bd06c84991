"""The numpy restatement of payload filters (include/hrag.h, "payload filters") and builders of random indexes and clause
programs.  One boolean array per clause, combined by role, then pack_mask: there is no tolerance anywhere in this feature,
every comparison is assert_array_equal on words."""

import numpy as np

from hipporag_amd._lib import (PAY_F64, PAY_I64, PAY_IN, PAY_MAX_CLAUSES, PAY_MUST, PAY_MUST_NOT, PAY_PRESENT, PAY_RANGE,
                               PAY_SHOULD, PAY_TILE)
from hipporag_amd.engine import pack_mask

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


def bits(x):
    """doubles -> the int64 words the ABI carries"""
    return np.asarray(x, np.float64).view(np.int64)


def op(role, kind):
    return int(role) | int(kind) << 8


def clamp_range(ptr, i, limit):
    beg = min(max(int(ptr[i]), 0), limit)
    end = min(max(int(ptr[i + 1]), beg), limit)
    return beg, end


def clause_hits(n, cols, col, o, lo, hi, svals):
    """(role, hit bool [n]) of one clause; an ill-formed clause hits nothing, an unknown role counts as MUST."""
    role, kind, high = o & 0xFF, (o >> 8) & 0xFF, o >> 16
    dead = high != 0 or not 0 <= col < len(cols) or kind > PAY_PRESENT or role > PAY_SHOULD
    if role > PAY_SHOULD or high != 0:
        role = PAY_MUST
    if dead:
        return role, np.zeros(n, bool)
    typ, values, present = cols[col]
    present = np.ones(n, bool) if present is None else np.asarray(present, bool)
    with np.errstate(invalid="ignore"):
        if kind == PAY_PRESENT:
            test = np.ones(n, bool)
        elif kind == PAY_RANGE:
            if typ == PAY_F64:
                x, a, b = values.view(np.float64), np.int64(lo).view(np.float64), np.int64(hi).view(np.float64)
            else:
                x, a, b = values, np.int64(lo), np.int64(hi)
            test = (a <= x) & (x <= b) if a <= b else np.zeros(n, bool)
        else:
            x, s = (values.view(np.float64), svals.view(np.float64)) if typ == PAY_F64 else (values, svals)
            test = (x[:, None] == s[None, :]).any(axis=1) if s.size else np.zeros(n, bool)
    return role, present & test


def payload_filter_np(n, cols, prog, batch, base=None, cap=PAY_MAX_CLAUSES):
    """allowed bool [batch, n] by the header's definition.  cols: (type, int64 values [n], present bool [n] or None) per
    column; prog: (f_ptr, c_col, c_op, c_lo, c_hi, c_set_ptr, set_vals); base: None, bool [n] or bool [batch, n]."""
    f_ptr, c_col, c_op, c_lo, c_hi, c_set_ptr, set_vals = prog
    nc, nnz = len(c_col), len(set_vals)
    out = np.zeros((batch, n), bool)
    for b in range(batch):
        allowed = np.ones(n, bool) if base is None else np.array(base[b] if np.ndim(base) == 2 else base, bool)
        beg, end = clamp_range(f_ptr, b, nc) if nc else (0, 0)
        should, has_should = np.zeros(n, bool), False
        for j in range(beg, min(end, beg + cap)):
            sb, se = clamp_range(c_set_ptr, j, nnz)
            role, hit = clause_hits(n, cols, int(c_col[j]), int(c_op[j]), int(c_lo[j]), int(c_hi[j]),
                                    np.asarray(set_vals[sb:se], np.int64))
            if role == PAY_MUST:
                allowed &= hit
            elif role == PAY_MUST_NOT:
                allowed &= ~hit
            else:
                has_should, should = True, should | hit
        out[b] = allowed & should if has_should else allowed
    return out


def payload_words_np(n, cols, prog, batch, base=None, cap=PAY_MAX_CLAUSES):
    return pack_mask(payload_filter_np(n, cols, prog, batch, base, cap))


def popcount_rows_np(words, n):
    """set bits among the first n of each row of uint32 words [B, >= ceil(n / 32)]"""
    w = np.ascontiguousarray(np.asarray(words, np.uint32)[:, :(n + 31) // 32])
    b = np.unpackbits(w.view(np.uint8), axis=1, bitorder="little")[:, :n]
    return b.sum(axis=1).astype(np.int32)


# ---------------------------------------------------------------------------------- builders
F64_SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308 / 4, 1.5, -1.5])
SET_1000 = np.arange(0, 2000, 2, dtype=np.int64)          # the 1000-value IN set of column 2 (codes 0 .. 999 live there)


def make_columns(rng, n):
    """Four columns: I64 with the int64 extremes and holes; F64 with NaN, +-inf, +-0.0, denormals and holes; I64 codes
    0 .. 999 without a presence bitset; F64 without one."""
    a = rng.integers(-5, 6, n).astype(np.int64)
    a[rng.random(n) < 0.1] = I64_MIN
    a[rng.random(n) < 0.1] = I64_MAX
    f = (rng.integers(-8, 9, n) / 4.0).astype(np.float64)
    sp = rng.random(n) < 0.5
    f[sp] = F64_SPECIALS[rng.integers(0, len(F64_SPECIALS), int(sp.sum()))]
    codes = rng.integers(0, 1000, n).astype(np.int64)
    g = rng.standard_normal(n)
    pa, pf = rng.random(n) < 0.7, rng.random(n) < 0.6
    if n > 40:
        pa[32:64] = False                                 # a whole presence word of zeros
    return [(PAY_I64, a, pa), (PAY_F64, bits(f), pf), (PAY_I64, codes, None), (PAY_F64, bits(g), None)]


def host_arrays(cols):
    """(types int32, values list, present words list-or-None) as hrag_payload_create takes them"""
    return (np.asarray([c[0] for c in cols], np.int32), [np.ascontiguousarray(c[1], np.int64) for c in cols],
            [None if c[2] is None else pack_mask(c[2]) for c in cols])


FULL_I64 = (0, op(PAY_MUST, PAY_RANGE), I64_MIN, I64_MAX, None)


def special_programs():
    """name -> list of clauses (col, op, lo, hi, set values or None): every case the header's definition names."""
    r, i_, p = PAY_RANGE, PAY_IN, PAY_PRESENT
    m, mn, s = PAY_MUST, PAY_MUST_NOT, PAY_SHOULD
    small = np.array([-3, 0, 2], np.int64)
    fl = lambda *v: bits(np.sort(np.asarray(v, np.float64)))
    return {
        "empty": [],
        "must": [(0, op(m, r), -2, 3, None)],
        "must_not": [(0, op(mn, r), -2, 3, None)],
        "must_not of a missing value": [(0, op(mn, p), 0, 0, None)],
        "should": [(0, op(s, i_), 0, 0, small), (1, op(s, r), bits(0.25), bits(np.inf), None)],
        "all roles": [(2, op(m, r), 100, 899, None), (0, op(mn, i_), 0, 0, small), (1, op(s, p), 0, 0, None),
                      (3, op(s, r), bits(-0.5), bits(0.5), None)],
        "64 clauses": [FULL_I64] * 63 + [(2, op(m, r), 0, 499, None)],
        "65 clauses": [FULL_I64] * 64 + [(2, op(m, i_), 0, 0, np.zeros(0, np.int64))],     # the 65th would allow nothing
        "empty set": [(2, op(m, i_), 0, 0, np.zeros(0, np.int64))],
        "empty set, must_not": [(2, op(mn, i_), 0, 0, np.zeros(0, np.int64))],
        "one value": [(2, op(m, i_), 0, 0, np.array([7], np.int64))],
        "1000 values": [(2, op(m, i_), 0, 0, SET_1000)],
        "lo > hi": [(0, op(m, r), 3, -2, None)],
        "lo > hi, f64": [(1, op(s, r), bits(1.0), bits(0.5), None)],
        "nan bound": [(1, op(mn, r), bits(np.nan), bits(np.inf), None)],
        "full range": [FULL_I64],
        "full range, f64": [(1, op(m, r), bits(-np.inf), bits(np.inf), None)],           # everything present but NaN
        "extremes": [(0, op(m, i_), 0, 0, np.array([I64_MIN, I64_MAX], np.int64))],
        "min only": [(0, op(m, r), I64_MIN, I64_MIN, None)],
        "zeros": [(1, op(m, i_), 0, 0, fl(0.0))],                                        # -0.0 matches 0.0
        "negative zero bounds": [(1, op(m, r), bits(-0.0), bits(-0.0), None)],
        "nan in no set": [(1, op(m, i_), 0, 0, fl(-np.inf, 5e-324, np.inf))],
        "denormal range": [(1, op(m, r), bits(-5e-324), bits(1e-308), None)],
        "column out of range": [(4, op(m, p), 0, 0, None)],
        "negative column, must_not": [(-1, op(mn, p), 0, 0, None)],
        "unknown kind": [(0, op(mn, 3), I64_MIN, I64_MAX, None), (0, op(s, 200), 0, 0, None)],
        "unknown role": [(0, op(3, p), 0, 0, None)],
        "high op bits": [(0, op(mn, p) | 1 << 16, 0, 0, None)],
        "present": [(0, op(m, p), 0, 0, None), (1, op(m, p), 0, 0, None)],
    }


def random_program(rng, n_cols=4):
    out = []
    for _ in range(int(rng.integers(1, 6))):
        col = int(rng.integers(0, n_cols))
        role = int(rng.integers(0, 3))
        kind = int(rng.integers(0, 3))
        f64 = col in (1, 3)
        if kind == PAY_RANGE:
            if f64:
                lo = float(rng.integers(-8, 9)) / 4
                c = (col, op(role, kind), int(bits(lo)), int(bits(lo + float(rng.integers(0, 8)) / 4)), None)
            else:
                lo = int(rng.integers(-6, 500))
                c = (col, op(role, kind), lo, lo + int(rng.integers(0, 400)), None)
        elif kind == PAY_IN:
            if f64:
                v = bits(np.unique(np.concatenate([rng.integers(-8, 9, 4) / 4.0, [np.inf]])))
            else:
                v = np.unique(rng.integers(-5, 30, int(rng.integers(0, 12)))).astype(np.int64)
            c = (col, op(role, kind), 0, 0, v)
        else:
            c = (col, op(role, kind), 0, 0, None)
        out.append(c)
    return out


def assemble(programs):
    """per-query clause lists -> the CSR arrays (f_ptr, c_col, c_op, c_lo, c_hi, c_set_ptr, set_vals)"""
    f_ptr, cols, ops, los, his, sp, sets = [0], [], [], [], [], [0], []
    nnz = 0
    for prog in programs:
        for col, o, lo, hi, vals in prog:
            cols.append(col)
            ops.append(o)
            los.append(int(lo))
            his.append(int(hi))
            if vals is not None and len(vals):
                sets.append(np.asarray(vals, np.int64))
                nnz += len(vals)
            sp.append(nnz)
        f_ptr.append(len(cols))
    return (np.asarray(f_ptr, np.int32), np.asarray(cols, np.int32), np.asarray(ops, np.int32), np.asarray(los, np.int64),
            np.asarray(his, np.int64), np.asarray(sp, np.int32),
            np.concatenate(sets) if sets else np.zeros(0, np.int64))


def make_programs(rng, b):
    """b = 1: the query at exactly the cap; b = 3: all roles, the 1000-value set, a random one; larger: every special
    program in order, then random ones."""
    sp = special_programs()
    if b == 1:
        return [sp["64 clauses"]]
    if b == 3:
        return [sp["all roles"], sp["1000 values"], random_program(rng)]
    progs = list(sp.values())
    assert b >= len(progs)
    return progs + [random_program(rng) for _ in range(b - len(progs))]


# ---------------------------------------------------------------------------------- random metadata for the grammar
def random_metadata(rng, n):
    """n metadata dicts of hashable scalars over a few keys, some missing: ints, bools, floats, strs."""
    users = ["alice", "bob", "carol", "dave"]
    out = []
    for _ in range(n):
        m = {}
        if rng.random() < 0.8:
            m["year"] = int(rng.integers(2018, 2024))
        if rng.random() < 0.7:
            m["user"] = users[int(rng.integers(0, 4))]
        if rng.random() < 0.6:
            m["score"] = float(rng.integers(0, 8)) / 2
        if rng.random() < 0.5:
            m["flag"] = bool(rng.integers(0, 2))
        if rng.random() < 0.5:
            m["mixed"] = [1, 2.5, 3][int(rng.integers(0, 3))]           # ints and floats: an F64 column
        out.append(m)
    return out


def columns_of(meta, keys=None):
    keys = keys or list(dict.fromkeys(k for m in meta for k in m))
    return {k: [m.get(k) for m in meta] for k in keys}


def cols_for_restatement(pc):
    """a PayloadColumns as the (type, values, present bool) triples payload_filter_np takes"""
    from hipporag_amd.retriever import unpack_mask
    n = pc.n_passages
    return [(t, v, None if p is None else unpack_mask(p, n)) for t, v, p in zip(pc.types, pc.values, pc.present)]
