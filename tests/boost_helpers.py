"""The numpy restatement of boosted retrieval (include/hrag.h, "boosted retrieval"), written from the header's definition:
exp_dec_np, boost_rows_np (vectorised over the passages, float64 operation by operation) and boost_rows_naive (a Python
loop over every element with Python floats, which are IEEE doubles rounded operation by operation), plus builders of random
term programs.  There is no tolerance anywhere in this feature: every comparison of score rows is on their bits."""

import math

import numpy as np

from hipporag_amd._lib import (BOOST_ADD, BOOST_CONST, BOOST_DECAY, BOOST_EXP, BOOST_FIELD, BOOST_GAUSS, BOOST_HAS_MISSING,
                               BOOST_LINEAR, BOOST_MAX_TERMS, BOOST_MUL, BOOST_NONE, BOOST_SQRT, PAY_F64, PAY_I64,
                               PAY_MAX_CLAUSES, PAY_MUST, PAY_MUST_NOT, PAY_RANGE)
from tests.payload_helpers import (FULL_I64, assemble, bits, clamp_range, clause_hits, make_columns, op, random_program,
                                   special_programs)

LOG2E = float.fromhex("0x1.71547652b82fep+0")
LN2_HI = float.fromhex("0x1.62e42fee00000p-1")
LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
EXP_C = [1.0 / math.factorial(i) for i in range(14)]        # c_i = fp64(1 / i!): an exact integer divided once
QNAN32 = np.uint32(0x7FC00000)


# ------------------------------------------------------------------------------------------ exp_dec
def exp_dec_np(x):
    """exp_dec of the header on a float64 array (or scalar): the same sequence of rounded float64 operations."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        xx = np.where(x > 0.0, 0.0, x)
        live = xx >= -708.0                                     # (False for NaN)
        z = np.where(live, xx, 0.0)
        k = np.rint(z * LOG2E)
        r = (z - k * LN2_HI) - k * LN2_LO
        p = np.full(z.shape, EXP_C[13])
        for i in range(12, -1, -1):
            p = p * r + EXP_C[i]                                # two rounded operations: numpy does not fuse
        out = np.ldexp(p, k.astype(np.int32))
        out = np.where(live, out, 0.0)
    return np.where(np.isnan(x), x, out)


def exp_dec_scalar(x: float) -> float:
    """exp_dec with Python floats, one element."""
    if x != x:
        return x
    if x > 0.0:
        x = 0.0
    if x < -708.0:
        return 0.0
    k = float(round(x * LOG2E))                                 # round(): half to even, as rint
    r = (x - k * LN2_HI) - k * LN2_LO
    p = EXP_C[13]
    for i in range(12, -1, -1):
        p = p * r
        p = p + EXP_C[i]
    return math.ldexp(p, int(k))


# ------------------------------------------------------------------------------------------ the definition
def _pos(y):
    return np.where(y > 0.0, y, 0.0)            # fmax(0, y): +0.0 for NaN and for -0.0


def _decode(op, col, n_cols):
    """(kind, mode, sub, has_missing) of a well-formed term, None of an ill-formed (neutral) one."""
    kind, mode, sub, has, high = op & 0xFF, (op >> 8) & 0xFF, (op >> 16) & 0xFF, (op >> 24) & 1, op >> 25
    if high != 0 or kind > BOOST_DECAY or mode > BOOST_ADD:
        return None
    if sub > (BOOST_GAUSS if kind == BOOST_DECAY else BOOST_SQRT if kind == BOOST_FIELD else 0):
        return None
    if kind != BOOST_CONST and not 0 <= col < n_cols:
        return None
    return kind, mode, sub, has


def _query_terms(prog, q, broadcast):
    """[(term index, clause begin, clauses taken)] of query q: both pointer ranges clamped, the caps applied in term order."""
    t_ptr, t_op, t_cl_ptr = prog[0], prog[1], prog[4]
    n_terms, n_clauses = len(t_op), len(prog[5])
    if n_terms == 0:
        return []
    beg, end = clamp_range(t_ptr, 0 if broadcast else q, n_terms)
    out, used = [], 0
    for j in range(beg, min(end, beg + BOOST_MAX_TERMS)):
        cb, ce = clamp_range(t_cl_ptr, j, n_clauses)
        take = min(ce - cb, PAY_MAX_CLAUSES - used)
        out.append((j, cb, take))
        used += take
    return out


def _condition(n, cols, prog, cb, take):
    """hit bool [n] of the clauses cb .. cb + take: the payload filter's rule without base words; empty: true."""
    c_col, c_op, c_lo, c_hi, c_set_ptr, set_vals = prog[5:]
    allowed, should, has_should = np.ones(n, bool), np.zeros(n, bool), False
    for j in range(cb, cb + take):
        sb, se = clamp_range(c_set_ptr, j, len(set_vals))
        role, hit = clause_hits(n, cols, int(c_col[j]), int(c_op[j]), int(c_lo[j]), int(c_hi[j]),
                                np.asarray(set_vals[sb:se], np.int64))
        if role == PAY_MUST:
            allowed &= hit
        elif role == PAY_MUST_NOT:
            allowed &= ~hit
        else:
            has_should, should = True, should | hit
    return allowed & should if has_should else allowed


def _column(cols, col, n):
    """(x float64 [n], have bool [n]) of a column: an I64 value converted to nearest-even, NaN and absent values missing."""
    typ, values, present = cols[col]
    x = values.view(np.float64) if typ == PAY_F64 else values.astype(np.float64)
    have = np.ones(n, bool) if present is None else np.asarray(present, bool).copy()
    return x, have & ~np.isnan(x)


def _store(s, M, A):
    with np.errstate(all="ignore"):
        out = ((s.astype(np.float64) * M) + A).astype(np.float32)
    u = out.view(np.uint32).copy()
    u[np.isnan(out)] = QNAN32
    return u.view(np.float32)


def _entries(row, mn, mx):
    """The fp32 entries the boost reads: the row, or its min-max by the library's rule (a zero range gives 1)."""
    s = np.asarray(row, np.float32)
    if mn is None:
        return s
    with np.errstate(all="ignore"):
        rng = np.float32(mx) - np.float32(mn)
        return np.ones_like(s) if rng == 0 else ((s - np.float32(mn)) / rng).astype(np.float32)


def boost_rows_np(rows, n, cols, prog, broadcast=False, mn=None, mx=None):
    """rows fp32 [B, ld >= n] boosted by the header's definition (a copy; the columns n .. ld and the rows of queries without
    terms keep their bits).  cols: (type, int64 values [n], present bool [n] or None) per column; prog: the eleven arrays
    (t_ptr, t_op, t_col, t_num [.., 5], t_cl_ptr, c_col, c_op, c_lo, c_hi, c_set_ptr, set_vals)."""
    out = np.array(rows, np.float32, copy=True)
    t_op, t_col, t_num = prog[1], prog[2], np.asarray(prog[3], np.float64).reshape(-1, 5)
    for q in range(out.shape[0]):
        terms = _query_terms(prog, q, broadcast)
        if not terms:
            continue
        s = _entries(out[q, :n], None if mn is None else mn[q], None if mx is None else mx[q])
        M, A = np.ones(n), np.zeros(n)
        for j, cb, take in terms:
            dec = _decode(int(t_op[j]), int(t_col[j]), len(cols))
            if dec is None:
                continue
            kind, mode, sub, has = dec
            w, p0, p1, p2, missing = (np.float64(v) for v in t_num[j])
            hit = _condition(n, cols, prog, cb, take)
            with np.errstate(all="ignore"):
                if kind == BOOST_CONST:
                    v = np.ones(n)
                else:
                    x, have = _column(cols, int(t_col[j]), n)
                    if kind == BOOST_FIELD:
                        v = np.sqrt(x) if sub == BOOST_SQRT else x
                    else:
                        d = _pos(np.abs(x - p0) - p1)
                        if sub == BOOST_LINEAR:
                            v = _pos((p2 - d) / p2)
                        elif sub == BOOST_EXP:
                            v = exp_dec_np(p2 * d)
                        else:
                            v = exp_dec_np(p2 * (d * d))
                    if has:
                        v = np.where(have, v, missing)
                    else:
                        hit = hit & have
                t = w * v
                if mode == BOOST_MUL:
                    M = np.where(hit, M * t, M)
                else:
                    A = np.where(hit, A + t, A)
        out[q, :n] = _store(s, M, A)
    return out


def boost_rows_naive(rows, n, cols, prog, broadcast=False, mn=None, mx=None):
    """boost_rows_np as a loop over every element with Python floats."""
    out = np.array(rows, np.float32, copy=True)
    t_op, t_col, t_num = prog[1], prog[2], np.asarray(prog[3], np.float64).reshape(-1, 5)
    for q in range(out.shape[0]):
        terms = _query_terms(prog, q, broadcast)
        if not terms:
            continue
        conds = [_condition(n, cols, prog, cb, take) for _, cb, take in terms]
        s32 = _entries(out[q, :n], None if mn is None else mn[q], None if mx is None else mx[q])
        for p in range(n):
            M, A = 1.0, 0.0
            for (j, _, _), cond in zip(terms, conds):
                dec = _decode(int(t_op[j]), int(t_col[j]), len(cols))
                if dec is None or not cond[p]:
                    continue
                kind, mode, sub, has = dec
                w, p0, p1, p2, missing = (float(v) for v in t_num[j])
                if kind == BOOST_CONST:
                    v = 1.0
                else:
                    typ, values, present = cols[int(t_col[j])]
                    have = present is None or bool(present[p])
                    x = float(values.view(np.float64)[p]) if typ == PAY_F64 else float(int(values[p]))
                    if not have or x != x:
                        if not has:
                            continue
                        v = missing
                    elif kind == BOOST_FIELD:
                        v = x if sub != BOOST_SQRT else (math.sqrt(x) if x >= 0 else math.nan)      # (sqrt(-0.0) is -0.0)
                    else:
                        d = abs(x - p0) - p1
                        d = d if d > 0.0 else 0.0
                        if sub == BOOST_LINEAR:
                            with np.errstate(all="ignore"):      # (Python raises on a division by zero; IEEE does not)
                                y = float(np.float64(p2 - d) / np.float64(p2))
                            v = y if y > 0.0 else 0.0
                        else:
                            a = p2 * d if sub == BOOST_EXP else p2 * (d * d)
                            v = exp_dec_scalar(a)
                t = w * v
                if mode == BOOST_MUL:
                    M = M * t
                else:
                    A = A + t
            with np.errstate(all="ignore"):
                f = np.float64(float(s32[p]) * M) + np.float64(A)
                f = np.float32(f)
            out[q, p] = f
            if f != f:
                out[q, p:p + 1].view(np.uint32)[0] = QNAN32
    return out


# ------------------------------------------------------------------------------------------ builders
def term(kind, mode, sub=0, col=0, w=1.0, p=(0.0, 0.0, 0.0), missing=None, clauses=()):
    """One term as (t_op, col, [w, p0, p1, p2, missing], clauses)."""
    o = kind | mode << 8 | sub << 16 | (BOOST_HAS_MISSING if missing is not None else 0)
    return o, col, [w, p[0], p[1], p[2], 0.0 if missing is None else missing], list(clauses)


def decay_c(sub, scale, decay=0.5):
    return scale / (1.0 - decay) if sub == BOOST_LINEAR else math.log(decay) / scale if sub == BOOST_EXP \
        else math.log(decay) / (scale * scale)


def assemble_boost(per_query):
    """per-query lists of term() tuples -> the eleven arrays of a program."""
    t_ptr, ops, cols, nums, cl_ptr, clauses = [0], [], [], [], [0], []
    for terms in per_query:
        for o, col, num, cl in terms:
            ops.append(o)
            cols.append(col)
            nums.append(num)
            clauses.extend(cl)
            cl_ptr.append(len(clauses))
        t_ptr.append(len(ops))
    _, c_col, c_op, c_lo, c_hi, c_set_ptr, set_vals = assemble([clauses])
    return (np.asarray(t_ptr, np.int32), np.asarray(ops, np.int32), np.asarray(cols, np.int32),
            np.asarray(nums, np.float64).reshape(len(ops), 5), np.asarray(cl_ptr, np.int32), c_col, c_op, c_lo, c_hi,
            c_set_ptr, set_vals)


def random_term(rng, n_cols=4, f64_cols=(1, 3)):
    """A well-formed random term over payload_helpers.make_columns' four columns."""
    kind = int(rng.integers(0, 3))
    mode = int(rng.integers(0, 2))
    col = int(rng.integers(0, n_cols))
    w = float(rng.choice([1.5, 0.5, -0.75, 0.0, 2.0, float(rng.standard_normal())]))
    missing = None if kind == BOOST_CONST or rng.random() < 0.5 else float(rng.choice([0.0, 1.0, -2.5]))
    clauses = random_program(rng, n_cols)[:int(rng.integers(0, 4))]
    sub, p = 0, (0.0, 0.0, 0.0)
    if kind == BOOST_FIELD:
        sub = int(rng.integers(0, 2))
    elif kind == BOOST_DECAY:
        sub = int(rng.integers(0, 3))
        scale = float(rng.choice([0.5, 2.0, 3.0, 100.0]))
        p = (float(rng.integers(-4, 5)) / 2, float(rng.choice([0.0, 0.0, 0.5, 2.0])), decay_c(sub, scale, float(rng.choice([0.5, 0.25, 0.9]))))
    return term(kind, mode, sub, col, w, p, missing, clauses)


def random_terms(rng, n_terms=None):
    return [random_term(rng) for _ in range(int(rng.integers(0, 6)) if n_terms is None else n_terms)]


def random_f64_column(rng, n, spread=50.0):
    """n finite doubles with full mantissas (what shows a contracted fma) as int64 words."""
    return bits(rng.standard_normal(n) * spread)


def boost_columns(rng, n):
    """payload_helpers.make_columns' four columns (int64 extremes -- beyond 2^53 --, NaN, +-inf, +-0.0, denormals, holes),
    a fifth of random doubles with full mantissas, a sixth of odd integers beyond 2^53 with holes, a seventh of small
    integers without holes."""
    big = (1 << 53) + 1 + 2 * rng.integers(0, 1 << 20, n).astype(np.int64)
    big[rng.random(n) < 0.3] *= -1
    return make_columns(rng, n) + [(PAY_F64, random_f64_column(rng, n), None), (PAY_I64, big, rng.random(n) < 0.8),
                                   (PAY_I64, rng.integers(-6, 7, n).astype(np.int64), None)]


# ---------------------------------------------------------------------------------- the programs
def special_boosts():
    """name -> the terms of one query: every case the header's definition names.  Columns: boost_columns."""
    C_, F, D, mul, add = BOOST_CONST, BOOST_FIELD, BOOST_DECAY, BOOST_MUL, BOOST_ADD
    r = PAY_RANGE
    sp = special_programs()
    lin2 = decay_c(BOOST_LINEAR, 2.0)            # c = 4: d = 4 is exactly c
    out = {
        "no terms": [],
        "const mul": [term(C_, mul, w=1.5, clauses=sp["must"])],
        "const add": [term(C_, add, w=-0.25, clauses=sp["must_not"])],
        "const should": [term(C_, mul, w=0.5, clauses=sp["should"])],
        "const all roles": [term(C_, add, w=2.0, clauses=sp["all roles"])],
        "const everywhere": [term(C_, mul, w=-3.0)],
        "zero weight": [term(C_, mul, w=0.0, clauses=sp["must"]), term(F, add, col=3, w=0.0)],
        "field i64": [term(F, mul, BOOST_NONE, col=0, w=1e-18)],
        "field f64 specials": [term(F, add, BOOST_NONE, col=1, w=0.5)],
        "field missing": [term(F, mul, BOOST_NONE, col=1, w=2.0, missing=-1.0), term(F, add, BOOST_SQRT, col=0, missing=0.25)],
        "sqrt": [term(F, add, BOOST_SQRT, col=3, w=1.0)],                      # NaN below zero
        "sqrt specials": [term(F, mul, BOOST_SQRT, col=1, w=1.0)],             # -0.0, denormals, +inf
        "beyond 2^53": [term(F, add, BOOST_NONE, col=5, w=2.0 ** -53), term(F, mul, BOOST_SQRT, col=5, w=1e-8, missing=3.0)],
        "linear": [term(D, mul, BOOST_LINEAR, col=6, p=(1.0, 0.0, lin2))],     # d in 0 .. 7: 0 exactly, c exactly, beyond c
        "linear offset": [term(D, add, BOOST_LINEAR, col=6, w=3.0, p=(0.0, 2.0, lin2))],        # inside the offset: d = 0
        "exp": [term(D, mul, BOOST_EXP, col=4, p=(0.5, 1.0, decay_c(BOOST_EXP, 30.0)))],
        "exp to zero": [term(D, mul, BOOST_EXP, col=0, p=(0.0, 0.0, decay_c(BOOST_EXP, 1e-3))),     # the int64 extremes
                        term(D, add, BOOST_EXP, col=6, w=1.0, p=(0.0, 0.0, -200.0))],              # d >= 4: below -708
        "gauss": [term(D, add, BOOST_GAUSS, col=4, w=-1.5, p=(-3.0, 0.25, decay_c(BOOST_GAUSS, 40.0, 0.3)))],
        "gauss specials": [term(D, mul, BOOST_GAUSS, col=1, p=(0.0, 0.0, decay_c(BOOST_GAUSS, 1.0)), missing=0.5)],
        "decay under a condition": [term(D, mul, BOOST_EXP, col=3, p=(0.0, 0.1, -0.7), clauses=sp["1000 values"])],
        "mixed": [term(C_, mul, w=1.5, clauses=sp["one value"]), term(D, mul, BOOST_EXP, col=4, p=(10.0, 0.0, -0.01)),
                  term(F, add, BOOST_SQRT, col=3, w=0.125, missing=0.0), term(C_, mul, w=0.5, clauses=sp["must_not"]),
                  term(D, add, BOOST_LINEAR, col=0, w=-2.0, p=(0.0, 1.0, 8.0))],
        "32 terms": [term(C_, mul, w=1.0 + 2.0 ** -20, clauses=[FULL_I64] * 2) for _ in range(31)] + [term(F, add, col=3, clauses=[FULL_I64] * 2)],
        "33 terms": [term(C_, add, w=0.5)] * 32 + [term(C_, mul, w=0.0)],      # the 33rd would zero everything
        "64 clauses": [term(C_, mul, w=2.0, clauses=[FULL_I64] * 31 + sp["must"]),
                       term(C_, add, w=1.0, clauses=[FULL_I64] * 31 + [(2, op(PAY_MUST, r), 0, 499, None)])],
        "65 clauses": [term(C_, mul, w=2.0, clauses=[FULL_I64] * 32), term(C_, add, w=1.0, clauses=[FULL_I64] * 32 + sp["lo > hi"]),
                       term(C_, add, w=7.0, clauses=sp["lo > hi"])],           # the 65th and 66th clause would have hit nothing:
        #                                                                        ignored, the third term hits everywhere
        "bad column": [term(F, mul, col=7, w=0.0), term(D, mul, BOOST_EXP, col=-1, w=0.0, p=(0.0, 0.0, -1.0)), term(C_, add, col=99)],
        "bad kind": [term(3, mul, w=0.0), term(200, add, w=5.0), term(C_, add, w=1.0)],
        "bad mode": [term(C_, 2, w=0.0), term(F, 255, col=3), term(C_, mul, w=2.0)],
        "bad sub": [term(C_, mul, 1, w=0.0), term(F, mul, 2, col=3, w=0.0), term(D, mul, 3, col=3, w=0.0), term(C_, add, w=0.5)],
        "high op bits": [(term(C_, mul, w=0.0)[0] | 1 << 25,) + term(C_, mul, w=0.0)[1:], term(C_, add, w=0.5)],
        "bad clause": [term(C_, mul, w=0.0, clauses=sp["column out of range"]), term(C_, add, w=1.0, clauses=sp["unknown role"]),
                       term(C_, add, w=2.0, clauses=sp["negative column, must_not"])],
    }
    assert len(out["64 clauses"][0][3]) + len(out["64 clauses"][1][3]) == 64
    assert len(out["32 terms"]) == 32 and sum(len(t[3]) for t in out["32 terms"]) == 64
    assert sum(len(t[3]) for t in out["65 clauses"][:2]) == 65
    return out


def make_boosts(rng, b):
    """b = 1: the query at both caps; b = 3: mixed, no terms, a random one; b = 65: every special program, then random ones."""
    sp = special_boosts()
    if b == 1:
        return [sp["32 terms"]]
    if b == 3:
        return [sp["mixed"], sp["no terms"], random_terms(rng, 4)]
    progs = list(sp.values())
    assert b >= len(progs)
    return progs + [random_terms(rng) for _ in range(b - len(progs))]
