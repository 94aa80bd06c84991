"""Boosted retrieval (include/hrag.h, boosted retrieval): the boost grammar compiled to the term programs hrag_boost_rows
evaluates over the columns of a payload index, and the engine-free binding of that call.  compile_boosts is host code: a
PayloadColumns stands in for the index there, as it does for compile_filters."""

from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional

import numpy as np

from . import _lib
from ._lib import (BOOST_ADD, BOOST_CONST, BOOST_DECAY, BOOST_EXP, BOOST_FIELD, BOOST_GAUSS, BOOST_HAS_MISSING, BOOST_LINEAR,
                   BOOST_MAX_TERMS, BOOST_MUL, BOOST_NONE, BOOST_SQRT, PAY_MAX_CLAUSES, BoostProgramDesc, check)
from .payload import query_clauses

DECAY_KINDS = {"linear": BOOST_LINEAR, "exp": BOOST_EXP, "gauss": BOOST_GAUSS}
MODIFIERS = {None: BOOST_NONE, "sqrt": BOOST_SQRT}
_NUMBERS = (int, float, np.integer, np.floating)
_ITEM_KEYS = {"if", "mul", "add", "field", "modifier", "missing", "decay"}
_DECAY_KEYS = {"field", "origin", "scale", "offset", "decay", "kind"}


def _finite(v, what) -> float:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, _NUMBERS):
        raise ValueError(f"{what}: a number expected, not {v!r}")
    try:
        f = float(v)
    except OverflowError:
        f = math.inf
    if not math.isfinite(f):
        raise ValueError(f"{what}: {v!r} is not a finite double")
    return f


def _column(index, field, what) -> int:
    try:
        cid = index.column_id(field)
    except (ValueError, TypeError):
        raise ValueError(f"{what}: unknown field {field!r} (the index holds {list(index.names)})") from None
    if field in index.vocab:
        raise ValueError(f"{what}: field {field!r} is a keyword column: its values are dictionary codes, not numbers "
                         '(use it in "if")')
    return cid


def decay_constant(kind: str, scale: float, decay: float) -> float:
    """c of a decay term, computed once in fp64: scale / (1 - decay) (linear), ln(decay) / scale (exp),
    ln(decay) / scale^2 (gauss)."""
    if kind == "linear":
        return scale / (1.0 - decay)
    if kind == "exp":
        return math.log(decay) / scale
    return math.log(decay) / (scale * scale)


def compile_term(index, item, what: str):
    """One item of the grammar as (t_op, column, [w, p0, p1, p2, missing], clauses): ValueError naming the item."""
    if not isinstance(item, dict):
        raise ValueError(f"{what}: a dict expected, not {type(item).__name__}")
    unknown = [k for k in item if k not in _ITEM_KEYS]
    if unknown:
        raise ValueError(f"{what}: unknown key {unknown[0]!r} ({sorted(_ITEM_KEYS)} expected)")
    if ("mul" in item) == ("add" in item):
        raise ValueError(f'{what}: exactly one of "mul" / "add" expected')
    mode = BOOST_MUL if "mul" in item else BOOST_ADD
    w = _finite(item["mul" if mode == BOOST_MUL else "add"], f'{what}: {"mul" if mode == BOOST_MUL else "add"}')
    if "field" in item and "decay" in item:
        raise ValueError(f'{what}: "field" and "decay" exclude each other (a decay names its field inside)')
    col, sub, p = 0, 0, [0.0, 0.0, 0.0]
    if "decay" in item:
        kind, d = BOOST_DECAY, item["decay"]
        if "modifier" in item:
            raise ValueError(f'{what}: unknown key \'modifier\' on a decay term')
        if not isinstance(d, dict):
            raise ValueError(f"{what}: decay: a dict expected, not {type(d).__name__}")
        unknown = [k for k in d if k not in _DECAY_KEYS]
        if unknown:
            raise ValueError(f"{what}: decay: unknown key {unknown[0]!r} ({sorted(_DECAY_KEYS)} expected)")
        for k in ("field", "origin", "scale"):
            if k not in d:
                raise ValueError(f"{what}: decay: {k!r} is missing")
        col = _column(index, d["field"], f"{what}: decay")
        shape = d.get("kind", "linear")
        if shape not in DECAY_KINDS:
            raise ValueError(f"{what}: decay: kind={shape!r}: one of {sorted(DECAY_KINDS)} expected")
        sub = DECAY_KINDS[shape]
        origin = _finite(d["origin"], f"{what}: decay: origin")
        scale = _finite(d["scale"], f"{what}: decay: scale")
        offset = _finite(d.get("offset", 0), f"{what}: decay: offset")
        decay = _finite(d.get("decay", 0.5), f"{what}: decay: decay")
        if not scale > 0:
            raise ValueError(f"{what}: decay: scale={scale}: must be > 0")
        if offset < 0:
            raise ValueError(f"{what}: decay: offset={offset}: must be >= 0")
        if not 0.0 < decay < 1.0:
            raise ValueError(f"{what}: decay: decay={decay}: outside (0, 1)")
        try:
            c = decay_constant(shape, scale, decay)
        except (OverflowError, ZeroDivisionError):
            c = math.inf
        if not math.isfinite(c) or c == 0.0:
            raise ValueError(f"{what}: decay: scale={scale} with decay={decay} gives no finite non-zero constant")
        p = [origin, offset, c]
    elif "field" in item:
        kind = BOOST_FIELD
        col = _column(index, item["field"], what)
        mod = item.get("modifier")
        if not (mod is None or isinstance(mod, str)) or mod not in MODIFIERS:
            raise ValueError(f"{what}: modifier={mod!r}: None or 'sqrt' expected")
        sub = MODIFIERS[mod]
    else:
        kind = BOOST_CONST
        for k in ("modifier", "missing"):
            if k in item:
                raise ValueError(f"{what}: unknown key {k!r} on a constant term (it reads no field)")
    missing, has = 0.0, 0
    if item.get("missing") is not None:
        missing, has = _finite(item["missing"], f"{what}: missing"), BOOST_HAS_MISSING
    clauses = query_clauses(index, item.get("if"), f"{what}: if")
    return kind | mode << 8 | sub << 16 | has, col, [w] + p + [missing], clauses


class BoostProgram:
    """compile_boosts' result: the term programs of `batch` queries (include/hrag.h, boosted retrieval) as host arrays --
    t_ptr int32 [batch + 1], t_op / t_col int32 [n_terms], t_num fp64 [n_terms, 5], t_cl_ptr int32 [n_terms + 1] and the
    clause arrays of a PayloadFilter -- and, once desc() ran, on the device.  broadcast: one list (batch 1) for every query
    of a call."""

    def __init__(self, n_passages, signature, per_query, broadcast):
        self.n_passages, self.signature = int(n_passages), signature
        self._per = [list(q) for q in per_query]
        self.batch, self.broadcast = len(self._per), bool(broadcast)
        t_ptr, ops, cols, nums, cl_ptr = [0], [], [], [], [0]
        c_col, c_op, c_lo, c_hi, set_ptr, sets = [], [], [], [], [0], []
        nnz = 0
        for terms in self._per:
            for op, col, num, clauses in terms:
                ops.append(op)
                cols.append(col)
                nums.append(num)
                for cid, cop, lo, hi, vals in clauses:
                    c_col.append(cid)
                    c_op.append(cop)
                    c_lo.append(lo)
                    c_hi.append(hi)
                    if vals is not None and vals.size:
                        sets.append(vals)
                        nnz += int(vals.size)
                    set_ptr.append(nnz)
                cl_ptr.append(len(c_col))
            t_ptr.append(len(ops))
        self.t_ptr = np.asarray(t_ptr, np.int32)
        self.t_op, self.t_col = np.asarray(ops, np.int32), np.asarray(cols, np.int32)
        self.t_num = np.asarray(nums, np.float64).reshape(len(ops), 5)
        self.t_cl_ptr = np.asarray(cl_ptr, np.int32)
        self.c_col, self.c_op = np.asarray(c_col, np.int32), np.asarray(c_op, np.int32)
        self.c_lo, self.c_hi = np.asarray(c_lo, np.int64), np.asarray(c_hi, np.int64)
        self.c_set_ptr = np.asarray(set_ptr, np.int32)
        self.set_vals = np.concatenate(sets) if sets else np.zeros(0, np.int64)
        self._dev = None

    @property
    def n_terms(self) -> int:
        return int(self.t_op.shape[0])

    @property
    def n_clauses(self) -> int:
        return int(self.c_col.shape[0])

    def arrays(self):
        return (self.t_ptr, self.t_op, self.t_col, self.t_num, self.t_cl_ptr, self.c_col, self.c_op, self.c_lo, self.c_hi,
                self.c_set_ptr, self.set_vals)

    def select(self, rows) -> "BoostProgram":
        """The program of the queries `rows` (host indices, in that order): a host CSR slice -- what a repeat of some rows of
        a batch runs.  A broadcast program is its own slice."""
        if self.broadcast:
            return self
        rows = np.asarray(rows, np.int64).reshape(-1)
        if rows.size and (rows.min() < 0 or rows.max() >= self.batch):
            raise ValueError(f"select: a row outside the {self.batch} queries of the program")
        return BoostProgram(self.n_passages, self.signature, [self._per[int(r)] for r in rows], False)

    def desc(self, device):
        """The hrag_boost_program of the arrays on `device` (uploaded once; the tensors live as long as the program)."""
        import torch
        if self._dev is None or self._dev[0] != device:
            ts = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in self.arrays())
            d = BoostProgramDesc(*(t.data_ptr() if t.numel() else None for t in ts), self.n_terms, self.n_clauses,
                                 int(self.set_vals.shape[0]))
            self._dev = (device, ts, d)
        return self._dev[2]


def compile_boosts(index, boosts, batch: Optional[int] = None) -> BoostProgram:
    """boosts: one list of items -- one program for the whole batch (broadcast) -- or a list of such lists (or None: no
    terms), one per query.  index: a PayloadIndex or PayloadColumns.  An item is one of
      {"if": <filter dict of compile_filters>, "mul": w} / {"if": ..., "add": w}           a constant under a condition
      {"field": name, "modifier": None | "sqrt", "mul" | "add": w, "missing": m, "if": ...}   the column value
      {"decay": {"field", "origin", "scale", "offset": 0, "decay": 0.5, "kind": "linear" | "exp" | "gauss"},
       "mul" | "add": w, "missing": m, "if": ...}                                          a decay of |value - origin|
    and the score becomes s * (product of the mul terms that hit) + (sum of the add terms that hit); a term hits where its
    "if" holds (absent: everywhere) and, for a field or decay, the passage has a value or the term a "missing" one.
    ValueError, naming the item: a number that is not finite, scale <= 0, decay outside (0, 1), offset < 0, an unknown
    key, field or kind, a keyword column as field, more than BOOST_MAX_TERMS terms or PAY_MAX_CLAUSES clauses for a query
    (the device would ignore the rest)."""
    if not isinstance(boosts, (list, tuple)):
        raise TypeError(f"boost: a list of items or a list of lists expected, not {type(boosts).__name__}")
    broadcast = all(isinstance(x, dict) for x in boosts)
    per = [list(boosts)] if broadcast else [[] if q is None else q for q in boosts]
    if not broadcast:
        for i, q in enumerate(per):
            if not isinstance(q, (list, tuple)):
                raise TypeError(f"boost[{i}]: a list of items (or None) expected, not {type(q).__name__}: give one list for "
                                "the batch or one list per query")
        if batch is not None and len(per) != batch:
            raise ValueError(f"boost: {len(per)} per-query lists for a batch of {batch}")
    out: List[list] = []
    for i, q in enumerate(per):
        name = "boost" if broadcast else f"boost[{i}]"
        if len(q) > BOOST_MAX_TERMS:
            raise ValueError(f"{name}: {len(q)} terms, at most BOOST_MAX_TERMS={BOOST_MAX_TERMS} are evaluated")
        terms = [compile_term(index, item, f"{name}[{j}]") for j, item in enumerate(q)]
        n_cl = sum(len(t[3]) for t in terms)
        if n_cl > PAY_MAX_CLAUSES:
            raise ValueError(f"{name}: {n_cl} condition clauses over its terms, at most PAY_MAX_CLAUSES={PAY_MAX_CLAUSES} "
                             "are evaluated")
        out.append(terms)
    return BoostProgram(index.n_passages, index.signature, out, broadcast)


def check_program(index, program, batch: int, name: str = "boost") -> BoostProgram:
    """`program` (a BoostProgram, or the grammar compile_boosts takes) as a BoostProgram that fits `index` and `batch`."""
    if not isinstance(program, BoostProgram):
        program = compile_boosts(index, program, batch)
    if program.n_passages != index.n_passages or program.signature != index.signature:
        raise ValueError(f"{name}: the BoostProgram was compiled for another index ({program.n_passages} passages, this one "
                         f"{index.n_passages}; or other columns)")
    if not program.broadcast and program.batch != batch:
        raise ValueError(f"{name}: the BoostProgram holds {program.batch} queries, the call {batch}")
    return program


def boost_rows(index, rows, program, mn=None, mx=None):
    """rows (a device fp32 tensor [B, >= n_passages], unit column stride) boosted IN PLACE by `program` over the payload
    index (hrag_boost_rows); mn / mx fp32 [B]: the kernel reads the min-max of an entry instead of the entry.  Enqueues on
    the current stream; returns rows."""
    import torch
    from .engine import _stream
    if not index._handle.value:
        raise ValueError("the payload index is closed")
    if (not isinstance(rows, torch.Tensor) or rows.dtype != torch.float32 or rows.dim() != 2 or rows.stride(1) != 1
            or rows.shape[1] < index.n_passages or rows.device != index.device):
        raise ValueError(f"rows: a device fp32 tensor [B, >= {index.n_passages}] with unit column stride expected")
    b = rows.shape[0]
    program = check_program(index, program, b)
    if (mn is None) != (mx is None):
        raise ValueError("mn and mx: both or neither")
    for t in (mn, mx):
        if t is not None and (t.dtype != torch.float32 or t.shape != (b,) or not t.is_contiguous() or t.device != index.device):
            raise ValueError(f"mn / mx: contiguous device fp32 tensors [{b}] expected")
    if b == 0:
        return rows
    with torch.cuda.device(index.device):
        check(_lib.load().hrag_boost_rows(index._handle, rows.data_ptr(), rows.stride(0), b,
                                          None if mn is None else mn.data_ptr(), None if mx is None else mx.data_ptr(),
                                          C.byref(program.desc(index.device)), 1 if program.broadcast else 0, _stream()))
    return rows
