"""Payload filters (include/hrag.h, payload filters): typed per-passage metadata columns, the Mongo-like filter grammar
compiled to the clause programs hrag_payload_filter evaluates, and the device index.  Everything up to PayloadIndex is
host code: encode_columns and compile_filters need no device (a PayloadColumns stands in for the index there)."""

from __future__ import annotations

import ctypes as C
import math
import struct
from typing import Dict, List, Optional

import numpy as np

from . import _lib
from ._lib import (PAY_F64, PAY_I64, PAY_IN, PAY_MAX_CLAUSES, PAY_MAX_COLS, PAY_MUST, PAY_MUST_NOT, PAY_PRESENT, PAY_RANGE,
                   PAY_SHOULD, check)

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
RANGE_OPS = ("$gt", "$gte", "$lt", "$lte")
_INTS = (bool, int, np.integer, np.bool_)
_FLOATS = (float, np.floating)


def f64_bits(x: float) -> int:
    """The bit pattern of a double as the int64 the clause arrays carry."""
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def _pack(mask: np.ndarray) -> np.ndarray:
    from .engine import pack_mask
    return pack_mask(mask)


class PayloadColumns:
    """The host form of a payload index: per column its name, HRAG_PAY_* type, 8-byte values int64 [n] (doubles as their bit
    patterns), presence words (None: every passage has a value) and, for a keyword column, the str -> code mapping."""

    def __init__(self, n_passages: int):
        self.n_passages = int(n_passages)
        self.names: List[str] = []
        self.types: List[int] = []
        self.values: List[np.ndarray] = []
        self.present: List[Optional[np.ndarray]] = []
        self.vocab: Dict[str, Dict[str, int]] = {}

    @property
    def columns(self) -> Dict[str, str]:
        """name -> "i64", "f64" or "keyword", in column order."""
        return {n: ("keyword" if n in self.vocab else "f64" if t == PAY_F64 else "i64") for n, t in zip(self.names, self.types)}

    @property
    def signature(self):
        return tuple((n, t, n in self.vocab) for n, t in zip(self.names, self.types))

    def column_id(self, name) -> int:
        return self.names.index(name)

    def _add(self, name, typ, values, present, vocab=None):
        self.names.append(name)
        self.types.append(typ)
        self.values.append(np.ascontiguousarray(values).view(np.int64))
        self.present.append(None if present is None or present.all() else _pack(present))
        if vocab is not None:
            self.vocab[name] = vocab


def _encode_column(name, seq, n: int):
    """(type, values 8-byte [n], present bool [n] or None, vocab or None) of one column; ValueError naming it."""
    if isinstance(seq, np.ndarray) and seq.dtype.kind in "iubf":
        if seq.shape != (n,):
            raise ValueError(f"column {name!r}: {seq.shape} values for {n} passages")
        if seq.dtype.kind == "f":
            return PAY_F64, seq.astype(np.float64), None, None
        if seq.dtype.kind == "u" and seq.size and int(seq.max()) > I64_MAX:
            raise ValueError(f"column {name!r}: an integer outside int64")
        return PAY_I64, seq.astype(np.int64), None, None
    seq = list(seq)
    if len(seq) != n:
        raise ValueError(f"column {name!r}: {len(seq)} values for {n} passages")
    present = np.fromiter((v is not None for v in seq), bool, n)
    kinds = set()
    for v in seq:
        if v is None:
            continue
        if isinstance(v, _INTS):
            kinds.add("i")
        elif isinstance(v, _FLOATS):
            kinds.add("f")
        elif isinstance(v, str):
            kinds.add("s")
        else:
            raise ValueError(f"column {name!r}: a value of type {type(v).__name__} (int, bool, float, str or None expected)")
    if kinds <= {"i"}:
        ints = [0 if v is None else int(v) for v in seq]
        if any(v < I64_MIN or v > I64_MAX for v in ints):
            raise ValueError(f"column {name!r}: an integer outside int64")
        return PAY_I64, np.asarray(ints, np.int64).reshape(n), present, None
    if kinds <= {"i", "f"}:
        if any(isinstance(v, _INTS) and abs(int(v)) > 1 << 53 for v in seq if v is not None):
            raise ValueError(f"column {name!r}: mixes floats with an integer beyond 2^53 (not exactly a double)")
        return PAY_F64, np.asarray([0.0 if v is None else float(v) for v in seq], np.float64).reshape(n), present, None
    if kinds == {"s"}:
        vocab = {s: i for i, s in enumerate(sorted({v for v in seq if v is not None}))}
        return PAY_I64, np.asarray([0 if v is None else vocab[v] for v in seq], np.int64).reshape(n), present, vocab
    raise ValueError(f"column {name!r}: mixes str with numbers")


def encode_columns(columns, n_passages: int) -> PayloadColumns:
    """columns: name -> a sequence of n_passages values.  Integers and bools give an I64 column, floats an F64 one, a mix of
    the two F64 when every integer is exactly a double (|v| <= 2^53); str values are dictionary-encoded (sorted unique
    values -> codes 0 ..) into an I64 column.  None: the passage has no value.  Any other mixture or value type: ValueError
    naming the column.  A numeric numpy array is taken as it is (every passage present; NaN is a value)."""
    n = int(n_passages)
    if n < 1:
        raise ValueError(f"n_passages={n_passages}: at least 1")
    if len(columns) > PAY_MAX_COLS:
        raise ValueError(f"{len(columns)} columns: at most PAY_MAX_COLS={PAY_MAX_COLS}")
    pc = PayloadColumns(n)
    for name, seq in columns.items():
        pc._add(name, *_encode_column(name, seq, n))
    return pc


# ---------------------------------------------------------------------------------------------- the filter grammar
class PayloadFilter:
    """compile_filters' result: the clause programs of `batch` queries in CSR form (include/hrag.h, payload filters) as host
    arrays -- f_ptr int32 [batch + 1], c_col / c_op int32, c_lo / c_hi int64 [n_clauses], c_set_ptr int32 [n_clauses + 1],
    set_vals int64 -- and, once tensors() ran, on the device.  broadcast: one program (batch 1) for every query of a call."""

    def __init__(self, index, batch, broadcast, f_ptr, c_col, c_op, c_lo, c_hi, c_set_ptr, set_vals):
        self.n_passages, self.signature = index.n_passages, index.signature
        self.batch, self.broadcast = int(batch), bool(broadcast)
        self.f_ptr = np.ascontiguousarray(f_ptr, np.int32)
        self.c_col, self.c_op = np.ascontiguousarray(c_col, np.int32), np.ascontiguousarray(c_op, np.int32)
        self.c_lo, self.c_hi = np.ascontiguousarray(c_lo, np.int64), np.ascontiguousarray(c_hi, np.int64)
        self.c_set_ptr, self.set_vals = np.ascontiguousarray(c_set_ptr, np.int32), np.ascontiguousarray(set_vals, np.int64)
        self._dev = None

    @property
    def n_clauses(self) -> int:
        return int(self.c_col.shape[0])

    def arrays(self):
        return self.f_ptr, self.c_col, self.c_op, self.c_lo, self.c_hi, self.c_set_ptr, self.set_vals

    def tensors(self, device):
        """The seven arrays on `device` (uploaded once)."""
        import torch
        if self._dev is None or self._dev[0] != device:
            self._dev = (device, tuple(torch.from_numpy(a).to(device) for a in self.arrays()))
        return self._dev[1]


def _number(v, what):
    if isinstance(v, _INTS):
        return int(v)
    if isinstance(v, _FLOATS):
        if math.isnan(v):
            raise ValueError(f"{what}: a NaN bound")
        return float(v)
    raise ValueError(f"{what}: a number expected, not {type(v).__name__}")


def _i64_bounds(ops, what):
    """Inclusive int64 (lo, hi) of the range operators; (1, 0) -- lo > hi, a clause that hits nothing -- when no int64
    satisfies them.  Bounds beyond the type saturate where that loses nothing."""
    lo, hi = I64_MIN, I64_MAX
    for op, v in ops.items():
        v = _number(v, f"{what}: {op}")
        if isinstance(v, float) and math.isinf(v):
            if (op in ("$gt", "$gte")) == (v > 0):
                return 1, 0                     # above +inf / below -inf
            continue
        if op == "$gt":
            lo = max(lo, math.floor(v) + 1)
        elif op == "$gte":
            lo = max(lo, math.ceil(v))
        elif op == "$lt":
            hi = min(hi, math.ceil(v) - 1)
        else:
            hi = min(hi, math.floor(v))
    return (1, 0) if lo > hi else (lo, hi)


def _f64_above(v, strict):
    """The smallest double > v (strict) or >= v; v a Python int or float (compared exactly)."""
    try:
        f = float(v)
    except OverflowError:
        f = math.inf if v > 0 else -math.inf
    if f > v or (not strict and f == v):
        return f
    return math.nextafter(f, math.inf)


def _f64_below(v, strict):
    try:
        f = float(v)
    except OverflowError:
        f = math.inf if v > 0 else -math.inf
    if f < v or (not strict and f == v):
        return f
    return math.nextafter(f, -math.inf)


def _f64_bounds(ops, what):
    """Inclusive double (lo, hi) of the range operators, or None when no double satisfies them."""
    lo, hi = -math.inf, math.inf
    for op, v in ops.items():
        v = _number(v, f"{what}: {op}")
        if isinstance(v, float) and math.isinf(v) and op in ("$gt", "$lt") and (op == "$gt") == (v > 0):
            return None                         # > +inf / < -inf
        if op in ("$gt", "$gte"):
            lo = max(lo, _f64_above(v, op == "$gt"))
        else:
            hi = min(hi, _f64_below(v, op == "$lt"))
    return None if lo > hi else (lo, hi)


def _set_values(index, cid, alts):
    """The sorted int64 words of the IN set `alts` on column cid: every value the column can hold, as Python's == would
    match it (True == 1 == 1.0); what it cannot hold -- an unknown keyword, 3.5 on an I64 column, a str on a number column,
    NaN -- is dropped: it equals nothing."""
    name, typ = index.names[cid], index.types[cid]
    vocab = index.vocab.get(name)
    out = []
    for v in alts:
        if vocab is not None:
            try:
                code = vocab.get(v) if isinstance(v, str) else None
            except TypeError:
                code = None
            if code is not None:
                out.append(code)
        elif typ == PAY_I64:
            if isinstance(v, _FLOATS):
                if not math.isfinite(v) or v != math.floor(v):
                    continue
                v = int(v)
            elif not isinstance(v, _INTS):
                continue
            if I64_MIN <= int(v) <= I64_MAX:
                out.append(int(v))
        else:
            if isinstance(v, _INTS):
                try:
                    f = float(int(v))
                except OverflowError:
                    continue
                if f != int(v):
                    continue
                v = f
            elif not isinstance(v, _FLOATS) or math.isnan(v):
                continue
            out.append(float(v))
    if typ == PAY_F64 and vocab is None:
        return np.unique(np.asarray(out, np.float64)).view(np.int64)
    return np.unique(np.asarray(out, np.int64))


def _field_clauses(index, field, cond, role, out, what):
    """Append the clauses (col, op, lo, hi, set) of one field condition."""
    try:
        cid = index.column_id(field)
    except (ValueError, TypeError):
        raise ValueError(f"{what}: unknown field {field!r} (the index holds {list(index.names)})") from None
    typ, keyword = index.types[cid], field in index.vocab
    if isinstance(cond, dict) and any(isinstance(k, str) and k.startswith("$") for k in cond):
        ops = {}
        for op, v in cond.items():
            if op == "$exists":
                if not isinstance(v, (bool, np.bool_)):
                    raise ValueError(f"{what}: {field!r}: $exists takes a bool, not {v!r}")
                if bool(v):
                    r = role
                elif role == PAY_SHOULD:
                    raise ValueError(f"{what}: {field!r}: $exists: False cannot be an alternative of $any")
                else:
                    r = PAY_MUST_NOT if role == PAY_MUST else PAY_MUST
                out.append((cid, r | PAY_PRESENT << 8, 0, 0, None))
            elif op in RANGE_OPS:
                ops[op] = v
            else:
                raise ValueError(f"{what}: {field!r}: unknown operator {op!r} ($gt, $gte, $lt, $lte, $exists expected)")
        if ops:
            if keyword:
                raise ValueError(f"{what}: {field!r}: a range ({', '.join(ops)}) on a keyword column")
            if typ == PAY_I64:
                lo, hi = _i64_bounds(ops, f"{what}: {field!r}")
            else:
                b = _f64_bounds(ops, f"{what}: {field!r}")
                lo, hi = (f64_bits(1.0), f64_bits(0.0)) if b is None else (f64_bits(b[0]), f64_bits(b[1]))
            out.append((cid, role | PAY_RANGE << 8, lo, hi, None))
        return
    alts = cond if isinstance(cond, (list, tuple, set, frozenset)) else [cond]
    out.append((cid, role | PAY_IN << 8, 0, 0, _set_values(index, cid, alts)))


def query_clauses(index, f, what="doc_filter") -> list:
    """The clauses of one query's filter dict (None: no clause): (col, op, lo, hi, set values or None) each."""
    out: list = []
    if f is None:
        return out
    if not isinstance(f, dict):
        raise TypeError(f"{what}: a filter dict (or None) expected, not {type(f).__name__}")
    for key, cond in f.items():
        if key in ("$not", "$any"):
            if not isinstance(cond, dict):
                raise ValueError(f"{what}: {key} takes a dict of field conditions")
            for field, c in cond.items():
                if isinstance(field, str) and field.startswith("$"):
                    raise ValueError(f"{what}: unknown operator {field!r} inside {key} (groups do not nest)")
                _field_clauses(index, field, c, PAY_MUST_NOT if key == "$not" else PAY_SHOULD, out, what)
        elif isinstance(key, str) and key.startswith("$"):
            raise ValueError(f"{what}: unknown operator {key!r} ($not, $any expected)")
        else:
            _field_clauses(index, key, cond, PAY_MUST, out, what)
    if len(out) > PAY_MAX_CLAUSES:
        raise ValueError(f"{what}: {len(out)} clauses, at most PAY_MAX_CLAUSES={PAY_MAX_CLAUSES} are evaluated")
    return out


def compile_filters(index, filters) -> PayloadFilter:
    """filters: one dict -- one program for the whole batch (a broadcast row) -- or a list of dicts / None, one per query.
    index: a PayloadIndex or PayloadColumns.  The grammar (Mongo-like, so that a plain metadata dict keeps its meaning):
      {"field": value}                     IN {value}, MUST
      {"field": [v1, v2]}                  IN (a list, tuple or set)
      {"field": {"$gt" | "$gte" | "$lt" | "$lte": number, ...}}    one RANGE, MUST
      {"field": {"$exists": bool}}         PRESENT: MUST when true, MUST_NOT when false
      {"$not": {...}} / {"$any": {...}}    the same field conditions with the role MUST_NOT / SHOULD
    Bounds become inclusive here: on an I64 column $gt v is floor(v) + 1 and $gte v is ceil(v) ($lt / $lte mirrored),
    saturating at the int64 limits; on an F64 column $gt v is the next double above v; an open end is the type's extreme
    (-+inf).  Operators no value can satisfy (above +inf, below INT64_MIN) give a clause that hits nothing.  ValueError,
    naming the key: a NaN bound, a range on a keyword column, an unknown field, an unknown $ operator, more than
    PAY_MAX_CLAUSES clauses for a query."""
    broadcast = isinstance(filters, dict)
    if not broadcast and not isinstance(filters, (list, tuple)):
        raise TypeError(f"filters: a dict or a list of dicts / None expected, not {type(filters).__name__}")
    per = [filters] if broadcast else list(filters)
    if not per:
        raise ValueError("filters: an empty list")
    f_ptr, cols, ops, los, his, set_ptr, sets = [0], [], [], [], [], [0], []
    nnz = 0
    for i, f in enumerate(per):
        for cid, op, lo, hi, vals in query_clauses(index, f, "doc_filter" if broadcast else f"doc_filter[{i}]"):
            cols.append(cid)
            ops.append(op)
            los.append(lo)
            his.append(hi)
            if vals is not None and vals.size:
                sets.append(vals)
                nnz += int(vals.size)
            set_ptr.append(nnz)
        f_ptr.append(len(cols))
    set_vals = np.concatenate(sets) if sets else np.zeros(0, np.int64)
    return PayloadFilter(index, len(per), broadcast, f_ptr, cols, ops, np.asarray(los, np.int64), np.asarray(his, np.int64),
                         set_ptr, set_vals)


# ---------------------------------------------------------------------------------------------- the device index
class PayloadIndex(PayloadColumns):
    """Typed per-passage columns on the device (hrag_payload_create; include/hrag.h, payload filters).  Independent of any
    engine -- HippoRAGEngine.set_payload_index takes it by reference, so engines and their workspaces over the same
    passages share one.  The host copy of the columns is dropped after the upload; names, types and keyword vocabularies
    stay."""

    def __init__(self, host: PayloadColumns, device: Optional[int] = None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("PayloadIndex needs an MI355X-class GPU: no HIP device is visible (there is no CPU fallback)")
        super().__init__(host.n_passages)
        self.names, self.types, self.vocab = list(host.names), list(host.types), dict(host.vocab)
        self._lib = _lib.load()
        self._handle = C.c_void_p(0)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        nc = len(self.names)
        types = (C.c_int32 * max(nc, 1))(*self.types)
        vals = (C.c_void_p * max(nc, 1))(*[v.ctypes.data for v in host.values])
        pres = (C.c_void_p * max(nc, 1))(*[None if p is None else p.ctypes.data for p in host.present])
        with torch.cuda.device(self.device):
            check(self._lib.hrag_payload_create(self.n_passages, nc, types, vals, pres, C.byref(self._handle)))

    @classmethod
    def from_columns(cls, columns, n_passages: int, device: Optional[int] = None) -> "PayloadIndex":
        """encode_columns, then the upload."""
        return cls(encode_columns(columns, n_passages), device)

    @property
    def words(self) -> int:
        return (self.n_passages + 31) // 32

    def evaluate(self, pf: PayloadFilter, and_with=None, out=None):
        """The doc filter words of a compiled filter (hrag_payload_filter): packed words [B, W] -- [W] for a broadcast
        filter -- in int32 storage, as doc_filter_words gives them and every doc_filter= takes them.  and_with: a doc
        filter (bool or packed, [n] / [W] or per query) ANDed in; out: int32 [B, >= W] to write into (the words beyond W of
        a row are left alone).  Enqueues on the current stream."""
        import torch
        from .engine import _stream, doc_filter_words
        if not self._handle.value:
            raise ValueError("the payload index is closed")
        if not isinstance(pf, PayloadFilter):
            raise TypeError(f"a PayloadFilter (compile_filters) expected, not {type(pf).__name__}")
        if pf.n_passages != self.n_passages or pf.signature != self.signature:
            raise ValueError(f"the PayloadFilter was compiled for another index ({pf.n_passages} passages, this one "
                             f"{self.n_passages}; or other columns)")
        b, w = pf.batch, self.words
        aw, ald = (None, 0) if and_with is None else doc_filter_words(and_with, self.n_passages, b, self.device)
        if out is None:
            out = torch.empty((b, w), dtype=torch.int32, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or out.dim() != 2 or out.shape[0] < b
              or out.shape[1] < w or out.stride(1) != 1 or out.device != self.device):
            raise ValueError(f"out: a device int32 tensor [>= {b}, >= {w}] expected")
        if aw is not None and aw.data_ptr() < out.data_ptr() + 4 * ((b - 1) * out.stride(0) + w) \
                and out.data_ptr() < aw.data_ptr() + 4 * aw.numel():
            raise ValueError("out must not overlap and_with")
        d = pf.tensors(self.device)
        nc, nnz = pf.n_clauses, int(pf.set_vals.shape[0])
        with torch.cuda.device(self.device):
            check(self._lib.hrag_payload_filter(self._handle, d[0].data_ptr(), *(t.data_ptr() if nc else None for t in d[1:5]),
                                                d[5].data_ptr(), d[6].data_ptr() if nnz else None, nc, nnz, b,
                                                aw.data_ptr() if aw is not None else None, ald, out.data_ptr(), out.stride(0),
                                                _stream()))
        rows = out[:b, :w]
        return rows[0] if pf.broadcast else rows

    def count(self, words):
        """int32 [B]: how many passages each row of packed doc filter words ([W] or [B, W]) allows (hrag_bitset_count_rows)."""
        return count_rows(words, self.n_passages)

    def facet(self, spec, words=None, *, ids=None, out=None):
        """The per-bin counts of a FacetSpec (facet.compile_facet; include/hrag.h, facets) as a FacetCounts: over the
        passages `words` allows -- None (all of them), packed words [W] / [B, W], a bool mask [n] / [B, n], or a PayloadFilter
        (evaluated first; a broadcast one gives one row) -- by hrag_payload_facet, or over the passage ids `ids` int32 device
        [B, k] as retrieve returns them (the -1 padding and ids outside the index are skipped, a repeated id counts each
        time) by hrag_payload_facet_ids.  out: int32 device [>= B, >= n_bins + 2] to write into (entries beyond n_bins + 2
        of a row are left alone).  The workspace is allocated per call; enqueues on the current stream."""
        from .facet import facet_counts
        return facet_counts(self, spec, words, ids=ids, out=out)

    def close(self):
        if getattr(self, "_handle", None) and self._handle.value:
            check(self._lib.hrag_payload_destroy(self._handle))
            self._handle = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def count_rows(words, n: int):
    """int32 [B] (B = 1 for one row): the set bits among the first n of each row of packed device words."""
    import torch
    from .engine import _stream
    if not isinstance(words, torch.Tensor) or not (words.dtype == torch.int32 or str(words.dtype) == "torch.uint32"):
        raise TypeError("words: a packed int32 / uint32 device tensor expected")
    w2 = words.reshape(1, -1) if words.dim() == 1 else words
    if w2.dim() != 2 or w2.shape[1] < (n + 31) // 32 or w2.stride(1) != 1:
        raise ValueError(f"words: [W] or [B, W] with W >= ceil({n} / 32) expected")
    out = torch.empty((w2.shape[0],), dtype=torch.int32, device=w2.device)
    with torch.cuda.device(w2.device):
        check(_lib.load().hrag_bitset_count_rows(w2.data_ptr(), w2.stride(0), n, w2.shape[0], out.data_ptr(), _stream()))
    return out
