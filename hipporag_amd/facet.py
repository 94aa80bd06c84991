"""Facets (include/hrag.h, facets): per-value counts of one payload column over the passages a doc filter allows, or over
the ids a retrieve call returned -- the facet specs compiled from a column's description, the device call and its result.
compile_facet is host code and needs no device (a PayloadColumns stands in for the index there)."""

from __future__ import annotations

import ctypes as C
import math
from typing import List

import numpy as np

from . import _lib
from ._lib import FACET_CODES, FACET_EDGES, FACET_MAX_BINS, PAY_F64, PAY_I64, check
from .payload import _FLOATS, _INTS, I64_MAX, I64_MIN, PayloadFilter


class FacetSpec:
    """compile_facet's result: one column of an index and the map from its values to n_bins bins (include/hrag.h, facets).
    kind FACET_CODES: bin = x - lo; kind FACET_EDGES: bin = the number of `edges` (8-byte words of the column's type,
    ascending) <= x.  labels: one per bin, in bin order."""

    def __init__(self, index, field, column, kind, n_bins, lo=0, edges=None, labels=None):
        self.n_passages, self.signature = index.n_passages, index.signature
        self.field, self.column, self.kind, self.n_bins, self.lo = field, int(column), int(kind), int(n_bins), int(lo)
        self.f64 = index.types[self.column] == PAY_F64
        self.edges = None if edges is None else np.ascontiguousarray(edges, np.int64)
        self.labels = labels
        self._dev = None

    @property
    def n_edges(self) -> int:
        return 0 if self.edges is None else int(self.edges.shape[0])

    def desc(self, device) -> "_lib.FacetSpecDesc":
        """The hrag_facet_spec of this spec with its edges on `device` (uploaded once)."""
        ptr = None
        if self.n_edges:
            import torch
            if self._dev is None or self._dev[0] != device:
                self._dev = (device, torch.from_numpy(self.edges).to(device))
            ptr = self._dev[1].data_ptr()
        return _lib.FacetSpecDesc(self.column, self.kind, self.n_bins, self.lo, ptr, self.n_edges)


def _edge_value(field, typ, v):
    """One edge as the column's type holds it, exactly -- _set_values' conversion, but what the type cannot hold raises."""
    if isinstance(v, _FLOATS) and math.isnan(v):
        raise ValueError(f"facet {field!r}: a NaN edge")
    if typ == PAY_I64:
        if isinstance(v, _FLOATS):
            if not math.isfinite(v) or v != math.floor(v):
                raise ValueError(f"facet {field!r}: the edge {v!r} is not an integer (the column is I64)")
            v = int(v)
        elif not isinstance(v, _INTS):
            raise ValueError(f"facet {field!r}: an edge of type {type(v).__name__} (a number expected)")
        if not I64_MIN <= int(v) <= I64_MAX:
            raise ValueError(f"facet {field!r}: the edge {v!r} is outside int64")
        return int(v)
    if isinstance(v, _INTS):
        try:
            f = float(int(v))
        except OverflowError:
            f = None
        if f is None or f != int(v):
            raise ValueError(f"facet {field!r}: the edge {v!r} is not exactly a double (the column is F64)")
        return f
    if not isinstance(v, _FLOATS):
        raise ValueError(f"facet {field!r}: an edge of type {type(v).__name__} (a number expected)")
    return float(v)


def compile_facet(ix, field, *, edges=None, lo=None, n_values=None) -> FacetSpec:
    """The facet spec of `field` on the index `ix` (a PayloadIndex or PayloadColumns).
      a keyword column          one bin per vocabulary entry, in code order (CODES with lo = 0); labels: the strings
      an I64 column, lo=, n_values=    one bin per integer lo .. lo + n_values - 1 (CODES); labels: the integers
      a number column, edges=[...]    len(edges) + 1 buckets: below the first edge, [edges[i - 1], edges[i]), from the last
                                edge on (EDGES); labels: (lo, hi) pairs, None at the open ends.  The edges are converted as the
                                members of an IN set are, but a value the column's type cannot hold exactly raises; equal
                                neighbours are allowed and give an empty bucket; no edges give one bucket.
    ValueError, naming the field: an unknown field, edges on a keyword column, lo / n_values on an F64 column, NaN or
    descending edges, more than FACET_MAX_BINS bins, a number column with neither form."""
    try:
        cid = ix.column_id(field)
    except (ValueError, TypeError):
        raise ValueError(f"facet: unknown field {field!r} (the index holds {list(ix.names)})") from None
    typ, vocab = ix.types[cid], ix.vocab.get(field)
    if vocab is not None:
        if edges is not None or lo is not None or n_values is not None:
            raise ValueError(f"facet {field!r}: a keyword column takes no edges / lo / n_values (one bin per vocabulary entry)")
        if len(vocab) > FACET_MAX_BINS:
            raise ValueError(f"facet {field!r}: {len(vocab)} bins, at most FACET_MAX_BINS={FACET_MAX_BINS}")
        labels = sorted(vocab, key=vocab.get)
        return FacetSpec(ix, field, cid, FACET_CODES, len(labels), 0, None, labels)
    if edges is not None:
        if lo is not None or n_values is not None:
            raise ValueError(f"facet {field!r}: edges or lo / n_values, not both")
        vals = [_edge_value(field, typ, v) for v in edges]
        if len(vals) + 1 > FACET_MAX_BINS:
            raise ValueError(f"facet {field!r}: {len(vals) + 1} bins, at most FACET_MAX_BINS={FACET_MAX_BINS}")
        if any(a > b for a, b in zip(vals, vals[1:])):
            raise ValueError(f"facet {field!r}: descending edges (ascending order expected; equal neighbours are allowed)")
        words = np.asarray(vals, np.float64).view(np.int64) if typ == PAY_F64 else np.asarray(vals, np.int64)
        ends = [None] + vals + [None]
        return FacetSpec(ix, field, cid, FACET_EDGES, len(vals) + 1, 0, words.reshape(-1), list(zip(ends[:-1], ends[1:])))
    if lo is None and n_values is None:
        raise ValueError(f"facet {field!r}: a number column needs edges=[...] or lo= and n_values=")
    if typ != PAY_I64:
        raise ValueError(f"facet {field!r}: lo / n_values on an F64 column (edges=[...] expected)")
    if lo is None or n_values is None or not isinstance(lo, _INTS) or not isinstance(n_values, _INTS):
        raise ValueError(f"facet {field!r}: lo and n_values are both needed, as integers")
    lo, n_values = int(lo), int(n_values)
    if not I64_MIN <= lo <= I64_MAX:
        raise ValueError(f"facet {field!r}: lo={lo} is outside int64")
    if not 1 <= n_values <= FACET_MAX_BINS:
        raise ValueError(f"facet {field!r}: {n_values} bins, outside [1, FACET_MAX_BINS={FACET_MAX_BINS}]")
    return FacetSpec(ix, field, cid, FACET_CODES, n_values, lo, None, range(lo, lo + n_values))


class FacetCounts:
    """The result of a facet call: raw int32 device [B, n_bins + 2] (the counts, then "other", then "missing"), viewed."""

    def __init__(self, raw, spec: FacetSpec):
        self.raw, self.spec, self.labels = raw, spec, spec.labels

    @property
    def counts(self):
        """int32 device [B, n_bins]"""
        return self.raw[:, :self.spec.n_bins]

    @property
    def other(self):
        """int32 device [B]: allowed passages whose value maps to no bin"""
        return self.raw[:, self.spec.n_bins]

    @property
    def missing(self):
        """int32 device [B]: allowed passages without a value"""
        return self.raw[:, self.spec.n_bins + 1]

    def top(self, limit: int = 10) -> List[list]:
        """Per query the (label, count) pairs of its `limit` largest bins: count descending, ties by bin ascending, zero
        counts dropped.  One readback, then a stable argsort on the host."""
        return top_of(self.counts.cpu().numpy(), self.labels, limit)


def top_of(counts: np.ndarray, labels, limit: int = 10) -> List[list]:
    out = []
    for row in np.asarray(counts):
        order = np.argsort(-row.astype(np.int64), kind="stable")[:max(int(limit), 0)]
        out.append([(labels[int(v)], int(row[v])) for v in order if row[v] > 0])
    return out


def facet_splits(ix, n_bins: int, batch: int) -> int:
    """How many splits of the passage range hrag_payload_facet uses for (ix.n_passages, n_bins, batch), read off
    hrag_payload_facet_ws_bytes (4 * batch * n_splits * (n_bins + 2) bytes, or 0 for one split)."""
    need = C.c_int64(0)
    check(ix._lib.hrag_payload_facet_ws_bytes(ix._handle, n_bins, batch, C.byref(need)))
    return max(1, need.value // (4 * batch * (n_bins + 2)))


def facet_counts(ix, spec: FacetSpec, words=None, *, ids=None, out=None) -> FacetCounts:
    """PayloadIndex.facet: see there."""
    import torch
    from .engine import _stream, doc_filter_words
    if not ix._handle.value:
        raise ValueError("the payload index is closed")
    if not isinstance(spec, FacetSpec):
        raise TypeError(f"a FacetSpec (compile_facet) expected, not {type(spec).__name__}")
    if spec.n_passages != ix.n_passages or spec.signature != ix.signature:
        raise ValueError(f"the FacetSpec was compiled for another index ({spec.n_passages} passages, this one "
                         f"{ix.n_passages}; or other columns)")
    if ids is not None and words is not None:
        raise ValueError("facet: words or ids, not both")
    n, width = ix.n_passages, spec.n_bins + 2
    w, ld = None, 0
    if ids is not None:
        if (not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or ids.dim() != 2 or ids.shape[1] < 1
                or ids.stride(1) != 1 or ids.device != ix.device):
            raise ValueError("ids: an int32 device tensor [B, k >= 1] expected")
        b = ids.shape[0]
    elif words is None:
        b = 1
    else:
        if isinstance(words, PayloadFilter):
            words = ix.evaluate(words)
        if not isinstance(words, torch.Tensor):
            raise TypeError(f"words: packed words, a bool mask or a PayloadFilter expected, not {type(words).__name__}")
        b = words.shape[0] if words.dim() == 2 else 1
        w, ld = doc_filter_words(words, n, b, ix.device)
    if b < 1:
        raise ValueError("facet: an empty batch")
    if out is None:
        out = torch.empty((b, width), dtype=torch.int32, device=ix.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or out.dim() != 2 or out.shape[0] < b
          or out.shape[1] < width or out.stride(1) != 1 or out.device != ix.device):
        raise ValueError(f"out: a device int32 tensor [>= {b}, >= {width}] expected")
    with torch.cuda.device(ix.device):
        desc = spec.desc(ix.device)
        if ids is not None:
            check(ix._lib.hrag_payload_facet_ids(ix._handle, C.byref(desc), ids.data_ptr(), ids.stride(0), ids.shape[1], b,
                                                 out.data_ptr(), out.stride(0), _stream()))
        else:
            need = C.c_int64(0)
            check(ix._lib.hrag_payload_facet_ws_bytes(ix._handle, spec.n_bins, b, C.byref(need)))
            ws = torch.empty((need.value // 4,), dtype=torch.int32, device=ix.device) if need.value else None
            check(ix._lib.hrag_payload_facet(ix._handle, C.byref(desc), w.data_ptr() if w is not None else None, ld, b,
                                             out.data_ptr(), out.stride(0), ws.data_ptr() if ws is not None else None,
                                             need.value, _stream()))
    return FacetCounts(out[:b, :width], spec)
