"""Late-interaction reranking (include/hrag.h, "late-interaction reranking"; csrc/late.hip): the token index, the late
queries of a batch and the checks of the `late=` option.  ColBERT-style MaxSim over per-token embeddings of the c
candidates a ranking returned -- the engine glue is in engine.py (set_token_index, late_scores, late_rerank, late=)."""

from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from ._lib import LATE_MAX_CANDIDATES, LATE_MAX_DIM, LATE_MAX_QUERY_TOKENS, check

LATE_DTYPES = {"bf16": 0, "fp16": 1}      # HRAG_BF16 / HRAG_FP16


def _torch():
    import torch
    return torch


def _torch_dtype(dtype: str):
    torch = _torch()
    return torch.bfloat16 if dtype == "bf16" else torch.float16


def check_late_dtype(dtype) -> str:
    if dtype not in LATE_DTYPES:
        raise ValueError(f"dtype={dtype!r}: 'bf16' or 'fp16' expected")
    return dtype


def check_late_dim(dim, name: str = "dim") -> int:
    """dim as the library takes it: a multiple of 8 in [8, LATE_MAX_DIM]."""
    if isinstance(dim, bool) or not isinstance(dim, (int, np.integer)) or dim < 8 or dim % 8:
        raise ValueError(f"{name}={dim!r}: a multiple of 8, at least 8, expected")
    if dim > LATE_MAX_DIM:
        raise ValueError(f"{name}={dim}: above LATE_MAX_DIM={LATE_MAX_DIM}")
    return int(dim)


def check_tok_ptr(tok_ptr, n_tokens: Optional[int] = None, name: str = "tok_ptr", cap: Optional[int] = None) -> np.ndarray:
    """A CSR pointer as the library takes it: one-dimensional integers from 0, never descending, ending at n_tokens (when
    given); cap: no range longer than this.  Returns int64."""
    p = np.asarray(tok_ptr)
    if p.ndim != 1 or p.shape[0] < 1 or p.dtype.kind not in "iu":
        raise ValueError(f"{name}: a one-dimensional integer array of n + 1 entries expected")
    p = p.astype(np.int64)
    if p[0] != 0:
        raise ValueError(f"{name}[0] = {int(p[0])}, 0 expected")
    lens = np.diff(p)
    if (lens < 0).any():
        at = int(np.argmax(lens < 0))
        raise ValueError(f"{name} descends at entry {at} ({int(p[at])} -> {int(p[at + 1])})")
    if n_tokens is not None and int(p[-1]) != int(n_tokens):
        raise ValueError(f"{name} ends at {int(p[-1])}, the {int(n_tokens)} token rows expected")
    if cap is not None and (lens > cap).any():
        at = int(np.argmax(lens > cap))
        raise ValueError(f"{name}: query {at} holds {int(lens[at])} tokens, at most LATE_MAX_QUERY_TOKENS={cap}")
    return np.ascontiguousarray(p)


def _ragged_rows(arrays, dtype: str, name: str):
    """list of [t_i, dim] float arrays (numpy or torch; t_i = 0 allowed) -> (ptr int64 [n + 1], rows: a host torch tensor
    [T, dim] of the 16-bit type, rounded to nearest).  dim comes from the first array."""
    torch = _torch()
    check_late_dtype(dtype)
    if isinstance(arrays, (np.ndarray,)) and arrays.ndim == 3:
        arrays = list(arrays)
    if not isinstance(arrays, (list, tuple)) or not len(arrays):
        raise ValueError(f"{name}: a non-empty list of [t_i, dim] arrays expected")
    rows, lens, dim = [], [], None
    for i, a in enumerate(arrays):
        t = a.detach().cpu() if hasattr(a, "detach") else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
        if t.dim() != 2:
            raise ValueError(f"{name}[{i}] has {t.dim()} dimensions: [t_i, dim] expected")
        if dim is None:
            dim = check_late_dim(int(t.shape[1]), f"{name}: dim")
        if t.shape[1] != dim:
            raise ValueError(f"{name}[{i}] has dim {t.shape[1]}, {dim} expected (that of {name}[0])")
        if not (t.dtype.is_floating_point):
            raise ValueError(f"{name}[{i}] has dtype {t.dtype}: floating-point token vectors expected")
        lens.append(int(t.shape[0]))
        rows.append(t.to(_torch_dtype(dtype)))
    ptr = np.zeros(len(lens) + 1, np.int64)
    ptr[1:] = np.cumsum(lens)
    return ptr, torch.cat(rows, 0).contiguous(), dim


def _device(device):
    torch = _torch()
    if isinstance(device, torch.device):
        return device
    if isinstance(device, str):
        return torch.device(device)
    return torch.device("cuda", torch.cuda.current_device() if device is None else device)


class TokenIndex:
    """The token vectors of n passages on the device (hrag_late_create): tok_ptr int64 [n + 1] and tok_emb, a torch bf16 /
    fp16 tensor [T, dim] that the index keeps alive and the library reads in place.  Independent of any engine --
    HippoRAGEngine.set_token_index takes it by reference; its vectors are NOT the engine's passage embeddings."""

    def __init__(self, tok_ptr, tok_emb, dtype: str = "bf16", device=None):
        torch = _torch()
        check_late_dtype(dtype)
        if not hasattr(tok_emb, "dtype") or tok_emb.dtype != _torch_dtype(dtype) or tok_emb.dim() != 2:
            raise ValueError(f"tok_emb: a torch {dtype} tensor [T, dim] expected")
        dim = check_late_dim(int(tok_emb.shape[1]), "tok_emb: dim")
        ptr = check_tok_ptr(tok_ptr, tok_emb.shape[0])
        if ptr.shape[0] < 2:
            raise ValueError("tok_ptr: at least one passage expected")
        if not torch.cuda.is_available():
            raise RuntimeError("TokenIndex needs an MI355X-class GPU: no HIP device is visible (there is no CPU fallback)")
        self._lib = _lib.load()
        self._handle = C.c_void_p(0)
        self.device = _device(device)
        self.tok_ptr = ptr
        self.tok_emb = tok_emb.to(self.device).contiguous()
        self.n_passages, self.n_tokens, self.dim, self.dtype = ptr.shape[0] - 1, int(ptr[-1]), dim, dtype
        with torch.cuda.device(self.device):
            check(self._lib.hrag_late_create(self.n_passages, ptr.ctypes.data,
                                             self.tok_emb.data_ptr() if self.n_tokens else None, dim, LATE_DTYPES[dtype],
                                             C.byref(self._handle)))

    @classmethod
    def from_ragged(cls, arrays, dtype: str = "bf16", device=None) -> "TokenIndex":
        """From one float array [t_i, dim] per passage (t_i = 0: a passage without tokens), rounded to `dtype`."""
        ptr, rows, _ = _ragged_rows(arrays, dtype, "arrays")
        return cls(ptr, rows, dtype, device)

    @classmethod
    def from_csr(cls, tok_ptr, tok_emb, dtype: str = "bf16", device=None) -> "TokenIndex":
        """From the CSR form itself: tok_ptr [n + 1] and tok_emb [T, dim], a torch bf16 / fp16 tensor (taken as it is) or a
        float array (rounded to `dtype`)."""
        torch = _torch()
        check_late_dtype(dtype)
        if not hasattr(tok_emb, "detach"):
            tok_emb = torch.from_numpy(np.ascontiguousarray(np.asarray(tok_emb)))
        if tok_emb.dim() != 2:
            raise ValueError("tok_emb: [T, dim] expected")
        if tok_emb.dtype != _torch_dtype(dtype):
            if tok_emb.dtype in (torch.bfloat16, torch.float16):
                raise ValueError(f"tok_emb is {tok_emb.dtype}, dtype={dtype!r} was asked for")
            tok_emb = tok_emb.to(_torch_dtype(dtype))
        return cls(tok_ptr, tok_emb, dtype, device)

    def close(self):
        if getattr(self, "_handle", None) and self._handle.value:
            check(self._lib.hrag_late_destroy(self._handle))
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


class LateQueries:
    """The token vectors of a batch of queries: q_ptr int32 [B + 1] (a host copy for the checks, a device copy for the
    kernel) and q_tok [T, dim] of the 16-bit type on the device."""

    def __init__(self, q_ptr, q_tok, dtype: str = "bf16", device=None):
        torch = _torch()
        check_late_dtype(dtype)
        if not hasattr(q_tok, "dtype") or q_tok.dtype != _torch_dtype(dtype) or q_tok.dim() != 2:
            raise ValueError(f"q_tok: a torch {dtype} tensor [T, dim] expected")
        self.dim = check_late_dim(int(q_tok.shape[1]), "q_tok: dim")
        ptr = check_tok_ptr(q_ptr, q_tok.shape[0], "q_ptr", LATE_MAX_QUERY_TOKENS)
        if ptr.shape[0] < 2:
            raise ValueError("q_ptr: at least one query expected")
        self.dtype = dtype
        self.device = _device(device) if device is not None or torch.cuda.is_available() else torch.device("cpu")
        self.q_ptr = ptr.astype(np.int32)
        self.q_ptr_dev = torch.from_numpy(self.q_ptr).to(self.device)
        self.q_tok = q_tok.to(self.device).contiguous()
        self.batch, self.n_tokens = ptr.shape[0] - 1, int(ptr[-1])

    @classmethod
    def from_ragged(cls, arrays, dtype: str = "bf16", device=None) -> "LateQueries":
        """From one float array [t_i, dim] per query (t_i = 0: a query without tokens; at most LATE_MAX_QUERY_TOKENS)."""
        ptr, rows, _ = _ragged_rows(arrays, dtype, "arrays")
        return cls(ptr, rows, dtype, device)

    def select(self, rows) -> "LateQueries":
        """The queries `rows` (positions in this batch, in the order given; repeats allowed) as a batch of their own."""
        torch = _torch()
        r = np.asarray(rows, np.int64).reshape(-1)
        if r.size == 0 or (r < 0).any() or (r >= self.batch).any():
            raise ValueError(f"rows: positions in [0, {self.batch}) expected, at least one")
        p = self.q_ptr.astype(np.int64)
        take = (np.concatenate([np.arange(p[i], p[i + 1]) for i in r]) if r.size else np.zeros(0, np.int64)).astype(np.int64)
        ptr = np.zeros(r.size + 1, np.int64)
        ptr[1:] = np.cumsum(p[r + 1] - p[r])
        tok = self.q_tok[torch.from_numpy(take).to(self.device)] if take.size else self.q_tok[:0]
        return LateQueries(ptr, tok, self.dtype, self.device)


def check_late(late, k, c, batch: Optional[int] = None) -> "LateQueries":
    """The arguments of a late call as the library takes them: late a LateQueries (of `batch` queries when given), ints
    1 <= k <= c <= LATE_MAX_CANDIDATES."""
    if not isinstance(late, LateQueries):
        raise ValueError(f"late: a LateQueries expected (LateQueries.from_ragged), not {type(late).__name__}")
    for name, v in (("k", k), ("late_candidates", c)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name}={v!r}: an int expected")
    if not 1 <= int(c) <= LATE_MAX_CANDIDATES:
        raise ValueError(f"late_candidates={c}: outside [1, {LATE_MAX_CANDIDATES}]")
    if not 1 <= int(k) <= int(c):
        raise ValueError(f"k={k}: outside [1, late_candidates={c}]")
    if batch is not None and late.batch != batch:
        raise ValueError(f"late: it holds {late.batch} queries, the call {batch}")
    return late


def late_plan(late, late_candidates, k: int):
    """None without late (late_candidates then has to be None too), else (late, c): the call ranks
    c = max(late_candidates, k) entries (late_candidates None: k), rescores them and keeps the k best by late score."""
    if late is None:
        if late_candidates is not None:
            raise ValueError("late_candidates needs late")
        return None
    c = k if late_candidates is None else late_candidates
    if isinstance(c, bool) or not isinstance(c, (int, np.integer)):
        raise ValueError(f"late_candidates={c!r}: an int expected")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError(f"k={k!r}: an int expected")
    c = max(int(c), int(k))
    return check_late(late, k, c), c


def refuse_late(who: str, kw: dict) -> None:
    """The callers that do not serve late-interaction reranking name the argument they refuse."""
    for name in ("late", "late_candidates"):
        if kw.get(name) is not None:
            raise NotImplementedError(f"{who} does not serve {name}: late reranking rescores the candidates of one unsharded "
                                      "engine's plain ranking against its token index -- use HippoRAGEngine.retrieve(late=...) "
                                      "or HippoRAGEngine.late_rerank")
