"""Torch-facing wrapper of the libhrag.so engine (include/hrag.h).

PyTorch supplies device memory and the current HIP stream; all arithmetic on the path happens in
the hand-written gfx950 kernels behind the C ABI.  There is no CPU or eager-torch fallback: without
a GPU (or without libhrag.so) constructing an engine raises.
"""

from __future__ import annotations

import ctypes as C
import logging
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import _lib
from ._lib import (EmbedDesc, FactDesc, GraphDesc, Opts, ShardLayout, Timings, check, FLAG_DPR_FALLBACK,
                   FLAG_FP8_SATURATED, FLAG_ZERO_MASS, FLAG_ZERO_PHRASE, SEED_STRIDE)
from .graph import CSRGraph
from .lexical import invert_postings
from .payload import PayloadFilter, PayloadIndex, compile_filters     # noqa: F401  (re-exported: the payload filters)
from .boost import BoostProgram, check_program, compile_boosts        # noqa: F401  (re-exported: boosted retrieval)
from .boost import boost_rows as _boost_rows
from .facet import FacetCounts, FacetSpec, compile_facet              # noqa: F401  (re-exported: facets)
from .late import (LATE_DTYPES, LateQueries, TokenIndex, check_late, late_plan,      # noqa: F401  (re-exported: late-interaction
                   refuse_late)                                                    # reranking)
from .reco import (Examples, check_examples, check_feedback_weight, check_strategy,  # noqa: F401  (re-exported: recommend by
                   refuse_reco)                                                      # example)


def _torch():
    import torch
    return torch


def _ptr(a) -> int:
    """Address of a numpy array (host) or torch tensor (host or device)."""
    if a is None:
        return 0
    if isinstance(a, np.ndarray):
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError("array must be C-contiguous")
        return a.ctypes.data
    if not a.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return a.data_ptr()


def _stream() -> int:
    return _torch().cuda.current_stream().cuda_stream


def pack_mask(mask) -> np.ndarray:
    """Host bool [..., n] -> the doc filter's bitset (include/hrag.h): uint32 [..., ceil(n / 32)], bit (j & 31) of word
    j >> 5 set when j is allowed -- np.packbits(bitorder="little"), each row padded to 4 bytes, read little-endian."""
    m = np.asarray(mask, dtype=bool)
    n = m.shape[-1]
    w = (n + 31) // 32
    b = np.packbits(m, axis=-1, bitorder="little")
    pad = np.zeros(m.shape[:-1] + (4 * w,), np.uint8)
    pad[..., :b.shape[-1]] = b
    return pad.view("<u4").astype(np.uint32, copy=False)


FILTER_SCOPES = ("ranking", "seeds")
GROUP_AGGS = {"max": 0, "sum": 1}      # HRAG_GROUP_MAX / HRAG_GROUP_SUM
GROUP_HITS_MAX = 64                    # HRAG_GROUP_HITS_MAX
FUSE_MODES = {"sum": 0, "max": 1, "rrf": 2}     # HRAG_FUSE_SUM / HRAG_FUSE_MAX / HRAG_FUSE_RRF
MMR_MAX_CANDIDATES = 1024              # HRAG_MMR_MAX_CANDIDATES
MMR_WORKSPACE_CAP = 256 << 20          # bytes of Gram workspace one hrag_mmr call may take: larger batches go in slices
LEX_TILE = _lib.LEX_TILE                               # HRAG_LEX_TILE
LEX_MAX_QUERY_TERMS = _lib.LEX_MAX_QUERY_TERMS         # HRAG_LEX_MAX_QUERY_TERMS


def check_group_agg(group_agg) -> Optional[int]:
    """None (ungrouped) or the HRAG_GROUP_* code of "max" / "sum"."""
    if group_agg is None:
        return None
    if group_agg not in GROUP_AGGS:
        raise ValueError(f"group_agg={group_agg!r}: None, 'max' or 'sum' expected")
    return GROUP_AGGS[group_agg]


def check_group_hits(group_hits, group_agg) -> Optional[int]:
    """None (the representative only) or m, the passages wanted per ranked group (include/hrag.h, group hits): an int in
    [1, GROUP_HITS_MAX], valid only on a grouped call."""
    if group_hits is None:
        return None
    if group_agg is None:
        raise ValueError("group_hits needs group_agg: it asks for the best passages of each ranked GROUP")
    if isinstance(group_hits, bool) or not isinstance(group_hits, (int, np.integer)):
        raise ValueError(f"group_hits={group_hits!r}: None or an int in [1, {GROUP_HITS_MAX}] expected")
    if not 1 <= int(group_hits) <= GROUP_HITS_MAX:
        raise ValueError(f"group_hits={group_hits}: outside [1, {GROUP_HITS_MAX}]")
    return int(group_hits)


def check_fuse(fuse, member_ptr, batch: int, weights=None, rrf_c: int = 60, rrf_depth=None, depth_max=None):
    """The arguments of a fused call (include/hrag.h, fused retrieval) as the library takes them: (mode, member_ptr int32
    [Q + 1], weights fp32 [batch] or None, rrf_c, rrf_depth).  member_ptr runs from 0 to batch, strictly increasing; every
    weight is finite and >= 0 and "max" takes none; "rrf": an int rrf_c >= 0 and 1 <= rrf_depth <= depth_max (min(max_topk,
    n_passages) of the engine; not checked when None).  The other modes return rrf_c = 0, rrf_depth = 0."""
    if fuse not in FUSE_MODES:
        raise ValueError(f"fuse={fuse!r}: 'sum', 'max' or 'rrf' expected")
    mp = np.asarray(member_ptr)
    if mp.ndim != 1 or mp.shape[0] < 2 or mp.dtype.kind not in "iu":
        raise ValueError("member_ptr: an integer array of Q + 1 >= 2 entries expected")
    mp = mp.astype(np.int64)
    if mp[0] != 0 or mp[-1] != batch:
        raise ValueError(f"member_ptr must run from 0 to the batch of {batch} member rows (it runs from {mp[0]} to {mp[-1]})")
    if (np.diff(mp) <= 0).any():
        raise ValueError("member_ptr must be strictly increasing: every question has at least one member")
    w = None
    if weights is not None:
        if fuse == "max":
            raise ValueError('fuse="max" takes no weights')
        w = np.asarray(weights, np.float32)
        if w.shape != (batch,):
            raise ValueError(f"weights of shape {w.shape}: one per member row, ({batch},), expected")
        if not np.isfinite(w).all() or (w < 0).any():
            raise ValueError("every weight must be finite and >= 0")
        w = np.ascontiguousarray(w)
    c = depth = 0
    if fuse == "rrf":
        if isinstance(rrf_c, bool) or not isinstance(rrf_c, (int, np.integer)) or not 0 <= int(rrf_c) < 2 ** 31:
            raise ValueError(f"rrf_c={rrf_c!r}: an int >= 0 expected")
        if isinstance(rrf_depth, bool) or not isinstance(rrf_depth, (int, np.integer)):
            raise ValueError(f"rrf_depth={rrf_depth!r}: an int >= 1 expected")
        if int(rrf_depth) < 1 or (depth_max is not None and int(rrf_depth) > depth_max):
            raise ValueError(f"rrf_depth={rrf_depth}: outside [1, {depth_max if depth_max is not None else 'min(max_topk, n_passages)'}]")
        c, depth = int(rrf_c), int(rrf_depth)
    return FUSE_MODES[fuse], np.ascontiguousarray(mp, dtype=np.int32), w, c, depth


def check_mmr(lam, k, c) -> float:
    """The arguments of an MMR call (include/hrag.h, diversified retrieval) as the library takes them: lambda a real number
    in [0, 1] (not NaN, not a bool), ints 1 <= k <= c <= MMR_MAX_CANDIDATES.  Returns lambda as a float."""
    if isinstance(lam, bool) or not isinstance(lam, (int, float, np.integer, np.floating)):
        raise ValueError(f"mmr_lambda={lam!r}: a number in [0, 1] expected")
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:           # (False for NaN)
        raise ValueError(f"mmr_lambda={lam}: outside [0, 1]")
    for name, v in (("k", k), ("mmr_candidates", c)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name}={v!r}: an int expected")
    if not 1 <= int(c) <= MMR_MAX_CANDIDATES:
        raise ValueError(f"mmr_candidates={c}: outside [1, {MMR_MAX_CANDIDATES}]")
    if not 1 <= int(k) <= int(c):
        raise ValueError(f"k={k}: outside [1, mmr_candidates={c}]")
    return lam


def mmr_plan(mmr_lambda, mmr_candidates, k: int):
    """None without mmr_lambda (mmr_candidates then has to be None too), else (lambda, c): the call ranks
    c = max(mmr_candidates, k) entries (mmr_candidates None: k) and MMR picks k of them."""
    if mmr_lambda is None:
        if mmr_candidates is not None:
            raise ValueError("mmr_candidates needs mmr_lambda")
        return None
    c = k if mmr_candidates is None else mmr_candidates
    if isinstance(c, bool) or not isinstance(c, (int, np.integer)):
        raise ValueError(f"mmr_candidates={c!r}: an int expected")
    c = max(int(c), int(k))
    return check_mmr(mmr_lambda, k, c), c


def refuse_mmr(who: str, kw: dict) -> None:
    """The callers that do not serve MMR name the argument they refuse."""
    for name in ("mmr_lambda", "mmr_candidates"):
        if kw.get(name) is not None:
            raise ValueError(f"{who} does not serve {name}: MMR reads the passage embeddings of one unsharded engine after a "
                             "plain ranking -- use HippoRAGEngine.retrieve(mmr_lambda=...) or HippoRAGEngine.mmr")


def _host_array(a, name: str) -> np.ndarray:
    if isinstance(a, np.ndarray):
        return a
    if hasattr(a, "detach") and hasattr(a, "cpu"):      # a torch tensor (a device tensor is read back: pass host arrays)
        return a.detach().cpu().numpy()
    raise ValueError(f"lexical: {name} must be a numpy array or a torch tensor, not {type(a).__name__}")


def check_lexical_weight(lexical_weight) -> float:
    """lexical_weight as the library takes it: a real number in [0, 1] (not NaN, not a bool)."""
    if isinstance(lexical_weight, bool) or not isinstance(lexical_weight, (int, float, np.integer, np.floating)):
        raise ValueError(f"lexical_weight={lexical_weight!r}: a number in [0, 1] expected")
    w = float(lexical_weight)
    if not 0.0 <= w <= 1.0:             # (False for NaN)
        raise ValueError(f"lexical_weight={w}: outside [0, 1]")
    return w


def check_lexical(lexical, lexical_weight, batch: Optional[int]):
    """The sparse queries of a lexical call (include/hrag.h, lexical retrieval) as the library takes them: lexical =
    (q_ptr int32 [batch + 1], q_term int32 [nnz], q_weight fp32 [nnz]), the terms of query b at q_ptr[b] .. q_ptr[b + 1].
    q_ptr runs from 0 to nnz without decreasing; the dtypes are exactly int32 / int32 / fp32 (a silent cast would hide a
    caller's float64 weights or int64 hashes); no query lists more than LEX_MAX_QUERY_TERMS terms -- the device would
    ignore the rest, so this RAISES instead of truncating; lexical_weight a number in [0, 1].  batch None: whatever
    q_ptr says.  Returns (q_ptr, q_term, q_weight, weight) as contiguous host arrays and a float."""
    if not isinstance(lexical, (tuple, list)) or len(lexical) != 3:
        raise ValueError("lexical: a (q_ptr, q_term, q_weight) triple expected")
    weight = check_lexical_weight(lexical_weight)
    qp, qt, qw = (_host_array(a, n) for a, n in zip(lexical, ("q_ptr", "q_term", "q_weight")))
    for a, name, dt in ((qp, "q_ptr", np.int32), (qt, "q_term", np.int32), (qw, "q_weight", np.float32)):
        if a.dtype != dt:
            raise ValueError(f"lexical: {name} has dtype {a.dtype}, {np.dtype(dt).name} expected")
        if a.ndim != 1:
            raise ValueError(f"lexical: {name} must be one-dimensional")
    if qp.shape[0] < 2 or (batch is not None and qp.shape[0] != batch + 1):
        raise ValueError(f"lexical: q_ptr has {qp.shape[0]} entries, batch + 1 = "
                         f"{'at least 2' if batch is None else batch + 1} expected")
    if qt.shape[0] != qw.shape[0]:
        raise ValueError(f"lexical: q_term has {qt.shape[0]} entries and q_weight {qw.shape[0]}")
    if qp[0] != 0 or qp[-1] != qt.shape[0]:
        raise ValueError(f"lexical: q_ptr must run from 0 to the {qt.shape[0]} listed terms (it runs from {qp[0]} to {qp[-1]})")
    lens = np.diff(qp.astype(np.int64))
    if (lens < 0).any():
        raise ValueError("lexical: q_ptr must not decrease")
    if (lens > LEX_MAX_QUERY_TERMS).any():
        raise ValueError(f"lexical: query {int(np.argmax(lens))} lists {int(lens.max())} terms, at most "
                         f"LEX_MAX_QUERY_TERMS={LEX_MAX_QUERY_TERMS} are scored (merge repeated terms or drop the rarest)")
    return np.ascontiguousarray(qp), np.ascontiguousarray(qt), np.ascontiguousarray(qw), weight


def refuse_lexical(who: str, kw: dict) -> None:
    """The callers that do not serve lexical retrieval name the argument they refuse."""
    if kw.get("lexical") is not None:
        raise NotImplementedError(f"{who} does not serve lexical: the lexical score rows cover every passage of one "
                                  "unsharded engine and are blended before the call's own min-max -- use "
                                  "HippoRAGEngine.retrieve(lexical=...)")
    if kw.get("lexical_weight") not in (None, 0, 0.0):
        raise NotImplementedError(f"{who} does not serve lexical_weight: use HippoRAGEngine.retrieve(lexical=..., "
                                  "lexical_weight=...)")


class LexicalIndex:
    """A sparse passage index on the device (hrag_lex_create; include/hrag.h, lexical retrieval): per term, the passages
    that hold it and a weight each.  Independent of any engine -- HippoRAGEngine.set_lexical_index takes it by reference,
    so several engines and their workspaces over the same passages share one.  The library scores whatever weights it is
    given (hipporag_amd.lexical.bm25_weights makes BM25 ones)."""

    def __init__(self, n_passages: int, n_terms: int, term_ptr, post_doc, post_w, device: Optional[int] = None):
        torch = _torch()
        if not torch.cuda.is_available():
            raise RuntimeError("LexicalIndex needs an MI355X-class GPU: no HIP device is visible (there is no CPU fallback)")
        self._lib = _lib.load()
        self._handle = C.c_void_p(0)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        tp = np.ascontiguousarray(term_ptr, dtype=np.int64)
        pd = np.ascontiguousarray(post_doc, dtype=np.int32)
        pw = np.ascontiguousarray(post_w, dtype=np.float32)
        if tp.ndim != 1 or tp.shape[0] != int(n_terms) + 1:
            raise ValueError(f"term_ptr: {int(n_terms) + 1} entries expected")
        if pd.ndim != 1 or pd.shape != pw.shape or (tp.size and int(tp[-1]) != pd.shape[0]):
            raise ValueError("post_doc / post_w: one entry per posting, term_ptr[-1] of them, expected")
        with torch.cuda.device(self.device):
            check(self._lib.hrag_lex_create(int(n_passages), int(n_terms), tp.ctypes.data, pd.ctypes.data if pd.size else None,
                                            pw.ctypes.data if pw.size else None, C.byref(self._handle)))
        self.n_passages, self.n_terms, self.nnz = int(n_passages), int(n_terms), int(pd.shape[0])

    @classmethod
    def from_postings(cls, n_passages: int, term_ptr, post_doc, post_w, device: Optional[int] = None) -> "LexicalIndex":
        """From the inverted form itself: the posting list of term t is post_doc[term_ptr[t] : term_ptr[t + 1]]."""
        return cls(n_passages, len(term_ptr) - 1, term_ptr, post_doc, post_w, device)

    @classmethod
    def from_csr(cls, row_ptr, term, weight, n_terms: Optional[int] = None, device: Optional[int] = None) -> "LexicalIndex":
        """From passage-major rows (invert_postings, on the host); a term repeated within a passage is rejected.
        n_terms None: the largest term id + 1."""
        n = len(row_ptr) - 1
        if n_terms is None:
            n_terms = int(np.max(term)) + 1 if np.size(term) else 0
        return cls(n, n_terms, *invert_postings(n, n_terms, row_ptr, term, weight), device)

    def close(self):
        if getattr(self, "_handle", None) and self._handle.value:
            check(self._lib.hrag_lex_destroy(self._handle))
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


def group_table_csr(group_of, n_groups: int):
    """The CSR the engine builds from a passage -> group table: (group_ptr int64 [n_groups + 1], members int32 [n],
    the members of a group in ascending passage position)."""
    g = np.asarray(group_of, np.int64)
    ptr = np.zeros(n_groups + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(g, minlength=n_groups))
    return ptr, np.argsort(g, kind="stable").astype(np.int32)


def refuse_group_agg(who: str, kw: dict) -> None:
    """The multi-GPU retrievers and the captured pipeline do not serve grouped retrieval."""
    if kw.get("group_agg") is not None:
        raise NotImplementedError(f"{who} does not serve group_agg: a group's members span the row shards and a sum across "
                                  "shards is not bit-reproducible without a defined order -- use HippoRAGEngine.retrieve")
    if kw.get("group_hits") is not None:
        raise NotImplementedError(f"{who} does not serve group_hits (the best passages of each ranked group): use "
                                  "HippoRAGEngine.retrieve")
    if kw.get("fuse") is not None:
        raise NotImplementedError(f"{who} does not serve fuse (one ranking per question from several member queries): the "
                                  "fusion works on the score rows of one unsharded handle -- use HippoRAGEngine.retrieve + "
                                  "last_fused")


def refuse_boost(who: str, kw: dict) -> None:
    """The callers that do not serve boosted retrieval name the argument they refuse."""
    if kw.get("boost") is not None:
        raise NotImplementedError(f"{who} does not serve boost: the boost rewrites the score rows of one unsharded handle and "
                                  "ranks them again -- use HippoRAGEngine.retrieve(boost=...)")


def check_filter_scope(filter_scope: str, doc_filter) -> bool:
    """True for the "seeds" scope (include/hrag.h, scoped doc filter), False for "ranking" (the post-filter)."""
    if filter_scope not in FILTER_SCOPES:
        raise ValueError(f"filter_scope={filter_scope!r}: one of {FILTER_SCOPES} expected")
    if filter_scope == "seeds" and doc_filter is None:
        raise ValueError('filter_scope="seeds" needs a doc_filter (the allowed passages)')
    return filter_scope == "seeds"


def doc_filter_words(doc_filter, n: int, batch: int, device):
    """A doc filter -- torch bool [n] or [batch, n], or the packed uint32 (or int32) words [W] or [batch, W],
    W >= ceil(n / 32) -- as (int32 device words, filter_ld_words): ld 0 for one row shared by the batch."""
    torch = _torch()
    t = doc_filter if isinstance(doc_filter, torch.Tensor) else None
    if t is None:
        raise TypeError(f"doc_filter must be a torch tensor (bool or packed uint32), not {type(doc_filter).__name__}")
    if t.dim() not in (1, 2) or (t.dim() == 2 and t.shape[0] != batch):
        raise ValueError(f"doc_filter of shape {tuple(t.shape)}: [n] or [batch={batch}, n] expected")
    words = (n + 31) // 32
    if t.dtype == torch.bool:
        if t.shape[-1] != n:
            raise ValueError(f"doc_filter has {t.shape[-1]} entries, the engine ranks {n} passages")
        bits = torch.zeros(t.shape[:-1] + (words * 32,), dtype=torch.int64, device=device)
        bits[..., :n] = t.to(device)
        w = (bits.view(*t.shape[:-1], words, 32) << torch.arange(32, device=device, dtype=torch.int64)).sum(-1)
        w = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
    elif t.dtype == torch.int32 or str(t.dtype) == "torch.uint32":
        if t.shape[-1] < words:
            raise ValueError(f"packed doc_filter has {t.shape[-1]} words per row, ceil({n} / 32) = {words} needed")
        w = t.view(torch.int32) if t.dtype != torch.int32 else t
        w = w.to(device)
    else:
        raise TypeError(f"doc_filter dtype {t.dtype}: torch.bool or packed uint32 words expected")
    w = w.contiguous()
    return w, (0 if w.dim() == 1 else w.shape[1])


class SplitRows:
    """Embedding rows already in an HRAG_F32_SPLIT engine's layout (fp16 [rows, 3 * dim] on the device): what
    gather_embeddings returns on such an engine, accepted by the constructor (HRAG_F32_SPLIT_ROWS)."""

    def __init__(self, tensor, dim: int):
        self.tensor, self.dim = tensor, int(dim)
        self.shape = (tensor.shape[0], self.dim)

    def __getitem__(self, rows):        # row slices (dist.build_shard_engine)
        return SplitRows(self.tensor[rows], self.dim)


def _as_16bit(emb):
    """Accept a torch bf16 / fp16 tensor, a numpy float16 array, uint16 bf16 bit patterns (numpy / torch), or fp32
    (numpy / torch: the fp32-faithful HRAG_F32_SPLIT engine); return (obj, rows, dim, dtype) with dtype 0 = bf16,
    1 = fp16, 2 = fp32 split (hrag_dtype)."""
    torch = _torch()
    if isinstance(emb, SplitRows):
        return emb.tensor.contiguous(), emb.tensor.shape[0], emb.dim, 3
    if isinstance(emb, np.ndarray):
        if emb.dtype == np.float32:
            emb = np.ascontiguousarray(emb)
            return emb, emb.shape[0], emb.shape[1], 2
        if emb.dtype == np.float16:
            emb = np.ascontiguousarray(emb)
            return emb, emb.shape[0], emb.shape[1], 1
        if emb.dtype != np.uint16:
            raise TypeError("numpy embeddings must be float32 (fp32-faithful engine), float16, or uint16 bf16 bit "
                            "patterns (hipporag_amd.graph.float_to_bf16_bits)")
        emb = np.ascontiguousarray(emb)
        return emb, emb.shape[0], emb.shape[1], 0
    if emb.dtype not in (torch.bfloat16, torch.float16, torch.uint16, torch.int16, torch.float32):
        raise TypeError("tensor embeddings must be torch.float32, torch.bfloat16 or torch.float16 (or raw bf16 bit patterns)")
    emb = emb.contiguous()
    return emb, emb.shape[0], emb.shape[1], 2 if emb.dtype == torch.float32 else 1 if emb.dtype == torch.float16 else 0


_TORCH_DTYPE_OF = {0: "bfloat16", 1: "float16", 2: "float32", 3: "float32"}


@dataclass
class RetrieveOutput:
    doc_idx: "object"     # torch int32 [B, k] passage positions, best first
    doc_score: "object"   # torch fp32  [B, k]
    flags: "object"       # torch int32 [B]
    residual: "object" = None    # torch fp32 [B]: damping / (1 - damping) * the relative size of the last sweep's update
                                 # of the passage scores (include/hrag.h, hrag_retrieve); -1 where not measured
    iters_used: "object" = None  # torch int32 [B]: PPR sweeps that ran
    all_scores: "object" = None  # torch fp32 [B, Np] (retrieve_converged(want_all_scores=True)): every passage's score
    group_idx: "object" = None   # grouped call (group_agg=): torch int32 [B, k] group ids, best first; doc_idx then holds
                                 # each ranked group's representative passage and doc_score the group score

    hit_idx: "object" = None     # group_hits=m: torch int32 [B, k, m], the m best allowed passages of each ranked group, best
                                 # first (entry 0 is the representative), -1 beyond the group's allowed members
    hit_score: "object" = None   # torch fp32 [B, k, m]: each hit's own passage score (0 where hit_idx is -1)
    mmr_value: "object" = None   # mmr_lambda=: torch fp32 [B, k], the MMR value of each pick; doc_idx / doc_score then hold
                                 # the picks in MMR order with their own retrieval scores
    first_score: "object" = None  # late=: torch fp32 [B, k], the first-stage score of each returned entry (0 where doc_idx is
                                  # -1); doc_score then holds the late scores

    @property
    def group_score(self):       # the grouped call's names for the two tensors above
        return self.doc_score

    @property
    def best_doc_idx(self):
        return self.doc_idx


logger = logging.getLogger(__name__)


def host_copy_async(t):
    """(host tensor, event): the copy of device tensor `t` to pinned host memory, enqueued on the current stream; the
    event (None for a tensor that already lives on the host) completes when the copy has.  Waiting for the event does
    not wait for anything enqueued after it -- what a pipeline over batches needs (t.cpu() drains the stream)."""
    torch = _torch()
    if not t.is_cuda:
        return t, None
    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    with torch.cuda.device(t.device):                 # the copy and its event on the tensor's own device and current stream
        h.copy_(t, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(t.device))
    return h, ev


def host_wait(pair):
    """The numpy view of a host_copy_async() result, once its copy has completed."""
    h, ev = pair
    if ev is not None:
        ev.synchronize()
    return h.numpy()


class PendingRetrieve:
    """A batch that HippoRAGEngine.retrieve_converged_start() enqueued.  finish() is the host half of the convergence
    contract (see retrieve_converged); `repeated` tells whether anything was run again (the output tensors then
    differ from what was enqueued first)."""

    def __init__(self, eng, run, out, flags_h, damping, ppr_iters, ppr_tol, ppr_max_iters, want_all_scores):
        self.eng, self.run, self.out, self.flags_h = eng, run, out, flags_h
        self.damping, self.ppr_iters, self.ppr_tol, self.ppr_max_iters = damping, ppr_iters, ppr_tol, ppr_max_iters
        self.want_all_scores = want_all_scores
        self.repeated, self.flags = False, None

    def finish(self) -> RetrieveOutput:
        torch = _torch()
        from ._lib import FLAG_FP8_SATURATED, FLAG_NOT_CONVERGED, OPT_NO_F16, OPT_NO_FP8
        eng, run, out = self.eng, self.run, self.out
        damping, ppr_iters, ppr_tol, ppr_max_iters = self.damping, self.ppr_iters, self.ppr_tol, self.ppr_max_iters

        def on_wider_state(fn, bits=OPT_NO_FP8):
            had = eng.opt_flags & bits               # restore what the engine was created with
            eng.set_flags(bits, True)
            try:
                return fn()
            finally:
                if bits & ~had:
                    eng.set_flags(bits & ~had, False)

        flags = host_wait(self.flags_h).copy()
        if (flags & FLAG_FP8_SATURATED).any() and (eng.opt_flags & _lib.OPT_ACCEL):
            # accelerated stages (HRAG_OPT_ACCEL): a violated scale bound falls back to the plain plan first
            logger.warning("fp8 PPR state saturated under HRAG_OPT_ACCEL for %d queries: repeating the batch on the plain plan",
                           int(((flags & FLAG_FP8_SATURATED) != 0).sum()))
            eng.set_flags(_lib.OPT_ACCEL, False)
            try:
                out = run()
            finally:
                eng.set_flags(_lib.OPT_ACCEL, True)
            self.repeated = True
            flags = out.flags.cpu().numpy()
        if (flags & FLAG_FP8_SATURATED).any():
            logger.warning("fp8 PPR state saturated for %d queries: repeating the batch on the wider state",
                           int(((flags & FLAG_FP8_SATURATED) != 0).sum()))
            out = on_wider_state(run)
            self.repeated = True
            flags = out.flags.cpu().numpy()
        self.out, self.flags = out, flags            # flags: the final flag words on the host (numpy)
        if ppr_tol <= 0 or not (flags & FLAG_NOT_CONVERGED).any():
            return out
        self.repeated = True
        resid, used = out.residual.cpu().numpy(), out.iters_used.cpu().numpy()
        for _ in range(6):
            rows = np.flatnonzero(flags & FLAG_NOT_CONVERGED)
            if not len(rows):
                break
            done = int(used[rows].max())
            need = done + int(np.ceil(np.log(max(float(resid[rows].max()) / ppr_tol, 1.0)) / -np.log(damping))) + 4
            need = min(max(need, done + 4), max(ppr_max_iters, ppr_iters))
            if need <= done:
                break                                   # ppr_max_iters reached: the flag stays
            logger.info("PPR not converged for %d queries after %d sweeps (residual %.2g > %.2g): repeating them "
                        "with %d sweeps", len(rows), done, float(resid[rows].max()), ppr_tol, need)
            rt = torch.as_tensor(rows, device=eng.device)
            # fp32 state: the scores that converge last are orders of magnitude below the largest one
            o2 = on_wider_state(lambda: run(rt, need, need), OPT_NO_FP8 | OPT_NO_F16)
            out.doc_idx[rt], out.doc_score[rt] = o2.doc_idx, o2.doc_score
            if out.group_idx is not None:
                out.group_idx[rt] = o2.group_idx
            if out.hit_idx is not None:
                out.hit_idx[rt], out.hit_score[rt] = o2.hit_idx, o2.hit_score
            if out.mmr_value is not None:
                out.mmr_value[rt] = o2.mmr_value
            if out.first_score is not None:
                out.first_score[rt] = o2.first_score
            out.flags[rt], out.residual[rt], out.iters_used[rt] = o2.flags, o2.residual, o2.iters_used
            if self.want_all_scores:
                out.all_scores[rt] = o2.all_scores
            flags[rows], resid[rows], used[rows] = (o2.flags.cpu().numpy(), o2.residual.cpu().numpy(),
                                                    o2.iters_used.cpu().numpy())
        left = (flags & FLAG_NOT_CONVERGED) != 0
        if left.any():
            logger.warning("PPR residual above ppr_tol=%.2g for %d queries after ppr_max_iters=%d sweeps (max %.2g)",
                           ppr_tol, int(left.sum()), ppr_max_iters, float(resid[left].max()))
        return out


def _graph_fingerprint(g) -> tuple:
    """A cheap identity of a CSR graph's arrays (sizes + strided samples of row_ptr / col_idx / val, no full pass): equal for
    the arrays an engine was created from, different -- with overwhelming likelihood -- once they were edited in place."""
    def sample(a):
        a = np.asarray(a)
        if a.size == 0:
            return b""
        step = max(1, a.size // 1024)
        return np.ascontiguousarray(a.reshape(-1)[::step][:1024]).tobytes()
    return (int(g.num_vertices), int(np.asarray(g.col_idx).shape[0]), hash(sample(g.row_ptr)), hash(sample(g.col_idx)),
            hash(sample(g.val)))


class HippoRAGEngine:
    """Device-resident retrieval state: CSR graph, bf16 fact / passage embeddings, lookup arrays.

    Mirrors what ``HippoRAG.prepare_retrieval_objects`` stages on the host (reference
    src/hipporag/HippoRAG.py:1287-1389).  Row-sharded construction (multi-GPU): pass the row shard
    of the CSR (``CSRGraph.rows``) with ``row_offset`` and the embedding shards with their offsets.
    """

    has_fact_sources = False     # set_fact_sources() was called (the scoped doc filter's phase A)

    def __init__(self, graph: CSRGraph, passage_vertex, passage_emb, fact_emb=None,
                 subj_vertex=None, obj_vertex=None, num_chunks=None, *, max_batch: int = 256,
                 max_topk: int = 200, slab_width: int = 0, long_row_nnz: int = 0,
                 row_offset: int = 0, passage_offset: int = 0, fact_offset: int = 0,
                 n_passages: Optional[int] = None, n_facts: Optional[int] = None,
                 device: Optional[int] = None, flags: int = 0, segment_nnz: int = 0, sell_seg_len: int = 0,
                 dim: Optional[int] = None, sell_sigma: int = 0, locality: Optional[str] = None):
        """locality ("auto" / "on" / "degree" / None): the graph compiler's vertex numbering; everything the caller sees --
        passage positions, fact ids, hrag_ppr's vertex order -- keeps the caller's numbering.  "on": graph.locality_order
        (vertices by the first passage that links them) + SELL-C-sigma windows + the XCD-blocked launch; "auto": that
        numbering, the two switches only when the renumbered matrix actually has locality (graph.locality_score >= 0.3);
        "degree": graph.degree_order (hubs first) -- an experiment switch, not a default: -4 ... -12 % per call for
        B <= 8 and +1.2 % for the wide batch on the 1M-vertex benchmark graph, but -6 % on the 100k-vertex one
        (docs/experiments/README.md).  Unsharded engines only.

        passage_emb=None (with dim=...): an engine WITHOUT embeddings -- the PPR side of the hybrid multi-GPU mode
        (dist.HybridRetriever): passage scores arrive through retrieve_scored(), seeds still come from subj_vertex /
        obj_vertex / num_chunks."""
        torch = _torch()
        if not torch.cuda.is_available():
            raise RuntimeError("HippoRAGEngine needs an MI355X-class GPU: no HIP device is visible "
                               "(there is no CPU fallback on this path)")
        self._lib = _lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self._handle = C.c_void_p(0)

        pv = np.ascontiguousarray(passage_vertex, dtype=np.int32)
        caller_graph = graph            # what the lazy undirected-graph test looks at (a relabelling changes nothing for it)
        self._perm = self._inv_perm = None
        self.locality_score = self.numbering = None
        if locality:
            if locality not in ("auto", "on", "degree"):
                raise ValueError("locality must be None, 'auto', 'on' or 'degree'")
            if row_offset != 0 or graph.row_ptr.shape[0] - 1 != graph.num_vertices:
                raise ValueError("the locality numbering is for unsharded engines (dist.shard_index relabels shards)")
            from .graph import degree_order, locality_order, locality_score, relabel_csr
            windows = False
            if locality == "degree":
                perm = degree_order(graph, pv)
            else:
                perm = locality_order(graph, pv)
                self.locality_score = locality_score(graph, perm=perm)       # of the matrix as it will be renumbered
                windows = locality == "on" or self.locality_score >= 0.3
            self.numbering = "degree" if locality == "degree" else "locality"
            graph = relabel_csr(graph, perm)
            pv = np.ascontiguousarray(perm[pv], dtype=np.int32)
            if subj_vertex is not None:
                sv_ = np.asarray(subj_vertex, dtype=np.int64)
                ov_ = np.asarray(obj_vertex, dtype=np.int64)
                subj_vertex = np.where(sv_ >= 0, perm[np.clip(sv_, 0, None)], -1).astype(np.int32)
                obj_vertex = np.where(ov_ >= 0, perm[np.clip(ov_, 0, None)], -1).astype(np.int32)
                nc_ = np.zeros(graph.num_vertices, dtype=np.int32)
                nc_[perm] = np.asarray(num_chunks, dtype=np.int32)
                num_chunks = nc_
            if windows:
                sell_sigma = sell_sigma or 16384
                flags |= _lib.OPT_XCD_BLOCKED
            self._perm = torch.from_numpy(perm).to(self.device)              # caller's vertex id -> engine's
            inv = np.empty_like(perm)
            inv[perm] = np.arange(perm.shape[0])
            self._inv_perm = torch.from_numpy(inv).to(self.device)
        self.n_passages = int(pv.shape[0]) if n_passages is None else int(n_passages)
        if passage_emb is None:
            if not dim or fact_emb is not None:
                raise ValueError("an engine without passage embeddings needs dim= and takes no fact embeddings")
            p_obj, p_rows, dt = None, self.n_passages, 0
        else:
            p_obj, p_rows, dim, dt = _as_16bit(passage_emb)
        self.emb_dtype = getattr(torch, _TORCH_DTYPE_OF[dt])    # the dtype queries travel in (fp32 on a split engine)
        self.f32_split = dt in (2, 3)
        row_ptr = np.ascontiguousarray(graph.row_ptr, dtype=np.int32)
        col_idx = np.ascontiguousarray(graph.col_idx, dtype=np.int32)
        val = np.ascontiguousarray(graph.val, dtype=np.float32)
        n_rows = row_ptr.shape[0] - 1
        # weighted degrees (optional): enable the fp8-state PPR for batches > 64 (csrc/ppr8.hip)
        col_sum = getattr(graph, "col_sum", None)
        if col_sum is not None:
            col_sum = np.ascontiguousarray(col_sum, dtype=np.float64)
            if col_sum.shape[0] != graph.num_vertices:
                raise ValueError("col_sum must have one entry per vertex")
        gd = GraphDesc(graph.num_vertices, row_offset, n_rows, col_idx.shape[0], _ptr(row_ptr),
                       _ptr(col_idx), _ptr(val), self.n_passages, _ptr(pv),
                       _ptr(col_sum) if col_sum is not None else None)
        pd = EmbedDesc(p_rows, passage_offset, dim, dt, _ptr(p_obj) if p_obj is not None else None)
        fdesc = fd = None
        keep = [pv, p_obj, row_ptr, col_idx, val, col_sum]
        self.n_facts = 0
        if fact_emb is None and passage_emb is None and subj_vertex is not None:
            # scores-only engine: the fact lookup arrays (seeds) without fact embeddings
            sv = np.ascontiguousarray(subj_vertex, dtype=np.int32)
            ov = np.ascontiguousarray(obj_vertex, dtype=np.int32)
            nc = np.ascontiguousarray(num_chunks, dtype=np.int32)
            self.n_facts = int(sv.shape[0])
            fdesc = EmbedDesc(0, 0, dim, dt, None)
            fd = FactDesc(self.n_facts, _ptr(sv), _ptr(ov), _ptr(nc))
            keep += [sv, ov, nc]
        if fact_emb is not None:
            f_obj, f_rows, f_dim, f_dt = _as_16bit(fact_emb)
            if f_dim != dim or (f_dt != dt and not (f_dt in (2, 3) and dt in (2, 3))):
                raise ValueError("fact / passage embedding dims or dtypes differ")
            sv = np.ascontiguousarray(subj_vertex, dtype=np.int32)
            ov = np.ascontiguousarray(obj_vertex, dtype=np.int32)
            nc = np.ascontiguousarray(num_chunks, dtype=np.int32)
            if nc.shape[0] != graph.num_vertices:
                raise ValueError("num_chunks must have one entry per vertex")
            self.n_facts = int(sv.shape[0]) if n_facts is None else int(n_facts)
            if sv.shape[0] != self.n_facts or ov.shape[0] != self.n_facts:
                raise ValueError("subj_vertex / obj_vertex must cover all (global) facts")
            fdesc = EmbedDesc(f_rows, fact_offset, dim, f_dt, _ptr(f_obj))
            fd = FactDesc(self.n_facts, _ptr(sv), _ptr(ov), _ptr(nc))
            keep += [f_obj, sv, ov, nc]
        # HRAG_OPT_ACCEL needs an undirected graph (real spectrum of the sweep operator): checked where the graph is at
        # hand (row sums of the adjacency == its column sums); a directed graph keeps the plain plan, loudly
        # -- evaluated only when the flag is asked for (here, or at the first set_flags(OPT_ACCEL)): the test walks the
        # whole matrix, which a plain engine (and every incremental re-prepare of one) has no use for
        import weakref
        self._undirected = None if (row_offset == 0 and n_rows == graph.num_vertices) else False
        self._graph_print = _graph_fingerprint(caller_graph)      # what was uploaded: the lazy test must see the same arrays
        try:
            self._graph_ref = weakref.ref(caller_graph)
        except TypeError:       # an object that cannot be weakly referenced: hold it only until the test has run
            self._graph_ref = lambda g=caller_graph: g
        if (flags & _lib.OPT_ACCEL) and not self._is_undirected():
            logger.warning("HRAG_OPT_ACCEL dropped: the graph does not look undirected (or has no col_sum / is a row shard)")
            flags &= ~_lib.OPT_ACCEL
        self.opt_flags = int(flags)      # HRAG_OPT_* bits as set_flags leaves them
        opts = Opts(max_batch, max_topk, slab_width, long_row_nnz, self.device.index, flags, segment_nnz, sell_seg_len, sell_sigma)
        with torch.cuda.device(self.device):
            check(self._lib.hrag_engine_create(C.byref(gd), C.byref(fdesc) if fdesc else None,
                                               C.byref(pd), C.byref(fd) if fd else None,
                                               C.byref(opts), C.byref(self._handle)))
        del keep
        self.num_vertices = int(graph.num_vertices)
        self.row_offset, self.n_rows = int(row_offset), int(n_rows)
        self.passage_rows, self.passage_offset = int(p_rows), int(passage_offset)
        self.fact_rows = int(fact_emb.shape[0]) if fact_emb is not None else 0
        self.fact_offset = int(fact_offset)
        self.dim = int(dim)
        self.max_batch, self.max_topk = int(max_batch), int(max_topk)

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        """Destroy the handle.  An engine closes the workspaces it handed out first (they borrow its index buffers)."""
        for w in list(getattr(self, "_workspaces", ())):
            w.close()
        if getattr(self, "_handle", None) and self._handle.value:
            check(self._lib.hrag_engine_destroy(self._handle))
            self._handle = C.c_void_p(0)
            parent = getattr(self, "_parent", None)
            if parent is not None and self in parent._workspaces:
                parent._workspaces.remove(self)

    def workspace(self) -> "HippoRAGEngine":
        """A second WORKSPACE on this index (hrag_workspace_create): an engine object with the same methods
        that shares this engine's device-resident index -- graph, SELL-8 matrices, embeddings: nothing is copied -- and owns
        its own per-call buffers, so another thread can run score_facts / retrieve on it, on its own stream, WHILE this
        engine (or another workspace) is inside a call.  Results are bit-identical.  Close workspaces before the engine
        (close() of the engine does it); gather_embeddings() on any handle needs all handles idle."""
        import copy
        root = getattr(self, "_parent", None) or self
        w = copy.copy(root)                      # plain attributes: sizes, numbering, dtype, the library
        w._handle = C.c_void_p(0)
        w._workspaces = []
        w._parent = root
        w._fuse_ws = w._fuse_host = w._mmr_ws = w._late_ws = None      # last_fused / mmr / late: scratch buffers of its own
        w._reco_ws = None                                    # ... and recommend's column table
        w._pay_words = None                                  # ... and the words of a PayloadFilter doc filter
        with _torch().cuda.device(root.device):
            check(root._lib.hrag_workspace_create(root._handle, C.byref(w._handle)))
        if not hasattr(root, "_workspaces"):
            root._workspaces = []
        root._workspaces.append(w)
        return w

    def stats(self) -> dict:
        """hrag_engine_stats: device bytes of the shared index / of this handle's workspace, the PPR state types the
        handle can run (and why not the e4m3 one), the state the last retrieve ran on, call counters."""
        from ._lib import FP8_UNAVAILABLE, Stats
        s = Stats()
        check(self._lib.hrag_engine_stats(self._handle, C.byref(s)))
        d = {name: int(getattr(s, name)) for name, _ in Stats._fields_ if name != "reserved"}
        d["fp8_unavailable_reasons"] = [txt for bit, txt in FP8_UNAVAILABLE.items() if s.fp8_unavailable & bit]
        return d

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------ helpers
    def _q(self, q):
        torch = _torch()
        if q.dtype != self.emb_dtype:      # queries travel in the engine's embedding dtype (bf16 / fp16)
            q = q.to(self.emb_dtype)
        q = q.to(self.device).contiguous()
        if q.dim() != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must be [B, {self.dim}]")
        return q

    def _empty(self, shape, dtype):
        return _torch().empty(shape, dtype=dtype, device=self.device)

    def set_profiling(self, on: bool):
        check(self._lib.hrag_set_profiling(self._handle, 1 if on else 0))

    def timings(self) -> dict:
        t = Timings()
        check(self._lib.hrag_get_timings(self._handle, C.byref(t)))
        return {name: getattr(t, name) for name, _ in Timings._fields_}

    def layout(self, batch: int) -> Tuple[int, int]:
        bc, ns = C.c_int32(), C.c_int32()
        check(self._lib.hrag_ppr_layout(self._handle, batch, C.byref(bc), C.byref(ns)))
        return bc.value, ns.value

    # ------------------------------------------------------------------ fused entry points
    def set_fact_sources(self, row_ptr, passage_pos):
        """The fact -> source-passage table of the scoped doc filter (hrag_engine_set_fact_sources): the sources of fact f
        are passage_pos[row_ptr[f]:row_ptr[f + 1]] (passage positions).  On the root engine, before any workspace."""
        if getattr(self, "_parent", None) is not None:
            raise ValueError("fact sources belong to the shared index: set them on the root engine")
        rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
        pp = np.ascontiguousarray(passage_pos, dtype=np.int32)
        if rp.ndim != 1 or rp.shape[0] < 1 or pp.ndim != 1:
            raise ValueError("row_ptr [n_facts + 1] and passage_pos [nnz] expected")
        check(self._lib.hrag_engine_set_fact_sources(self._handle, rp.ctypes.data, pp.ctypes.data if pp.size else None,
                                                     rp.shape[0] - 1, pp.shape[0]))
        self.has_fact_sources = True

    def set_passage_groups(self, group_of):
        """The passage -> group table of grouped retrieval (hrag_engine_set_passage_groups): group_of[p] in [0, G) for every
        passage position p, G = max + 1 (None clears it).  On the root engine, with no live workspaces."""
        if getattr(self, "_parent", None) is not None:
            raise ValueError("passage groups belong to the shared index: set them on the root engine")
        if group_of is None:
            check(self._lib.hrag_engine_set_passage_groups(self._handle, None, 0))
            self.n_groups = 0
            return
        g = np.asarray(group_of)
        if g.ndim != 1 or g.shape[0] != self.n_passages or g.dtype.kind not in "iu":
            raise ValueError(f"group_of: an integer array of {self.n_passages} entries (one per passage) expected")
        if g.size and (int(g.min()) < 0 or int(g.max()) >= self.n_passages):
            raise ValueError("group ids must lie in [0, n_passages)")
        g = np.ascontiguousarray(g, dtype=np.int32)
        n_groups = int(g.max()) + 1
        check(self._lib.hrag_engine_set_passage_groups(self._handle, g.ctypes.data, n_groups))
        self.n_groups = n_groups

    def score_facts(self, q_fact, k: int = 5, scope_filter=None):
        """Phase A: (fact ids int32 [B,k], min-max normalised scores fp32 [B,k]).
        scope_filter: a doc filter (doc_filter_words) -- the top k among the facts of those passages, normalised over
        them (hrag_score_facts_scoped; needs set_fact_sources)."""
        torch = _torch()
        q = self._q(q_fact)
        b = q.shape[0]
        idx = self._empty((b, k), torch.int32)
        sc = self._empty((b, k), torch.float32)
        if scope_filter is None:
            check(self._lib.hrag_score_facts(self._handle, q.data_ptr(), b, k, idx.data_ptr(), sc.data_ptr(),
                                             _stream()))
        else:
            fw, fld = self._filter_words(scope_filter, b, "scope_filter")
            check(self._lib.hrag_score_facts_scoped(self._handle, q.data_ptr(), b, k, idx.data_ptr(), sc.data_ptr(),
                                                    _stream(), fw.data_ptr(), fld))
        return idx, sc

    def retrieve(self, q_pass, kept_idx, kept_score, kept_count, *, link_top_k: int = 5,
                 damping: float = 0.5, passage_node_weight: float = 0.05, ppr_iters: int = 20,
                 k: int = 200, ppr_tol: float = 0.0, ppr_max_iters: int = 0,
                 want_residual: bool = True, doc_filter=None, filter_scope: str = "ranking",
                 group_agg: Optional[str] = None, group_hits: Optional[int] = None,
                 mmr_lambda: Optional[float] = None, mmr_candidates: Optional[int] = None,
                 lexical=None, lexical_weight: float = 0.5, boost=None, late=None,
                 late_candidates: Optional[int] = None, feedback=None, feedback_weight: float = 0.3,
                 feedback_strategy: str = "best_score") -> RetrieveOutput:
        """Phase B: seeds + passage prior + PPR + ranking (DPR ranking where kept_count == 0).
        ppr_tol / ppr_max_iters: the convergence contract of include/hrag.h (0 = exactly ppr_iters sweeps);
        the output carries the per-query residual and the sweeps that ran.
        doc_filter: only these passages may be ranked (doc_filter_words; hrag_retrieve_filtered): each row is the first
        min(k, allowed) allowed entries of the unfiltered ranking, then -1 / 0.  Scoring is unchanged.
        filter_scope="seeds": the passage prior and the DPR fallback are normalised over the allowed passages as well
        (hrag_retrieve_scoped; the kept facts should come from score_facts(scope_filter=) with the same filter).
        group_agg="max" | "sum" (after set_passage_groups; hrag_retrieve_grouped): the k best GROUPS -- group_idx, their
        scores (group_score = doc_score) and each group's best passage (best_doc_idx = doc_idx); composes with both.
        group_hits=m (with group_agg; hrag_last_group_hits right behind the grouped call): hit_idx / hit_score [B, k, m],
        the m best allowed passages of each ranked group with their own scores; every other output is unchanged.
        mmr_lambda in [0, 1] (include/hrag.h, diversified retrieval; hrag_mmr behind the ranking): the call ranks
        c = max(mmr_candidates, k) <= min(max_topk, 1024) entries (mmr_candidates None: k) and returns the k MMR picks among
        them in doc_idx / doc_score (their own scores, MMR order) and mmr_value; relevance is the min-max of the candidates'
        scores.  With group_agg the candidates are the groups' best passages with the group scores, and group_idx / the
        hits follow the picks.  None: the call and its outputs are exactly the plain ones.
        lexical=(q_ptr, q_term, q_weight) (check_lexical; after set_lexical_index; include/hrag.h, lexical retrieval): the
        passage scores are the dense ones (hrag_sim_scores) blended with the lexical rows of these sparse queries at
        lexical_weight in [0, 1] (hrag_row_minmax, hrag_lex_scores, hrag_lex_blend_rows), handed to hrag_retrieve_scored*:
        the doc filter (scope "ranking"), group_agg, group_hits, mmr_* and a following last_fused work as they do there.  A
        query whose terms match nothing keeps its dense row bit for bit.  None: the call is exactly the plain one.
        boost= a BoostProgram or the grammar of compile_boosts (after set_payload_index; include/hrag.h, boosted retrieval):
        the call runs as it does without it, then hrag_last_boosted rewrites the score rows it left as s * M + A and ranks
        them again with the call's k, doc filter, group_agg, group_hits and mmr_*: every ranking output is that of the
        boosted rows, flags / residual / iters_used stay the call's, and last_doc_scores / last_fused afterwards read the
        boosted rows.  The first ranking is computed and discarded.  None: the call is exactly the plain one.
        late= a LateQueries (after set_token_index; include/hrag.h, late-interaction reranking): the call ranks
        c = max(late_candidates, k) <= min(max_topk, 1024) entries (late_candidates None: k) as it does without it -- under
        the doc filter, the lexical blend and the boost -- then hrag_late_rerank rescores them by MaxSim over the token index
        and the k best by late score are returned: doc_score carries the late scores, first_score each entry's first-stage
        score, a tie goes to the earlier first-stage rank.  With mmr_lambda, MMR picks its k among the c rescored entries
        with the late scores as relevance (mmr_candidates is then refused: the candidates are the late ones).  Not with
        group_agg / group_hits: a group's score is not a passage's.  None: the call is exactly the plain one.
        feedback= an Examples (include/hrag.h, recommend by example): relevance feedback into the passage prior -- the
        passage scores are the dense ones (hrag_sim_scores) blended with the recommend rows of these examples
        (hrag_reco_scores, feedback_strategy "best_score" | "sum_scores") at feedback_weight in [0, 1]: hrag_row_minmax of
        each, hrag_lex_blend_rows, then hrag_retrieve_scored* -- the path lexical= takes, so everything behind it composes.
        The examples are NOT excluded: the caller's doc_filter decides.  Not with lexical (both own the blend);
        feedback_weight=0 leaves the call bit-identical to the plain one.  None: the call is exactly the plain one."""
        lp = late_plan(late, late_candidates, k)
        if feedback is not None:
            if lexical is not None:
                raise ValueError("feedback together with lexical: both own the blend of the passage scores -- blend the "
                                 "rows yourself (lexical_scores, recommend_scores) and call retrieve_scored")
            check_examples(feedback, None, "feedback")
            check_strategy(feedback_strategy, True, "feedback_strategy")
            if check_feedback_weight(feedback_weight) != 0.0:
                mmr = mmr_plan(mmr_lambda, mmr_candidates, k)     # (refused before the blend is enqueued)
                self._check_mmr_fits(mmr)
                self._check_late_fits(lp, mmr, group_agg, group_hits)
                rows = self._feedback_blend(q_pass, feedback, feedback_weight, feedback_strategy, filter_scope, doc_filter)
                return self._retrieve("hrag_retrieve_scored", rows, (kept_idx, kept_score, kept_count),
                                      (link_top_k, damping, passage_node_weight, ppr_iters, max(ppr_max_iters, ppr_iters),
                                       ppr_tol),
                                      k, want_residual or ppr_tol > 0, doc_filter=doc_filter, filter_scope=filter_scope,
                                      group_agg=group_agg, group_hits=group_hits, mmr=mmr, boost=boost, late=lp)
        if lexical is not None:
            mmr = mmr_plan(mmr_lambda, mmr_candidates, k)     # (refused before the blend is enqueued)
            self._check_mmr_fits(mmr)
            self._check_late_fits(lp, mmr, group_agg, group_hits)
            rows = self._lexical_blend(None, q_pass, lexical, lexical_weight, filter_scope, doc_filter)
            return self._retrieve("hrag_retrieve_scored", rows, (kept_idx, kept_score, kept_count),
                                  (link_top_k, damping, passage_node_weight, ppr_iters, max(ppr_max_iters, ppr_iters), ppr_tol),
                                  k, want_residual or ppr_tol > 0, doc_filter=doc_filter, filter_scope=filter_scope,
                                  group_agg=group_agg, group_hits=group_hits, mmr=mmr, boost=boost, late=lp)
        return self._retrieve("hrag_retrieve", q_pass, (kept_idx, kept_score, kept_count),
                              (link_top_k, damping, passage_node_weight, ppr_iters, max(ppr_max_iters, ppr_iters), ppr_tol), k,
                              want_residual or ppr_tol > 0, doc_filter=doc_filter, filter_scope=filter_scope,
                              group_agg=group_agg, group_hits=group_hits, mmr=mmr_plan(mmr_lambda, mmr_candidates, k),
                              boost=boost, late=lp)

    def _retrieve(self, base, source, kept, ppr, k, report, *, doc_filter, filter_scope, group_agg, group_hits, mmr=None,
                  boost=None, late=None):
        """The one binding behind retrieve / retrieve_scored / dense_retrieve (base = "hrag_retrieve", "hrag_retrieve_scored"
        or "hrag_dense_retrieve"): the scope / agg / hits checks, inputs and outputs on the device, the filter words, the
        argument list from its named pieces, and the exported function that serves this combination -- base itself, or base +
        "_filtered" / "_scoped" / "_grouped".  kept (idx, score, count) and ppr (link_top_k .. ppr_tol, in the ABI's order)
        are None / () for the dense call, which has no flags either; report: allocate residual / iters_used.
        mmr: None or mmr_plan's (lambda, c): c entries are ranked and _mmr_picks keeps k of them.
        boost: None, or the rows the call left are boosted and ranked again (_last_boosted) before MMR and the hits.
        late: None or late_plan's (LateQueries, c): c entries are ranked, _late_picks rescores them and keeps the k best
        (all c of them in late order when MMR follows)."""
        torch = _torch()
        k_out, k = k, (k if mmr is None else mmr[1])
        self._check_mmr_fits(mmr)
        self._check_late_fits(late, mmr, group_agg, group_hits)
        if late is not None:
            k = late[1]
        scoped = check_filter_scope(filter_scope, doc_filter)
        agg = check_group_agg(group_agg)
        hits = check_group_hits(group_hits, group_agg)
        if base == "hrag_retrieve_scored":      # raw passage scores fp32 [B, >= Np], any row stride
            src = source.to(self.device, torch.float32)
            if src.stride(-1) != 1:
                src = src.contiguous()
            head = (self._handle, src.data_ptr(), src.stride(0), src.shape[0])
        else:
            src = self._q(source)
            head = (self._handle, src.data_ptr(), src.shape[0])
        b = src.shape[0]
        if late is not None:
            check_late(late[0], k_out, late[1], b)
        prog = None if boost is None else self._boost_program(boost, b)      # (refused before anything is enqueued)
        out = RetrieveOutput(self._empty((b, k), torch.int32), self._empty((b, k), torch.float32), None)
        tail = (_stream(),)
        if kept is not None:
            kept_idx = kept[0].to(self.device, torch.int32).contiguous()
            kept_score = kept[1].to(self.device, torch.float32).contiguous()
            kept_count = kept[2].to(self.device, torch.int32).contiguous()
            kf = kept_idx.shape[1]
            if base == "hrag_retrieve" and (kept_idx.shape != (b, kf) or kept_score.shape != (b, kf) or kept_count.shape != (b,)):
                raise ValueError("kept_idx / kept_score must be [B, kf], kept_count [B]")
            head += (kept_idx.data_ptr(), kept_score.data_ptr(), kept_count.data_ptr(), kf) + tuple(ppr)
            out.flags = self._empty((b,), torch.int32)
            if report:
                out.residual, out.iters_used = self._empty((b,), torch.float32), self._empty((b,), torch.int32)
            tail = (out.flags.data_ptr(), out.residual.data_ptr() if report else None,
                    out.iters_used.data_ptr() if report else None, _stream())
        fw, fld = (None, 0) if doc_filter is None else self._filter_words(doc_filter, b)
        docs = (out.doc_idx.data_ptr(), out.doc_score.data_ptr())
        if agg is not None:     # the ungrouped ranking is left out; its two tensors carry the group scores / representatives
            out.group_idx = self._empty((b, k), torch.int32)
            check(getattr(self._lib, base + "_grouped")(
                *head, k, None, None, *tail, fw.data_ptr() if fw is not None else None, fld, 1 if scoped else 0, agg,
                out.group_idx.data_ptr(), docs[1], docs[0]))
        elif fw is None:
            check(getattr(self._lib, base)(*head, k, *docs, *tail))
        else:
            check(getattr(self._lib, base + ("_scoped" if scoped else "_filtered"))(*head, k, *docs, *tail, fw.data_ptr(), fld))
        if prog is not None:
            self._last_boosted(out, prog, b, k, fw, fld, agg)
        if late is not None:
            self._late_picks(out, late[0], k if mmr is not None else k_out)
        if mmr is not None:
            self._mmr_picks(out, k_out, mmr[0])
        if hits is not None:    # over the rows this call left, with its group ids and its filter
            out.hit_idx, out.hit_score = self.last_group_hits(out.group_idx, hits, fw, fld)
        return out

    # ------------------------------------------------------------------ boosted retrieval
    def _payload_ix(self, name: str) -> "PayloadIndex":
        ix = getattr(getattr(self, "_parent", None) or self, "_payload_index", None)
        if ix is None or not ix._handle.value:
            raise ValueError(f"{name} needs a payload index on this engine (set_payload_index)")
        return ix

    def _boost_program(self, boost, batch: int) -> "BoostProgram":
        """boost= of a call as a BoostProgram that fits the engine's payload index and the call's batch."""
        if self.n_rows != self.num_vertices or self.passage_rows != self.n_passages:
            raise NotImplementedError("boost on a row-shard engine: its score rows are slices of the passages (boosted "
                                      "retrieval is served by the unsharded engine only)")
        return check_program(self._payload_ix("boost"), boost, batch)

    def boost_rows(self, rows, program, mn=None, mx=None):
        """Any device score rows fp32 [B, >= n_passages] boosted IN PLACE by a BoostProgram (or compile_boosts' grammar) over
        the engine's payload index (hrag_boost_rows); mn / mx fp32 [B]: the min-max of an entry is read instead of it."""
        return _boost_rows(self._payload_ix("boost_rows"), rows, program, mn, mx)

    def _last_boosted(self, out: RetrieveOutput, prog, b: int, k: int, fw, fld: int, agg) -> None:
        """hrag_last_boosted over the rows the last call left: the ranking fields of `out` are written again."""
        torch = _torch()
        ix = self._payload_ix("boost")
        if agg is not None and out.group_idx is None:
            out.group_idx = self._empty((b, k), torch.int32)
        check(self._lib.hrag_last_boosted(
            self._handle, ix._handle, b, C.byref(prog.desc(self.device)), 1 if prog.broadcast else 0, k,
            fw.data_ptr() if fw is not None else None, fld, -1 if agg is None else agg,
            None if agg is not None else out.doc_idx.data_ptr(), None if agg is not None else out.doc_score.data_ptr(),
            out.group_idx.data_ptr() if agg is not None else None, out.doc_score.data_ptr() if agg is not None else None,
            out.doc_idx.data_ptr() if agg is not None else None, _stream()))

    def last_boosted(self, boost, batch: int, *, k: int = 200, doc_filter=None, group_agg: Optional[str] = None,
                     group_hits: Optional[int] = None, mmr_lambda: Optional[float] = None,
                     mmr_candidates: Optional[int] = None) -> RetrieveOutput:
        """The boosted ranking over the first `batch` score rows the last retrieve / retrieve_scored / grouped
        dense_retrieve / last_fused on this handle left (hrag_last_boosted): the rows are boosted in place -- calling it
        twice boosts twice -- and ranked under doc_filter, with group_agg / group_hits / mmr_* as on retrieve.  flags /
        residual / iters_used are None: they belong to the call that wrote the rows."""
        torch = _torch()
        mmr = mmr_plan(mmr_lambda, mmr_candidates, k)
        k_out, k = k, (k if mmr is None else mmr[1])
        self._check_mmr_fits(mmr)
        agg = check_group_agg(group_agg)
        hits = check_group_hits(group_hits, group_agg)
        prog = self._boost_program(boost, batch)
        fw, fld = (None, 0) if doc_filter is None else self._filter_words(doc_filter, batch)
        out = RetrieveOutput(self._empty((batch, k), torch.int32), self._empty((batch, k), torch.float32), None)
        self._last_boosted(out, prog, batch, k, fw, fld, agg)
        if mmr is not None:
            self._mmr_picks(out, k_out, mmr[0])
        if hits is not None:
            out.hit_idx, out.hit_score = self.last_group_hits(out.group_idx, hits, fw, fld)
        return out

    # ------------------------------------------------------------------ payload filters
    def set_payload_index(self, ix: Optional["PayloadIndex"]):
        """The PayloadIndex that doc_filter=PayloadFilter / scope_filter=PayloadFilter calls of this engine and of its
        workspaces evaluate against (None: none; include/hrag.h, payload filters).  Held by reference on the Python side
        only: the library's engine does not know it, and closing it is the caller's."""
        root = getattr(self, "_parent", None) or self
        if ix is not None:
            if ix.n_passages != root.n_passages:
                raise ValueError(f"the payload index covers {ix.n_passages} passages, the engine {root.n_passages}")
            if ix.device != root.device:
                raise ValueError(f"the payload index lives on {ix.device}, the engine on {root.device}")
        root._payload_index = ix

    def _filter_words(self, doc_filter, batch: int, name: str = "doc_filter", own: bool = False):
        """(int32 device words, filter_ld_words) of a doc filter: doc_filter_words for a tensor; a PayloadFilter
        (payload.compile_filters) is evaluated on the device (hrag_payload_filter) into this handle's [max_batch, W] scratch,
        allocated on first use -- own: into a tensor of its own, for a caller that reads the words after later calls."""
        if not isinstance(doc_filter, PayloadFilter):
            return doc_filter_words(doc_filter, self.n_passages, batch, self.device)
        ix = getattr(getattr(self, "_parent", None) or self, "_payload_index", None)
        if ix is None or not ix._handle.value:
            raise ValueError(f"{name}: a PayloadFilter needs a payload index on this engine (set_payload_index)")
        if doc_filter.n_passages != self.n_passages:
            raise ValueError(f"{name}: the PayloadFilter was compiled for {doc_filter.n_passages} passages, the engine ranks "
                             f"{self.n_passages}")
        if not doc_filter.broadcast and doc_filter.batch != batch:
            raise ValueError(f"{name}: the PayloadFilter holds {doc_filter.batch} queries, the call {batch}")
        out = None
        if not own and doc_filter.batch <= self.max_batch:
            out = getattr(self, "_pay_words", None)
            if out is None:
                out = self._pay_words = self._empty((self.max_batch, ix.words), _torch().int32)
        words = ix.evaluate(doc_filter, out=out)
        return words, (0 if doc_filter.broadcast else words.stride(0))

    # ------------------------------------------------------------------ facets
    def facet(self, spec_or_field, doc_filter=None, *, ids=None, batch: Optional[int] = None) -> "FacetCounts":
        """The per-bin counts of one column of the engine's payload index (include/hrag.h, facets): spec_or_field a
        FacetSpec (compile_facet) or the name of a keyword column; over the passages doc_filter allows -- anything a
        doc_filter= takes, a PayloadFilter included (None: every passage) -- or over the ids int32 [B, k] a retrieve call
        returned.  batch: the rows of a per-query doc_filter (None: what the filter itself holds); one filter for the batch
        gives one row.  A workspace handle counts over its parent's index."""
        ix = self._payload_ix("facet")
        spec = spec_or_field if isinstance(spec_or_field, FacetSpec) else compile_facet(ix, spec_or_field)
        if ids is not None:
            if doc_filter is not None:
                raise ValueError("facet: doc_filter or ids, not both")
            return ix.facet(spec, ids=ids)
        if doc_filter is None:
            return ix.facet(spec)
        if batch is None:
            batch = (doc_filter.batch if isinstance(doc_filter, PayloadFilter)
                     else doc_filter.shape[0] if getattr(doc_filter, "ndim", 1) == 2 else 1)
        words, _ = self._filter_words(doc_filter, batch, own=True)
        return ix.facet(spec, words)

    # ------------------------------------------------------------------ lexical retrieval
    def set_lexical_index(self, ix: Optional["LexicalIndex"]):
        """The LexicalIndex the lexical= calls of this engine and of its workspaces score against (None: none).  Held by
        reference on the Python side only: the library's engine does not know it, and closing it is the caller's."""
        root = getattr(self, "_parent", None) or self
        if ix is not None:
            if root.n_rows != root.num_vertices or root.passage_rows != root.n_passages:
                raise NotImplementedError("set_lexical_index on a row-shard engine: lexical retrieval is served by the "
                                          "unsharded engine only")
            if ix.n_passages != root.n_passages:
                raise ValueError(f"the lexical index covers {ix.n_passages} passages, the engine {root.n_passages}")
            if ix.device != root.device:
                raise ValueError(f"the lexical index lives on {ix.device}, the engine on {root.device}")
        root._lexical_index = ix

    def _lex_index(self) -> "LexicalIndex":
        ix = getattr(getattr(self, "_parent", None) or self, "_lexical_index", None)
        if ix is None or not ix._handle.value:
            raise ValueError("lexical: no lexical index on this engine (set_lexical_index)")
        return ix

    def _lex_rows(self, qp, qt, qw):
        """(rows fp32 [B, n_passages], mn [B], mx [B]) of checked host CSR queries (hrag_lex_scores)."""
        torch = _torch()
        ix = self._lex_index()
        b, nnz = qp.shape[0] - 1, qt.shape[0]
        d_p = torch.from_numpy(qp).to(self.device)
        d_t = torch.from_numpy(qt).to(self.device)
        d_w = torch.from_numpy(qw).to(self.device)
        rows = self._empty((b, ix.n_passages), torch.float32)
        mn, mx = self._empty((b,), torch.float32), self._empty((b,), torch.float32)
        check(self._lib.hrag_lex_scores(ix._handle, d_p.data_ptr(), d_t.data_ptr() if nnz else None,
                                        d_w.data_ptr() if nnz else None, nnz, b, rows.data_ptr(), rows.stride(0),
                                        mn.data_ptr(), mx.data_ptr(), _stream()))
        return rows, mn, mx

    def lexical_scores(self, q_ptr, q_term, q_weight, want_minmax: bool = False):
        """The lexical score rows fp32 [B, n_passages] of sparse queries (check_lexical's triple) against the engine's
        lexical index; want_minmax: (rows, mn [B], mx [B]), the row min / max as hrag_row_minmax gives them."""
        qp, qt, qw, _ = check_lexical((q_ptr, q_term, q_weight), 0.0, None)
        rows, mn, mx = self._lex_rows(qp, qt, qw)
        return (rows, mn, mx) if want_minmax else rows

    def _lexical_blend(self, dense_rows, q_pass, lexical, lexical_weight, filter_scope: str = "ranking", doc_filter=None):
        """The blended passage score rows fp32 [B, n_passages] of a lexical= call: dense_rows (the caller's, left as they
        are) or, when None, hrag_sim_scores of q_pass (blended in place)."""
        torch = _torch()
        if check_filter_scope(filter_scope, doc_filter):
            raise NotImplementedError('filter_scope="seeds" is not served with lexical: the blend\'s two min-maxes would '
                                      'have to run over the allowed passages -- use filter_scope="ranking"')
        ix = self._lex_index()
        n = ix.n_passages
        if dense_rows is None:
            q = self._q(q_pass)
            b = q.shape[0]
        else:
            src = dense_rows.to(self.device, torch.float32)
            if src.dim() != 2 or src.shape[1] < n:
                raise ValueError(f"pass_scores must be [B, >= {n}]")
            if src.stride(-1) != 1:
                src = src.contiguous()
            b = src.shape[0]
        qp, qt, qw, alpha = check_lexical(lexical, lexical_weight, b)      # before anything is enqueued
        if dense_rows is None:
            src = out = self.sim_scores("passages", q)
        else:
            out = self._empty((b, n), torch.float32)
        lex, mn_l, mx_l = self._lex_rows(qp, qt, qw)
        mn_d, mx_d = self._empty((b,), torch.float32), self._empty((b,), torch.float32)
        check(self._lib.hrag_row_minmax(src.data_ptr(), b, n, src.stride(0), mn_d.data_ptr(), mx_d.data_ptr(), _stream()))
        check(self._lib.hrag_lex_blend_rows(src.data_ptr(), src.stride(0), lex.data_ptr(), lex.stride(0), b, n,
                                            mn_d.data_ptr(), mx_d.data_ptr(), mn_l.data_ptr(), mx_l.data_ptr(), alpha,
                                            out.data_ptr(), out.stride(0), _stream()))
        return out

    def _rank_rows(self, rows, k: int, normalize: bool, doc_filter=None):
        """(idx int32, score fp32) [B, k]: the library ranking of score rows over the engine's passages
        (hrag_topk_rows_ws, or hrag_topk_rows_masked under a doc filter); normalize: min-max normalised scores."""
        torch = _torch()
        b, n = rows.shape[0], self.n_passages
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError(f"k={k!r}: an int >= 1 expected")
        idx, val = self._empty((b, k), torch.int32), self._empty((b, k), torch.float32)
        need = int(self._lib.hrag_topk_rows_workspace_bytes(b, n, k))
        ws = _topk_workspace(self.device, _stream(), need).data_ptr() if need > 0 else None
        if doc_filter is None:
            check(self._lib.hrag_topk_rows_ws(rows.data_ptr(), b, n, rows.stride(0), k, 0, 1 if normalize else 0,
                                              idx.data_ptr(), val.data_ptr(), None, None, ws, max(need, 0), _stream()))
        else:
            fw, fld = self._filter_words(doc_filter, b)
            check(self._lib.hrag_topk_rows_masked(rows.data_ptr(), b, n, rows.stride(0), k, 0, 1 if normalize else 0,
                                                  fw.data_ptr(), fld, 0, idx.data_ptr(), val.data_ptr(), None, None, ws,
                                                  max(need, 0), _stream()))
        return idx, val

    def lexical_retrieve(self, lexical, k: int = 200, doc_filter=None):
        """The pure lexical ranking: (idx int32, score fp32) [B, k] of the lexical score rows as they are (no
        normalisation, no dense side), under doc_filter; -1 / 0 beyond the passages there are (or are allowed)."""
        qp, qt, qw, _ = check_lexical(lexical, 0.0, None)
        rows, _, _ = self._lex_rows(qp, qt, qw)
        return self._rank_rows(rows, k, False, doc_filter)

    # ------------------------------------------------------------------ recommend by example
    def _reco_args(self, examples, name: str = "examples"):
        """The checked examples of a call as the library takes them: (host ex_ptr, ex_ptr_dev, ex_idx, ex_sign, batch)."""
        ex = check_examples(examples, None, name)
        if ex.device != self.device:
            raise ValueError(f"{name}: the examples live on {ex.device}, the engine on {self.device}")
        if self.n_rows != self.num_vertices or self.passage_rows != self.n_passages:
            raise NotImplementedError("recommend on a row-shard engine: it holds a slice of the passage embeddings (recommend "
                                      "is served by the unsharded engine only)")
        if ex.batch > self.max_batch:
            raise ValueError(f"{name}: {ex.batch} queries, the engine serves at most max_batch={self.max_batch}")
        return (ex.ex_ptr.ctypes.data, ex.ex_ptr_dev.data_ptr(), ex.ex_idx.data_ptr(), ex.ex_sign.data_ptr(), ex.batch)

    def recommend_scores(self, examples, strategy: str = "best_score"):
        """The recommend score rows fp32 [B, n_passages] (hrag_reco_scores) of an Examples batch over the engine's passage
        embeddings: strategy "best_score" or "sum_scores" (include/hrag.h, recommend by example)."""
        torch = _torch()
        mode = check_strategy(strategy, True)
        args = self._reco_args(examples)
        b = args[-1]
        out = self._empty((b, self.n_passages), torch.float32)
        need = int(self._lib.hrag_reco_workspace_bytes(b))
        ws = getattr(self, "_reco_ws", None)
        if ws is None or ws.numel() < need or ws.device != self.device:
            ws = self._reco_ws = torch.empty((need,), dtype=torch.uint8, device=self.device)
        check(self._lib.hrag_reco_scores(self._handle, *args, mode, out.data_ptr(), out.stride(0), ws.data_ptr(), ws.numel(),
                                         _stream()))
        return out

    def recommend_query(self, examples, return_bits: bool = False):
        """The average_vector query of an Examples batch (hrag_reco_query): (q, flags) -- q [B, dim] in the dtype this
        engine's calls take their queries in (bf16 / fp16; fp32 on a split engine, which splits it again exactly), not
        normalised; flags int32 [B], bit 0: the query has no positive example (q is all zero).  return_bits: (q16, v, flags)
        with q16 int16 [B, kdim] the 16-bit query as the similarity kernels read it and v fp32 [B, dim] before that
        rounding."""
        torch = _torch()
        args = self._reco_args(examples)
        b = args[-1]
        q16 = self._empty((b, self.dim * (3 if self.f32_split else 1)), torch.int16)
        v = self._empty((b, self.dim), torch.float32)
        flags = self._empty((b,), torch.int32)
        check(self._lib.hrag_reco_query(self._handle, *args, q16.data_ptr(), v.data_ptr(), flags.data_ptr(), _stream()))
        if return_bits:
            return q16, v, flags
        return (v if self.f32_split else q16.view(self.emb_dtype)), flags

    def recommend_filter(self, examples, doc_filter=None):
        """The doc filter of a recommend call with exclusion: int32 words [B, W] -- doc_filter (anything a doc_filter=
        takes; None: every passage) as one row per query, in a tensor of its own, with the bits of every query's non-empty
        examples cleared (hrag_reco_exclude).  The caller's filter is left as it is."""
        torch = _torch()
        args = self._reco_args(examples)
        b, n = args[-1], self.n_passages
        words = (n + 31) // 32
        if doc_filter is None:
            w = torch.full((b, words), -1, dtype=torch.int32, device=self.device)
            if n % 32:
                w[:, -1] = (1 << (n % 32)) - 1
        else:
            fw, fld = self._filter_words(doc_filter, b, own=True)
            w = (fw.unsqueeze(0).expand(b, -1) if fld == 0 else fw).clone().contiguous()
        check(self._lib.hrag_reco_exclude(w.data_ptr(), w.stride(0), n, args[1], args[2], args[3], b, _stream()))
        return w

    def recommend(self, examples, k: int = 200, strategy: str = "best_score", doc_filter=None, exclude_examples: bool = True,
                  mmr_lambda: Optional[float] = None, mmr_candidates: Optional[int] = None, late=None,
                  late_candidates: Optional[int] = None, group_agg: Optional[str] = None, group_hits: Optional[int] = None,
                  boost=None, lexical=None):
        """Recommend by example: (idx int32, score fp32) [B, k], the k best passages for each query's liked and disliked
        passage ids -- plus mmr_value / first_score entries as on dense_retrieve.  strategy "best_score" | "sum_scores":
        the raw recommend rows (recommend_scores) ranked under doc_filter (hrag_topk_rows_ws / hrag_topk_rows_masked), then
        the mmr and late_rerank seams as retrieve chains them.  "average_vector" IS dense_retrieve(recommend_query(...)),
        so every option of that call is served.  exclude_examples: the examples themselves are never returned
        (recommend_filter)."""
        check_strategy(strategy)
        self._reco_args(examples)
        rows_strategy = strategy != "average_vector"
        mmr = lp = None
        if rows_strategy:        # (everything is refused before anything is enqueued)
            for name, v in (("group_agg", group_agg), ("group_hits", group_hits), ("boost", boost), ("lexical", lexical)):
                if v is not None:
                    raise ValueError(f"recommend(strategy={strategy!r}) does not serve {name}: it ranks the recommend rows and "
                                     "keeps no score rows on the handle -- hand recommend_scores to retrieve_scored, or use "
                                     'strategy="average_vector"')
            mmr = mmr_plan(mmr_lambda, mmr_candidates, k)
            lp = late_plan(late, late_candidates, k)
            self._check_mmr_fits(mmr)
            self._check_late_fits(lp, mmr)
            if lp is not None:
                check_late(lp[0], k, lp[1], examples.batch)
        filt = self.recommend_filter(examples, doc_filter) if exclude_examples else doc_filter
        if not rows_strategy:
            q, _ = self.recommend_query(examples)
            return self.dense_retrieve(q, k=k, doc_filter=filt, mmr_lambda=mmr_lambda, mmr_candidates=mmr_candidates, late=late,
                                       late_candidates=late_candidates, group_agg=group_agg, group_hits=group_hits, boost=boost,
                                       lexical=lexical)
        c = k if mmr is None else mmr[1]
        if lp is not None:
            c = lp[1]
        rows = self.recommend_scores(examples, strategy)
        idx, sc = self._rank_rows(rows, c, False, filt)
        out = RetrieveOutput(idx, sc, None)
        if lp is not None:
            self._late_picks(out, lp[0], c if mmr is not None else k)
        if mmr is not None:
            self._mmr_picks(out, k, mmr[0])
        extra = () if out.mmr_value is None else (out.mmr_value,)
        extra += () if out.first_score is None else (out.first_score,)
        return (out.doc_idx, out.doc_score) + extra

    def _feedback_blend(self, q_pass, feedback, feedback_weight, feedback_strategy, filter_scope: str = "ranking",
                        doc_filter=None):
        """The blended passage score rows fp32 [B, n_passages] of a feedback= call: hrag_sim_scores of q_pass blended in
        place with the recommend rows, each min-max normalised (hrag_row_minmax, hrag_lex_blend_rows)."""
        torch = _torch()
        if check_filter_scope(filter_scope, doc_filter):
            raise NotImplementedError('filter_scope="seeds" is not served with feedback: the blend\'s two min-maxes would '
                                      'have to run over the allowed passages -- use filter_scope="ranking"')
        q = self._q(q_pass)
        b, n = q.shape[0], self.n_passages
        check_examples(feedback, b, "feedback")
        alpha = check_feedback_weight(feedback_weight)
        rec = self.recommend_scores(feedback, feedback_strategy)
        src = self.sim_scores("passages", q)
        mm = [self._empty((b,), torch.float32) for _ in range(4)]
        check(self._lib.hrag_row_minmax(src.data_ptr(), b, n, src.stride(0), mm[0].data_ptr(), mm[1].data_ptr(), _stream()))
        check(self._lib.hrag_row_minmax(rec.data_ptr(), b, n, rec.stride(0), mm[2].data_ptr(), mm[3].data_ptr(), _stream()))
        check(self._lib.hrag_lex_blend_rows(src.data_ptr(), src.stride(0), rec.data_ptr(), rec.stride(0), b, n,
                                            mm[0].data_ptr(), mm[1].data_ptr(), mm[2].data_ptr(), mm[3].data_ptr(), alpha,
                                            src.data_ptr(), src.stride(0), _stream()))
        return src

    # ------------------------------------------------------------------ late-interaction reranking
    def set_token_index(self, ix: Optional["TokenIndex"]):
        """The TokenIndex the late= calls of this engine and of its workspaces rescore against (None: none; include/hrag.h,
        late-interaction reranking).  Held by reference on the Python side only: the library's engine does not know it, and
        closing it is the caller's."""
        root = getattr(self, "_parent", None) or self
        if ix is not None:
            if root.n_rows != root.num_vertices or root.passage_rows != root.n_passages:
                raise NotImplementedError("set_token_index on a row-shard engine: late reranking is served by the unsharded "
                                          "engine only")
            if ix.n_passages != root.n_passages:
                raise ValueError(f"the token index covers {ix.n_passages} passages, the engine {root.n_passages}")
            if ix.device != root.device:
                raise ValueError(f"the token index lives on {ix.device}, the engine on {root.device}")
        root._token_index = ix

    def _token_ix(self, late: "LateQueries") -> "TokenIndex":
        ix = getattr(getattr(self, "_parent", None) or self, "_token_index", None)
        if ix is None or not ix._handle.value:
            raise ValueError("late: no token index on this engine (set_token_index)")
        if late.dim != ix.dim or late.dtype != ix.dtype:
            raise ValueError(f"late: the queries are {late.dtype} of dim {late.dim}, the token index {ix.dtype} of dim {ix.dim}")
        if late.device != self.device:
            raise ValueError(f"late: the queries live on {late.device}, the engine on {self.device}")
        return ix

    def _late_cand(self, cand_idx, late, k: int):
        torch = _torch()
        ci = cand_idx.to(self.device, torch.int32).contiguous()
        if ci.dim() != 2:
            raise ValueError("cand_idx must be [B, c]")
        check_late(late, k, ci.shape[1], ci.shape[0])
        return ci, self._token_ix(late)

    def late_scores(self, cand_idx, late: "LateQueries"):
        """The late scores fp32 [B, c] (hrag_late_scores) of candidates int32 [B, c] (passage positions; -1 or an id outside
        [0, n_passages): an empty slot, 0.0) under the late queries of the batch, over the engine's token index."""
        torch = _torch()
        ci, ix = self._late_cand(cand_idx, late, 1)
        b, c = ci.shape
        out = self._empty((b, c), torch.float32)
        check(self._lib.hrag_late_scores(ix._handle, late.q_ptr.ctypes.data, late.q_ptr_dev.data_ptr(),
                                         late.q_tok.data_ptr() if late.n_tokens else None, b, ci.data_ptr(), c,
                                         out.data_ptr(), out.stride(0), _stream()))
        return out

    def late_rerank(self, cand_idx, late: "LateQueries", k: int, return_sel: bool = False):
        """Late reranking (hrag_late_rerank) of candidates int32 [B, c] in the order a ranking returned them: (idx int32,
        score fp32) [B, k], the k best by late score -- a tie to the smaller slot -- and -1 / 0 once the non-empty slots
        run out.  return_sel: a third entry, the slot of each pick in its candidate row (-1 beyond).  Everything stays on
        the device."""
        torch = _torch()
        ci, ix = self._late_cand(cand_idx, late, k)
        b, c = ci.shape
        idx, sc = self._empty((b, k), torch.int32), self._empty((b, k), torch.float32)
        sel = self._empty((b, k), torch.int32)
        need = int(self._lib.hrag_late_workspace_bytes(b, c))
        ws = getattr(self, "_late_ws", None)
        if ws is None or ws.numel() < need or ws.device != self.device:
            ws = self._late_ws = torch.empty((need,), dtype=torch.uint8, device=self.device)
        check(self._lib.hrag_late_rerank(ix._handle, late.q_ptr.ctypes.data, late.q_ptr_dev.data_ptr(),
                                         late.q_tok.data_ptr() if late.n_tokens else None, b, ci.data_ptr(), c, k,
                                         sel.data_ptr(), idx.data_ptr(), sc.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        return (idx, sc, sel) if return_sel else (idx, sc)

    def _check_late_fits(self, late, mmr=None, group_agg=None, group_hits=None) -> None:
        """What a late= call refuses before any work: grouping, mmr_candidates, c entries beyond max_topk."""
        if late is None:
            return
        for name, v in (("group_agg", group_agg), ("group_hits", group_hits)):
            if v is not None:
                raise ValueError(f"late does not serve {name}: a group's score is not a passage's -- rescore the passages "
                                 "(retrieve(late=...)) and group the result, or use late_rerank on the representatives")
        if mmr is not None and mmr[1] > late[1]:
            raise ValueError(f"late with mmr_candidates={mmr[1]}: MMR picks among the c = {late[1]} late candidates -- pass "
                             "late_candidates, not mmr_candidates")
        if late[1] > self.max_topk:
            raise ValueError(f"late_candidates: the call would rank c = max(late_candidates, k) = {late[1]} entries, the "
                             f"engine ranks at most max_topk={self.max_topk}")

    def _late_picks(self, out: RetrieveOutput, late: "LateQueries", k: int) -> None:
        """Replace the ranked c entries of `out` by their k best by late score: doc_idx, doc_score (the late scores) and
        first_score (each entry's first-stage score, by the slot of the pick)."""
        torch = _torch()
        idx, sc, sel = self.late_rerank(out.doc_idx, late, k, return_sel=True)
        first = torch.gather(out.doc_score, 1, sel.clamp_min(0).long())
        out.first_score = torch.where(sel >= 0, first, torch.zeros_like(first))
        out.doc_idx, out.doc_score = idx, sc

    def mmr(self, cand_idx, cand_score, k: int, lam: float = 0.5, normalize: bool = True, return_sel: bool = False):
        """MMR re-ranking (hrag_mmr; include/hrag.h, diversified retrieval) of candidates int32 [B, c] (passage positions in
        the order a ranking returned them; -1 or an id outside [0, n_passages): an empty slot) with their scores fp32
        [B, c] over this engine's passage embeddings: (idx int32, score fp32, value fp32), each [B, k] -- the picks in MMR
        order, their own scores, the MMR value of each pick; -1 / 0 / 0 once the candidates run out.  normalize: relevance is
        the min-max of the candidates' scores (else the scores as they are).  Everything stays on the device; a batch whose
        Gram workspace would exceed MMR_WORKSPACE_CAP (or max_batch) is processed in slices.  return_sel: a fourth entry, the
        slot of each pick in its candidate row int32 [B, k] (hrag_mmr_sel; -1 once the candidates run out)."""
        torch = _torch()
        ci = cand_idx.to(self.device, torch.int32).contiguous()
        cs = cand_score.to(self.device, torch.float32).contiguous()
        if ci.dim() != 2 or cs.shape != ci.shape:
            raise ValueError("cand_idx / cand_score must both be [B, c]")
        b, c = ci.shape
        lam = check_mmr(lam, k, c)
        idx = self._empty((b, k), torch.int32)
        sc = self._empty((b, k), torch.float32)
        val = self._empty((b, k), torch.float32)
        sel = self._empty((b, k), torch.int32) if return_sel else None
        if b == 0:
            return (idx, sc, val, sel) if return_sel else (idx, sc, val)
        per = int(self._lib.hrag_mmr_workspace_bytes(1, c))
        step = max(1, min(b, self.max_batch, MMR_WORKSPACE_CAP // per))
        need = per * step
        ws = getattr(self, "_mmr_ws", None)
        if ws is None or ws.numel() < need or ws.device != self.device:
            ws = self._mmr_ws = torch.empty((need,), dtype=torch.uint8, device=self.device)
        for lo in range(0, b, step):
            n = min(step, b - lo)
            check(self._lib.hrag_mmr_sel(self._handle, ci[lo:].data_ptr(), cs[lo:].data_ptr(), n, c, k, lam,
                                         1 if normalize else 0, sel[lo:].data_ptr() if return_sel else None,
                                         idx[lo:].data_ptr(), sc[lo:].data_ptr(), val[lo:].data_ptr(), ws.data_ptr(),
                                         ws.numel(), _stream()))
        return (idx, sc, val, sel) if return_sel else (idx, sc, val)

    def _check_mmr_fits(self, mmr) -> None:
        """The c entries an MMR call ranks must fit the engine: c <= max_topk (mmr_plan holds c to MMR_MAX_CANDIDATES)."""
        if mmr is not None and mmr[1] > self.max_topk:
            raise ValueError(f"mmr_candidates: the call would rank c = max(mmr_candidates, k) = {mmr[1]} entries, the engine "
                             f"ranks at most max_topk={self.max_topk}")

    def _mmr_picks(self, out: RetrieveOutput, k: int, lam: float) -> None:
        """Replace the ranked c entries of `out` by their k MMR picks (doc_idx / doc_score / mmr_value); a grouped call's
        group_idx follows them by the slot of each pick."""
        torch = _torch()
        idx, sc, val, sel = self.mmr(out.doc_idx, out.doc_score, k, lam, return_sel=True)
        if out.group_idx is not None:
            gi = torch.gather(out.group_idx, 1, sel.clamp_min(0).long())
            out.group_idx = torch.where(sel >= 0, gi, torch.full_like(gi, -1))
        if out.first_score is not None:      # (after _late_picks: the first-stage scores follow the picks)
            fs = torch.gather(out.first_score, 1, sel.clamp_min(0).long())
            out.first_score = torch.where(sel >= 0, fs, torch.zeros_like(fs))
        out.doc_idx, out.doc_score, out.mmr_value = idx, sc, val

    def last_group_hits(self, group_idx, hits: int, filter_words=None, filter_ld: int = 0):
        """(hit_idx int32, hit_score fp32) [B, k, hits] for group ids int32 [B, k] over the score rows the last retrieve /
        retrieve_scored / grouped dense_retrieve on this handle left (hrag_last_group_hits).  filter_words / filter_ld: what
        doc_filter_words made of that call's doc filter (None: every passage)."""
        torch = _torch()
        gi = group_idx.to(self.device, torch.int32).contiguous()
        b, k = gi.shape
        hi = self._empty((b, k, hits), torch.int32)
        hs = self._empty((b, k, hits), torch.float32)
        check(self._lib.hrag_last_group_hits(self._handle, b, gi.data_ptr(), k, hits,
                                             filter_words.data_ptr() if filter_words is not None else None, filter_ld,
                                             hi.data_ptr(), hs.data_ptr(), _stream()))
        return hi, hs

    def last_fused(self, member_ptr, *, weights=None, fuse: str = "rrf", rrf_c: int = 60, rrf_depth: Optional[int] = None,
                   k: int = 200, doc_filter=None, group_agg: Optional[str] = None,
                   group_hits: Optional[int] = None, mmr_lambda: Optional[float] = None,
                   mmr_candidates: Optional[int] = None, boost=None, late=None,
                   late_candidates: Optional[int] = None) -> RetrieveOutput:
        """One ranking per QUESTION from the score rows the last retrieve / retrieve_scored / grouped dense_retrieve on this
        handle left (hrag_last_fused; include/hrag.h, fused retrieval): member_ptr int [Q + 1] cuts those B = member_ptr[-1]
        rows into Q questions of consecutive member rows, weights [B] (None: all 1) weigh them, fuse = "sum" (fp64, in member
        order), "max" or "rrf" (rrf_c, rrf_depth: default min(k, max_topk, n_passages)).  Returns doc_idx / doc_score [Q, k]
        of the fused rows under doc_filter ([n] for every question or [Q, n]; for "rrf" also the filter of the member
        rankings); with group_agg the grouped ranking instead (group_idx, group_score = doc_score, best_doc_idx = doc_idx)
        and with group_hits=m its hits.  flags / residual / iters_used are None: they belong to the member rows.
        Afterwards last_doc_scores(Q) returns the fused rows.  mmr_lambda / mmr_candidates: as on retrieve, over the fused
        ranking.  boost= (one list for the questions, or one per question): the fused rows are boosted (hrag_last_boosted)
        and the ranking, the groups, the hits and MMR are those of the boosted fused rows; the fusion itself then ranks
        nothing.  (After a retrieve(boost=) the member rows are boosted already: last_fused fuses boosted rows.)
        late= / late_candidates= (one LateQueries entry per QUESTION): as on retrieve, over the fused ranking."""
        torch = _torch()
        mmr = mmr_plan(mmr_lambda, mmr_candidates, k)
        lp = late_plan(late, late_candidates, k)
        k_out, k = k, (k if mmr is None else mmr[1])
        self._check_mmr_fits(mmr)
        self._check_late_fits(lp, mmr, group_agg, group_hits)
        if lp is not None:
            k = lp[1]
        agg = check_group_agg(group_agg)
        hits = check_group_hits(group_hits, group_agg)
        b = int(np.asarray(member_ptr).reshape(-1)[-1]) if np.size(member_ptr) else 0
        dmax = min(self.max_topk, self.n_passages)
        mode, mp, w, c, depth = check_fuse(fuse, member_ptr, b, weights, rrf_c,
                                           min(k, dmax) if rrf_depth is None else rrf_depth, dmax)
        nq = mp.shape[0] - 1
        if lp is not None:
            check_late(lp[0], k_out, lp[1], nq)
        prog = None if boost is None else self._boost_program(boost, nq)
        fw, fld = (None, 0) if doc_filter is None else self._filter_words(doc_filter, nq)
        need = int(self._lib.hrag_fuse_workspace_bytes(b, self.n_passages, mode, depth, 1 if fld else 0))
        if need < 0:
            raise ValueError(f"hrag_fuse_workspace_bytes rejects batch={b}, mode={fuse!r}, depth={depth}")
        ws = getattr(self, "_fuse_ws", None)
        if ws is None or ws.numel() < need:
            ws = self._fuse_ws = torch.empty((need,), dtype=torch.uint8, device=self.device)
        idx = self._empty((nq, k), torch.int32)
        sc = self._empty((nq, k), torch.float32)
        gi = self._empty((nq, k), torch.int32) if agg is not None else None
        self._fuse_host = (getattr(self, "_fuse_host", None) or [])[-1:] + [(mp, w)]   # alive until the stream copied them
        check(self._lib.hrag_last_fused(
            self._handle, b, mp.ctypes.data, nq, w.ctypes.data if w is not None else None, mode, c, depth, k,
            fw.data_ptr() if fw is not None else None, fld, -1 if agg is None or prog is not None else agg,
            None if agg is not None or prog is not None else idx.data_ptr(),
            None if agg is not None or prog is not None else sc.data_ptr(),
            gi.data_ptr() if agg is not None and prog is None else None,
            sc.data_ptr() if agg is not None and prog is None else None,
            idx.data_ptr() if agg is not None and prog is None else None, ws.data_ptr(), ws.numel(), _stream()))
        out = RetrieveOutput(idx, sc, None)
        out.group_idx = gi
        if prog is not None:        # (the fusion above ranked nothing: the boosted fused rows are ranked here)
            self._last_boosted(out, prog, nq, k, fw, fld, agg)
        if lp is not None:
            self._late_picks(out, lp[0], k if mmr is not None else k_out)
        if mmr is not None:
            self._mmr_picks(out, k_out, mmr[0])
        if hits is not None:
            out.hit_idx, out.hit_score = self.last_group_hits(out.group_idx, hits, fw, fld)
        return out

    def retrieve_scored(self, pass_scores, kept_idx, kept_score, kept_count, *, link_top_k: int = 5,
                        damping: float = 0.5, passage_node_weight: float = 0.05, ppr_iters: int = 20, k: int = 200,
                        ppr_tol: float = 0.0, ppr_max_iters: int = 0, doc_filter=None,
                        filter_scope: str = "ranking", group_agg: Optional[str] = None,
                        group_hits: Optional[int] = None, mmr_lambda: Optional[float] = None,
                        mmr_candidates: Optional[int] = None, lexical=None, lexical_weight: float = 0.5,
                        boost=None, late=None, late_candidates: Optional[int] = None) -> RetrieveOutput:
        """retrieve() with the raw passage scores fp32 [B, >= Np] supplied by the caller (hrag_retrieve_scored).
        lexical / lexical_weight: as on retrieve(), blended into the caller's rows (which are left as they are).
        boost, late / late_candidates: as on retrieve()."""
        mmr = mmr_plan(mmr_lambda, mmr_candidates, k)
        lp = late_plan(late, late_candidates, k)
        if lexical is not None:
            self._check_mmr_fits(mmr)                         # (refused before the blend is enqueued)
            self._check_late_fits(lp, mmr, group_agg, group_hits)
            pass_scores = self._lexical_blend(pass_scores, None, lexical, lexical_weight, filter_scope, doc_filter)
        return self._retrieve("hrag_retrieve_scored", pass_scores, (kept_idx, kept_score, kept_count),
                              (link_top_k, damping, passage_node_weight, ppr_iters, max(ppr_max_iters, ppr_iters), ppr_tol), k,
                              True, doc_filter=doc_filter, filter_scope=filter_scope, group_agg=group_agg,
                              group_hits=group_hits, mmr=mmr, boost=boost, late=lp)

    def retrieve_converged(self, q_pass, kept_idx, kept_score, kept_count, *, damping: float = 0.5,
                           ppr_iters: int = 20, ppr_tol: float = 1.5e-6, ppr_max_iters: int = 400,
                           want_all_scores: bool = False, **kw) -> RetrieveOutput:
        """retrieve() + what the host owes the convergence contract (include/hrag.h): a batch whose fp8 state
        saturated is repeated on the wider state (never clipped scores); queries the engine flags
        HRAG_FLAG_NOT_CONVERGED -- its sweep budget did not reach ppr_tol: a slowly mixing graph -- are repeated,
        those queries only, on the wider state with the sweeps their residual asks for (it contracts by `damping`
        per sweep), up to ppr_max_iters.  The reference's PRPACK does the same thing implicitly: it iterates to
        1e-10 whatever the graph (HippoRAG.py:1736-1743).  A flag that survives means ppr_max_iters was too small.

        = retrieve_converged_start(...).finish(); callers that have host work to do while the batch runs (the mirror's
        batch pipeline, retriever.iter_batched_retrieve) use the two halves."""
        return self.retrieve_converged_start(q_pass, kept_idx, kept_score, kept_count, damping=damping, ppr_iters=ppr_iters,
                                             ppr_tol=ppr_tol, ppr_max_iters=ppr_max_iters,
                                             want_all_scores=want_all_scores, **kw).finish()

    def retrieve_converged_start(self, q_pass, kept_idx, kept_score, kept_count, *, damping: float = 0.5,
                                 ppr_iters: int = 20, ppr_tol: float = 1.5e-6, ppr_max_iters: int = 400,
                                 want_all_scores: bool = False, **kw) -> "PendingRetrieve":
        """Enqueue the batch and the copy of its flag words to (pinned) host memory; nothing waits.  .finish() waits for
        the flags -- not for whatever was enqueued behind them -- and does the host half of the contract."""
        mmr = mmr_plan(kw.get("mmr_lambda"), kw.get("mmr_candidates"), kw.get("k", 200))
        self._check_mmr_fits(mmr)   # before any work
        q = self._q(q_pass)
        # late: every run rescores its own rows by its own late queries (LateQueries.select)
        late = kw.pop("late", None)
        lp = late_plan(late, kw.get("late_candidates"), kw.get("k", 200))
        self._check_late_fits(lp, mmr, kw.get("group_agg"), kw.get("group_hits"))
        if lp is not None:
            check_late(late, kw.get("k", 200), lp[1], q.shape[0])
        kept_idx, kept_score, kept_count = (t.to(self.device) for t in (kept_idx, kept_score, kept_count))
        doc_filter = kw.pop("doc_filter", None)
        check_filter_scope(kw.get("filter_scope", "ranking"), doc_filter)   # (filter_scope travels in kw to every run)
        lexical, lexical_weight = kw.pop("lexical", None), kw.pop("lexical_weight", 0.5)
        # feedback: like lexical, the blended rows are formed ONCE (a weight of 0 is the plain call)
        feedback, feedback_weight = kw.pop("feedback", None), kw.pop("feedback_weight", 0.3)
        feedback_strategy = kw.pop("feedback_strategy", "best_score")
        if feedback is not None:
            if lexical is not None:
                raise ValueError("feedback together with lexical: both own the blend of the passage scores -- blend the "
                                 "rows yourself (lexical_scores, recommend_scores) and call retrieve_scored")
            check_examples(feedback, q.shape[0], "feedback")
            check_strategy(feedback_strategy, True, "feedback_strategy")
            if check_feedback_weight(feedback_weight) == 0.0:
                feedback = None
        # boost: compiled ONCE; every run boosts its own rows by its own program rows (BoostProgram.select)
        boost = kw.pop("boost", None)
        prog = None if boost is None else self._boost_program(boost, q.shape[0])
        # lexical: the blended rows are formed ONCE; every run, the repeats of finish() included, is retrieve_scored on its
        # rows of them (a repeat never re-encodes or re-slices the sparse queries)
        blended = None if lexical is None else self._lexical_blend(None, q, lexical, lexical_weight,
                                                                   kw.get("filter_scope", "ranking"), doc_filter)
        if feedback is not None:
            blended = self._feedback_blend(q, feedback, feedback_weight, feedback_strategy, kw.get("filter_scope", "ranking"),
                                           doc_filter)
        # (a PayloadFilter is evaluated ONCE, into words of its own: the repeats of finish() read them after later calls)
        fw, fld = (None, 0) if doc_filter is None else self._filter_words(doc_filter, q.shape[0], own=True)

        def run(rows=None, iters=ppr_iters, max_iters=ppr_max_iters):
            sel = slice(None) if rows is None else rows
            if fw is not None:    # the repeats of finish() rerun rows of the batch: each keeps its own filter row
                kw["doc_filter"] = fw if fld == 0 else fw[sel]
            if prog is not None:
                kw["boost"] = prog if rows is None else prog.select(rows.cpu().numpy())
            if late is not None:
                kw["late"] = late if rows is None else late.select(rows.cpu().numpy())
            if blended is not None:
                o = self.retrieve_scored(blended[sel], kept_idx[sel], kept_score[sel], kept_count[sel], damping=damping,
                                         ppr_iters=iters, ppr_tol=ppr_tol, ppr_max_iters=max(max_iters, iters),
                                         **{n: v for n, v in kw.items() if n != "want_residual"})
            else:
                o = self.retrieve(q[sel], kept_idx[sel], kept_score[sel], kept_count[sel], damping=damping,
                                  ppr_iters=iters, ppr_tol=ppr_tol, ppr_max_iters=max(max_iters, iters), **kw)
            if want_all_scores:     # every passage's score (callers that want more than max_topk documents)
                o.all_scores = self.last_doc_scores(o.doc_idx.shape[0])
            return o

        out = run()
        return PendingRetrieve(self, run, out, host_copy_async(out.flags), damping, ppr_iters, ppr_tol, ppr_max_iters,
                               want_all_scores)

    def last_doc_scores(self, batch: int):
        """fp32 [batch, Np]: the scores of ALL passages behind the last retrieve() / retrieve_scored() (hrag_last_doc_scores)."""
        torch = _torch()
        out = self._empty((batch, self.passage_rows), torch.float32)
        check(self._lib.hrag_last_doc_scores(self._handle, batch, out.data_ptr(), self.passage_rows, _stream()))
        return out

    def dense_retrieve(self, q_pass, k: int = 200, doc_filter=None, filter_scope: str = "ranking",
                       group_agg: Optional[str] = None, group_hits: Optional[int] = None,
                       mmr_lambda: Optional[float] = None, mmr_candidates: Optional[int] = None,
                       lexical=None, lexical_weight: float = 0.5, boost=None, late=None,
                       late_candidates: Optional[int] = None):
        """DPR top-k; filter_scope="seeds": normalised over the allowed passages (hrag_dense_retrieve_scoped).
        group_agg="max" | "sum": (group ids, group scores, best passage of each group) over the normalised scores
        (hrag_dense_retrieve_grouped); group_hits=m adds two entries, (hit_idx, hit_score) [B, k, m] over those scores.
        mmr_lambda / mmr_candidates: as on retrieve; the tuple then ends with one more entry, mmr_value [B, k].
        lexical / lexical_weight (as on retrieve): (idx, score) of the blended rows, ranked by the normalising top-k
        (hrag_topk_rows_ws, hrag_topk_rows_masked under a doc_filter); not with group_agg, group_hits, mmr_* or
        filter_scope="seeds".
        boost= (as on retrieve): (idx, score) of the boosted min-max scores -- hrag_sim_scores, hrag_row_minmax,
        hrag_boost_rows with the row min / max, then the plain top-k (under a doc_filter of scope "ranking"); a program
        without any term is the plain call, and in a per-query program a query without terms keeps its raw scores (its
        ranking is the plain one).  Not with group_agg, group_hits, mmr_*, lexical or filter_scope="seeds".
        late / late_candidates: as on retrieve (the scores are then the late ones); the tuple ends with one more entry,
        first_score [B, k].  Not with boost or lexical here."""
        if boost is not None:
            for name, v in (("group_agg", group_agg), ("group_hits", group_hits), ("mmr_lambda", mmr_lambda),
                            ("mmr_candidates", mmr_candidates), ("lexical", lexical), ("late", late),
                            ("late_candidates", late_candidates)):
                if v is not None:
                    raise ValueError(f"dense_retrieve(boost=) does not serve {name}: it ranks the boosted rows and keeps no "
                                     "score rows on the handle -- use retrieve(boost=...) or boost_rows yourself")
            if filter_scope == "seeds":
                raise ValueError('dense_retrieve(boost=) does not serve filter_scope="seeds": the min-max it boosts runs '
                                 "over every passage")
            check_filter_scope(filter_scope, doc_filter)
            q = self._q(q_pass)
            prog = self._boost_program(boost, q.shape[0])
            if prog.n_terms:
                rows = self.sim_scores("passages", q)
                mn, mx = row_minmax(rows, self.n_passages)
                self.boost_rows(rows, prog, mn, mx)
                return self._rank_rows(rows, k, False, doc_filter)
        if lexical is not None:
            for name, v in (("group_agg", group_agg), ("group_hits", group_hits), ("mmr_lambda", mmr_lambda),
                            ("mmr_candidates", mmr_candidates), ("late", late), ("late_candidates", late_candidates)):
                if v is not None:
                    raise ValueError(f"dense_retrieve(lexical=) does not serve {name}: it ranks the blended rows and keeps "
                                     "no score rows on the handle -- use retrieve(lexical=...) or rank lexical_scores yourself")
            if filter_scope == "seeds":
                raise ValueError('dense_retrieve(lexical=) does not serve filter_scope="seeds": the blend\'s min-maxes run '
                                 "over every passage")
            rows = self._lexical_blend(None, q_pass, lexical, lexical_weight, filter_scope, doc_filter)
            return self._rank_rows(rows, k, True, doc_filter)
        out = self._retrieve("hrag_dense_retrieve", q_pass, None, (), k, False, doc_filter=doc_filter,
                             filter_scope=filter_scope, group_agg=group_agg, group_hits=group_hits,
                             mmr=mmr_plan(mmr_lambda, mmr_candidates, k), late=late_plan(late, late_candidates, k))
        extra = () if out.mmr_value is None else (out.mmr_value,)
        extra += () if out.first_score is None else (out.first_score,)
        if out.group_idx is None:
            return (out.doc_idx, out.doc_score) + extra
        return (out.group_idx, out.doc_score, out.doc_idx) + (() if out.hit_idx is None else (out.hit_idx, out.hit_score)) + extra

    # ------------------------------------------------------------------ seams
    def sim_scores(self, which: str, q):
        """Raw cosine scores fp32 [B, rows] against "facts" or "passages" (np.dot seam)."""
        torch = _torch()
        qq = self._q(q)
        rows = self.fact_rows if which == "facts" else self.passage_rows
        out = self._empty((qq.shape[0], rows), torch.float32)
        check(self._lib.hrag_sim_scores(self._handle, 0 if which == "facts" else 1, qq.data_ptr(),
                                        qq.shape[0], out.data_ptr(), _stream()))
        return out

    def ppr(self, reset, damping: float = 0.5, iters: int = 20):
        """run_ppr core for B reset vectors fp32 [B, V] -> (x fp32 [B, V], flags int32 [B])."""
        torch = _torch()
        r = reset.to(self.device, torch.float32).contiguous()
        if r.dim() != 2 or r.shape[1] != self.num_vertices:
            raise ValueError(f"reset must be [B, {self.num_vertices}]")
        b = r.shape[0]
        if self._perm is not None:      # the engine's vertex numbering: reset_engine[:, new] = reset[:, old]
            r = r.index_select(1, self._inv_perm).contiguous()
        x = self._empty((b, self.num_vertices), torch.float32)
        flags = self._empty((b,), torch.int32)
        check(self._lib.hrag_ppr(self._handle, r.data_ptr(), b, damping, iters, x.data_ptr(),
                                 flags.data_ptr(), _stream()))
        if self._perm is not None:
            x = x.index_select(1, self._perm).contiguous()
        return x, flags

    def ppr_sweeps(self, batch: int, n: int, damping: float = 0.5, main_only: bool = False,
                   f16: bool = False, small: bool = False, f8: bool = False, f8_mode: str = "C", f8_rio: int = 0,
                   f8_gather_replay: bool = False):
        """Measurement hook: n sweeps of the fp32 slab kernel, of the fp16-state kernel (f16=True), of
        the small-batch kernel (small=True, batch <= 8) or of the fp8-state kernel (f8=True; f8_mode picks
        the kernel instantiation: "C" stage sweep, "B" boundary, "B0" first boundary, "F" final;
        f8_gather_replay=True: only the state-row gathers of a stage sweep, nothing computed or written)."""
        flags = (1 if main_only else 0) | (2 if f16 else 0) | (4 if small else 0) | (8 if f8 else 0)
        flags |= ({"C": 0, "B": 1, "F": 2, "B0": 3}[f8_mode] << 4) | ((f8_rio & 3) << 6)
        flags |= 256 if (f8 and f8_gather_replay) else 0
        check(self._lib.hrag_ppr_sweeps(self._handle, batch, n, damping, flags, _stream()))

    def _is_undirected(self) -> bool:
        """graph.looks_undirected of the engine's graph, evaluated once, on first use (needs the graph object the engine
        was created from to be alive still: the mirror and the adapter keep theirs)."""
        if self._undirected is None:
            from .graph import looks_undirected
            g = self._graph_ref() if getattr(self, "_graph_ref", None) else None
            if g is None:
                raise ValueError("HRAG_OPT_ACCEL was not asked for at creation and the graph object is gone: the "
                                 "undirected-graph test cannot run -- pass flags=OPT_ACCEL to HippoRAGEngine()")
            if _graph_fingerprint(g) != self._graph_print:
                raise ValueError("the graph object was modified after the engine was created from it: the undirected-graph "
                                 "test would look at another matrix than the one on the device -- create the engine with "
                                 "flags=OPT_ACCEL, or keep the graph arrays unchanged until set_flags(OPT_ACCEL)")
            self._undirected = bool(looks_undirected(g))
            self._graph_ref = None
        return self._undirected

    def set_flags(self, flags: int, on: bool = True):
        """Set / clear HRAG_OPT_* bits after creation (e.g. _lib.OPT_NO_FP8 to rerun a saturated batch).
        OPT_ACCEL, first time: runs graph.looks_undirected on the graph OBJECT the engine was created from -- it must
        still be alive and unchanged (a fingerprint of its arrays is checked); engines that will need the flag later can
        pass it at creation instead, which runs the test there."""
        if on and (flags & _lib.OPT_ACCEL) and not self._is_undirected():
            raise ValueError("HRAG_OPT_ACCEL needs an undirected graph with col_sum on an unsharded engine "
                             "(hipporag_amd.graph.looks_undirected): this engine's graph does not qualify")
        check(self._lib.hrag_engine_set_flags(self._handle, flags, 1 if on else 0))
        self.opt_flags = (self.opt_flags | flags) if on else (self.opt_flags & ~flags)

    def gather_embeddings(self, which: str, src_rows, new_rows=None):
        """The embedding matrix of the next engine after an index update, composed ON THE DEVICE:
        out[i] = this engine's row src_rows[i] (>= 0) or new_rows[-src_rows[i] - 1].  new_rows: bf16 / fp16
        tensor or uint16 bit patterns (host or device).  Returns a device tensor [n, dim] in the engine's dtype."""
        torch = _torch()
        src = torch.as_tensor(np.ascontiguousarray(src_rows, dtype=np.int32)).to(self.device)
        n = int(src.shape[0])
        fresh = None
        if new_rows is not None and len(new_rows):
            obj, rows, dim, dt = _as_16bit(new_rows)
            if dim != self.dim or getattr(torch, _TORCH_DTYPE_OF[dt]) != self.emb_dtype or dt == 3:
                raise ValueError("new rows must match the engine's embedding dim / dtype")
            if self.f32_split:     # fp32 rows -> the engine's [hi | lo | hi] layout, on the device
                x = (torch.from_numpy(obj) if isinstance(obj, np.ndarray) else obj).to(self.device).contiguous()
                fresh = torch.empty((rows, 3 * self.dim), dtype=torch.int16, device=self.device)
                check(self._lib.hrag_split_f32(x.data_ptr(), rows, self.dim, 0, 0, fresh.data_ptr(), _stream()))
            else:
                fresh = (torch.from_numpy(obj.view(np.int16)) if isinstance(obj, np.ndarray) else obj.view(torch.int16)).to(self.device).contiguous()
        if n and int(src.min().item()) < 0 and (fresh is None or int((-src.min()).item()) > fresh.shape[0]):
            raise ValueError("src_rows refers to a new row that was not given")
        # (a split engine's rows are 3 * dim fp16 elements; the result is only ever handed to the next engine)
        out = (torch.empty((n, 3 * self.dim), dtype=torch.float16, device=self.device) if self.f32_split
               else torch.empty((n, self.dim), dtype=self.emb_dtype, device=self.device))
        if which not in ("facts", "passages"):
            raise ValueError("which must be 'facts' or 'passages'")
        held = self.fact_rows if which == "facts" else self.passage_rows
        if n and int(src.max().item()) >= held:
            raise ValueError(f"src_rows refers to row {int(src.max().item())} of {held} held {which} rows")
        check(self._lib.hrag_engine_gather_embeddings(self._handle, 0 if which == "facts" else 1, src.data_ptr(), n,
                                                      fresh.data_ptr() if fresh is not None else None,
                                                      out.data_ptr(), _stream()))
        return SplitRows(out, self.dim) if self.f32_split else out

    # ------------------------------------------------------------------ row shard (include/hrag.h hrag_shard_*)
    def shard_layout(self, batch: int, groups: int = 0) -> ShardLayout:
        lay = ShardLayout()
        check(self._lib.hrag_shard_layout_query(self._handle, batch, groups, C.byref(lay)))
        return lay

    def shard_score_facts(self, q_fact, k: int = 5, scope_filter=None):
        """Local phase A: (global fact ids [B,k], RAW scores [B,k], local min [B], local max [B]).
        scope_filter: the GLOBAL doc filter (doc_filter_words forms over every passage) -- the "seeds" scope: only the
        owned facts with an allowed source, min / max over them (hrag_shard_score_facts_scoped; set_fact_sources)."""
        torch = _torch()
        q = self._q(q_fact)
        b = q.shape[0]
        idx = self._empty((b, k), torch.int32)
        val = self._empty((b, k), torch.float32)
        mn = self._empty((b,), torch.float32)
        mx = self._empty((b,), torch.float32)
        args = (self._handle, q.data_ptr(), b, k, idx.data_ptr(), val.data_ptr(), mn.data_ptr(), mx.data_ptr(), _stream())
        if scope_filter is None:
            check(self._lib.hrag_shard_score_facts(*args))
        else:
            fw, fld = doc_filter_words(scope_filter, self.n_passages, b, self.device)
            check(self._lib.hrag_shard_score_facts_scoped(*args, fw.data_ptr(), fld))
        return idx, val, mn, mx

    def shard_passage_scores(self, q_pass, scope_filter=None):
        """(local min [B], local max [B]) of the owned passage scores; scope_filter (the GLOBAL doc filter): over the
        allowed owned passages only (hrag_shard_passage_scores_scoped; +inf / -inf where there are none)."""
        torch = _torch()
        q = self._q(q_pass)
        b = q.shape[0]
        mn = self._empty((b,), torch.float32)
        mx = self._empty((b,), torch.float32)
        args = (self._handle, q.data_ptr(), b, mn.data_ptr(), mx.data_ptr(), _stream())
        if scope_filter is None:
            check(self._lib.hrag_shard_passage_scores(*args))
        else:
            fw, fld = doc_filter_words(scope_filter, self.n_passages, b, self.device)
            check(self._lib.hrag_shard_passage_scores_scoped(*args, fw.data_ptr(), fld))
        return mn, mx

    def shard_mask_prior(self, mn, mx, scope_filter):
        """The "seeds" prior on the owned passages from the all-reduced allowed min / max (hrag_shard_mask_prior):
        returns the local (min [B], max [B]) of the rewritten scores, to be all-reduced in turn."""
        torch = _torch()
        b = mn.shape[0]
        mn_out = self._empty((b,), torch.float32)
        mx_out = self._empty((b,), torch.float32)
        fw, fld = doc_filter_words(scope_filter, self.n_passages, b, self.device)
        check(self._lib.hrag_shard_mask_prior(self._handle, mn.data_ptr(), mx.data_ptr(), b, mn_out.data_ptr(),
                                              mx_out.data_ptr(), _stream(), fw.data_ptr(), fld))
        return mn_out, mx_out

    def shard_prior_stats(self, mn, mx, passage_node_weight: float, flags):
        torch = _torch()
        b = mn.shape[0]
        zmax = self._empty((b,), torch.float32)
        mass = self._empty((2 * b,), torch.float64)
        check(self._lib.hrag_shard_prior_stats(self._handle, mn.data_ptr(), mx.data_ptr(), passage_node_weight,
                                               flags.data_ptr(), b, zmax.data_ptr(), mass.data_ptr(), _stream()))
        return zmax, mass

    def shard_ppr_begin(self, mn, mx, zmax, mass, passage_node_weight, seeds, flags, damping, ppr_iters,
                        n_groups, bufs, ppr_tol: float = 0.0, ppr_max_iters: int = 0) -> int:
        """Returns the number of steps of the session (ppr_iters, plus the conditional steps of the convergence
        contract when ppr_tol > 0: run them all, the device decides which ones do anything)."""
        sv, sw, sc = seeds
        b = mn.shape[0]
        self._p8_batch = b
        n_steps = C.c_int32(0)
        check(self._lib.hrag_shard_ppr_begin(self._handle, mn.data_ptr(), mx.data_ptr(), zmax.data_ptr(),
                                             mass.data_ptr(), passage_node_weight, sv.data_ptr(), sw.data_ptr(),
                                             sc.data_ptr(), flags.data_ptr(), b, damping, ppr_iters,
                                             max(ppr_max_iters, ppr_iters), ppr_tol, n_groups,
                                             bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                                             C.byref(n_steps), _stream()))
        return n_steps.value

    def shard_ppr_step(self, step: int, group: int):
        """(state buffer to exchange or -1, True when the step is a final sweep that measures the residual: the convergence
        contract's all-reduce + decision follow it)."""
        x, ck = C.c_int32(-1), C.c_int32(0)
        check(self._lib.hrag_shard_ppr_sweep(self._handle, step, group, C.byref(x), C.byref(ck), _stream()))
        return x.value, bool(ck.value)

    def shard_ppr_sweep(self, sweep: int, group: int) -> int:
        return self.shard_ppr_step(sweep, group)[0]

    def shard_ppr_est(self, est=None):
        """est=None: this shard's measure of the latest final sweep (fp32 [B]); est given: write the all-reduced values
        back."""
        torch = _torch()
        b = self._p8_batch
        if est is None:
            out = self._empty((b,), torch.float32)
            check(self._lib.hrag_shard_ppr_est(self._handle, out.data_ptr(), 0, _stream()))
            return out
        check(self._lib.hrag_shard_ppr_est(self._handle, est.data_ptr(), 1, _stream()))
        return est

    def shard_ppr_decide(self, step: int):
        check(self._lib.hrag_shard_ppr_decide(self._handle, step, _stream()))

    def shard_ppr_gate_open(self, step: int) -> bool:
        """Will step `step` do anything (hrag_shard_ppr_gate; synchronises the stream)?"""
        o = C.c_int32(0)
        check(self._lib.hrag_shard_ppr_gate(self._handle, step, C.byref(o), _stream()))
        return bool(o.value)

    def shard_finish(self, mn, mx, flags, k: int, want_residual: bool = False, doc_filter=None, boost=None, late=None,
                     late_candidates=None, feedback=None, recommend=None):
        """doc_filter: the GLOBAL filter ([B, n_passages of the whole index] or packed); the shard reads its slice."""
        refuse_boost("shard_finish", {"boost": boost})
        refuse_reco("shard_finish", {"feedback": feedback, "recommend": recommend})
        refuse_late("shard_finish", {"late": late, "late_candidates": late_candidates})
        torch = _torch()
        b = mn.shape[0]
        idx = self._empty((b, k), torch.int32)
        val = self._empty((b, k), torch.float32)
        resid = self._empty((b,), torch.float32) if want_residual else None
        used = self._empty((b,), torch.int32) if want_residual else None
        args = (self._handle, mn.data_ptr(), mx.data_ptr(), flags.data_ptr(), b, k, idx.data_ptr(), val.data_ptr(),
                resid.data_ptr() if want_residual else None, used.data_ptr() if want_residual else None, _stream())
        if doc_filter is None:
            check(self._lib.hrag_shard_finish(*args))
        else:
            fw, fld = doc_filter_words(doc_filter, self.n_passages, b, self.device)
            check(self._lib.hrag_shard_finish_filtered(*args, fw.data_ptr(), fld))
        return (idx, val, resid, used) if want_residual else (idx, val)


class CapturedPipeline:
    """Phase A + identity filter + phase B of one fixed batch size captured into a HIP graph.

    The C ABI only enqueues kernels (no allocation, no synchronisation), so the ~35 launches of a
    single-query retrieval (``retrieve_ircot`` issues one per reasoning step, HippoRAG.py:526,539)
    collapse into one graph launch.  ``__call__`` copies the new queries into the graph's static input
    buffers, replays, and returns views of the static outputs (valid until the next call):

        pipe = CapturedPipeline(engine, batch=1, k=200)
        fact_idx, fact_score, doc_idx, doc_score, flags = pipe(q_fact, q_pass)

    A host-side LLM filter cannot sit inside a graph: use score_facts / retrieve directly for that.
    """

    def __init__(self, engine: "HippoRAGEngine", batch: int, *, k_f: int = 5, k: int = 200, **retrieve_kw):
        torch = _torch()
        refuse_group_agg("CapturedPipeline", retrieve_kw)
        refuse_mmr("CapturedPipeline", retrieve_kw)
        refuse_lexical("CapturedPipeline", retrieve_kw)
        refuse_boost("CapturedPipeline", retrieve_kw)
        refuse_late("CapturedPipeline", retrieve_kw)
        refuse_reco("CapturedPipeline", retrieve_kw)
        self.engine, self.batch = engine, int(batch)
        dev, dt = engine.device, engine.emb_dtype
        self._qf = torch.zeros((batch, engine.dim), dtype=dt, device=dev)
        self._qp = torch.zeros((batch, engine.dim), dtype=dt, device=dev)
        self._cnt = torch.full((batch,), k_f, dtype=torch.int32, device=dev)

        def run():
            idx, sc = engine.score_facts(self._qf, k=k_f)
            out = engine.retrieve(self._qp, idx, sc, self._cnt, link_top_k=k_f, k=k, **retrieve_kw)
            return idx, sc, out.doc_idx, out.doc_score, out.flags

        with torch.cuda.device(dev):
            run()                                    # warm-up (lazy module loads) outside the capture
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._out = run()

    def __call__(self, q_fact, q_pass):
        self._qf.copy_(q_fact)
        self._qp.copy_(q_pass)
        self.graph.replay()
        return self._out


_TOPK_WS = {}   # (device, stream) -> the K4' scratch of topk_rows at k > 2048, grown on demand


def _topk_workspace(device, stream: int, nbytes: int):
    torch = _torch()
    key = (device, stream)
    ws = _TOPK_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _TOPK_WS[key] = torch.empty((nbytes,), dtype=torch.uint8, device=device)
    return ws


def topk_rows(scores, k: int, *, n: Optional[int] = None, idx_offset: int = 0, normalize: bool = False,
              want_minmax: bool = False):
    """Row-wise top-k of a device fp32 matrix with the library ranking rule (hrag_topk_rows; any k > 2048 through
    hrag_topk_rows_ws with a workspace cached per device and stream)."""
    torch = _torch()
    lib = _lib.load()
    if not scores.is_cuda:
        raise RuntimeError("topk_rows runs on the GPU only")
    s = scores.to(torch.float32).contiguous()
    b, ld = s.shape
    n = ld if n is None else n
    idx = torch.empty((b, k), dtype=torch.int32, device=s.device)
    val = torch.empty((b, k), dtype=torch.float32, device=s.device)
    mn = torch.empty((b,), dtype=torch.float32, device=s.device)
    mx = torch.empty((b,), dtype=torch.float32, device=s.device)
    if k <= 2048:
        check(lib.hrag_topk_rows(s.data_ptr(), b, n, ld, k, idx_offset, 1 if normalize else 0, idx.data_ptr(),
                                 val.data_ptr(), mn.data_ptr(), mx.data_ptr(), _stream()))
    else:
        need = int(lib.hrag_topk_rows_workspace_bytes(b, n, k))
        ws = _topk_workspace(s.device, _stream(), need).data_ptr() if need else None
        check(lib.hrag_topk_rows_ws(s.data_ptr(), b, n, ld, k, idx_offset, 1 if normalize else 0, idx.data_ptr(),
                                    val.data_ptr(), mn.data_ptr(), mx.data_ptr(), ws, need, _stream()))
    return (idx, val, mn, mx) if want_minmax else (idx, val)


def row_minmax(scores, n: Optional[int] = None):
    """Per-row (min, max) of a device fp32 matrix (hrag_row_minmax)."""
    torch = _torch()
    lib = _lib.load()
    s = scores.contiguous()
    b, ld = s.shape
    mn = torch.empty((b,), dtype=torch.float32, device=s.device)
    mx = torch.empty((b,), dtype=torch.float32, device=s.device)
    check(lib.hrag_row_minmax(s.data_ptr(), b, ld if n is None else n, ld, mn.data_ptr(), mx.data_ptr(),
                              _stream()))
    return mn, mx


class EngineStages:
    """The stage-level operators of include/hrag.h on caller-owned torch buffers -- what
    hipporag_amd.dist composes with its exchange steps.  One instance per (possibly row-sharded)
    engine."""

    def __init__(self, engine: HippoRAGEngine):
        self.e = engine
        self.lib = engine._lib
        self.h = engine._handle
        self.device = engine.device

    # --- metadata
    def layout(self, batch):
        return self.e.layout(batch)

    def new_state(self, batch):
        bc, ns = self.layout(batch)
        return _torch().zeros((ns, self.e.num_vertices, bc), dtype=_torch().float32, device=self.device)

    # --- similarity / selection
    def sim_scores(self, which, q):
        return self.e.sim_scores(which, q)

    def topk(self, scores, k, idx_offset=0):
        return topk_rows(scores, k, idx_offset=idx_offset, want_minmax=True)

    def row_minmax(self, scores):
        return row_minmax(scores)

    # --- reset vector
    def seeds(self, kept_idx, kept_score, kept_count, link_top_k, out=None):
        """hrag_stage_seeds -> (seed_vtx, seed_w, seed_cnt, flags), into fresh zeroed buffers or into out= (the same
        four tensors: int32 [B, 32], fp32 [B, 32], int32 [B], int32 [B]; flags is read-modify-written)."""
        torch = _torch()
        b, kf = kept_idx.shape
        if out is not None:
            sv, sw, sc, flags = out
        else:
            sv = torch.zeros((b, SEED_STRIDE), dtype=torch.int32, device=self.device)
            sw = torch.zeros((b, SEED_STRIDE), dtype=torch.float32, device=self.device)
            sc = torch.zeros((b,), dtype=torch.int32, device=self.device)
            flags = torch.zeros((b,), dtype=torch.int32, device=self.device)
        if sv.shape != (b, SEED_STRIDE) or sw.shape != (b, SEED_STRIDE) or sc.shape != (b,) or flags.shape != (b,):
            raise ValueError("seeds out=: seed_vtx / seed_w must be [B, 32], seed_cnt / flags [B]")
        check(self.lib.hrag_stage_seeds(self.h, kept_idx.data_ptr(), kept_score.data_ptr(),
                                        kept_count.data_ptr(), kf, link_top_k, b, sv.data_ptr(),
                                        sw.data_ptr(), sc.data_ptr(), flags.data_ptr(), _stream()))
        return sv, sw, sc, flags

    def teleport(self, scores_full, mn, mx, weight, flags):
        torch = _torch()
        b, ld = scores_full.shape
        bc, ns = self.layout(b)
        tele = torch.empty((ns, self.e.n_passages, bc), dtype=torch.float32, device=self.device)
        check(self.lib.hrag_stage_teleport(self.h, scores_full.data_ptr(), ld, mn.data_ptr(), mx.data_ptr(),
                                           weight, flags.data_ptr(), b, tele.data_ptr(), _stream()))
        return tele

    # --- PPR on the owned rows
    def ppr_init(self, tele, seeds, batch, x):
        sv, sw, sc = seeds
        check(self.lib.hrag_stage_ppr_init(self.h, tele.data_ptr(), sv.data_ptr(), sw.data_ptr(),
                                           sc.data_ptr(), batch, x.data_ptr(), _stream()))

    def ppr_step(self, tele, seeds, batch, damping, x, y):
        sv, sw, sc = seeds
        check(self.lib.hrag_stage_ppr_step(self.h, tele.data_ptr(), sv.data_ptr(), sw.data_ptr(),
                                           sc.data_ptr(), batch, damping, x.data_ptr(), y.data_ptr(),
                                           _stream()))

    def colsum(self, x, batch):
        torch = _torch()
        nbytes = self.lib.hrag_colsum_workspace_bytes(self.h, batch)
        ws = torch.empty((max(nbytes, 8) // 8,), dtype=torch.float64, device=self.device)
        sums = torch.empty((batch,), dtype=torch.float64, device=self.device)
        check(self.lib.hrag_stage_colsum(self.h, x.data_ptr(), batch, ws.data_ptr(), sums.data_ptr(), _stream()))
        return sums

    def doc_scores(self, x, sums, batch, scores_full, mn, mx, flags):
        torch = _torch()
        out = torch.empty((batch, self.e.n_passages), dtype=torch.float32, device=self.device)
        check(self.lib.hrag_stage_doc_scores(self.h, x.data_ptr(), sums.data_ptr(), batch,
                                             scores_full.data_ptr(), scores_full.shape[1], mn.data_ptr(),
                                             mx.data_ptr(), flags.data_ptr(), out.data_ptr(),
                                             self.e.n_passages, _stream()))
        return out


def fp8_stage_plan(iters: int, damping: float = 0.5, tol: float = 0.0):
    """Python mirror of ppr8_plan (csrc/shard.hip): the stage lengths of the plain staged-fp8 PPR for `iters` sweeps.
    bench.py prices its per-instantiation launch times with it and tools/exp_fp8_final.py emulates it; the library
    never calls this.  iters < 19 or damping < 0.46: 1, 2, 3-sweep stages, remainder last.  Otherwise 1, 2, 3, 3-sweep
    stages, as many 4-sweep stages as fit, then: a 2-sweep stage last at a fixed count (20 = 1+2+3+4+4+4+2: five
    boundaries instead of six); 2 + 1 under a tolerance (20 = 1+2+3+3+4+4+2+1: the final measure reads lower)."""
    if iters < 19 or not damping >= 0.46:
        left = iters - 3
        return [1, 2] + [3] * (left // 3) + ([left % 3] if left % 3 else [])
    t = iters - (9 if tol > 0 else 8)
    a = t // 4
    while a > 0 and (t - 4 * a) % 3:
        a -= 1
    return [1, 2, 3] + [3] * ((t - 4 * a) // 3) + [4] * a + ([2, 1] if tol > 0 else [2])


class ShardStages(EngineStages):
    """The hrag_shard_* operators of a row-shard engine (staged fp8 PPR state) -- what
    hipporag_amd.dist.ShardedRetriever composes with its exchange steps."""

    def shard_layout(self, batch, groups=0):
        return self.e.shard_layout(batch, groups)

    def new_state(self, lay):           # one e4m3 state buffer, zero (row V of every group must stay zero)
        return _torch().zeros((lay.state_bytes,), dtype=_torch().uint8, device=self.device)

    @property
    def has_fact_sources(self) -> bool:     # the "seeds" scope can be served (set_fact_sources on the shard engine)
        return self.e.has_fact_sources

    def shard_score_facts(self, q_fact, k, scope_filter=None):
        return self.e.shard_score_facts(q_fact, k, scope_filter)

    def shard_passage_scores(self, q_pass, scope_filter=None):
        return self.e.shard_passage_scores(q_pass, scope_filter)

    def shard_mask_prior(self, mn, mx, scope_filter):
        return self.e.shard_mask_prior(mn, mx, scope_filter)

    def shard_prior_stats(self, mn, mx, weight, flags):
        return self.e.shard_prior_stats(mn, mx, weight, flags)

    def shard_ppr_begin(self, *a):
        return self.e.shard_ppr_begin(*a)

    def shard_ppr_sweep(self, sweep, group):
        return self.e.shard_ppr_sweep(sweep, group)

    def shard_ppr_step(self, step, group):
        return self.e.shard_ppr_step(step, group)

    def shard_ppr_est(self, est=None):
        return self.e.shard_ppr_est(est)

    def shard_ppr_decide(self, step):
        return self.e.shard_ppr_decide(step)

    def shard_ppr_gate_open(self, step):
        return self.e.shard_ppr_gate_open(step)

    def shard_finish(self, mn, mx, flags, k, want_residual=False, **kw):
        return self.e.shard_finish(mn, mx, flags, k, want_residual, **kw)
