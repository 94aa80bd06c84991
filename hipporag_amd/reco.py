"""Recommend by example (include/hrag.h, "recommend by example"; csrc/reco.hip): the examples of a batch -- liked and
disliked passage ids per query -- and the checks of the recommend calls and of the `feedback=` option.  The engine glue
is in engine.py (recommend_scores, recommend_query, recommend_filter, recommend, retrieve(feedback=))."""

from __future__ import annotations

from typing import Optional

import numpy as np

from ._lib import RECO_AVERAGE_VECTOR, RECO_BEST_SCORE, RECO_MAX_EXAMPLES, RECO_SUM_SCORES

RECO_STRATEGIES = {"best_score": RECO_BEST_SCORE, "sum_scores": RECO_SUM_SCORES, "average_vector": RECO_AVERAGE_VECTOR}
RECO_ROW_STRATEGIES = ("best_score", "sum_scores")       # the strategies that produce score rows
_I32_MIN, _I32_MAX = -(2 ** 31), 2 ** 31 - 1


def _torch():
    import torch
    return torch


def check_strategy(strategy, rows_only: bool = False, name: str = "strategy") -> int:
    """The HRAG_RECO_* code of a strategy name; rows_only: "average_vector" produces a query, not rows."""
    if strategy not in RECO_STRATEGIES:
        raise ValueError(f"{name}={strategy!r}: one of {tuple(RECO_STRATEGIES)} expected")
    if rows_only and strategy not in RECO_ROW_STRATEGIES:
        raise ValueError(f"{name}={strategy!r} produces a query, not score rows: one of {RECO_ROW_STRATEGIES} expected here "
                         "(recommend_query + the ordinary calls serve it)")
    return RECO_STRATEGIES[strategy]


def check_feedback_weight(w) -> float:
    if isinstance(w, bool) or not isinstance(w, (int, float, np.integer, np.floating)) or not 0.0 <= float(w) <= 1.0:
        raise ValueError(f"feedback_weight={w!r}: a number in [0, 1] expected")
    return float(w)


def _id_lists(lists, name: str, batch: Optional[int]):
    if lists is None:
        return None
    if isinstance(lists, np.ndarray) and lists.ndim == 2:
        lists = list(lists)
    if not isinstance(lists, (list, tuple)):
        raise ValueError(f"{name}: a list of per-query id lists expected")
    if batch is not None and len(lists) != batch:
        raise ValueError(f"{name} holds {len(lists)} queries, positive {batch}")
    out = []
    for b, ids in enumerate(lists):
        a = np.asarray(ids if ids is not None else [])
        if a.size == 0:
            a = np.zeros(0, np.int64)
        if a.ndim != 1 or a.dtype.kind not in "iu":
            raise ValueError(f"{name}[{b}]: a flat list of integer passage ids expected")
        a = a.astype(np.int64)
        if a.size and (a.min() < _I32_MIN or a.max() > _I32_MAX):
            raise ValueError(f"{name}[{b}]: ids must fit int32")
        out.append(a)
    return out


class Examples:
    """The examples of a batch of queries in CSR form: ex_ptr int32 [B + 1] (a host copy for the checks, a device copy for
    the kernels), ex_idx / ex_sign int32 [E] on the device (host copies alongside).  An id outside the engine's passages
    or a sign 0 is an empty example: it contributes nothing."""

    def __init__(self, ex_ptr, ex_idx, ex_sign, device=None):
        torch = _torch()
        p = np.asarray(ex_ptr)
        if p.ndim != 1 or p.shape[0] < 2 or p.dtype.kind not in "iu":
            raise ValueError("ex_ptr: a one-dimensional integer array of B + 1 entries, B >= 1, expected")
        p = p.astype(np.int64)
        if p[0] != 0:
            raise ValueError(f"ex_ptr[0] = {int(p[0])}, 0 expected")
        lens = np.diff(p)
        if (lens < 0).any():
            at = int(np.argmax(lens < 0))
            raise ValueError(f"ex_ptr descends at entry {at} ({int(p[at])} -> {int(p[at + 1])})")
        if (lens > RECO_MAX_EXAMPLES).any():
            at = int(np.argmax(lens > RECO_MAX_EXAMPLES))
            raise ValueError(f"query {at} holds {int(lens[at])} examples, at most RECO_MAX_EXAMPLES={RECO_MAX_EXAMPLES}")
        if (lens == 0).any():
            raise ValueError(f"query {int(np.argmax(lens == 0))} holds no example: at least one per query expected")
        idx, sign = np.asarray(ex_idx), np.asarray(ex_sign)
        if idx.ndim != 1 or sign.ndim != 1 or idx.shape[0] != int(p[-1]) or sign.shape[0] != int(p[-1]):
            raise ValueError(f"ex_idx / ex_sign: one-dimensional arrays of ex_ptr[-1] = {int(p[-1])} entries expected")
        if idx.dtype.kind not in "iu" or sign.dtype.kind not in "iu":
            raise ValueError("ex_idx / ex_sign: integer arrays expected")
        if idx.size and (idx.min() < _I32_MIN or idx.max() > _I32_MAX):
            raise ValueError("ex_idx: ids must fit int32")
        if sign.size and (np.abs(sign.astype(np.int64)) > 1).any():
            raise ValueError("ex_sign: +1 (positive), -1 (negative) or 0 (empty) expected")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.device = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
        if self.device.type == "cuda" and self.device.index is None:          # "cuda": the current device, by its number
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.ex_ptr = np.ascontiguousarray(p, dtype=np.int32)
        self.ex_idx_host = np.ascontiguousarray(idx, dtype=np.int32)
        self.ex_sign_host = np.ascontiguousarray(sign, dtype=np.int32)
        self.ex_ptr_dev = torch.from_numpy(self.ex_ptr).to(self.device)
        self.ex_idx = torch.from_numpy(self.ex_idx_host).to(self.device)
        self.ex_sign = torch.from_numpy(self.ex_sign_host).to(self.device)
        self.batch, self.n_examples = p.shape[0] - 1, int(p[-1])

    @classmethod
    def from_lists(cls, positive, negative=None, device=None) -> "Examples":
        """From per-query lists of liked (positive) and disliked (negative) passage ids; query b's list is its positives in
        the order given, then its negatives.  negative None: no negatives anywhere."""
        pos = _id_lists(positive, "positive", None)
        if not pos:
            raise ValueError("positive: at least one query expected")
        neg = _id_lists(negative, "negative", len(pos)) or [np.zeros(0, np.int64)] * len(pos)
        for b, (a, c) in enumerate(zip(pos, neg)):
            if a.size + c.size > RECO_MAX_EXAMPLES:
                raise ValueError(f"query {b} holds {a.size + c.size} examples, at most RECO_MAX_EXAMPLES={RECO_MAX_EXAMPLES}")
            if a.size + c.size == 0:
                raise ValueError(f"query {b} holds no example: at least one per query expected")
        ptr = np.zeros(len(pos) + 1, np.int64)
        ptr[1:] = np.cumsum([a.size + c.size for a, c in zip(pos, neg)])
        idx = np.concatenate([np.concatenate([a, c]) for a, c in zip(pos, neg)])
        sign = np.concatenate([np.concatenate([np.ones(a.size, np.int64), -np.ones(c.size, np.int64)]) for a, c in zip(pos, neg)])
        return cls(ptr, idx, sign, device)

    def select(self, rows) -> "Examples":
        """The queries `rows` (positions in this batch, in the order given; repeats allowed) as a batch of their own."""
        r = np.asarray(rows, np.int64).reshape(-1)
        if r.size == 0 or (r < 0).any() or (r >= self.batch).any():
            raise ValueError(f"rows: positions in [0, {self.batch}) expected, at least one")
        p = self.ex_ptr.astype(np.int64)
        take = np.concatenate([np.arange(p[i], p[i + 1]) for i in r])
        ptr = np.zeros(r.size + 1, np.int64)
        ptr[1:] = np.cumsum(p[r + 1] - p[r])
        return Examples(ptr, self.ex_idx_host[take], self.ex_sign_host[take], self.device)


def check_examples(examples, batch: Optional[int] = None, name: str = "examples") -> Examples:
    if not isinstance(examples, Examples):
        raise ValueError(f"{name}: an Examples expected (Examples.from_lists), not {type(examples).__name__}")
    if batch is not None and examples.batch != batch:
        raise ValueError(f"{name}: it holds {examples.batch} queries, the call {batch}")
    return examples


def refuse_reco(who: str, kw: dict) -> None:
    """The callers that do not serve recommend / relevance feedback name the argument they refuse."""
    for name in ("feedback", "recommend"):
        if kw.get(name) is not None:
            raise NotImplementedError(f"{who} does not serve {name}: the example rows are read by id from one unsharded "
                                      "engine's passage embeddings -- use HippoRAGEngine.recommend or "
                                      "HippoRAGEngine.retrieve(feedback=...)")
