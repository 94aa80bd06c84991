"""Numpy restatement of fused retrieval (include/hrag.h, "fused retrieval"): the fused row of every question, straight from
the sentences of the header -- plain loops over the members, no device code, nothing from hipporag_amd."""

import numpy as np

from tests.group_helpers import canonical, rank_order


def fuse_sum_np(rows, member_ptr, weights=None):
    """[Q, n] fp32: acc = +0.0; acc += float64(w_i) * float64(s_i) in member order, rounded once; NaN canonical."""
    s = np.asarray(rows, np.float32)
    mp = np.asarray(member_ptr, np.int64)
    out = np.empty((len(mp) - 1, s.shape[1]), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(len(mp) - 1):
            acc = np.zeros(s.shape[1], np.float64)
            for i in range(mp[q], mp[q + 1]):
                w = np.float64(1.0 if weights is None else np.float32(weights[i]))
                acc = acc + w * s[i].astype(np.float64)
            out[q] = acc.astype(np.float32)
    out[np.isnan(out)] = np.float32(np.nan)
    return out


def fuse_max_np(rows, member_ptr):
    """[Q, n] fp32: per column the member score that ranks first (any NaN wins), as the ranking returns scores."""
    s = np.asarray(rows, np.float32)
    mp = np.asarray(member_ptr, np.int64)
    out = np.empty((len(mp) - 1, s.shape[1]), np.float32)
    for q in range(len(mp) - 1):
        m = s[mp[q]: mp[q + 1]]
        nan = np.isnan(m).any(axis=0)
        with np.errstate(invalid="ignore"):
            best = np.where(np.isnan(m), -np.inf, m).max(axis=0)
        out[q] = np.where(nan, np.float32(np.nan), best)
    return canonical(out)


def member_lists_np(rows, member_ptr, depth, allowed=None):
    """int32 [B, depth]: every member row ranked at `depth` by the project rule under its QUESTION's filter row (allowed:
    None, bool [n] or [Q, n]); -1 beyond the allowed passages."""
    s = np.asarray(rows, np.float32)
    mp = np.asarray(member_ptr, np.int64)
    lists = np.full((s.shape[0], depth), -1, np.int32)
    for q in range(len(mp) - 1):
        a = None if allowed is None else (allowed if np.ndim(allowed) == 1 else allowed[q])
        for i in range(mp[q], mp[q + 1]):
            order = rank_order(s[i])
            if a is not None:
                order = order[np.asarray(a, bool)[order]]
            order = order[:depth]
            lists[i, :len(order)] = order
    return lists


def rrf_np(lists, member_ptr, n, weights=None, c=60):
    """[Q, n] fp32 from ranked lists int [B, depth] (-1 or an id outside [0, n): skipped): the fp32 chain acc = 0.0f;
    acc = acc + float32(float64(w_i) / float64(c + rank)) in member order over the members that list the passage."""
    lists = np.asarray(lists, np.int64)
    mp = np.asarray(member_ptr, np.int64)
    out = np.zeros((len(mp) - 1, n), np.float32)
    rank = np.arange(1, lists.shape[1] + 1, dtype=np.float64)
    for q in range(len(mp) - 1):
        for i in range(mp[q], mp[q + 1]):
            w = np.float64(1.0 if weights is None else np.float32(weights[i]))
            t = (w / (np.float64(c) + rank)).astype(np.float32)
            keep = (lists[i] >= 0) & (lists[i] < n)
            out[q, lists[i][keep]] = out[q, lists[i][keep]] + t[keep]        # the ids of one member are unique
    return out


def fuse_np(rows, member_ptr, mode, weights=None, c=60, depth=None, allowed=None):
    """The fused rows [Q, n] of a mode ("sum" / "max" / "rrf")."""
    if mode == "sum":
        return fuse_sum_np(rows, member_ptr, weights)
    if mode == "max":
        assert weights is None
        return fuse_max_np(rows, member_ptr)
    assert mode == "rrf"
    n = np.asarray(rows).shape[1]
    return rrf_np(member_lists_np(rows, member_ptr, depth, allowed), member_ptr, n, weights, c)


def rank_np(fused, k, allowed=None):
    """(ids int32 [Q, k], scores fp32 [Q, k]): the ranking of fused rows under the filter (None, [n] or [Q, n]), -1 / 0
    beyond the allowed passages; scores as every ranking returns them."""
    f = np.asarray(fused, np.float32)
    idx = np.full((f.shape[0], k), -1, np.int32)
    sc = np.zeros((f.shape[0], k), np.float32)
    for q in range(f.shape[0]):
        order = rank_order(f[q])
        if allowed is not None:
            a = np.asarray(allowed if np.ndim(allowed) == 1 else allowed[q], bool)
            order = order[a[order]]
        order = order[:k]
        idx[q, :len(order)] = order
        sc[q, :len(order)] = canonical(f[q][order])
    return idx, sc


def partitions(rng, b):
    """The member_ptr arrays the tests cut a batch of b rows by: all singletons, one question, random sizes, a question
    of size 1 followed by one big question (the ones that exist at this b, without repeats)."""
    out = {"singletons": np.arange(b + 1)}
    out["one"] = np.array([0, b])
    if b >= 3:
        cuts = np.sort(rng.choice(np.arange(1, b), size=min(b - 1, max(1, b // 3)), replace=False))
        out["random"] = np.concatenate([[0], cuts, [b]])
    if b >= 2:
        out["one_then_big"] = np.array([0, 1, b])
    seen, keep = set(), {}
    for name, mp in out.items():
        key = tuple(int(v) for v in mp)
        if key not in seen:
            seen.add(key)
            keep[name] = np.asarray(mp, np.int32)
    return keep
