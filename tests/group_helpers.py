"""numpy restatement of grouped retrieval (include/hrag.h, "grouped retrieval") -- the definition the device is held to."""

import numpy as np


def rank_order(x):
    """The project's ranking rule: score descending, ties -> larger index first, every NaN above +inf (NaN ties by index)."""
    x = np.asarray(x, np.float32)
    nan = np.isnan(x)
    v = np.where(nan, np.float32(0), x) + np.float32(0)            # -0 -> +0: the two zeros tie
    idx = np.arange(len(x))
    return np.lexsort((idx, v, nan))[::-1]                         # last key first: NaN class, then value, then index


def group_reduce_np(scores, g, allowed, n_groups, agg):
    """One row: (gscore fp32 [G], gbest int32 [G]): the group score (0 for a group without an allowed member) and the
    representative (-1).  MAX: the representative's score as stored; SUM: np.bincount over fp64 weights, rounded once."""
    s = np.asarray(scores, np.float32)
    g = np.asarray(g, np.int64)
    allowed = np.ones(len(s), bool) if allowed is None else np.asarray(allowed, bool)
    gbest = np.full(n_groups, -1, np.int32)
    order = rank_order(s)
    order = order[allowed[order]][::-1]                            # worst first: the last write per group is its best
    gbest[g[order]] = order
    has = gbest >= 0
    gscore = np.zeros(n_groups, np.float32)
    if agg == "sum":
        with np.errstate(invalid="ignore", over="ignore"):
            tot = np.bincount(g[allowed], weights=s[allowed].astype(np.float64), minlength=n_groups).astype(np.float32)
        gscore[has] = tot[has]
    else:
        gscore[has] = s[gbest[has]]
    return gscore, gbest


def group_rank_np(scores, g, allowed, k, agg, n_groups=None):
    """One row: (group ids int32 [k], group scores fp32 [k], representatives int32 [k]); -1 / 0 / -1 beyond the groups
    with an allowed member.  Scores as the ranking returns them: NaN canonical, -0 as +0."""
    n_groups = int(np.max(g)) + 1 if n_groups is None else n_groups
    gscore, gbest = group_reduce_np(scores, g, allowed, n_groups, agg)
    order = rank_order(gscore)
    order = order[gbest[order] >= 0][:k]
    gi = np.full(k, -1, np.int32)
    gs = np.zeros(k, np.float32)
    rep = np.full(k, -1, np.int32)
    gi[:len(order)], rep[:len(order)] = order, gbest[order]
    gs[:len(order)] = canonical(gscore[order])
    return gi, gs, rep


def canonical(x):
    """Scores as the top-k kernels return them: every NaN the quiet NaN 0x7fc00000, -0 folded into +0."""
    x = np.asarray(x, np.float32).copy()
    x[np.isnan(x)] = np.float32(np.nan)
    return x + np.float32(0)


def same_bits(a, b):
    """Bit equality of fp32 arrays with all NaNs in one class (IEEE 754 leaves the sign / payload of a NaN that an
    operation produces to the implementation: inf - inf is 0xffc00000 on x86 and 0x7fc00000 on gfx950)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.uint32)[~na] == b.view(np.uint32)[~nb]).all())


def dedup_full_ranking(scores, g, allowed, k):
    """MAX by its consequence: the full ranking by the project rule, every passage but the first of each group dropped.
    Returns (group ids, scores, passages) of the first k, or None when two groups have bit-equal best keys (the ranking
    among those groups is then by group id, not by passage position)."""
    s = np.asarray(scores, np.float32)
    g = np.asarray(g, np.int64)
    allowed = np.ones(len(s), bool) if allowed is None else np.asarray(allowed, bool)
    order = rank_order(s)
    order = order[allowed[order]]
    _, first = np.unique(g[order], return_index=True)
    keep = order[np.sort(first)]
    best = canonical(s[keep])
    keyed = np.where(np.isnan(best), np.float32(np.inf), best)
    nan_groups = int(np.isnan(best).sum())
    if nan_groups > 1 or len(np.unique(keyed[~np.isnan(best)])) != len(best) - nan_groups:
        return None
    keep = keep[:k]
    return g[keep].astype(np.int32), canonical(s[keep]), keep.astype(np.int32)


def random_groups(rng, n, kind):
    """A passage -> group table over n passages."""
    if kind == "one":
        return np.zeros(n, np.int32)
    if kind == "singletons":
        return rng.permutation(n).astype(np.int32)
    if kind == "two":
        g = (rng.random(n) < 0.5).astype(np.int32)
        g[:2] = (0, 1)
        return g
    if kind == "contiguous":
        return (np.arange(n) // 8).astype(np.int32)
    # power law sizes, shuffled membership
    sizes = []
    left = n
    while left > 0:
        sz = int(min(left, max(1, rng.pareto(1.0) * 3)))
        sizes.append(sz)
        left -= sz
    g = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    return g[rng.permutation(n)] if kind == "shuffled" else g


def csr_of(g, n_groups):
    ptr = np.zeros(n_groups + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(g, minlength=n_groups))
    return ptr, np.argsort(g, kind="stable").astype(np.int32)
