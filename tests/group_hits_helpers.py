"""numpy restatement of the group hits (include/hrag.h, "group hits") -- the definition the device and the host form are
held to: the ranking rule of tests/group_helpers.py, restricted to the allowed members of one group, cut after m."""

import numpy as np

from tests.group_helpers import canonical, rank_order


def group_hits_np(scores, g, allowed, group_ids, m):
    """One row: (hit_idx int32 [k, m], hit_score fp32 [k, m]) for the k entries of group_ids (-1, or an id no passage
    carries: an empty row).  rank_order -> keep allowed -> keep g == id -> first m; -1 / 0 beyond them; scores canonical."""
    s = np.asarray(scores, np.float32)
    g = np.asarray(g, np.int64)
    ids = np.asarray(group_ids, np.int64)
    allowed = np.ones(len(s), bool) if allowed is None else np.asarray(allowed, bool)
    order = rank_order(s)
    order = order[allowed[order]]
    go = g[order]
    hi = np.full((len(ids), m), -1, np.int32)
    hs = np.zeros((len(ids), m), np.float32)
    for gid in np.unique(ids):                                     # a repeated id gets the same row every time
        if gid < 0:
            continue
        top = order[go == gid][:m]
        at = np.flatnonzero(ids == gid)
        hi[at, :len(top)] = top
        hs[at, :len(top)] = canonical(s[top])
    return hi, hs


def group_hits_loop(scores, g, allowed, group_ids, m):
    """The same by a plain loop: repeated selection of the best remaining member, no sort."""
    s = [float(v) for v in np.asarray(scores, np.float32)]
    hi = np.full((len(group_ids), m), -1, np.int32)
    hs = np.zeros((len(group_ids), m), np.float32)

    def better(a, b):                                              # is position a ranked before position b?
        na, nb = s[a] != s[a], s[b] != s[b]
        if na or nb:
            return (na and not nb) or (na and nb and a > b)
        return s[a] > s[b] or (s[a] == s[b] and a > b)             # -0.0 == 0.0 in Python as in the rule

    for j, gid in enumerate(group_ids):
        left = [p for p in range(len(s)) if gid >= 0 and g[p] == gid and (allowed is None or allowed[p])]
        for slot in range(m):
            if not left:
                break
            best = left[0]
            for p in left[1:]:
                if better(p, best):
                    best = p
            left.remove(best)
            hi[j, slot] = best
            hs[j, slot] = np.float32(np.nan) if s[best] != s[best] else np.float32(s[best]) + np.float32(0)
    return hi, hs


def random_group_ids(rng, n_groups, b, k):
    """[b, k] group ids in [-1, n_groups): repeats and -1 included."""
    ids = rng.integers(-1, n_groups, (b, k)).astype(np.int32)
    if k > 2:
        ids[:, 1] = ids[:, 0]                                      # a repeated id
        ids[:, 2] = -1
    return ids
