"""Lexical retrieval restated in numpy (include/hrag.h, "lexical retrieval"): the fp64 chain of hrag_lex_scores as a
plain loop over the query's terms in list order, and the blend of hrag_lex_blend_rows from its formula.  Written from the
header's definition, not from the kernel; the tests hold the device to these bit for bit."""

import numpy as np

QNAN = np.uint32(0x7FC00000)
LEX_MAX_QUERY_TERMS = 256      # HRAG_LEX_MAX_QUERY_TERMS
LEX_TILE = 2048                # HRAG_LEX_TILE


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def canonical(x):
    """fp32 array with every NaN replaced by the quiet NaN 0x7fc00000."""
    x = np.array(x, np.float32, copy=True)
    x.view(np.uint32)[np.isnan(x)] = QNAN
    return x


def lex_scores_np(n_passages, term_ptr, post_doc, post_w, q_ptr, q_term, q_weight, cap=LEX_MAX_QUERY_TERMS):
    """fp32 [B, n_passages]: per query the chain acc = +0.0; for every listed term in list order (at most `cap` of them;
    a term id outside [0, n_terms) contributes nothing): acc[p] += (double)q_weight * (double)post_w for every passage p
    of the term's posting list -- one fp64 add per (term occurrence, passage), the passages of a list being unique --
    rounded once to fp32, NaN as the quiet NaN."""
    n_terms = len(term_ptr) - 1
    b = len(q_ptr) - 1
    out = np.zeros((b, n_passages), np.float32)
    pw64 = np.asarray(post_w, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        for q in range(b):
            acc = np.zeros(n_passages, np.float64)                     # +0.0
            beg, end = int(q_ptr[q]), int(q_ptr[q + 1])
            for j in range(beg, min(end, beg + cap)):
                t = int(q_term[j])
                if not 0 <= t < n_terms:
                    continue
                lo, hi = int(term_ptr[t]), int(term_ptr[t + 1])
                w = np.float64(np.float32(q_weight[j]))
                docs = post_doc[lo:hi]                                  # unique within a list: one add per passage
                acc[docs] = acc[docs] + w * pw64[lo:hi]
            out[q] = acc.astype(np.float32)
    return canonical(out)


def row_minmax_np(x):
    """(mn, mx) fp32 [B]: fminf / fmaxf over each row from +inf / -inf, NaN skipped (the rule of include/hrag.h)."""
    x = np.asarray(x, np.float32)
    mn = np.fmin.reduce(x, axis=1, initial=np.float32(np.inf)).astype(np.float32)
    mx = np.fmax.reduce(x, axis=1, initial=np.float32(-np.inf)).astype(np.float32)
    return mn, mx


def minmax_np(x, mn, mx):
    """(x - mn) / (mx - mn) in fp32, a zero range giving 1 (tests/helpers.py prior_np's normalisation)."""
    with np.errstate(all="ignore"):
        rng = np.float32(mx) - np.float32(mn)
        if rng == 0:
            return np.ones_like(x, np.float32)
        return ((x - np.float32(mn)) / rng).astype(np.float32)


def blend_np(dense, lex, alpha):
    """fp32 [B, n]: per row, the dense row bit for bit when alpha == 0 or the lexical row has no range (mx == mn, or no
    number at all); else (float)((double)(1.0f - alpha) * (double)nd + (double)alpha * (double)nl) of the two fp32
    min-maxes, NaN as the quiet NaN."""
    dense, lex = np.asarray(dense, np.float32), np.asarray(lex, np.float32)
    a = np.float32(alpha)
    mn_d, mx_d = row_minmax_np(dense)
    mn_l, mx_l = row_minmax_np(lex)
    out = dense.copy()
    with np.errstate(all="ignore"):
        for r in range(dense.shape[0]):
            if a == 0 or not mx_l[r] > mn_l[r]:
                continue
            nd = minmax_np(dense[r], mn_d[r], mx_d[r]).astype(np.float64)
            nl = minmax_np(lex[r], mn_l[r], mx_l[r]).astype(np.float64)
            v = np.float64(np.float32(1) - a) * nd + np.float64(a) * nl
            out[r] = canonical(v.astype(np.float32))
    return out


def rank_np(rows, k, allowed=None):
    """(idx int32 [B, k], score fp32 [B, k]): np.argsort(kind="stable")[::-1] per row over the allowed entries, -1 / 0
    beyond them; scores canonical as every ranking returns them (-0 as +0, the quiet NaN)."""
    rows = np.asarray(rows, np.float32)
    b, n = rows.shape
    idx = np.full((b, k), -1, np.int32)
    sc = np.zeros((b, k), np.float32)
    for r in range(b):
        order = np.argsort(rows[r], kind="stable")[::-1]
        if allowed is not None:
            m = allowed if allowed.ndim == 1 else allowed[r]
            order = order[m[order]]
        order = order[:k]
        idx[r, :len(order)] = order
        sc[r, :len(order)] = canonical(rows[r][order] + np.float32(0))
    return idx, sc


def make_index(rng, n, n_terms=40, tile=LEX_TILE):
    """An inverted index over n passages with the posting lists the tile logic can get wrong: term 0 empty, term 1 every
    passage, term 2 the first passage of every tile, term 3 the last passage of every tile (and of the row), term 4 only
    the last (partial) tile, terms 5 / 6 the same passages with weights 1.5 / 3.0 (a query weighing them 2 / -1 cancels
    to exactly 0), the rest random lists of random density with weights of both signs.  -> (term_ptr int64, post_doc
    int32, post_w fp32)."""
    lists = []
    first = np.arange(0, n, tile)
    last = np.unique(np.minimum(first + tile - 1, n - 1))
    tail = np.arange((n - 1) // tile * tile, n)
    some = np.unique(rng.integers(0, n, max(1, n // 7)))
    for t in range(n_terms):
        if t == 0:
            docs = np.zeros(0, np.int64)
        elif t == 1:
            docs = np.arange(n)
        elif t == 2:
            docs = first
        elif t == 3:
            docs = last
        elif t == 4:
            docs = tail[::2] if len(tail) > 1 else tail
        elif t in (5, 6):
            docs = some
        else:
            dens = (0.002, 0.05, 0.5)[t % 3]
            docs = np.flatnonzero(rng.random(n) < dens)
        if t == 5:
            w = np.full(len(docs), 1.5, np.float32)
        elif t == 6:
            w = np.full(len(docs), 3.0, np.float32)
        else:
            w = (rng.integers(-24, 25, len(docs)).astype(np.float32) / 8 * (1 + rng.random(len(docs)).astype(np.float32)))
        lists.append((docs.astype(np.int32), w.astype(np.float32)))
    ptr = np.zeros(n_terms + 1, np.int64)
    ptr[1:] = np.cumsum([len(d) for d, _ in lists])
    return ptr, np.concatenate([d for d, _ in lists]).astype(np.int32), np.concatenate([w for _, w in lists]).astype(np.float32)


def make_queries(rng, b, n_terms=40, cap=LEX_MAX_QUERY_TERMS):
    """b sparse queries -> (q_ptr int32, q_term int32, q_weight fp32).  In this order, as far as b reaches: a query at
    exactly the cap (random terms, so with repeats), an empty query, a one-term query, a repeated term, out-of-range term
    ids between valid ones, the cancelling pair (2 x term 5, -1 x term 6), a NaN weight (on the list that holds every
    passage), the empty posting list alone, the last-tile list alone, the tile-edge lists, an inf weight, then random
    queries of 1 .. 12 terms."""
    special = [
        (rng.integers(0, n_terms, cap), rng.integers(-16, 17, cap) / 4),
        ([], []),
        ([1], [0.75]),
        ([7, 9, 7, 7], [1.0, -2.0, 0.5, 3.25]),
        ([-1, 8, n_terms, 10, n_terms + 5, 2 ** 31 - 1], [1.0, 2.0, 3.0, -1.5, 5.0, 7.0]),
        ([5, 6], [2.0, -1.0]),
        ([11, 1, 13], [1.0, np.nan, 2.0]),
        ([0], [4.0]),
        ([4], [-1.25]),
        ([2, 3, 2], [1.0, 1.0, 0.5]),
        ([1, 14], [np.inf, 1.0]),
    ]
    terms, weights, ptr = [], [], [0]
    for q in range(b):
        if q < len(special):
            t, w = special[q]
        else:
            m = int(rng.integers(1, 13))
            t, w = rng.integers(0, n_terms, m), rng.integers(-16, 17, m) / 4
        terms.extend(np.asarray(t, np.int64).tolist())
        weights.extend(np.asarray(w, np.float64).tolist())
        ptr.append(len(terms))
    return np.asarray(ptr, np.int32), np.asarray(terms, np.int32), np.asarray(weights, np.float32)
