"""Diversified retrieval (include/hrag.h, "diversified retrieval") restated in numpy, element by element, and the
planted-duplicate corpus the feature exists for."""

import numpy as np

from hipporag_amd.graph import bf16_bits_to_float, float_to_bf16_bits


def gram_np(rows, ids, lo=None):
    """The gathered Gram of one query: rows float64 [n, d] (the stored values; an exact-input split engine passes its hi
    halves here and the lo halves as `lo`), ids int [c] -> float64 [c, c].  Element [i][j], i <= j, is row ids[i] (the
    embedding side) against row ids[j] (the query side): hi_i . hi_j + lo_i . hi_j + hi_i . lo_j with lo given; the lower
    triangle is its mirror; an id outside [0, n) is a zero row."""
    rows = np.asarray(rows, np.float64)
    ids = np.asarray(ids, np.int64)
    ok = (ids >= 0) & (ids < rows.shape[0])
    safe = np.where(ok, ids, 0)
    a = rows[safe] * ok[:, None]
    g = a @ a.T
    if lo is not None:
        l = np.asarray(lo, np.float64)[safe] * ok[:, None]
        g = g + l @ a.T + a @ l.T          # [i][j]: lo_i . hi_j + hi_i . lo_j
    up = np.triu(g)
    return up + np.triu(g, 1).T


def _key(v, slot):
    """The ranking key of a value: every NaN above +inf, -0 tying +0; the SMALLER slot wins a tie."""
    if np.isnan(v):
        return (2, 0.0, -slot)
    return (1, float(v) + 0.0, -slot)


def mmr_np(score, ids, G, k, lam, normalize=True, n_ids=None):
    """One query: score fp32 [c], ids int [c], G fp32 [c, c] (row j is read once slot j is selected), lambda -> (sel, idx,
    score, value), each [k].  n_ids: an id >= n_ids is an empty slot too (the engine call); None: negative ids only."""
    score = np.asarray(score, np.float32)
    ids = np.asarray(ids, np.int64)
    G = np.asarray(G, np.float32)
    c = score.shape[0]
    live = [bool(ids[i] >= 0 and (n_ids is None or ids[i] < n_ids)) for i in range(c)]
    lam = np.float32(lam)
    mu = np.float32(1.0) - lam
    with np.errstate(all="ignore"):
        if normalize:
            mn, mx = np.float32(np.inf), np.float32(-np.inf)
            for i in range(c):
                if live[i]:
                    mn, mx = np.fmin(mn, score[i]), np.fmax(mx, score[i])
            rel = [np.float32(1.0) if mx == mn else np.float32(np.float32(score[i] - mn) / np.float32(mx - mn))
                   for i in range(c)]
        else:
            rel = list(score)
        sel = np.full(k, -1, np.int32)
        idx = np.full(k, -1, np.int32)
        sc = np.zeros(k, np.float32)
        val = np.zeros(k, np.float32)
        pen = [None] * c
        for t in range(k):
            best, best_v = None, None
            for i in range(c):
                if not live[i]:
                    continue
                if t == 0:
                    v = np.float32(np.float64(lam) * np.float64(rel[i]))
                else:
                    g = G[sel[t - 1], i]
                    pen[i] = g if t == 1 else np.fmax(pen[i], g)
                    v = np.float32(np.float64(lam) * np.float64(rel[i]) - np.float64(mu) * np.float64(pen[i]))
                key = _key(v, i)
                if best is None or key > best:
                    best, best_v = key, v
            if best is None:
                break
            j = -best[2]
            live[j] = False
            sel[t], idx[t] = j, ids[j]
            sc[t] = np.float32(np.nan) if np.isnan(score[j]) else score[j] + np.float32(0.0)
            val[t] = np.float32(np.nan) if np.isnan(best_v) else best_v + np.float32(0.0)
    return sel, idx, sc, val


def same_bits(a, b):
    """fp32 arrays equal bit for bit, every NaN counted as one value"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def bf16_round(x):
    return bf16_bits_to_float(float_to_bf16_bits(np.asarray(x, np.float32))).astype(np.float32)


PLANTED_CLUSTERS, PLANTED_COPIES, PLANTED_FILLERS, PLANTED_DIM = 8, 4, 8, 128


def planted_corpus(seed):
    """8 clusters of 4 near-copies (cosine ~ 0.999) + 8 unrelated fillers, dim 128, in the order a ranking returns them:
    -> (emb fp32 [40, 128] unit rows, cluster int [40] (-1: a filler), score fp32 [40] descending).  Scores: 1 - 0.02 *
    cluster - 0.001 * copy for the copies, ~0.05 for the fillers."""
    rng = np.random.default_rng(seed)

    def unit(v):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)

    centres = unit(rng.standard_normal((PLANTED_CLUSTERS, PLANTED_DIM)))
    emb, cluster, score = [], [], []
    for cl in range(PLANTED_CLUSTERS):
        for cp in range(PLANTED_COPIES):
            emb.append(unit(centres[cl] + 0.0316 * unit(rng.standard_normal(PLANTED_DIM))))     # cos ~ 0.999 to each other
            cluster.append(cl)
            score.append(1.0 - 0.02 * cl - 0.001 * cp)
    for f in range(PLANTED_FILLERS):
        emb.append(unit(rng.standard_normal(PLANTED_DIM)))
        cluster.append(-1)
        score.append(0.05 - 0.0001 * f)
    return np.asarray(emb, np.float32), np.asarray(cluster), np.asarray(score, np.float32)


def _ordered(v):
    """common.h f32_to_ordered with every NaN at 0xffc00000, as uint64"""
    v = np.asarray(v, np.float32)
    u = (v + np.float32(0.0)).view(np.uint32).astype(np.uint64)
    o = np.where(u & np.uint64(0x80000000), (~u) & np.uint64(0xffffffff), u | np.uint64(0x80000000))
    return np.where(np.isnan(v), np.uint64(0xffc00000), o)


def mmr_batch_np(score, ids, G, k, lam, normalize=True, n_ids=None):
    """mmr_np for a whole batch at once ([B, c] / [B, c, c] or [1, c, c] in, [B, k] out), written the way the device selects: the
    arg-max of the 64-bit key ordered(value) << 32 | ~slot.  tests/test_mmr_host.py holds it to mmr_np bit for bit; the GPU
    tests use it where the per-element loops of mmr_np would take minutes."""
    score = np.asarray(score, np.float32)
    ids = np.asarray(ids, np.int64)
    G = np.asarray(G, np.float32)
    b, c = score.shape
    live = ids >= 0 if n_ids is None else (ids >= 0) & (ids < n_ids)
    lam = np.float32(lam)
    dl, dm = np.float64(lam), np.float64(np.float32(1.0) - lam)
    rows = np.arange(b)
    notslot = (np.uint64(0xffffffff) - np.arange(c, dtype=np.uint64))[None, :]
    with np.errstate(all="ignore"):
        if normalize:
            mn = np.fmin.reduce(np.where(live, score, np.float32(np.inf)), axis=1, initial=np.float32(np.inf))[:, None]
            mx = np.fmax.reduce(np.where(live, score, np.float32(-np.inf)), axis=1, initial=np.float32(-np.inf))[:, None]
            rel = np.where(mx == mn, np.float32(1.0), ((score - mn).astype(np.float32) / (mx - mn).astype(np.float32))).astype(np.float32)
        else:
            rel = score
        sel = np.full((b, k), -1, np.int32)
        idx = np.full((b, k), -1, np.int32)
        sc = np.zeros((b, k), np.float32)
        val = np.zeros((b, k), np.float32)
        pen = np.zeros((b, c), np.float32)
        a = dl * rel.astype(np.float64)
        last = np.zeros(b, np.int64)
        for t in range(k):
            if t == 0:
                v = a.astype(np.float32)
            else:
                g = G[rows % G.shape[0], last]          # (G [1, c, c]: one matrix shared by the batch)
                pen = g if t == 1 else np.fmax(pen, g)
                v = (a - dm * pen.astype(np.float64)).astype(np.float32)
            key = np.where(live, (_ordered(v) << np.uint64(32)) | notslot, np.uint64(0))
            j = key.argmax(axis=1)
            has = key[rows, j] != 0
            r = rows[has]
            jj = j[has]
            sel[r, t], idx[r, t] = jj, ids[r, jj]
            s_, v_ = score[r, jj], v[r, jj]
            sc[r, t] = np.where(np.isnan(s_), np.float32(np.nan), s_ + np.float32(0.0))
            val[r, t] = np.where(np.isnan(v_), np.float32(np.nan), v_ + np.float32(0.0))
            live[r, jj] = False
            last = np.where(has, j, last)
    return sel, idx, sc, val
