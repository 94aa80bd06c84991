"""The fp32 CSR sweep and the stage-level operators of include/hrag.h restated in numpy, in fp64 -- what
tests/test_gpu_csr_sweep.py and tests/test_gpu_stage_ops.py hold the kernels of csrc/ppr_spmm.hip and csrc/layout.hip to.
tests/test_stage_helpers_host.py pins these helpers themselves against oracle.ppr_power (no GPU).

Dense states are [B, n] (one row per query, as the caller-facing matrices); the device layout ("slab layout") is
[n_slabs][n][bc] with query q in slab q // bc, column q % bc: to_slab / from_slab."""

from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from hipporag_amd.graph import build_csr

SEED_STRIDE = 32


# ----------------------------------------------------------------------------- layout
def to_slab(rows, bc: int) -> np.ndarray:
    """[B, n] -> [n_slabs][n][bc], padding columns (q >= B) zero"""
    rows = np.asarray(rows)
    b, n = rows.shape
    ns = -(-b // bc)
    pad = np.zeros((ns * bc, n), rows.dtype)
    pad[:b] = rows
    return np.ascontiguousarray(pad.reshape(ns, bc, n).transpose(0, 2, 1))


def from_slab(x, batch: int) -> np.ndarray:
    """[n_slabs][n][bc] -> [batch, n]"""
    x = np.asarray(x)
    ns, n, bc = x.shape
    return np.ascontiguousarray(x.transpose(0, 2, 1).reshape(ns * bc, n)[:batch])


# ----------------------------------------------------------------------------- the sweep
def seed_dense(seeds, batch: int, num_vertices: int) -> np.ndarray:
    """float32 [B, V]: seed_w scattered to seed_vtx for the first seed_cnt slots of every query (vertices are unique
    per query; ids outside [0, V) are skipped as the device skips what lies outside its row window)"""
    out = np.zeros((batch, num_vertices), np.float32)
    if seeds is None:
        return out
    vtx, w, cnt = seeds
    for q in range(batch):
        c = int(cnt[q])
        v = np.asarray(vtx[q, :c], np.int64)
        ok = (v >= 0) & (v < num_vertices)
        out[q, v[ok]] = np.asarray(w[q, :c], np.float32)[ok]
    return out


def _tele_rows(tele, r2t, row_offset: int, n_rows: int) -> np.ndarray:
    """[B, n_rows]: the teleport entry of every owned row -- tele[:, r2t[i]] (0 where r2t[i] < 0), or, with r2t None,
    the dense reset vector's own window (the row_to_tele == NULL branch of write_row)"""
    tele = np.asarray(tele)
    if r2t is None:
        return tele[:, row_offset:row_offset + n_rows]
    r2t = np.asarray(r2t, np.int64)
    t = tele[:, np.clip(r2t, 0, None)]
    return np.where(r2t[None, :] >= 0, t, np.zeros((), tele.dtype))


def csr_matrix64(csr) -> sp.csr_matrix:
    """the fp32 values the device sees, widened to fp64; rows = the CSR's own (possibly a row window)"""
    n_rows = csr.row_ptr.shape[0] - 1
    val = np.asarray(csr.val, np.float32).astype(np.float64)
    return sp.csr_matrix((val, np.asarray(csr.col_idx, np.int32), np.asarray(csr.row_ptr, np.int32)),
                         shape=(n_rows, csr.num_vertices))


def step_np(csr, x64, tele64, r2t, seeds, alpha32, row_offset: int = 0):
    """One sweep on the rows of `csr` (rows [row_offset, row_offset + n_rows) of the graph), in fp64:
        y[i] = a * sum_j val[i,j] * x[col[i,j]] + b * (tele[r2t[i]] if r2t[i] >= 0 else 0) + b * seed_w[i]
    a = float32(damping), b = float32(1) - a formed in float32, both then widened.  x64 [B, V], tele64 [B, Np] (r2t
    None: [B, V], the dense reset vector).  -> (y [B, n_rows], mag [B, n_rows], deg [n_rows]): mag is the same
    expression over absolute values (the rounding bound's scale), deg the entry count of every row."""
    n_rows = csr.row_ptr.shape[0] - 1
    a32 = np.float32(alpha32)
    b32 = np.float32(np.float32(1) - a32)
    a, b = float(a32), float(b32)
    p = csr_matrix64(csr)
    x64 = np.asarray(x64, np.float64)
    batch = x64.shape[0]
    t = _tele_rows(np.asarray(tele64, np.float64), r2t, row_offset, n_rows)
    sw = seed_dense(seeds, batch, csr.num_vertices)[:, row_offset:row_offset + n_rows].astype(np.float64)
    y = a * (p @ x64.T).T + b * t + b * sw
    mag = a * (abs(p) @ np.abs(x64).T).T + b * np.abs(t) + b * np.abs(sw)
    return y, mag, np.diff(np.asarray(csr.row_ptr, np.int64))


def init_np(tele32, r2t, seeds, n_rows: int, row_offset: int = 0, num_vertices: int | None = None) -> np.ndarray:
    """x0 on the owned rows, float32 [B, n_rows]: the teleport entry (or 0) plus 1.0 * seed_w -- one fp32 add"""
    tele32 = np.asarray(tele32, np.float32)
    batch = tele32.shape[0]
    v = num_vertices if num_vertices is not None else row_offset + n_rows
    t = _tele_rows(tele32, r2t, row_offset, n_rows)
    sw = seed_dense(seeds, batch, v)[:, row_offset:row_offset + n_rows]
    return (t + sw).astype(np.float32)


def colsum_np(x, lo: int = 0, hi: int | None = None) -> np.ndarray:
    """fp64 [B]: the sum of x[:, lo:hi], every entry widened first"""
    return np.asarray(x)[:, lo:hi].astype(np.float64).sum(axis=1)


def doc_scores_np(x32, sums64, pv, flags, scores, mn, mx):
    """hrag_stage_doc_scores: float32(float64(x32[:, pv]) / sums), 0 where not sums > 0; rows with flags & 1 (the DPR
    fallback) get the fp32 min-max (s - mn) / (mx - mn) of their scores, 1 where mx == mn (minmax_norm, csrc/layout.hip).
    -> (out float32 [B, Np], flags with bit 1 set where not sums > 0 on a non-fallback row)"""
    x32 = np.asarray(x32, np.float32)
    sums = np.asarray(sums64, np.float64)
    flags = np.asarray(flags, np.int32)
    pv = np.asarray(pv, np.int64)
    b = x32.shape[0]
    pos = sums > 0
    with np.errstate(all="ignore"):
        ppr = (x32[:, pv].astype(np.float64) / np.where(pos, sums, 1.0)[:, None]).astype(np.float32)
        ppr[~pos] = 0
        s = np.asarray(scores, np.float32)[:b, :pv.shape[0]]
        mn = np.asarray(mn, np.float32)[:, None]
        mx = np.asarray(mx, np.float32)[:, None]
        rng_ = (mx - mn).astype(np.float32)
        nrm = np.where(rng_ == 0, np.float32(1), ((s - mn).astype(np.float32) / rng_)).astype(np.float32)
    fb = (flags & 1) != 0
    out = np.where(fb[:, None], nrm, ppr).astype(np.float32)
    return out, (flags | np.where(~pos & ~fb, 2, 0)).astype(np.int32)


# ----------------------------------------------------------------------------- test inputs
THRESHOLD_DEGREES = (7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 191, 192, 193, 255, 256, 257, 385,
                     511, 512, 513, 1025)


def edge_graph(seed: int = 5, n_base: int = 6000):
    """A graph whose rows sit on every short / long / segment threshold of the CSR sweep.
    Vertices: [0, n_base) a random graph of mean degree ~10; then two "probe" rows per degree of THRESHOLD_DEGREES
    (8 G - 1, 8 G, 8 G + 1 for G = 1 .. 16; seg - 1, seg, seg + 1, 2 seg + 1 for segment lengths 64, 128, 512), each
    linked to that many distinct base vertices and to nothing else, so its degree is exact; then 40 pairs of degree-1
    rows linked only to each other; then 24 rows without entries.  The ids are shuffled, so the classes are spread over
    the row range (and over any row window).
    -> dict(csr, passage_vertex, r2t, probes {degree: [vertex, vertex]}, tail, isolated, subj, obj, num_chunks)"""
    rng = np.random.default_rng(seed)
    n_probe, n_tail, n_iso = 2 * len(THRESHOLD_DEGREES), 80, 24
    n = n_base + n_probe + n_tail + n_iso
    m = 5 * n_base
    src, dst = [rng.integers(0, n_base, m)], [rng.integers(0, n_base, m)]
    v = n_base
    probes = {}
    for d in THRESHOLD_DEGREES:
        probes[d] = []
        for _ in range(2):
            src.append(np.full(d, v))
            dst.append(rng.choice(n_base, size=d, replace=False))
            probes[d].append(v)
            v += 1
    tail = np.arange(v, v + n_tail)
    src.append(tail[0::2])
    dst.append(tail[1::2])
    v += n_tail
    isolated = np.arange(v, v + n_iso)
    src, dst = np.concatenate(src), np.concatenate(dst)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    w = rng.choice([1.0, 2.0, 4.0, 0.9, 0.37], len(src))
    perm = rng.permutation(n)
    csr = build_csr(n, perm[src], perm[dst], w)
    deg = np.diff(csr.row_ptr)
    probes = {d: [int(perm[u]) for u in us] for d, us in probes.items()}
    for d, us in probes.items():
        assert all(deg[u] == d for u in us), d
    tail, isolated = perm[tail], perm[isolated]
    assert np.all(deg[tail] == 1) and np.all(deg[isolated] == 0)
    # passages: every 8th vertex, the first probe of every degree, half of the rows without entries, a few tail rows
    pv = np.unique(np.concatenate([np.arange(0, n, 8), [us[0] for us in probes.values()], isolated[::2], tail[::5]]))
    pv = rng.permutation(pv).astype(np.int32)
    r2t = np.full(n, -1, np.int32)
    r2t[pv] = np.arange(len(pv), dtype=np.int32)
    is_p = np.zeros(n, bool)
    is_p[pv] = True
    ents = np.flatnonzero(~is_p)
    n_f = 2000
    subj = ents[rng.integers(0, len(ents), n_f)]
    obj = ents[rng.integers(0, len(ents), n_f)]
    # facts 0 .. 31 sit on rows without entries, on the second probe of every degree and on tail rows
    special = np.concatenate([isolated[1::2], [us[1] for us in probes.values()], tail[1::5]])
    special = special[~is_p[special]]
    subj[:len(special)] = special
    num_chunks = np.zeros(n, np.int32)
    num_chunks[ents] = rng.integers(0, 4, len(ents))
    return dict(csr=csr, passage_vertex=pv, r2t=r2t, probes=probes, tail=tail, isolated=isolated,
                subj=subj.astype(np.int32), obj=obj.astype(np.int32), num_chunks=num_chunks, seed_pool=special)


def random_state(rng, batch: int, n: int) -> np.ndarray:
    """float32 [B, n], non-negative: magnitudes spread over 1e-12 .. 1, a fifth exact zeros, every number normal"""
    x = (10.0 ** rng.uniform(-12, 0, (batch, n))).astype(np.float32)
    x[rng.random((batch, n)) < 0.2] = 0
    return x


def random_tele(rng, batch: int, n_p: int) -> np.ndarray:
    """float32 [B, Np]: a prior-like teleport block -- values in [0, 0.05], a tenth exact zeros"""
    t = (0.05 * rng.random((batch, n_p))).astype(np.float32)
    t[rng.random((batch, n_p)) < 0.1] = 0
    return t


def random_seeds(rng, batch: int, num_vertices: int, pool=None):
    """(seed_vtx int32 [B, 32], seed_w float32 [B, 32], seed_cnt int32 [B]): 0 .. 32 distinct vertices per query, half
    of them from `pool` when given; the slots past seed_cnt hold -1 / NaN (never read)"""
    vtx = np.full((batch, SEED_STRIDE), -1, np.int32)
    w = np.full((batch, SEED_STRIDE), np.nan, np.float32)
    cnt = rng.integers(0, SEED_STRIDE + 1, batch).astype(np.int32)
    if batch > 1:
        cnt[0], cnt[-1] = SEED_STRIDE, 0
    for q in range(batch):
        c = int(cnt[q])
        ids = rng.choice(num_vertices, size=c, replace=False)
        if pool is not None and c:
            k = min(c // 2, len(pool))
            ids = np.unique(np.concatenate([rng.choice(pool, size=k, replace=False), ids]))
            ids = rng.permutation(ids)[:c]
        vtx[q, :c] = ids
        w[q, :c] = (10.0 ** rng.uniform(-3, 0, c)).astype(np.float32)
    return vtx, w, cnt
