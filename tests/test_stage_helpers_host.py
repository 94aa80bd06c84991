"""tests/stage_helpers.py is the reference the GPU tests of the fp32 CSR sweep are held to; here it is held to the
oracle: K applications of step_np from init_np, normalised by colsum_np, equal oracle.ppr_power on the same reset vector
to fp64 rounding -- whole and stitched from row windows -- and the slab layout round-trips."""

import os

import numpy as np
import pytest
import scipy.sparse as sp

import oracle
from hipporag_amd import synth
from hipporag_amd.graph import build_csr
from tests import stage_helpers as sh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REL = 1e-13


def _oracle_matrix(csr):
    """the matrix the device sees (fp32 values) in the oracle's form"""
    return sp.csr_matrix((np.asarray(csr.val, np.float32).astype(np.float64), csr.col_idx, csr.row_ptr),
                         shape=(csr.num_vertices, csr.num_vertices))


def _windows(v, parts):
    """uneven contiguous row windows, one of them empty"""
    cuts = {2: [0, v // 3, v], 3: [0, v // 5, v // 5, v]}[parts]
    return list(zip(cuts[:-1], cuts[1:]))


def _run(csr, tele32, r2t, seeds, damping, iters, windows):
    v = csr.num_vertices
    x = np.concatenate([sh.init_np(tele32, None if r2t is None else r2t[lo:hi], seeds, hi - lo, lo, v)
                        for lo, hi in windows], axis=1).astype(np.float64)
    tele64 = np.asarray(tele32, np.float32).astype(np.float64)
    for _ in range(iters):
        x = np.concatenate([sh.step_np(csr.rows(lo, hi), x, tele64, None if r2t is None else r2t[lo:hi], seeds,
                                       np.float32(damping), lo)[0] for lo, hi in windows], axis=1)
    sums = sum(sh.colsum_np(x, lo, hi) for lo, hi in windows)
    return x / sums[:, None]


def _check(got, p, resets, damping, iters):
    a = float(np.float32(damping))     # the damping the device sees; 1 - a is then exact in both precisions
    for q in range(resets.shape[0]):
        want = oracle.ppr_power(p, resets[q], a, iters)
        assert np.all(np.abs(got[q] - want) <= REL * want), (q, float(np.abs(got[q] - want).max()))


@pytest.mark.parametrize("name", ["graph_100", "graph_200"])
@pytest.mark.parametrize("damping", [0.5, 0.85])
@pytest.mark.parametrize("parts", [1, 2, 3])
def test_dense_reset_sweeps_equal_the_oracle(name, damping, parts):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    n = int(z["n"])
    csr = build_csr(n, z["src"], z["dst"], z["w"])
    reset32 = z["reset"].astype(np.float32)
    windows = [(0, n)] if parts == 1 else _windows(n, parts)
    for iters in (0, 1, 12):
        got = _run(csr, reset32, None, None, damping, iters, windows)
        _check(got, _oracle_matrix(csr), reset32.astype(np.float64), damping, iters)


@pytest.mark.parametrize("damping", [0.5, 0.85])
@pytest.mark.parametrize("parts", [1, 2, 3])
def test_passage_prior_and_seeds_equal_the_oracle(damping, parts):
    """tele + row_to_tele + seeds on a synth graph: the reset vector is the prior at the passage vertices plus the seed
    weights at entity vertices (disjoint, as the pipeline has them)"""
    kg = synth.make_kg(1500, 9000, seed=31)
    rng = np.random.default_rng(7)
    b, v = 5, kg.num_vertices
    r2t = np.full(v, -1, np.int32)
    r2t[kg.passage_vertex] = np.arange(kg.n_passages, dtype=np.int32)
    tele32 = sh.random_tele(rng, b, kg.n_passages)
    seeds = sh.random_seeds(rng, b, kg.n_entities)         # entity vertices are [0, n_entities)
    resets = np.zeros((b, v))
    resets[:, kg.passage_vertex] = tele32
    resets += sh.seed_dense(seeds, b, v)
    windows = [(0, v)] if parts == 1 else _windows(v, parts)
    got = _run(kg.csr, tele32, r2t, seeds, damping, 9, windows)
    _check(got, _oracle_matrix(kg.csr), resets, damping, 9)


def test_step_reports_degree_and_magnitude():
    g = sh.edge_graph()
    csr = g["csr"]
    rng = np.random.default_rng(1)
    x = sh.random_state(rng, 3, csr.num_vertices).astype(np.float64)
    tele = sh.random_tele(rng, 3, len(g["passage_vertex"]))
    seeds = sh.random_seeds(rng, 3, csr.num_vertices, g["seed_pool"])
    y, mag, deg = sh.step_np(csr, x, tele, g["r2t"], seeds, np.float32(0.3))
    assert np.array_equal(deg, np.diff(csr.row_ptr)) and np.array_equal(y, mag)      # non-negative data
    y2, mag2, _ = sh.step_np(csr, -x, tele, g["r2t"], seeds, np.float32(0.3))
    assert np.array_equal(mag2, mag) and np.any(y2 != y)
    iso = g["isolated"]
    b32 = np.float32(1) - np.float32(0.3)
    want = float(b32) * (np.where(g["r2t"][iso] >= 0, tele[:, np.clip(g["r2t"][iso], 0, None)], 0).astype(np.float64)
                         + sh.seed_dense(seeds, 3, csr.num_vertices)[:, iso].astype(np.float64))
    np.testing.assert_allclose(y[:, iso], want, rtol=1e-15, atol=0)
    assert set(sh.THRESHOLD_DEGREES) <= set(deg.tolist()) and (deg == 0).sum() == 24 and (deg == 1).sum() >= 80


@pytest.mark.parametrize("bc", [4, 8, 16, 32, 64])
def test_slab_round_trip(bc):
    rng = np.random.default_rng(bc)
    for b in (1, 3, 4, 5, 33, 64, 70):
        rows = rng.standard_normal((b, 37)).astype(np.float32)
        slab = sh.to_slab(rows, bc)
        ns = -(-b // bc)
        assert slab.shape == (ns, 37, bc) and slab.flags["C_CONTIGUOUS"]
        assert np.array_equal(sh.from_slab(slab, b), rows)
        for q in (0, b // 2, b - 1):
            assert np.array_equal(slab[q // bc, :, q % bc], rows[q])
        pad = slab.transpose(0, 2, 1).reshape(ns * bc, 37)[b:]
        assert np.all(pad == 0)


def test_doc_scores_restatement():
    x = np.array([[0.25, 0.5, 0.25, 0.0], [0, 0, 0, 0], [1, 2, 3, 4], [0, 0, 0, 0]], np.float32)
    sums = sh.colsum_np(x)
    scores = np.array([[1, 2], [3, 3], [5, 1], [4, 6]], np.float32)
    out, flags = sh.doc_scores_np(x, sums, [1, 3], np.array([0, 1, 4, 0], np.int32), scores, scores.min(1), scores.max(1))
    assert np.array_equal(out, np.array([[0.5, 0], [1, 1], [0.2, 0.4], [0, 0]], np.float32))
    assert flags.tolist() == [0, 1, 4, 2]
