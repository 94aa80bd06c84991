"""Diversified retrieval without a GPU (include/hrag.h, "diversified retrieval"): the ABI surface, the workspace
arithmetic, hand-worked cases of the numpy restatement (tests/mmr_helpers.py mmr_np), the mirror's numpy form against it,
the validators, and the planted-duplicate corpus on the restatement."""

import os
import re

import numpy as np
import pytest

from hipporag_amd import _lib
from tests.mmr_helpers import bf16_round, gram_np, mmr_np, planted_corpus, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hrag_gram_rows", "hrag_mmr_rows", "hrag_mmr_workspace_bytes", "hrag_mmr", "hrag_mmr_sel")


def test_symbols_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "hrag.h")).read()
    declared = set(re.findall(r"\b(hrag_[a-z_0-9]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    assert lib.hrag_version() == _lib.HRAG_VERSION == 8
    assert re.search(r"#define HRAG_MMR_MAX_CANDIDATES 1024\b", header)
    from hipporag_amd.engine import MMR_MAX_CANDIDATES
    assert MMR_MAX_CANDIDATES == 1024


def test_workspace_bytes_is_the_padded_gram_matrix():
    lib = _lib.load()
    for b, c in ((1, 1), (1, 4), (3, 5), (256, 200), (256, 1024), (7, 1023)):
        assert lib.hrag_mmr_workspace_bytes(b, c) == b * c * (-(-c // 4) * 4) * 4, (b, c)
    assert lib.hrag_mmr_workspace_bytes(1, 1) == 16
    for bad in ((0, 10), (-1, 10), (4, 0), (4, -3), (4, 1025)):
        assert lib.hrag_mmr_workspace_bytes(*bad) < 0, bad


# ---------------------------------------------------------------------------------- hand-worked cases of mmr_np
G4 = np.array([[1.0, 0.9, 0.1, 0.2],
               [0.9, 1.0, 0.3, 0.8],
               [0.1, 0.3, 1.0, 0.4],
               [0.2, 0.8, 0.4, 1.0]], np.float32)
S4 = np.array([4.0, 3.0, 2.0, 1.0], np.float32)
I4 = np.array([10, 11, 12, 13])


def test_lambda_one_is_the_identity_on_finite_scores():
    sel, idx, sc, val = mmr_np(S4, I4, G4, 4, 1.0)
    assert sel.tolist() == [0, 1, 2, 3] and idx.tolist() == [10, 11, 12, 13]
    assert same_bits(sc, S4)
    assert same_bits(val, np.array([1.0, 2 / 3, 1 / 3, 0.0], np.float32))       # rel: one fp32 division each
    sel, idx, sc, val = mmr_np(S4, I4, G4, 2, 1.0, normalize=False)
    assert idx.tolist() == [10, 11] and same_bits(val, S4[:2])


def test_lambda_zero_minimises_the_similarity_after_the_first_pick():
    # t = 0: every value is +0 -> slot 0 (tie to the smaller slot); then -pen: slot 2 (0.1), then max(G[0], G[2]) =
    # [., 0.9, ., 0.4] -> slot 3, then slot 1
    sel, idx, sc, val = mmr_np(S4, I4, G4, 4, 0.0)
    assert sel.tolist() == [0, 2, 3, 1]
    assert same_bits(val, np.array([0.0, -0.1, -0.4, -0.9], np.float32))
    assert same_bits(sc, S4[[0, 2, 3, 1]])


def test_half_lambda_worked_by_hand():
    # rel = [1, 2/3, 1/3, 0]; t0: slot 0 (0.5).  t1: 0.5 rel - 0.5 G[0]: [., 1/3 - .45, 1/6 - .05, -.1] -> slot 2.
    sel, idx, sc, val = mmr_np(S4, I4, G4, 2, 0.5)
    assert sel.tolist() == [0, 2]
    rel2 = np.float32(np.float32(2.0 - 1.0) / np.float32(3.0))
    want = np.float32(np.float64(np.float32(0.5)) * np.float64(rel2) - np.float64(np.float32(0.5)) * np.float64(np.float32(0.1)))
    assert same_bits(val, np.array([0.5, want], np.float32))


def test_equal_scores_give_ones_and_ties_go_to_the_smaller_slot():
    s = np.full(4, 0.25, np.float32)
    sel, _, _, val = mmr_np(s, I4, np.zeros((4, 4), np.float32), 4, 0.5)
    assert sel.tolist() == [0, 1, 2, 3] and same_bits(val, np.full(4, 0.5, np.float32))
    # -0 ties +0: the smaller slot still wins
    sel, _, sc, _ = mmr_np(np.array([0.0, -0.0, 0.0], np.float32), [1, 2, 3], np.zeros((3, 3), np.float32), 3, 1.0,
                           normalize=False)
    assert sel.tolist() == [0, 1, 2] and same_bits(sc, np.zeros(3, np.float32))     # -0 is returned as +0


def test_nan_score_ranks_first_and_is_skipped_by_the_minmax():
    s = np.array([3.0, np.nan, 1.0], np.float32)
    sel, idx, sc, val = mmr_np(s, [5, 6, 7], np.zeros((3, 3), np.float32), 3, 1.0)
    assert sel.tolist() == [1, 0, 2] and np.isnan(sc[0]) and np.isnan(val[0])
    assert same_bits(val[1:], np.array([1.0, 0.0], np.float32))                      # mn / mx over 3 and 1 only
    s = np.array([1.0, np.inf, -np.inf], np.float32)
    sel, _, _, _ = mmr_np(s, [5, 6, 7], np.zeros((3, 3), np.float32), 3, 1.0, normalize=False)
    assert sel.tolist() == [1, 0, 2]


def test_empty_slots_and_k_equal_c():
    ids = np.array([10, -1, 12, -5])
    sel, idx, sc, val = mmr_np(S4, ids, G4, 4, 1.0)
    assert sel.tolist() == [0, 2, -1, -1] and idx.tolist() == [10, 12, -1, -1]
    assert same_bits(sc, np.array([4.0, 2.0, 0.0, 0.0], np.float32)) and same_bits(val, np.array([1.0, 0.0, 0, 0], np.float32))
    sel, idx, _, _ = mmr_np(S4, [-1] * 4, G4, 3, 0.5)
    assert sel.tolist() == [-1] * 3 and idx.tolist() == [-1] * 3
    sel, idx, _, _ = mmr_np(S4, [0, 1, 99, 3], G4, 4, 1.0, n_ids=50)               # the engine call: id >= n_passages
    assert idx.tolist() == [0, 1, 3, -1]
    sel, _, _, _ = mmr_np(S4[:1], [3], G4[:1, :1], 1, 0.3)
    assert sel.tolist() == [0]


def test_gram_np_is_the_upper_triangle_mirrored():
    rows = np.arange(12, dtype=np.float64).reshape(4, 3)
    g = gram_np(rows, [2, -1, 0, 7, 2])
    assert np.array_equal(g, g.T) and g[0, 4] == rows[2] @ rows[2] and g[0, 2] == rows[2] @ rows[0]
    assert not g[1].any() and not g[3].any()
    hi, lo = rows, rows / 1024
    g = gram_np(hi, [0, 3], lo)
    assert g[0, 1] == g[1, 0] == hi[0] @ hi[3] + lo[0] @ hi[3] + hi[0] @ lo[3]


# ---------------------------------------------------------------------------------- inputs of the restatement tests
def _planted_scores(rng, n):
    x = (rng.integers(-40, 40, n).astype(np.float32) / 8 * rng.random(n).astype(np.float32)).astype(np.float32)
    at = rng.integers(0, n, 6)
    x[at[0]], x[at[1]], x[at[2]], x[at[3]] = np.nan, np.inf, -np.inf, -0.0
    x[at[4]] = x[at[5]]
    return x


# ---------------------------------------------------------------------------------- validators
def test_check_mmr_rejects_what_the_header_rejects():
    from hipporag_amd.engine import check_mmr, mmr_plan, refuse_mmr
    assert check_mmr(0.5, 5, 200) == 0.5 and check_mmr(0, 1, 1) == 0.0 and check_mmr(1, 1024, 1024) == 1.0
    for lam, k, c in ((-0.1, 5, 10), (1.5, 5, 10), (float("nan"), 5, 10), ("0.5", 5, 10), (True, 5, 10), (None, 5, 10),
                      (0.5, 0, 10), (0.5, 11, 10), (0.5, 5, 0), (0.5, 5, 1025), (0.5, 2.0, 10), (0.5, 5, True)):
        with pytest.raises(ValueError):
            check_mmr(lam, k, c)
    assert mmr_plan(None, None, 5) is None
    assert mmr_plan(0.25, None, 5) == (0.25, 5) and mmr_plan(0.25, 3, 5) == (0.25, 5) and mmr_plan(0.25, 50, 5) == (0.25, 50)
    with pytest.raises(ValueError, match="mmr_candidates needs mmr_lambda"):
        mmr_plan(None, 50, 5)
    with pytest.raises(ValueError, match="mmr_candidates"):
        mmr_plan(0.5, 2000, 5)
    refuse_mmr("X", {"group_agg": "max"})
    with pytest.raises(ValueError, match="mmr_lambda"):
        refuse_mmr("X", {"mmr_lambda": 0.5})
    with pytest.raises(ValueError, match="mmr_candidates"):
        refuse_mmr("X", {"mmr_candidates": 5})


def test_the_mirror_validates_without_touching_the_device():
    from hipporag_amd.retriever import HippoRAG, RetrievalConfig
    assert RetrievalConfig().mmr_lambda is None and RetrievalConfig().mmr_candidates is None
    rag = HippoRAG(RetrievalConfig(mmr_lambda=0.5))
    assert rag._mmr(None, None) == {"mmr_lambda": 0.5, "mmr_candidates": 200}            # retrieval_top_k
    assert HippoRAG(RetrievalConfig(mmr_lambda=0.5, retrieval_top_k=5000))._mmr(None, None)["mmr_candidates"] == 1024
    assert HippoRAG(RetrievalConfig(mmr_lambda=0.5, mmr_candidates=30))._mmr(None, None)["mmr_candidates"] == 30
    assert rag._mmr(0.25, 7) == {"mmr_lambda": 0.25, "mmr_candidates": 7}
    assert HippoRAG(RetrievalConfig())._mmr(None, None) == {}
    with pytest.raises(ValueError, match="mmr_candidates needs mmr_lambda"):
        HippoRAG(RetrievalConfig())._mmr(None, 5)
    for who in ("retrieve_fused", "retrieve_ircot"):
        with pytest.raises(ValueError, match="mmr_lambda"):
            rag._refuse_mmr(who, None, None)                   # the config asks for it
        with pytest.raises(ValueError, match="mmr_lambda"):
            HippoRAG(RetrievalConfig())._refuse_mmr(who, 0.5, None)
    with pytest.raises(ValueError, match="mmr_lambda"):
        rag.retrieve_fused([["a"]])
    with pytest.raises(ValueError, match="mmr_lambda"):
        rag.retrieve_ircot(["a"], 1)


# ---------------------------------------------------------------------------------- planted duplicates
def test_planted_duplicates_one_pick_per_cluster_on_200_seeds():
    for seed in range(200):
        emb, cluster, score = planted_corpus(seed)
        rows = bf16_round(emb).astype(np.float64)
        g = gram_np(rows, np.arange(len(rows))).astype(np.float32)
        sel, _, _, _ = mmr_np(score, np.arange(len(rows)), g, 8, 0.5)
        assert sorted(cluster[sel].tolist()) == list(range(8)), seed
        assert len(set(cluster[:8].tolist())) == 2          # the plain top 8 cover two clusters


@pytest.mark.parametrize("b,c,k", [(3, 1, 1), (5, 7, 7), (4, 40, 13), (2, 130, 130), (2, 1100, 12)])
def test_the_batched_restatement_is_the_restatement(b, c, k):
    from tests.mmr_helpers import mmr_batch_np
    rng = np.random.default_rng(b * 1000 + c)
    for lam in (0.0, 0.3, 0.5, 1.0):
        for normalize in (True, False):
            s = np.stack([_planted_scores(rng, c) if c >= 7 else rng.random(c).astype(np.float32) for _ in range(b)])
            ids = np.stack([rng.permutation(c) for _ in range(b)]).astype(np.int64)
            ids[rng.random((b, c)) < 0.15] = -1
            ids[0, :] = -1 if c > 1 else ids[0, :]
            shared = c == 40                                       # one similarity matrix for the whole batch: [1, c, c]
            g = rng.standard_normal((1 if shared else b, c, c)).astype(np.float32)
            g = np.triu(g) + np.swapaxes(np.triu(g, 1), 1, 2)
            if c >= 7:
                g[:, 1, 2] = g[:, 2, 1] = np.nan
            got = mmr_batch_np(s, ids, g, k, lam, normalize)
            for q in range(b):
                want = mmr_np(s[q], ids[q], g[0 if shared else q], k, lam, normalize)
                assert np.array_equal(got[0][q], want[0]) and np.array_equal(got[1][q], want[1]), (q, lam, normalize)
                assert same_bits(got[2][q], want[2]) and same_bits(got[3][q], want[3]), (q, lam, normalize)


def test_mmr_pool_is_the_clamped_candidate_count():
    from hipporag_amd.retriever import mmr_pool
    assert mmr_pool(None, 5, 100) == 5 and mmr_pool(200, 5, 13) == 13 and mmr_pool(200, 5, 1000) == 200
    assert mmr_pool(3, 5, 100) == 5 and mmr_pool(50, 60, 55) == 60 and mmr_pool("x", 5, 100) == "x"


def test_the_multi_gpu_retrievers_refuse_by_name():
    """The refusal is the first thing each retrieve() does: no engine, communicator or device is needed to reach it."""
    from hipporag_amd import dist
    for cls in (dist.ShardedRetriever, dist.NativeShardedRetriever, dist.HybridRetriever):
        obj = object.__new__(cls)
        for kw, name in ((dict(mmr_lambda=0.5), "mmr_lambda"), (dict(mmr_candidates=50), "mmr_candidates")):
            with pytest.raises(ValueError, match=f"{cls.__name__} does not serve {name}"):
                obj.retrieve(None, None, None, None, **kw)
