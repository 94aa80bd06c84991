"""The reset vector's seed rule restated in numpy (tests/helpers.py seeds_np, what tests/test_gpu_reset_vector.py holds
hrag_stage_seeds to bit for bit) pinned to the reference semantics of oracle.seed_weights (HippoRAG.py:1574-1623,
:1505-1542) on random finite cases, ties included: same phrases in the same order, the same weights once rounded to
fp32 and sanitised, and the reference's assert (:1541) exactly where flag bit 2 is set."""

import types

import numpy as np
import pytest

import oracle
from tests.helpers import prior_np, seeds_np


def _random_case(rng):
    v = int(rng.integers(2, 14))
    n_facts = int(rng.integers(1, 20))
    subj = rng.integers(-1, v, n_facts)
    obj = rng.integers(-1, v, n_facts)
    same = rng.random(n_facts) < 0.15
    obj[same] = subj[same]                                       # subject == object
    num_chunks = rng.integers(0, 5, v)
    # few distinct values: exact ties between facts and between phrase means; zeros and negatives included
    palette = np.array([0.0, -0.0, 0.25, 0.5, 0.5, 1.0, 0.75, -0.5, 3.0, 1e-3], np.float32)
    scores = palette[rng.integers(0, palette.size, n_facts)] if rng.random() < 0.5 else \
        rng.standard_normal(n_facts).astype(np.float32)
    kf = int(rng.integers(1, 17))
    c = int(rng.integers(0, min(kf, n_facts) + 1))
    kept = rng.permutation(n_facts)[:c]                          # distinct facts: the reference indexes scores by id
    link_top_k = int(rng.choice([0, 1, 2, 3, 5, 8, 32]))
    return v, subj, obj, num_chunks, scores, kf, kept, link_top_k


@pytest.mark.parametrize("seed", range(4))
def test_seeds_np_matches_the_reference_seed_weights(seed):
    rng = np.random.default_rng(9100 + seed)
    asserted_cases = checked = 0
    for _ in range(1000):
        v, subj, obj, num_chunks, scores, kf, kept, link_top_k = _random_case(rng)
        index = types.SimpleNamespace(num_vertices=v, subj_vertex=subj, obj_vertex=obj, num_chunks=num_chunks,
                                      linking_top_k=link_top_k)
        kept_idx = np.full((1, kf), -1, np.int32)
        kept_score = np.zeros((1, kf), np.float32)
        kept_idx[0, :kept.size] = kept
        kept_score[0, :kept.size] = scores[kept]
        vtx, w, cnt, flags, _ = seeds_np(kept_idx, kept_score, [kept.size], link_top_k, subj, obj, num_chunks)
        assert bool(flags[0] & 1) == (kept.size == 0)
        try:
            ids, wts = oracle.seed_weights(index, scores, list(kept), link_top_k)
            asserted = False
        except AssertionError:
            asserted = True
        if link_top_k:
            assert bool(flags[0] & 4) == asserted, (seed, kept, link_top_k)
        if asserted:
            asserted_cases += 1
            continue
        n = int(cnt[0])
        np.testing.assert_array_equal(vtx[0, :n], ids)
        w32 = wts.astype(np.float32)
        np.testing.assert_array_equal(w[0, :n], np.where(w32 > 0, w32, np.float32(0)))
        assert np.all(vtx[0, n:] == -1) and np.all(w[0, n:] == 0)
        checked += 1
    assert checked > 500 and asserted_cases > 20, (checked, asserted_cases)


def test_seeds_np_nan_rule():
    """NaN means rank above every number in first-occurrence order; their weight is +0 and they do not set bit 2."""
    subj = np.array([0, 1, 2, 3, 4], np.int64)
    obj = np.array([-1, -1, -1, -1, -1], np.int64)
    nch = np.zeros(5, np.int64)
    kept_idx = np.array([[0, 1, 2, 3, 4]], np.int32)
    kept_score = np.array([[0.5, np.nan, 2.0, np.nan, -1.0]], np.float32)
    vtx, w, cnt, flags, _ = seeds_np(kept_idx, kept_score, [5], 0, subj, obj, nch)
    assert cnt[0] == 5 and flags[0] == 0
    np.testing.assert_array_equal(vtx[0, :5], [1, 3, 2, 0, 4])
    np.testing.assert_array_equal(w[0, :5], np.array([0, 0, 2.0, 0.5, 0], np.float32))
    assert not np.signbit(w[0, :5]).any()


def test_prior_np_sanitises_like_the_reference_where_they_agree():
    """prior_np against HippoRAG.py:1626-1635 + :1735 restated with numpy's own min / max (which propagate NaN): equal
    on rows of numbers and +-inf (every entry NaN or 0 there, i.e. a zero prior); a NaN zeroes only its own entry
    here (the documented difference: the reference's whole prior becomes 0)."""
    rng = np.random.default_rng(5)
    rows = [rng.standard_normal(9).astype(np.float32), np.ones(9, np.float32),
            np.array([0.1, np.inf, 0.3, -2.0, 0, 0, 1, 2, 3], np.float32),
            np.array([0.1, -np.inf, 0.3, 5.0, 0, 0, 1, 2, 3], np.float32),
            np.array([np.inf, -np.inf, 0.3, 5.0, 0, 0, 1, 2, 3], np.float32)]
    for r in rows:
        with np.errstate(all="ignore"):
            mn, mx = r.min(), r.max()
            ref = np.float32(1) if mx - mn == 0 else (r - mn) / (mx - mn)
            ref = (np.broadcast_to(ref, r.shape) * np.float32(0.05)).astype(np.float32)
        ref = np.where(np.isnan(ref) | (ref < 0), 0, ref)
        np.testing.assert_array_equal(prior_np(r[None], 0.05)[0], ref)
    r = np.array([0.2, np.nan, 0.8, 0.5], np.float32)
    got = prior_np(r[None], 0.05)[0]
    assert got[1] == 0 and got[0] == 0 and got[2] == np.float32(0.05)
