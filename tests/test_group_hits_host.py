"""Group hits, host side (no GPU): the numpy restatement against a plain loop, the package's host form against the
restatement, the documented consequences in numpy, validation, and the classes that refuse."""

import numpy as np
import pytest

from hipporag_amd.retriever import HippoRAG, RetrievalConfig, group_hits_rows, group_rank_rows, rank_allowed
from tests.group_helpers import canonical, group_rank_np, random_groups, same_bits
from tests.group_hits_helpers import group_hits_loop, group_hits_np, random_group_ids

KINDS = ("one", "singletons", "two", "contiguous", "shuffled")


def _row(rng, n, flavour):
    if flavour == "ties":
        s = rng.integers(-2, 3, n).astype(np.float32) / 2              # five values: heavy ties, +0 among them
    else:
        s = (rng.integers(-40, 40, n).astype(np.float32) / 8 * rng.random(n).astype(np.float32)).astype(np.float32)
    for v in (np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0):
        if rng.random() < 0.6:
            s[rng.integers(0, n, 2)] = v
    return s


def _cases(rng, count):
    for c in range(count):
        n = int(rng.integers(2, 90))
        g = random_groups(rng, n, KINDS[c % len(KINDS)])
        n_groups = int(g.max()) + 1 + (c % 3 == 0)                    # sometimes an id no passage carries: an empty group
        s = _row(rng, n, "ties" if c % 2 else "mixed")
        mode = c % 4
        allowed = None if mode == 0 else rng.random(n) < 0.5
        if mode == 3:
            allowed = allowed & (g != g[0])                            # a filter that empties a group
        ids = random_group_ids(rng, n_groups, 1, int(rng.integers(1, 9)))[0]
        yield s, g, allowed, n_groups, ids


def test_the_restatement_is_a_plain_loop():
    rng = np.random.default_rng(20261016)
    for s, g, allowed, n_groups, ids in _cases(rng, 400):
        for m in (1, 3, 64):
            hi, hs = group_hits_np(s, g, allowed, ids, m)
            li, ls = group_hits_loop(s, g, allowed, ids, m)
            assert hi.tolist() == li.tolist()
            assert same_bits(hs, ls)
            assert ((hi >= 0) | (hs.view(np.uint32) == 0)).all()       # -1 slots carry +0


def test_the_packages_host_form_is_the_restatement():
    rng = np.random.default_rng(7)
    for s, g, allowed, n_groups, ids in _cases(rng, 400):
        rows = np.stack([s, s[::-1].copy()])
        al = None if allowed is None else np.stack([allowed, ~allowed])
        for m in (1, 3, 64):
            hi, hs = group_hits_rows(rows, g, al, np.stack([ids, ids]), m)
            assert hi.dtype == np.int32 and hs.dtype == np.float32 and hi.shape == (2, len(ids), m)
            for i in range(2):
                e = group_hits_np(rows[i], g, None if al is None else al[i], ids, m)
                assert hi[i].tolist() == e[0].tolist()
                assert same_bits(hs[i], e[1])
        shared = group_hits_rows(rows, g, allowed, np.stack([ids, ids]), 3)      # one filter row for the batch
        assert shared[0][0].tolist() == group_hits_np(s, g, allowed, ids, 3)[0].tolist()


def test_group_rank_rows_hits_option_agrees_with_the_two_steps():
    rng = np.random.default_rng(8)
    for s, g, allowed, n_groups, _ in _cases(rng, 120):
        al = None if allowed is None else allowed[None]
        for agg in ("max", "sum"):
            plain = group_rank_rows(s[None], g, al, 5, agg)
            got = group_rank_rows(s[None], g, al, 5, agg, 3)
            assert len(plain) == 3 and len(got) == 5
            for a, b in zip(plain, got):
                assert np.array_equal(a.view(np.int32), b.view(np.int32))     # the first three entries are unchanged
            e = group_hits_np(s, g, allowed, got[0][0], 3)
            assert got[3][0].tolist() == e[0].tolist() and same_bits(got[4][0], e[1])


def test_consequence_1_first_hit_is_the_representative():
    rng = np.random.default_rng(9)
    for s, g, allowed, _, _ in _cases(rng, 300):
        n_groups = int(g.max()) + 1
        for agg in ("max", "sum"):
            gi, gs, rep = group_rank_np(s, g, allowed, 6, agg, n_groups)
            hi, hs = group_hits_np(s, g, allowed, gi, 3)
            assert hi[:, 0].tolist() == rep.tolist()
            if agg == "max":
                assert same_bits(hs[:, 0], gs)                                  # bit for bit the group score
            else:
                own = np.where(rep >= 0, canonical(s[np.maximum(rep, 0)]), np.float32(0))
                assert same_bits(hs[:, 0], own)                                 # each member's own score, not the sum
            one = group_hits_np(s, g, allowed, gi, 1)                           # consequence 3: m = 1 adds nothing
            assert one[0][:, 0].tolist() == rep.tolist()


def test_consequence_2_hits_are_the_filtered_ranking_under_allowed_and_member():
    rng = np.random.default_rng(10)
    for s, g, allowed, n_groups, ids in _cases(rng, 300):
        a = np.ones(len(s), bool) if allowed is None else allowed
        hi, hs = group_hits_np(s, g, allowed, ids, 4)
        for j, gid in enumerate(ids):
            fi, fs = rank_allowed(s[None], (a & (g == gid))[None], 4)           # the package's filtered ranking on the host
            assert hi[j].tolist() == fi[0].tolist()
            assert same_bits(hs[j], canonical(fs[0]))


def test_validation():
    from hipporag_amd import engine
    assert engine.check_group_hits(None, None) is None and engine.check_group_hits(None, "max") is None
    assert engine.check_group_hits(1, "max") == 1 and engine.check_group_hits(np.int64(64), "sum") == 64
    assert engine.GROUP_HITS_MAX == 64
    for bad in (0, 65, -1, 2.5, "3", True):
        with pytest.raises(ValueError):
            engine.check_group_hits(bad, "max")
    with pytest.raises(ValueError, match="group_agg"):
        engine.check_group_hits(3, None)                                        # hits without groups
    for name in ("retrieve", "retrieve_scored", "dense_retrieve"):              # checked before the device is touched
        with pytest.raises(ValueError, match="group_agg"):
            getattr(engine.HippoRAGEngine, name)(object.__new__(engine.HippoRAGEngine), *([None] * (1 if "dense" in name else 4)),
                                                 group_hits=3)
    rag = object.__new__(HippoRAG)
    rag.global_config = RetrievalConfig()
    assert rag.global_config.group_hits is None and rag._hits(None, "max") is None and rag._hits(None, None) is None
    assert rag._hits(5, "sum") == 5
    with pytest.raises(ValueError):
        rag._hits(3, None)                                                      # group_hits without group_by
    with pytest.raises(ValueError):
        rag._hits(65, "max")
    rag.global_config = RetrievalConfig(group_by="source_id", group_hits=4)
    assert rag._hits(None, "max") == 4 and rag._hits(2, "max") == 2


def test_the_sharded_hybrid_and_captured_classes_refuse():
    from hipporag_amd import dist, engine
    for cls in (dist.ShardedRetriever, dist.NativeShardedRetriever):
        with pytest.raises(NotImplementedError, match="group_hits"):
            cls.retrieve(object.__new__(cls), None, None, None, None, group_hits=3)
        with pytest.raises(NotImplementedError, match="group_agg"):
            cls.retrieve(object.__new__(cls), None, None, None, None, group_agg="max", group_hits=3)
    with pytest.raises(NotImplementedError, match="group_hits"):
        dist.HybridRetriever.retrieve(object.__new__(dist.HybridRetriever), None, None, None, None, group_hits=1)
    with pytest.raises(NotImplementedError, match="group_hits"):
        engine.CapturedPipeline(None, 1, group_hits=3)
    with pytest.raises(NotImplementedError, match="group_agg"):
        engine.CapturedPipeline(None, 1, group_agg="max", group_hits=3)
