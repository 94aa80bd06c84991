"""Grouped retrieval, host side (no GPU): the numpy restatement pinned against "the full ranking with the repeats of a group
dropped", the package's host form against the restatement, and the mirror's surface -- the group table from
Chunk.source_id, its life across index / delete, validation, and the classes that refuse."""

import numpy as np
import pytest

from hipporag_amd.retriever import Chunk, HippoRAG, RetrievalConfig, group_rank_rows
from tests.group_helpers import dedup_full_ranking, group_rank_np, group_reduce_np, same_bits


def _case(rng):
    n = int(rng.integers(1, 60))
    n_groups = int(rng.integers(1, n + 1))
    g = rng.integers(0, n_groups, n).astype(np.int32)
    g[rng.permutation(n)[:n_groups]] = np.arange(n_groups)[: min(n, n_groups)]        # every group id carried
    # distinct values, then duplicates drawn INSIDE groups (most cases), so that group maxima rarely tie across groups
    s = rng.permutation(4 * n)[:n].astype(np.float32) / 4 - n / 2
    for _ in range(int(rng.integers(0, 4))):
        members = np.flatnonzero(g == rng.integers(0, n_groups))
        if len(members) > 1:
            a, b = rng.choice(members, 2, replace=False)
            s[a] = s[b]
    special = rng.random()
    if special < 0.3:
        at = rng.integers(0, n, 3)
        s[at[0]] = (np.nan, np.inf, -np.inf, -0.0, 0.0)[int(rng.integers(0, 5))]
        if special < 0.05:
            s[at[1]] = s[at[2]]                                                       # a duplicate anywhere
    mode = rng.random()
    allowed = None if mode < 0.4 else (np.zeros(n, bool) if mode < 0.45 else rng.random(n) < rng.random())
    return s, g, allowed, n_groups


def test_max_is_the_full_ranking_with_the_repeats_of_a_group_dropped():
    rng = np.random.default_rng(20261016)
    skipped, cases = 0, 2000
    for _ in range(cases):
        s, g, allowed, n_groups = _case(rng)
        k = int(rng.integers(1, len(s) + 2))
        want = dedup_full_ranking(s, g, allowed, k)
        if want is None:
            skipped += 1
            continue
        gi, gs, rep = group_rank_np(s, g, allowed, k, "max", n_groups)
        m = len(want[0])
        assert gi[:m].tolist() == want[0].tolist() and rep[:m].tolist() == want[2].tolist()
        assert same_bits(gs[:m], want[1])
        assert (gi[m:] == -1).all() and (rep[m:] == -1).all() and (gs[m:] == 0).all()
    assert skipped <= 0.10 * cases, skipped


def test_sum_is_a_sequential_fp64_loop_in_passage_order():
    rng = np.random.default_rng(5)
    for _ in range(200):
        s, g, allowed, n_groups = _case(rng)
        s = (s * rng.random(len(s)).astype(np.float32) * np.float32(1e-3)).astype(np.float32)
        gscore, gbest = group_reduce_np(s, g, allowed, n_groups, "sum")
        a = np.ones(len(s), bool) if allowed is None else allowed
        for grp in range(n_groups):
            acc, any_ = 0.0, False
            for p in range(len(s)):
                if g[p] == grp and a[p]:
                    acc, any_ = acc + float(s[p]), True
            assert (gbest[grp] >= 0) == any_
            assert same_bits(gscore[grp:grp + 1], np.array([np.float32(acc) if any_ else 0], np.float32))


def test_the_packages_host_form_is_the_restatement():
    rng = np.random.default_rng(9)
    for _ in range(300):
        s, g, allowed, n_groups = _case(rng)
        if int(g.max()) + 1 != n_groups:
            continue
        for agg in ("max", "sum"):
            for want in (1, 3, n_groups + 2):
                gi, gs, rep = group_rank_rows(s[None], g, None if allowed is None else allowed[None], want, agg)
                e = group_rank_np(s, g, allowed, want, agg, n_groups)
                if np.isnan(s).any() or (s == 0).any():        # the host form returns stored bits; the device canonical ones
                    assert gi[0].tolist() == e[0].tolist()
                    continue
                assert gi[0].tolist() == e[0].tolist() and rep[0].tolist() == e[2].tolist() and same_bits(gs[0], e[1])


# ------------------------------------------------------------------ mirror surface
class _Embedder:
    def batch_encode(self, texts, instruction=None, norm=True):
        texts = [texts] if isinstance(texts, str) else list(texts)
        out = np.stack([np.random.default_rng(abs(hash(t)) % 2 ** 32).standard_normal(16) for t in texts])
        return (out / np.linalg.norm(out, axis=1, keepdims=True)).astype(np.float32)


CHUNKS = [Chunk("Alice wrote the first report.", source_id="s1"), Chunk("Bob wrote the second report.", source_id="s2"),
          Chunk("Alice reviewed the budget.", source_id="s1"), Chunk("Carol filed a note."),
          Chunk("Bob and Carol met Alice.", source_id="s2"), Chunk("Dave left.")]
TRIPLES = [[("Alice", "wrote", "first report")], [("Bob", "wrote", "second report")], [("Alice", "reviewed", "budget")],
           [("Carol", "filed", "note")], [("Bob", "met", "Alice")], [("Dave", "left", "town")]]


def _mirror():
    rag = HippoRAG(RetrievalConfig(max_batch=4), embedding_model=_Embedder())
    rag.index_from_openie(list(CHUNKS), list(TRIPLES))
    return rag


def test_group_table_from_source_id_first_occurrence_order_and_singletons():
    rag = _mirror()
    group_of, values, sizes = rag.group_table("source_id")
    assert group_of.dtype == np.int32 and group_of.tolist() == [0, 1, 0, 2, 1, 3]
    assert values == ["s1", "s2", None, None] and sizes.tolist() == [2, 2, 1, 1]
    assert rag.group_table("source_id")[0] is group_of                       # cached
    extra = Chunk("Erin joined.", source_id="s2")
    rag.index_from_openie([extra], [[("Erin", "joined", "team")]])
    g2, v2, s2 = rag.group_table("source_id")
    assert g2.tolist() == [0, 1, 0, 2, 1, 3, 1] and s2.tolist() == [2, 3, 1, 1]
    rag.delete([CHUNKS[0].content, CHUNKS[2].content])                       # source s1 disappears: ids are reassigned
    g3, v3, s3 = rag.group_table("source_id")
    assert len(g3) == len(rag.passage_node_keys) == 5
    assert g3.tolist() == [0, 1, 0, 2, 0] and v3 == ["s2", None, None] and s3.tolist() == [3, 1, 1]


def test_int_array_form_and_validation():
    rag = _mirror()
    n = len(rag.passage_node_keys)
    group_of, values, sizes = rag.group_table(np.array([7, 7, 3, 3, 9, 7]))
    assert group_of.tolist() == [0, 0, 1, 1, 2, 0] and values == [7, 3, 9] and sizes.tolist() == [3, 2, 1]
    with pytest.raises(ValueError):
        rag.group_table(np.zeros(n + 1, np.int64))
    with pytest.raises(TypeError):
        rag.group_table(np.zeros(n, np.float32))
    with pytest.raises(TypeError):
        rag.group_table(3.5)
    with pytest.raises(ValueError):
        rag._grouping("source_id", "mean")
    with pytest.raises(ValueError):
        rag._grouping(None, "sum")                                           # an aggregation without groups
    assert rag._grouping(None, None) == (None, None)
    agg, table = rag._grouping("source_id", None)
    assert agg == "max" and table[0].tolist() == [0, 1, 0, 2, 1, 3]          # RetrievalConfig.group_agg
    cfg = RetrievalConfig(group_by="source_id", group_agg="sum")
    rag.global_config = cfg
    assert rag._grouping(None, None)[0] == "sum"


def test_the_sharded_hybrid_and_captured_classes_refuse():
    from hipporag_amd import dist, engine
    for cls in (dist.ShardedRetriever, dist.NativeShardedRetriever):
        with pytest.raises(NotImplementedError, match="group_agg"):
            cls.retrieve(object.__new__(cls), None, None, None, None, group_agg="max")
    with pytest.raises(NotImplementedError, match="group_agg"):
        dist.HybridRetriever.retrieve(object.__new__(dist.HybridRetriever), None, None, None, None, group_agg="sum")
    with pytest.raises(NotImplementedError, match="group_agg"):
        engine.CapturedPipeline(None, 1, group_agg="max")
    with pytest.raises(ValueError):
        engine.check_group_agg("mean")
    assert engine.check_group_agg(None) is None and engine.check_group_agg("max") == 0 and engine.check_group_agg("sum") == 1
