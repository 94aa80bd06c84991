"""The scoped doc filter's host side (no GPU): the mirror's fact -> source-passage table through index, incremental
index and delete, and the argument checks of the scope (unknown scope, no sources, the multi-GPU retrievers)."""

import numpy as np
import pytest

from hipporag_amd.retriever import Chunk, HippoRAG, RetrievalConfig, masked_minmax_rows, min_max_normalize
from tests.golden.make_golden import DOCS, TRIPLES, MockEmbeddingModel


def _table_as_sets(rag):
    row_ptr, pos = rag.fact_source_table()
    assert row_ptr.dtype == np.int64 and pos.dtype == np.int32
    assert row_ptr[0] == 0 and row_ptr[-1] == len(pos) and (np.diff(row_ptr) >= 0).all()
    return [set(pos[row_ptr[f]:row_ptr[f + 1]].tolist()) for f in range(len(rag.facts))]


def _expected(rag):
    """Restated from the stores: fact f's sources are the passages whose processed triples contain it."""
    want = [set() for _ in rag.facts]
    at = {f: i for i, f in enumerate(rag.facts)}
    for p, key in enumerate(rag.passage_node_keys):
        for t in rag._chunk_triples[key]:
            want[at[t]].add(p)
    return want


def _rag():
    return HippoRAG(RetrievalConfig(embedding_precision="bf16"), embedding_model=MockEmbeddingModel())


def test_fact_sources_follow_index_incremental_index_and_delete():
    rag = _rag()
    half = len(DOCS) // 2
    rag.index_from_openie(DOCS[:half], TRIPLES[:half])
    assert _table_as_sets(rag) == _expected(rag)
    # a second call: new chunks, a fact shared with an old chunk gains a source
    shared = TRIPLES[0][0]
    rag.index_from_openie(DOCS[half:] + ["A new note."], TRIPLES[half:] + [[shared]])
    got = _table_as_sets(rag)
    assert got == _expected(rag)
    f = rag.facts.index(tuple(x.lower() for x in shared))
    assert len(got[f]) >= 2
    # delete renumbers passages and facts: the table is rebuilt in the new numbering
    rag.delete([DOCS[1], DOCS[half]])
    assert _table_as_sets(rag) == _expected(rag)
    assert all(src for src in _table_as_sets(rag))          # every fact left has a source


def test_scope_argument_checks():
    rag = _rag()
    rag.index_from_openie(DOCS, TRIPLES)
    with pytest.raises(ValueError, match="filter_scope"):
        rag._scope("everything", {"a": 1})
    assert rag._scope(None, None) == "ranking"
    assert rag._scope("seeds", None) == "ranking"           # no filter: nothing to scope
    assert rag._scope("seeds", {"a": 1}) == "seeds"
    rag.global_config.doc_filter_scope = "seeds"
    assert rag._scope(None, {"a": 1}) == "seeds"
    # an index without recorded sources (from_arrays) refuses the scoped form instead of serving DPR for every query
    a = rag._arrays
    bare = HippoRAG.from_arrays(a["csr"], a["passage_vertex"], a["passage_emb"], a["fact_emb"], a["subj"], a["obj"],
                                a["num_chunks"])
    with pytest.raises(ValueError, match="source passages"):
        bare._scope("seeds", {"a": 1})


def test_engine_scope_checks_without_a_device():
    from hipporag_amd.engine import check_filter_scope
    with pytest.raises(ValueError, match="filter_scope"):
        check_filter_scope("tenant", object())
    with pytest.raises(ValueError, match="needs a doc_filter"):
        check_filter_scope("seeds", None)
    assert check_filter_scope("seeds", object()) and not check_filter_scope("ranking", None)


def test_multi_gpu_retrievers_refuse_the_seeds_scope():
    from hipporag_amd.dist import HybridRetriever, NativeShardedRetriever, ShardedRetriever, refuse_seeds_scope
    refuse_seeds_scope("ranking")
    with pytest.raises(ValueError, match="not supported"):
        refuse_seeds_scope("seeds")
    for cls in (ShardedRetriever, NativeShardedRetriever):
        r = cls.__new__(cls)                                 # the refusal comes before any device work
        with pytest.raises(ValueError, match="not supported"):
            r.retrieve(None, None, None, None, doc_filter=object(), filter_scope="seeds")
        with pytest.raises(ValueError, match="not supported"):
            r.score_facts(None, 5, scope_filter=object())
    h = HybridRetriever.__new__(HybridRetriever)
    with pytest.raises(ValueError, match="not supported"):
        h.retrieve(None, None, None, None, doc_filter=object(), filter_scope="seeds")
    with pytest.raises(ValueError, match="not supported"):
        h.score_facts(None, 5, scope_filter=object())


def test_masked_minmax_rows():
    rng = np.random.default_rng(0)
    raw = rng.standard_normal((4, 50)).astype(np.float32)
    allowed = rng.random((4, 50)) < 0.3
    allowed[1] = False
    allowed[2] = False
    allowed[2, 7] = True
    out = masked_minmax_rows(raw, allowed)
    assert (out[~allowed] == 0).all()
    assert (out[1] == 0).all() and out[2, 7] == 1.0
    for i in (0, 3):
        np.testing.assert_array_equal(out[i, allowed[i]], min_max_normalize(raw[i, allowed[i]]))


def test_chunks_with_metadata_feed_the_table():
    rag = _rag()
    rag.index_from_openie([Chunk(d, metadata={"tenant": i % 2}) for i, d in enumerate(DOCS)], TRIPLES)
    assert _table_as_sets(rag) == _expected(rag)
