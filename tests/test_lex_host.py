"""Lexical retrieval, host side (hipporag_amd/lexical.py, the validators of hipporag_amd/engine.py, the mirror's argument
plumbing): nothing here touches a device."""

import math

import numpy as np
import pytest

from tests.lex_helpers import LEX_MAX_QUERY_TERMS, LEX_TILE, blend_np, lex_scores_np, same_bits


def test_the_constants_are_the_headers():
    import os
    import re
    from hipporag_amd import _lib, engine
    hdr = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "hrag.h")).read()
    assert int(re.search(r"#define HRAG_LEX_TILE (\d+)", hdr).group(1)) == LEX_TILE == _lib.LEX_TILE == engine.LEX_TILE
    cap = int(re.search(r"#define HRAG_LEX_MAX_QUERY_TERMS (\d+)", hdr).group(1))
    assert cap == LEX_MAX_QUERY_TERMS == _lib.LEX_MAX_QUERY_TERMS == engine.LEX_MAX_QUERY_TERMS and cap >= 64
    for name in ("hrag_lex_create", "hrag_lex_destroy", "hrag_lex_scores", "hrag_lex_blend_rows"):
        assert name in _lib.SIGNATURES and re.search(r"hrag_status " + name + r"\(", hdr)
    assert _lib.HRAG_VERSION == 8


# ---------------------------------------------------------------------------------- tokenizer, vocabulary, BM25
def test_default_tokenizer_is_lowercase_word_runs():
    from hipporag_amd.lexical import default_tokenize
    assert default_tokenize("Hello, World! it's A-1 x_y  42") == ["hello", "world", "it", "s", "a", "1", "x_y", "42"]
    assert default_tokenize("") == [] and default_tokenize("  ...  ") == []
    assert default_tokenize("Ünïcode Straße") == ["ünïcode", "straße"]


def test_bm25_weights_are_the_formula_per_passage_and_term():
    from hipporag_amd.lexical import bm25_weights, default_tokenize
    docs = ["the cat sat on the mat", "the dog", "", "cat cat cat dog bird", "a quick brown fox jumps over the lazy dog the end"]
    toks = [default_tokenize(d) for d in docs]
    for k1, b in ((1.2, 0.75), (0.9, 0.4), (2.0, 0.0), (1.2, 1.0)):
        m = bm25_weights(toks, k1, b)
        n = len(docs)
        avg = sum(len(t) for t in toks) / n
        assert m.avg_len == avg and m.doc_len.tolist() == [len(t) for t in toks]
        assert m.row_ptr[0] == 0 and m.row_ptr[-1] == len(m.term) == len(m.weight) and m.weight.dtype == np.float32
        for p, t in enumerate(toks):
            row = slice(int(m.row_ptr[p]), int(m.row_ptr[p + 1]))
            first = list(dict.fromkeys(t))                                       # order of first occurrence
            assert [m.vocab.tokens[j] for j in m.term[row]] == first
            for j, w in zip(m.term[row].tolist(), m.weight[row]):
                tok = m.vocab.tokens[j]
                df = sum(tok in d for d in toks)
                tf = float(t.count(tok))
                idf = math.log(1.0 + (n - df + 0.5) / (df + 0.5))
                want = idf * tf * (k1 + 1.0) / (tf + k1 * (1.0 - b + b * len(t) / avg))
                assert m.df[j] == df and m.idf[j] == idf
                assert np.float32(want).view(np.uint32) == w.view(np.uint32), (p, tok)
    empty = bm25_weights([[], []])
    assert empty.avg_len == 1.0 and len(empty.term) == 0 and len(empty.vocab) == 0
    assert len(bm25_weights([]).row_ptr) == 1


def test_encode_queries_order_counts_unknown_terms_and_cap():
    from hipporag_amd.lexical import LexicalModel, Vocabulary, encode_queries
    m = LexicalModel(["alpha beta gamma", "beta delta", "epsilon"])
    qp, qt, qw = m.encode_queries(["gamma unknown ALPHA gamma, gamma!", "", "nothing known", "delta"])
    assert qp.dtype == np.int32 and qt.dtype == np.int32 and qw.dtype == np.float32
    assert qp.tolist() == [0, 2, 2, 2, 3]
    v = m.vocab.id_of
    assert qt.tolist() == [v["gamma"], v["alpha"], v["delta"]] and qw.tolist() == [3.0, 1.0, 1.0]
    # the cap applies to DISTINCT known terms, after the repeats were merged, and keeps the first ones
    vocab = Vocabulary()
    for i in range(LEX_MAX_QUERY_TERMS + 44):
        vocab.add(f"t{i}")
    long_q = " ".join(f"t{i} t{i}" for i in range(LEX_MAX_QUERY_TERMS + 44))
    rep_q = " ".join(["t3 t1"] * 400)                                            # 800 tokens, two distinct terms
    qp, qt, qw = encode_queries([long_q, rep_q], vocab)
    assert qp.tolist() == [0, LEX_MAX_QUERY_TERMS, LEX_MAX_QUERY_TERMS + 2]
    assert qt[:LEX_MAX_QUERY_TERMS].tolist() == list(range(LEX_MAX_QUERY_TERMS)) and (qw[:LEX_MAX_QUERY_TERMS] == 2).all()
    assert qt[-2:].tolist() == [3, 1] and qw[-2:].tolist() == [400.0, 400.0]
    # a caller-supplied tokenizer replaces the default for passages and queries alike
    m2 = LexicalModel(["A-1 b-2"], tokenize_fn=lambda s: s.split())
    assert m2.vocab.tokens == ["A-1", "b-2"] and m2.encode_queries(["b-2 a-1"])[1].tolist() == [1]


def test_from_csr_inversion():
    from hipporag_amd.lexical import LexicalModel, invert_postings
    rng = np.random.default_rng(5)
    n, n_terms = 37, 11
    rows = [np.sort(rng.permutation(n_terms)[:rng.integers(0, 6)]) for _ in range(n)]
    rows = [rng.permutation(r) for r in rows]                                    # any order within a passage
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    term = np.concatenate(rows).astype(np.int32)
    w = rng.standard_normal(len(term)).astype(np.float32)
    ptr, doc, pw = invert_postings(n, n_terms, rp, term, w)
    assert ptr.dtype == np.int64 and doc.dtype == np.int32 and pw.dtype == np.float32 and ptr[0] == 0 and ptr[-1] == len(term)
    dense = np.zeros((n, n_terms), np.float32)
    for p in range(n):
        dense[p, term[rp[p]:rp[p + 1]]] = w[rp[p]:rp[p + 1]]
    for t in range(n_terms):
        d = doc[ptr[t]:ptr[t + 1]]
        assert (np.diff(d) > 0).all() and d.tolist() == np.flatnonzero(dense[:, t]).tolist()
        assert same_bits(pw[ptr[t]:ptr[t + 1]], dense[d, t])
    with pytest.raises(ValueError, match="repeated within passage 1"):
        invert_postings(2, 3, [0, 1, 4], [0, 2, 1, 2], [1, 1, 1, 1])
    with pytest.raises(ValueError, match="term ids"):
        invert_postings(1, 3, [0, 1], [3], [1.0])
    with pytest.raises(ValueError, match="row_ptr"):
        invert_postings(2, 3, [0, 2, 1], [0], [1.0])
    # the model's postings score like its passage-major weights
    m = LexicalModel(["red green", "green blue green", "blue"])
    ptr, doc, pw = m.postings()
    q = m.encode_queries(["green blue"])
    got = lex_scores_np(3, ptr, doc, pw, *q)[0]
    g, b_ = m.vocab.id_of["green"], m.vocab.id_of["blue"]
    want = np.zeros(3)
    for p in range(3):
        for j in range(int(m.bm25.row_ptr[p]), int(m.bm25.row_ptr[p + 1])):
            if m.bm25.term[j] in (g, b_):
                want[p] += float(m.bm25.weight[j])
    assert same_bits(got, want.astype(np.float32))


# ---------------------------------------------------------------------------------- the restatement itself
def test_the_restatement_follows_the_headers_rules():
    ptr = np.array([0, 2, 2, 3], np.int64)
    doc = np.array([0, 2, 2], np.int32)
    pw = np.array([1.5, -2.0, 4.0], np.float32)
    q = (np.array([0, 0, 3, 5, 6], np.int32), np.array([0, 2, 0, 7, -1, 0], np.int32),
         np.array([2.0, 0.5, 1.0, 9.0, 9.0, np.nan], np.float32))
    got = lex_scores_np(3, ptr, doc, pw, *q)
    assert same_bits(got[0], [0, 0, 0]) and same_bits(got[1], [4.5, 0, -4.0]) and same_bits(got[2], [0, 0, 0])
    assert np.isnan(got[3][[0, 2]]).all() and got[3][1] == 0 and (got[3].view(np.uint32)[[0, 2]] == 0x7FC00000).all()
    assert same_bits(lex_scores_np(3, ptr, doc, pw, *q, cap=1)[1], [3.0, 0, -4.0])          # terms beyond the cap are ignored
    dense = np.array([[1, 2, 3], [1, 2, 3], [5, 5, 5], [1, 2, 3]], np.float32)
    lex = np.array([[0, 0, 0], [0, 1, 4], [0, 1, 4], [np.nan, np.nan, np.nan]], np.float32)
    out = blend_np(dense, lex, 0.25)
    assert same_bits(out[0], dense[0]) and same_bits(out[3], dense[3])
    assert same_bits(out[1], np.float32([0.0, 0.75 * 0.5 + 0.25 * 0.25, 1.0]))
    assert same_bits(out[2], np.float32([0.75, 0.75 + 0.25 * 0.25, 1.0]))                   # a constant dense row: range 0 -> 1
    assert same_bits(blend_np(dense, lex, 0.0), dense)


# ---------------------------------------------------------------------------------- validators
def _triple(ptr=(0, 2, 3), term=(1, 2, 0), weight=(1.0, 2.0, 0.5)):
    return np.asarray(ptr, np.int32), np.asarray(term, np.int32), np.asarray(weight, np.float32)


def test_check_lexical_accepts_and_rejects():
    from hipporag_amd.engine import check_lexical, check_lexical_weight, refuse_lexical
    qp, qt, qw, a = check_lexical(_triple(), 0.3, 2)
    assert qp.tolist() == [0, 2, 3] and qt.tolist() == [1, 2, 0] and a == 0.3 and qw.dtype == np.float32
    assert check_lexical(_triple(), 0, None)[3] == 0.0 and check_lexical(_triple(), 1, 2)[3] == 1.0
    assert check_lexical(_triple((0, 0), (), ()), 0.5, 1)[1].shape == (0,)                # an empty query
    full = np.arange(LEX_MAX_QUERY_TERMS, dtype=np.int32)
    check_lexical((np.array([0, LEX_MAX_QUERY_TERMS], np.int32), full, full.astype(np.float32)), 0.5, 1)   # exactly the cap
    over = np.arange(LEX_MAX_QUERY_TERMS + 1, dtype=np.int32)
    bad = [
        (_triple(), -0.1, 2, "lexical_weight"), (_triple(), 1.5, 2, "lexical_weight"), (_triple(), float("nan"), 2, "lexical_weight"),
        (_triple(), "0.3", 2, "lexical_weight"), (_triple(), True, 2, "lexical_weight"), (_triple(), None, 2, "lexical_weight"),
        (_triple(), 0.3, 3, "q_ptr has 3 entries"),                                     # batch + 1 entries
        (_triple((1, 2, 3)), 0.3, 2, "q_ptr must run from 0"), (_triple((0, 2, 2)), 0.3, 2, "q_ptr must run from 0"),
        (_triple((0, 3, 2, 3), (1, 2, 0)), 0.3, 3, "must not decrease"),
        (_triple(term=(1, 2)), 0.3, 2, "q_term has 2 entries"),
        ((np.array([0, 2, 3], np.int64),) + _triple()[1:], 0.3, 2, "q_ptr has dtype int64"),
        ((_triple()[0], np.array([1, 2, 0], np.int64), _triple()[2]), 0.3, 2, "q_term has dtype int64"),
        (_triple()[:2] + (np.array([1, 2, 0.5], np.float64),), 0.3, 2, "q_weight has dtype float64"),
        ((_triple()[0].reshape(1, 3),) + _triple()[1:], 0.3, 2, "one-dimensional"),
        ((np.array([0, LEX_MAX_QUERY_TERMS + 1], np.int32), over, over.astype(np.float32)), 0.3, 1, "LEX_MAX_QUERY_TERMS"),
        (_triple()[:2], 0.3, 2, "triple"), (None, 0.3, 2, "triple"), (([0, 2, 3], [1, 2, 0], [1.0, 2.0, 0.5]), 0.3, 2, "numpy array"),
    ]
    for lexical, w, b, msg in bad:
        with pytest.raises(ValueError, match=msg):
            check_lexical(lexical, w, b)
    assert check_lexical_weight(np.float32(0.5)) == 0.5
    refuse_lexical("X", {"lexical": None, "lexical_weight": 0.0, "group_agg": "max"})
    with pytest.raises(NotImplementedError, match="X does not serve lexical"):
        refuse_lexical("X", {"lexical": _triple()})
    with pytest.raises(NotImplementedError, match="lexical_weight"):
        refuse_lexical("X", {"lexical_weight": 0.3})


# ---------------------------------------------------------------------------------- refusals
def test_the_multi_gpu_retrievers_and_the_captured_pipeline_refuse_by_name():
    """The refusal is the first thing each call does: no engine, communicator or device is needed to reach it."""
    from hipporag_amd import dist
    from hipporag_amd.engine import CapturedPipeline
    for cls in (dist.ShardedRetriever, dist.NativeShardedRetriever, dist.HybridRetriever):
        obj = object.__new__(cls)
        for kw, name in ((dict(lexical=_triple()), "lexical"), (dict(lexical_weight=0.5), "lexical_weight")):
            with pytest.raises(NotImplementedError, match=f"{cls.__name__} does not serve {name}"):
                obj.retrieve(None, None, None, None, **kw)
    with pytest.raises(NotImplementedError, match="CapturedPipeline does not serve lexical"):
        CapturedPipeline(None, 1, lexical=_triple())


def _bare_engine(**attrs):
    from hipporag_amd.engine import HippoRAGEngine
    eng = object.__new__(HippoRAGEngine)
    eng.__dict__.update(dict(n_passages=10, passage_rows=10, n_rows=5, num_vertices=5, _lexical_index=None), **attrs)
    return eng


def test_the_engine_refuses_what_lexical_does_not_serve():
    eng = _bare_engine()
    lex = _triple()
    mask = object()                                           # never looked at: the refusal comes first
    for call in (lambda: eng.retrieve(None, None, None, None, lexical=lex, doc_filter=mask, filter_scope="seeds"),
                 lambda: eng.retrieve_scored(None, None, None, None, lexical=lex, doc_filter=mask, filter_scope="seeds")):
        with pytest.raises(NotImplementedError, match='filter_scope="seeds" is not served with lexical'):
            call()
    for kw, name in ((dict(group_agg="max"), "group_agg"), (dict(group_agg="max", group_hits=2), "group_agg"),
                     (dict(group_hits=2), "group_hits"), (dict(mmr_lambda=0.5), "mmr_lambda"),
                     (dict(mmr_candidates=9), "mmr_candidates"),
                     (dict(doc_filter=mask, filter_scope="seeds"), 'filter_scope="seeds"')):
        with pytest.raises(ValueError, match=f"dense_retrieve\\(lexical=\\) does not serve {name}"):
            eng.dense_retrieve(None, lexical=lex, **kw)
    # no index set; a row-shard engine cannot take one
    with pytest.raises(ValueError, match="set_lexical_index"):
        eng.lexical_scores(*lex)
    with pytest.raises(ValueError, match="set_lexical_index"):
        eng.lexical_retrieve(lex, 3)
    with pytest.raises(NotImplementedError, match="row-shard"):
        _bare_engine(n_rows=3).set_lexical_index(object())
    # the sparse queries are checked before anything is enqueued
    with pytest.raises(ValueError, match="q_weight has dtype float64"):
        eng.lexical_scores(lex[0], lex[1], lex[2].astype(np.float64))


# ---------------------------------------------------------------------------------- the mirror
class _Out:
    def __init__(self, b, k):
        import torch
        self.doc_idx = torch.arange(k, dtype=torch.int32).repeat(b, 1)
        self.doc_score = torch.ones((b, k))
        self.flags = torch.zeros(b, dtype=torch.int32)


class _Double:
    """An engine with the one-call form only: records what phase B was called with."""
    max_batch, max_topk = 2, 4

    def __init__(self):
        self.calls = []

    def retrieve_converged(self, *args, **kw):
        self.calls.append(kw)
        return _Out(args[0].shape[0], kw["k"])


def _run_mirror_body(**extra):
    import torch
    from hipporag_amd.retriever import iter_batched_retrieve
    eng = _Double()
    qs = ["alpha beta", "gamma", "beta beta"]
    rows = [r for _, rs in iter_batched_retrieve(eng, qs, lambda q, kind: torch.zeros((len(q), 8)), [], None, linking_top_k=5,
                                                 damping=0.5, passage_node_weight=0.05, ppr_iters=20, num_to_retrieve=3,
                                                 n_passages=6, **extra) for r in rs]
    assert len(rows) == 3
    return eng.calls


def test_lexical_weight_zero_leaves_the_mirrors_call_arguments_unchanged():
    from hipporag_amd.lexical import LexicalModel
    from hipporag_amd.retriever import HippoRAG, RetrievalConfig
    cfg = RetrievalConfig()
    assert cfg.lexical_weight == 0.0 and cfg.lexical_tokenize_fn is None
    rag = HippoRAG(cfg)
    assert rag._lexical(None) == {} and rag._lexical(0) == {} and getattr(rag, "lexical_model", None) is None
    model = LexicalModel(["alpha beta", "gamma delta"])
    plain = _run_mirror_body()
    zero = _run_mirror_body(lexical_encode=model.encode_queries, lexical_weight=0.0)
    assert [sorted(c) for c in zero] == [sorted(c) for c in plain] and all("lexical" not in c for c in zero)
    assert [{k: v for k, v in c.items()} for c in zero] == plain
    on = _run_mirror_body(lexical_encode=model.encode_queries, lexical_weight=0.25)
    assert len(on) == 2 and all(c["lexical_weight"] == 0.25 for c in on)
    assert on[0]["lexical"][0].tolist() == [0, 2, 3] and on[1]["lexical"][0].tolist() == [0, 1]      # batch by batch
    assert on[1]["lexical"][1].tolist() == [model.vocab.id_of["beta"]] and on[1]["lexical"][2].tolist() == [2.0]
    assert [{k: v for k, v in c.items() if not k.startswith("lexical")} for c in on] == plain
    with pytest.raises(NotImplementedError, match='filter_scope="seeds" is not served with lexical_weight'):
        _run_mirror_body(lexical_encode=model.encode_queries, lexical_weight=0.25, doc_filter=np.ones(1, np.uint32),
                         filter_scope="seeds")


def test_the_mirror_validates_and_refuses_without_touching_the_device():
    from hipporag_amd.retriever import HippoRAG, RetrievalConfig
    rag = HippoRAG(RetrievalConfig())
    for w in (-0.1, 1.5, float("nan"), "0.5", True):
        with pytest.raises(ValueError, match="lexical_weight"):
            rag._lexical(w)
    on = HippoRAG(RetrievalConfig(lexical_weight=0.4))
    with pytest.raises(ValueError, match="retrieve_fused does not serve lexical_weight=0.4"):
        on.retrieve_fused([["a"]])
    rag._refuse_lexical("retrieve_fused")
    # the mirror builds the model from the passages it holds (an engine without set_lexical_index gets the model only)
    on.passage_texts = ["alpha beta", "gamma"]
    on.engine = object()
    plan = on._lexical(None)
    assert plan["lexical_weight"] == 0.4 and on.lexical_model.vocab.tokens == ["alpha", "beta", "gamma"]
    assert on.lexical_index is None and plan["lexical_encode"](["gamma"])[1].tolist() == [2]
    sols = [type("S", (), {"doc_metadata": [{}, {"x": 1}]})()]
    HippoRAG._lexical_metadata(sols, plan)
    assert sols[0].doc_metadata == [{"lexical_weight": 0.4}, {"x": 1, "lexical_weight": 0.4}]
    HippoRAG._lexical_metadata(sols, {})
