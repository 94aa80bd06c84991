"""Late-interaction reranking off the device (include/hrag.h, "late-interaction reranking"): the symbols, the numpy
restatements against their naive loops, the checks of the option and of its two objects, LateQueries.select, every refusal by
name, the planted corpus on the CPU, and what the mirror's batch pipeline hands to the engine (a recording double)."""

import os
import re
import types

import numpy as np
import pytest

from tests.late_helpers import (PlantedEmbedder, PlantedTokenEncoder, exact_tokens, late_rank_naive, late_rank_np,
                                late_scores_naive, late_scores_np, planted_late_corpus, planted_texts, ragged)

NEW = ["hrag_late_create", "hrag_late_destroy", "hrag_late_scores", "hrag_late_rank_rows", "hrag_late_rerank"]


def test_symbols_are_declared_bound_and_exported():
    from hipporag_amd import _lib
    hdr = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "hrag.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and re.search(r"hrag_status " + name + r"\(", hdr) and getattr(lib, name) is not None
    assert "hrag_late_workspace_bytes" in _lib.SIGNATURES and re.search(r"int64_t hrag_late_workspace_bytes\(", hdr)
    assert lib.hrag_late_workspace_bytes is not None
    for name, value in (("DIM", _lib.LATE_MAX_DIM), ("QUERY_TOKENS", _lib.LATE_MAX_QUERY_TOKENS),
                        ("CANDIDATES", _lib.LATE_MAX_CANDIDATES)):
        assert int(re.search(rf"#define HRAG_LATE_MAX_{name} (\d+)", hdr).group(1)) == value, name
    assert (_lib.LATE_MAX_DIM, _lib.LATE_MAX_QUERY_TOKENS, _lib.LATE_MAX_CANDIDATES) == (256, 64, 1024)
    assert "late-interaction reranking" in hdr
    assert _lib.HRAG_VERSION == 8 and lib.hrag_version() == 8            # additive: the version does not move
    from hipporag_amd.csrc import build
    assert "late.hip" in build.SOURCES


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_vectorised_restatement_is_the_naive_loop(seed):
    """Zero-token passages and queries, empty slots, duplicate ids in a row, ties, a NaN token."""
    rng = np.random.default_rng(seed)
    dim = (8, 24, 40)[seed]
    p_tok = exact_tokens(rng, [0, 1, 15, 16, 17, 5, 0, 3], dim)
    q_tok = exact_tokens(rng, [0, 1, 17, 4], dim)
    p_tok[3][2, 1] = np.nan                                   # every s_ij of that token is NaN: ignored by the maximum
    p_tok[5] = p_tok[7][[0, 1, 2, 0, 1]].copy()               # passages 5 and 7 tie under every query
    n = len(p_tok)
    cand = rng.integers(-2, n + 3, size=(4, 11))
    cand[:, 3] = cand[:, 2]                                   # a duplicate id
    cand[:, 5], cand[:, 6] = 5, 7
    cand[:, 0], cand[:, 1], cand[:, 4] = 1, 2, 4                # live slots for the special scores below
    tok, qry = ragged(p_tok, dim), ragged(q_tok, dim)
    got, want = late_scores_np(*tok, *qry, cand), late_scores_naive(*tok, *qry, cand)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    live = (cand >= 0) & (cand < n)
    assert not got[~live].any() and not got[0].any()          # empty slots and the query without tokens read +0.0
    assert (got[1:, :][(cand[1:] == 0) | (cand[1:] == 6)] == -np.inf).all()   # passages without tokens
    assert np.array_equal(got[:, 5], got[:, 6])
    # the ranking: ties to the smaller slot, NaN above +inf, -0 ties +0
    s = got.copy()
    s[2, 0], s[2, 1], s[2, 4], s[3, 0], s[3, 1] = np.nan, np.inf, -0.0, 0.0, -0.0
    for k in (1, 4, 11):
        for n_ids in (n, 0):
            a, b = late_rank_np(s, cand, n_ids, k), late_rank_naive(s, cand, n_ids, k)
            for x, y in zip(a, b):
                assert np.array_equal(x, y, equal_nan=True), (k, n_ids)
    sel, idx, sc = late_rank_np(s, cand, n, 11)
    assert sel[2, 0] == 0 and np.isnan(sc[2, 0]) and sel[2, 1] == 1 and sc[2, 1] == np.inf
    first56 = [int(np.flatnonzero(sel[q] == 5)[0]) < int(np.flatnonzero(sel[q] == 6)[0]) for q in range(1, 4)]
    assert all(first56)                                       # the tie of slots 5 and 6 goes to slot 5
    assert (sel[0] == np.flatnonzero(live[0])[:11].tolist() + [-1] * (11 - live[0].sum())).all()   # all +0.0: slot order
    assert (idx[sel < 0] == -1).all() and not sc[sel < 0].any()


def test_check_late_and_late_plan():
    import torch
    from hipporag_amd.engine import check_late, late_plan, LateQueries
    rng = np.random.default_rng(0)
    lq = LateQueries.from_ragged(exact_tokens(rng, [2, 0, 5], 8), "bf16", device="cpu")
    assert lq.batch == 3 and lq.n_tokens == 7 and lq.q_ptr.tolist() == [0, 2, 2, 7] and lq.q_ptr.dtype == np.int32
    assert lq.q_tok.dtype == torch.bfloat16 and lq.q_ptr_dev.dtype == torch.int32
    assert late_plan(None, None, 5) is None
    with pytest.raises(ValueError, match="late_candidates needs late"):
        late_plan(None, 10, 5)
    assert late_plan(lq, None, 5) == (lq, 5) and late_plan(lq, 3, 5) == (lq, 5) and late_plan(lq, 40, 5) == (lq, 40)
    for c, name in ((1025, "late_candidates"), (True, "late_candidates"), (2.5, "late_candidates")):
        with pytest.raises(ValueError, match=name):
            late_plan(lq, c, 5)
    for k, name in ((0, "k=0"), (True, "k=True"), (1.5, "k=1.5")):
        with pytest.raises(ValueError, match=name):
            late_plan(lq, 10, k)
    with pytest.raises(ValueError, match="k=11: outside \\[1, late_candidates=10\\]"):
        check_late(lq, 11, 10)
    with pytest.raises(ValueError, match="late: a LateQueries expected"):
        late_plan((np.zeros(2), np.zeros(1)), 10, 5)
    with pytest.raises(ValueError, match="late: it holds 3 queries, the call 4"):
        check_late(lq, 1, 10, 4)


def test_token_index_and_late_queries_reject_malformed_input_by_name():
    """Everything is refused before a device is looked for."""
    import torch
    from hipporag_amd.late import LateQueries, TokenIndex, check_tok_ptr
    ok = [np.zeros((2, 8), np.float32), np.zeros((0, 8), np.float32)]
    for cls in (TokenIndex, LateQueries):
        for bad, what in (([np.zeros((2, 12), np.float32)], "dim=12"), ([np.zeros((2, 264), np.float32)], "LATE_MAX_DIM"),
                          ([np.zeros((2, 4), np.float32)], "dim=4"), ([np.zeros(8, np.float32)], r"arrays\[0\] has 1 dimensions"),
                          (ok + [np.zeros((1, 16), np.float32)], r"arrays\[2\] has dim 16, 8 expected"),
                          ([np.zeros((2, 8), np.int32)], "floating-point"), ([], "non-empty list")):
            with pytest.raises(ValueError, match=what):
                cls.from_ragged(bad, "bf16")
        with pytest.raises(ValueError, match="dtype='fp32'"):
            cls.from_ragged(ok, "fp32")
    with pytest.raises(ValueError, match="query 1 holds 65 tokens, at most LATE_MAX_QUERY_TOKENS=64"):
        LateQueries.from_ragged([np.zeros((64, 8), np.float32), np.zeros((65, 8), np.float32)], "fp16")
    emb = torch.zeros((5, 8), dtype=torch.bfloat16)
    for ptr, what in (([0, 3, 2, 5], "tok_ptr descends at entry 1"), ([1, 3, 5], r"tok_ptr\[0\] = 1"), ([0, 2, 4], "tok_ptr ends at 4"),
                      (np.zeros((2, 2), np.int64), "tok_ptr: a one-dimensional"), ([0.0, 5.0], "tok_ptr: a one-dimensional"),
                      ):
        with pytest.raises(ValueError, match=what):
            TokenIndex.from_csr(ptr, emb, "bf16")
        with pytest.raises(ValueError, match=what.replace("tok_ptr", "q_ptr")):
            LateQueries(ptr, emb, "bf16", device="cpu")
    with pytest.raises(ValueError, match="at least one passage"):
        TokenIndex.from_csr([0], emb[:0], "bf16")
    with pytest.raises(ValueError, match="tok_emb is torch.bfloat16, dtype='fp16'"):
        TokenIndex.from_csr([0, 5], emb, "fp16")
    with pytest.raises(ValueError, match="tok_emb: a torch bf16 tensor"):
        TokenIndex([0, 5], np.zeros((5, 8), np.float32), "bf16")
    assert check_tok_ptr(np.array([0, 0, 3], np.int32), 3).dtype == np.int64


def test_select_keeps_order_and_content():
    import torch
    from hipporag_amd.late import LateQueries
    rng = np.random.default_rng(4)
    lens = [3, 0, 5, 1, 64, 2]
    toks = exact_tokens(rng, lens, 16)
    for dtype in ("bf16", "fp16"):
        lq = LateQueries.from_ragged(toks, dtype, device="cpu")
        for rows in ([1, 2, 3, 5], [4], [5, 0, 0, 2], np.array([1]), range(6)):
            sub = lq.select(rows)
            rows = list(rows)
            assert sub.batch == len(rows) and sub.dtype == dtype and sub.dim == 16
            assert np.diff(sub.q_ptr).tolist() == [lens[r] for r in rows] and sub.q_ptr_dev.tolist() == sub.q_ptr.tolist()
            for i, r in enumerate(rows):
                got = sub.q_tok[sub.q_ptr[i]:sub.q_ptr[i + 1]].double().numpy()
                assert np.array_equal(got, toks[r]), (dtype, rows, i)
        for bad in ([], [6], [-1]):
            with pytest.raises(ValueError, match="rows"):
                lq.select(bad)
    assert torch.equal(lq.select(range(6)).q_tok, lq.q_tok)


def test_what_does_not_serve_late_refuses_it_by_name():
    from hipporag_amd.dist import HybridRetriever, NativeShardedRetriever, ShardedRetriever
    from hipporag_amd.engine import CapturedPipeline, HippoRAGEngine, LateQueries, refuse_late
    lq = LateQueries.from_ragged([np.zeros((2, 8), np.float32)], "bf16", device="cpu")
    refuse_late("X", {"late": None, "late_candidates": None, "boost": 1})
    for kw, name in ((dict(late=lq), "late"), (dict(late_candidates=50), "late_candidates")):
        with pytest.raises(NotImplementedError, match=f"X does not serve {name}:"):
            refuse_late("X", kw)
        for cls in (ShardedRetriever, NativeShardedRetriever, HybridRetriever):
            with pytest.raises(NotImplementedError, match=f"{cls.__name__} does not serve {name}:"):
                cls.retrieve(object.__new__(cls), None, None, None, None, **kw)
        with pytest.raises(NotImplementedError, match=f"CapturedPipeline does not serve {name}:"):
            CapturedPipeline(None, 1, **kw)
        with pytest.raises(NotImplementedError, match=f"shard_finish does not serve {name}:"):
            HippoRAGEngine.shard_finish(object(), None, None, None, 5, **kw)
    # the engine's own refusals: grouping, mmr_candidates, beyond max_topk, a row shard, no index, another index
    eng = types.SimpleNamespace(max_topk=50, _parent=None, device="cpu")
    fits = lambda *a, **k: HippoRAGEngine._check_late_fits(eng, *a, **k)
    fits(None, group_agg="max")
    fits((lq, 50), (0.5, 50))
    for kw, name in ((dict(group_agg="max"), "late does not serve group_agg"), (dict(group_hits=2), "late does not serve group_hits"),
                     (dict(mmr=(0.5, 60)), "late with mmr_candidates=60")):
        with pytest.raises(ValueError, match=name):
            fits((lq, 50), **kw)
    with pytest.raises(ValueError, match="late_candidates: the call would rank c = .* = 51 entries"):
        fits((lq, 51))
    shard = types.SimpleNamespace(n_rows=10, num_vertices=20, passage_rows=5, n_passages=5, _parent=None)
    with pytest.raises(NotImplementedError, match="set_token_index on a row-shard engine"):
        HippoRAGEngine.set_token_index(shard, types.SimpleNamespace(n_passages=5))
    whole = types.SimpleNamespace(n_rows=20, num_vertices=20, passage_rows=5, n_passages=5, _parent=None, device="cpu")
    with pytest.raises(ValueError, match="the token index covers 6 passages, the engine 5"):
        HippoRAGEngine.set_token_index(whole, types.SimpleNamespace(n_passages=6, device="cpu"))
    with pytest.raises(ValueError, match=r"late: no token index on this engine \(set_token_index\)"):
        HippoRAGEngine._token_ix(eng, lq)
    ix = types.SimpleNamespace(n_passages=5, device="cpu", dim=16, dtype="bf16", _handle=types.SimpleNamespace(value=1))
    HippoRAGEngine.set_token_index(whole, ix)
    child = types.SimpleNamespace(_parent=whole, device="cpu")             # a workspace handle reads its parent's index
    with pytest.raises(ValueError, match="late: the queries are bf16 of dim 8, the token index bf16 of dim 16"):
        HippoRAGEngine._token_ix(child, lq)
    HippoRAGEngine.set_token_index(whole, None)
    assert whole._token_index is None
    # dense_retrieve with the two options that rank once
    for kw in (dict(boost=[{"mul": 2.0}]), dict(lexical=(np.zeros(2, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)))):
        with pytest.raises(ValueError, match="does not serve late"):
            HippoRAGEngine.dense_retrieve(eng, None, k=5, late=lq, **kw)


class _Recorder:
    """An engine double for iter_batched_retrieve: records the keywords of every call and answers with tagged rows."""

    def __init__(self, max_batch, max_topk):
        self.max_batch, self.max_topk, self.calls = max_batch, max_topk, []
        self.device = "cpu"

    def retrieve_converged(self, q, kept_idx, kept_score, kept_count, **kw):
        import torch
        from hipporag_amd.engine import RetrieveOutput
        self.calls.append(kw)
        b, k = len(q), kw["k"]
        out = RetrieveOutput(torch.arange(k, dtype=torch.int32).repeat(b, 1), torch.full((b, k), 2.0), torch.zeros(b, dtype=torch.int32))
        if kw.get("late") is not None:
            out.first_score = torch.full((b, k), 0.25)
        if kw.get("mmr_lambda") is not None:
            out.mmr_value = torch.full((b, k), 0.5)
        return out


def _mirror(corpus, eng, **cfg):
    from hipporag_amd.retriever import HippoRAG, RetrievalConfig
    docs, triples, queries = planted_texts(corpus)
    enc = PlantedTokenEncoder(corpus)
    rag = HippoRAG(RetrievalConfig(max_batch=eng.max_batch, retrieval_top_k=eng.max_topk, **cfg),
                   embedding_model=PlantedEmbedder(corpus), token_encoder=enc)
    rag.index_from_openie(docs, triples)
    rag.engine, rag.ready_to_retrieve = eng, True
    rag._q_tensor = lambda qs, kind: list(qs)
    rag.get_query_embeddings = lambda qs: None
    rag.facts, rag.fact_node_keys = [], []
    return rag, enc, docs, queries


def test_the_mirror_hands_each_batch_its_own_late_queries():
    from hipporag_amd.engine import LateQueries
    corpus = planted_late_corpus(1)
    eng = _Recorder(4, 20)
    rag, enc, docs, queries = _mirror(corpus, eng)
    assert rag.retrieve(queries, num_to_retrieve=3)[0].doc_metadata[0] == {} and "late" not in eng.calls[0] and not enc.calls
    eng.calls.clear()
    sols = rag.retrieve(queries, num_to_retrieve=3, late_candidates=10)
    assert [texts for texts, is_q in enc.calls if not is_q] == [docs]                    # the passages once, by the cache
    assert [texts for texts, is_q in enc.calls if is_q] == [queries[:4], queries[4:]]    # every batch its own strings
    for kw, lo in zip(eng.calls, (0, 4)):
        lq = kw["late"]
        assert isinstance(lq, LateQueries) and kw["late_candidates"] == 10 and kw["k"] == 3 and "mmr_lambda" not in kw
        want = np.concatenate(corpus["q_tokens"][lo:lo + 4])
        assert np.array_equal(lq.q_tok.double().numpy(), want) and lq.batch == len(queries[lo:lo + 4])
    assert all(d == {"late_score": 2.0, "first_score": 0.25} for s in sols for d in s.doc_metadata) and len(sols[0].docs) == 3
    # the default of the config; MMR then picks among the late candidates
    enc.calls.clear()
    eng.calls.clear()
    rag.global_config.late_candidates = 15
    rag.retrieve(queries[:1], num_to_retrieve=3, mmr_lambda=0.5)
    kw = eng.calls[0]
    assert kw["late_candidates"] == 15 and kw["mmr_lambda"] == 0.5 and "mmr_candidates" not in kw
    assert not [1 for _, is_q in enc.calls if not is_q]                                   # nothing is encoded again
    rag.global_config.late_candidates = None
    # what the mirror refuses, by name
    with pytest.raises(ValueError, match="late_candidates=21 .* exceeds"):
        rag.retrieve(queries[:1], num_to_retrieve=21, late_candidates=5)
    with pytest.raises(ValueError, match=r"late_candidates=22 .* exceeds .* max_topk=20"):      # (the 22 passages there are)
        rag.retrieve(queries[:1], num_to_retrieve=3, late_candidates=500)
    for bad in (0, True, 2.5):
        with pytest.raises(ValueError, match="late_candidates="):
            rag.retrieve(queries[:1], num_to_retrieve=3, late_candidates=bad)
    with pytest.raises(ValueError, match="retrieve_fused does not serve late_candidates=7"):
        rag.retrieve_fused([[queries[0]]], late_candidates=7)
    with pytest.raises(ValueError, match="retrieve_ircot does not serve late_candidates=7"):
        rag.retrieve_ircot(queries[:1], 1, late_candidates=7)
    rag.chunk_metadata[rag.passage_node_keys[0]] = {"source_id": "a"}
    with pytest.raises(ValueError, match="late_candidates with group_by"):
        rag.retrieve(queries[:1], num_to_retrieve=3, late_candidates=5, group_by="source_id")
    rag.token_encoder = None
    for call in (rag.retrieve, rag.retrieve_dpr):
        with pytest.raises(ValueError, match=r"late_candidates=5\) needs HippoRAG\(token_encoder="):
            call(queries[:1], num_to_retrieve=3, late_candidates=5)
    # delete() drops the passage from the cache at the next build; index() encodes the new chunk only
    rag.token_encoder = enc
    enc.calls.clear()
    rag.delete([docs[3]])
    rag.engine, rag.ready_to_retrieve = eng, True
    rag.index_from_openie(["passage 3 again"], [[("ent3", "is", "thing3")]])
    rag.engine, rag.ready_to_retrieve = eng, True
    rag.facts, rag.fact_node_keys = [], []
    rag._build_late()
    assert enc.calls == [(["passage 3 again"], False)] and len(rag._token_cache) == len(docs)


def test_the_planted_corpus_needs_the_late_stage():
    """On the CPU: the single vectors rank the distractor first for every planted query, MaxSim the right passage."""
    for seed in (1, 5):
        c = planted_late_corpus(seed)
        n, dim = len(c["p_tokens"]), c["dim"]
        first = c["q_vec"].astype(np.float64) @ c["p_vec"].astype(np.float64).T
        assert np.array_equal(first.argmax(1), c["distractor"])
        assert (np.argsort(-first, axis=1)[:, 1] == c["right"]).all()                    # ... and the right one second
        cand = np.tile(np.arange(n), (len(c["q_tokens"]), 1))
        late = late_scores_np(*ragged(c["p_tokens"], dim), *ragged(c["q_tokens"], dim), cand)
        assert np.array_equal(late.argmax(1), c["right"])
        assert all(late[q, c["right"][q]] == len(c["q_tokens"][q]) for q in range(len(c["q_tokens"])))
        import torch                                                                     # exact in both 16-bit types
        for t in c["p_tokens"] + c["q_tokens"]:
            x = torch.from_numpy(np.asarray(t, np.float32))
            assert torch.equal(x.to(torch.bfloat16).float(), x) and torch.equal(x.to(torch.float16).float(), x)
