"""Recommend by example on the host (include/hrag.h, "recommend by example"): the numpy restatement of tests/reco_helpers.py
held to a brute-force fp64 statement of Qdrant's formulas on dyadic inputs, the ordered-sum case, the argument checks of
Examples, the refusals by name, and the mirror's plumbing against an engine double."""

import re
import types

import numpy as np
import pytest

from tests.reco_helpers import (COUNTS, all_bits, effective_sign, exclude_np, make_examples, ordered_sum_case, query_bits,
                                reco_query_np, reco_rows_np, same_bits, tree_sum_rows_np)

NEW = ("hrag_reco_rows", "hrag_reco_workspace_bytes", "hrag_reco_scores_rows", "hrag_reco_scores", "hrag_reco_query",
       "hrag_reco_exclude")


def test_header_and_binding_agree():
    import os
    from hipporag_amd import _lib
    hdr = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "hrag.h")).read()
    for name, value in (("HRAG_RECO_MAX_EXAMPLES", _lib.RECO_MAX_EXAMPLES), ("HRAG_RECO_TILE", _lib.RECO_TILE),
                        ("HRAG_RECO_BEST_SCORE", _lib.RECO_BEST_SCORE), ("HRAG_RECO_SUM_SCORES", _lib.RECO_SUM_SCORES),
                        ("HRAG_RECO_AVERAGE_VECTOR", _lib.RECO_AVERAGE_VECTOR)):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == value, name
    for name in NEW:
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\(", hdr), name
        n_args = len(re.search(rf"\b{name}\(([^;]*?)\);", hdr, re.S).group(1).split(","))
        assert n_args == len(_lib.SIGNATURES[name][1]), name


def _dyadic(rng, n, dim):
    return rng.integers(-3, 4, (n, dim)).astype(np.float64) / 8


def test_the_restatement_is_qdrants_formulas_on_dyadic_inputs():
    """every product and sum exact: any order, any precision gives the same number"""
    rng = np.random.default_rng(0)
    n, dim = 40, 24
    x = _dyadic(rng, n, dim)
    ptr, idx, sign = make_examples(rng, n, COUNTS + [(2, 2)])
    eff = effective_sign(idx, sign, n)
    s = (x[np.where(eff != 0, idx, 0)] @ x.T).astype(np.float32)
    best, total = reco_rows_np(s, ptr, eff, "best_score"), reco_rows_np(s, ptr, eff, "sum_scores")
    values_v, flags = reco_query_np(x, ptr, idx, sign)
    for q in range(len(ptr) - 1):
        ex = [(int(idx[e]), int(eff[e])) for e in range(ptr[q], ptr[q + 1]) if eff[e]]
        pos, neg = [i for i, sg in ex if sg > 0], [i for i, sg in ex if sg < 0]
        for p in range(n):
            sim = lambda i: float(np.dot(x[i], x[p]))                       # noqa: E731
            bp = max([sim(i) for i in pos], default=-np.inf)
            bn = max([sim(i) for i in neg], default=-np.inf)
            want = bp if bp > bn else -(bn * bn)                            # Qdrant's best_score
            assert best[q, p] == np.float32(want), (q, p)
            assert total[q, p] == np.float32(sum(sim(i) for i in pos) - sum(sim(i) for i in neg)), (q, p)
        if pos:                                                             # Qdrant's average_vector
            a = np.mean(x[pos], axis=0)
            want_v = a + (a - np.mean(x[neg], axis=0)) if neg else a
            assert flags[q] == 0 and np.allclose(values_v[q], want_v, rtol=1e-6, atol=0)
        else:
            assert flags[q] == 1 and not values_v[q].any()
    assert flags[1] == 1 and np.isneginf(reco_rows_np(s[:0], [0, 0], eff[:0], "best_score")).all()
    # the batch is the queries one by one
    for q in range(len(ptr) - 1):
        one = reco_rows_np(s[ptr[q]:ptr[q + 1]], [0, ptr[q + 1] - ptr[q]], eff[ptr[q]:ptr[q + 1]], "best_score")
        assert same_bits(one[0], best[q])
    # the three-step composition -- gather the example rows (an empty id: a zero row), the [E, n] matrix query by query as
    # the similarity restatement forms it, the reduce with the empties' signs 0 -- against the fused statement written
    # directly from the ids: one pass over (query, passage) that forms each s(p, e) where it is consumed and never
    # holds a matrix
    ok = (idx >= 0) & (idx < n)
    gathered = np.where(ok[:, None], x[np.where(ok, idx, 0)], 0.0)
    matrix = np.stack([np.array([np.dot(x[p], gathered[e]) for p in range(n)]) for e in range(len(idx))]).astype(np.float32)
    three = {m: reco_rows_np(matrix, ptr, np.where(ok, np.sign(sign), 0), m) for m in ("best_score", "sum_scores")}
    for q in range(len(ptr) - 1):
        for p in range(n):
            bp = bn = np.float32(-np.inf)
            acc_p, acc_n = [], []
            for e in range(ptr[q], ptr[q + 1]):
                if not (0 <= idx[e] < n) or sign[e] == 0:
                    continue
                v = np.float32(np.dot(x[p], x[idx[e]]))
                if sign[e] > 0:
                    bp = v if v > bp else bp
                    acc_p.append(float(v))
                else:
                    bn = v if v > bn else bn
                    acc_n.append(float(v))
            acc = 0.0
            for v in acc_p:
                acc += v
            for v in acc_n:
                acc -= v
            assert same_bits(three["best_score"][q, p], bp if bp > bn else -(bn * bn)), (q, p)
            assert same_bits(three["sum_scores"][q, p], np.float32(acc)), (q, p)


def test_special_values_of_the_reduce():
    s = np.array([[np.nan, 1.0, -0.0, -2.0, np.inf], [0.5, np.nan, 0.0, -1.0, 1.0], [2.0, 2.0, -1.0, np.nan, np.inf]], np.float32)
    sign = np.array([1, 1, -1])
    best = reco_rows_np(s, [0, 3], sign, "best_score")
    # a NaN is never taken; -0 then +0: the first stays; positives all below the negative: -(bn^2); inf ties: -(inf^2)
    assert same_bits(best[0], np.array([-4.0, -4.0, -0.0, -1.0, -np.inf], np.float32))
    total = reco_rows_np(s, [0, 3], sign, "sum_scores")
    assert np.isnan(total[0, 0]) and total[0, 0].view(np.uint32) == 0x7fc00000 and total[0, 2] == 1.0 and np.isnan(total[0, 4])
    assert same_bits(reco_rows_np(s, [0, 3], np.array([0, 0, 0]), "sum_scores")[0], np.zeros(5, np.float32))


def test_the_ordered_sum_differs_from_a_tree_in_the_last_bit():
    sc, in_order, tree = ordered_sum_case()
    rows = sc[:, None].copy()
    ptr, sign = [0, 4], np.ones(4, np.int32)
    a, b = reco_rows_np(rows, ptr, sign, "sum_scores")[0, 0], tree_sum_rows_np(rows, ptr, sign)[0, 0]
    assert a == in_order and b == tree and abs(int(a.view(np.uint32)) - int(b.view(np.uint32))) == 1
    acc = 0.0
    for v in sc:
        acc += float(v)
    assert np.float32(acc) == in_order and np.float32((float(sc[0]) + float(sc[1])) + (float(sc[2]) + float(sc[3]))) == tree
    from hipporag_amd.graph import bf16_bits_to_float, float_to_bf16_bits
    assert np.array_equal(bf16_bits_to_float(float_to_bf16_bits(sc)), sc)       # bf16 holds every value


def test_query_bits_and_exclusion_restatements():
    v = np.array([[1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, -0.3, 0.0]], np.float32)
    assert query_bits("bf16", v).tolist() == [[0x3f80, 0x3f80, 0x3f82, 0xbe9a, 0]]          # ties to even, both ways
    assert query_bits("fp16", v)[0, 0] == 0x3c00 and query_bits("split", v).shape == (1, 15)
    s = query_bits("split", v).view(np.float16).astype(np.float64)
    assert np.array_equal(s[:, :5], s[:, 5:10]) and np.abs(s[0, :5] + s[0, 10:] - v[0]).max() <= 2.0 ** -22
    n = 70
    w = all_bits(2, n)
    assert w.shape == (2, 3) and w[0, 2] == 0x3f
    ptr, idx, sign = [0, 4, 6], np.array([0, 31, 32, 69, 64, 200]), np.array([1, -1, 1, 1, 0, 1])
    got = exclude_np(w, ptr, idx, sign, n)
    assert got[0].tolist() == [0x7ffffffe, 0xfffffffe, 0x1f] and got[1].tolist() == w[1].tolist() and w[0, 0] == 0xffffffff


def test_examples_argument_checking():
    from hipporag_amd.reco import Examples, check_examples, check_feedback_weight, check_strategy
    e = Examples.from_lists([[3, 4], [5], []], [[9], [], [7, 7]], device="cpu")
    assert e.batch == 3 and e.n_examples == 6 and e.ex_ptr.tolist() == [0, 3, 4, 6]
    assert e.ex_idx_host.tolist() == [3, 4, 9, 5, 7, 7] and e.ex_sign_host.tolist() == [1, 1, -1, 1, -1, -1]
    assert e.ex_ptr_dev.tolist() == e.ex_ptr.tolist() and e.ex_idx.tolist() == e.ex_idx_host.tolist()
    assert Examples.from_lists([[1]], device="cpu").ex_sign_host.tolist() == [1]
    assert Examples.from_lists([[-1, 2 ** 31 - 1]], device="cpu").n_examples == 2           # empty ids are legal
    sub = e.select([2, 0, 2])
    assert sub.ex_ptr.tolist() == [0, 2, 5, 7] and sub.ex_idx_host.tolist() == [7, 7, 3, 4, 9, 7, 7]
    assert sub.ex_sign_host.tolist() == [-1, -1, 1, 1, -1, -1, -1]
    for bad in ([], [3], [-1]):
        with pytest.raises(ValueError, match="rows"):
            e.select(bad)
    with pytest.raises(ValueError, match="query 0 holds 33 examples, at most RECO_MAX_EXAMPLES=32"):
        Examples.from_lists([list(range(20))], [list(range(13))], device="cpu")
    assert Examples.from_lists([list(range(20))], [list(range(12))], device="cpu").n_examples == 32
    with pytest.raises(ValueError, match="query 1 holds no example"):
        Examples.from_lists([[1], []], [[2], []], device="cpu")
    with pytest.raises(ValueError, match="negative holds 1 queries, positive 2"):
        Examples.from_lists([[1], [2]], [[2]], device="cpu")
    with pytest.raises(ValueError, match="integer passage ids"):
        Examples.from_lists([[1.5]], device="cpu")
    with pytest.raises(ValueError, match="must fit int32"):
        Examples.from_lists([[2 ** 31]], device="cpu")
    for args, what in ((([1, 2], [0], [1]), r"ex_ptr\[0\] = 1"), (([0, 2, 1], [0, 1], [1, 1]), "ex_ptr descends"),
                       (([0, 1], [0, 1], [1, 1]), "ex_ptr\\[-1\\] = 1 entries"), (([0, 1], [0], [2]), "ex_sign"),
                       (([0, 0], [], []), "holds no example"), (([0], [], []), "B \\+ 1 entries")):
        with pytest.raises(ValueError, match=what):
            Examples(*[np.asarray(a, np.int64) for a in args], device="cpu")
    assert Examples([0, 2], [5, 6], [0, -1], device="cpu").ex_sign_host.tolist() == [0, -1]  # the CSR form takes a sign 0
    with pytest.raises(ValueError, match="an Examples expected"):
        check_examples([[1]])
    with pytest.raises(ValueError, match="feedback: it holds 3 queries, the call 2"):
        check_examples(e, 2, "feedback")
    assert check_strategy("sum_scores") == 1 and check_strategy("average_vector") == 2
    with pytest.raises(ValueError, match="produces a query"):
        check_strategy("average_vector", True)
    with pytest.raises(ValueError, match="strategy='max'"):
        check_strategy("max")
    assert check_feedback_weight(0) == 0.0 and check_feedback_weight(1) == 1.0
    for bad in (-0.1, 1.01, True, "0.3", float("nan")):
        with pytest.raises(ValueError, match="feedback_weight="):
            check_feedback_weight(bad)


def test_what_does_not_serve_recommend_refuses_it_by_name():
    from hipporag_amd.dist import HybridRetriever, NativeShardedRetriever, ShardedRetriever
    from hipporag_amd.engine import CapturedPipeline, Examples, HippoRAGEngine, refuse_reco
    e = Examples.from_lists([[1]], device="cpu")
    refuse_reco("X", {"feedback": None, "recommend": None, "late": 1})
    for kw, name in ((dict(feedback=e), "feedback"), (dict(recommend=e), "recommend")):
        with pytest.raises(NotImplementedError, match=f"X does not serve {name}:"):
            refuse_reco("X", kw)
        for cls in (ShardedRetriever, NativeShardedRetriever, HybridRetriever):
            with pytest.raises(NotImplementedError, match=f"{cls.__name__} does not serve {name}:"):
                cls.retrieve(object.__new__(cls), None, None, None, None, **kw)
        with pytest.raises(NotImplementedError, match=f"CapturedPipeline does not serve {name}:"):
            CapturedPipeline(None, 1, **kw)
        with pytest.raises(NotImplementedError, match=f"shard_finish does not serve {name}:"):
            HippoRAGEngine.shard_finish(object(), None, None, None, 5, **kw)
    shard = types.SimpleNamespace(n_rows=10, num_vertices=20, passage_rows=5, n_passages=5, device=e.device, max_batch=4)
    with pytest.raises(NotImplementedError, match="recommend on a row-shard engine"):
        HippoRAGEngine._reco_args(shard, e)
    whole = types.SimpleNamespace(n_rows=20, num_vertices=20, passage_rows=5, n_passages=5, device=e.device, max_batch=1)
    assert HippoRAGEngine._reco_args(whole, e)[-1] == 1
    with pytest.raises(ValueError, match="2 queries, the engine serves at most max_batch=1"):
        HippoRAGEngine._reco_args(whole, Examples.from_lists([[1], [2]], device="cpu"))
    with pytest.raises(ValueError, match="the examples live on cpu, the engine on cuda:0"):
        HippoRAGEngine._reco_args(types.SimpleNamespace(device="cuda:0"), e)
    # the row strategies refuse what they do not serve before anything else; feedback and lexical both own the blend
    def enqueues(*a, **k):
        raise AssertionError("something was enqueued before the refusal")
    eng = types.SimpleNamespace(recommend_filter=enqueues, recommend_scores=enqueues, recommend_query=enqueues,
                                _reco_args=lambda ex: HippoRAGEngine._reco_args(whole, ex))
    for kw, name in ((dict(group_agg="max"), "group_agg"), (dict(group_hits=3), "group_hits"), (dict(boost=[{"mul": 2.0}]), "boost"),
                     (dict(lexical=(0, 0, 0)), "lexical")):
        for strategy in ("best_score", "sum_scores"):
            with pytest.raises(ValueError, match=rf"recommend\(strategy='{strategy}'\) does not serve {name}: .* retrieve_scored"):
                HippoRAGEngine.recommend(eng, e, strategy=strategy, **kw)
    with pytest.raises(ValueError, match="feedback together with lexical"):
        HippoRAGEngine.retrieve(eng, None, None, None, None, feedback=e, lexical=(0, 0, 0))


class _Recorder:
    """An engine double for the mirror: records the keywords of every call and answers with tagged rows."""

    def __init__(self, max_batch, max_topk):
        self.max_batch, self.max_topk, self.calls, self.reco = max_batch, max_topk, [], []
        self.device = "cpu"

    def retrieve_converged(self, q, kept_idx, kept_score, kept_count, **kw):
        import torch
        from hipporag_amd.engine import RetrieveOutput
        self.calls.append(kw)
        b, k = len(q), kw["k"]
        return RetrieveOutput(torch.arange(k, dtype=torch.int32).repeat(b, 1), torch.full((b, k), 2.0), torch.zeros(b, dtype=torch.int32))

    def recommend(self, examples, **kw):
        import torch
        self.reco.append((examples, kw))
        b, k = examples.batch, kw["k"]
        idx = torch.arange(k, dtype=torch.int32).repeat(b, 1)
        idx[:, -1] = -1                                          # fewer allowed passages than k
        out = (idx, torch.full((b, k), 0.5))
        return out + ((torch.full((b, k), 0.25),) if kw.get("mmr_lambda") is not None else ())


def _mirror(eng, **cfg):
    from hipporag_amd.retriever import HippoRAG, RetrievalConfig
    from tests.late_helpers import PlantedEmbedder, planted_late_corpus, planted_texts
    corpus = planted_late_corpus(1)
    docs, triples, queries = planted_texts(corpus)
    rag = HippoRAG(RetrievalConfig(max_batch=eng.max_batch, retrieval_top_k=eng.max_topk, **cfg), embedding_model=PlantedEmbedder(corpus))
    rag.index_from_openie(docs, triples)
    rag.engine, rag.ready_to_retrieve = eng, True
    rag._q_tensor = lambda qs, kind: list(qs)
    rag.get_query_embeddings = lambda qs: None
    rag.facts, rag.fact_node_keys = [], []
    return rag, list(rag.passage_texts), queries


def test_the_mirror_maps_documents_to_examples_and_hands_each_batch_its_own():
    from hipporag_amd.reco import Examples
    eng = _Recorder(4, 20)
    rag, docs, queries = _mirror(eng)
    keys = rag.passage_node_keys
    n_q = len(queries)
    assert n_q > 4
    like = [[docs[q], keys[q + 1]] for q in range(n_q)]
    unlike = [[docs[q + 2]] if q % 2 else [] for q in range(n_q)]
    # recommend: per-query lists of strings or hash ids -> positions; batches of max_batch; -1 entries dropped
    sols = rag.recommend(like, unlike, num_to_retrieve=5, strategy="sum_scores", exclude_examples=False, mmr_lambda=0.5)
    assert [ex.batch for ex, _ in eng.reco] == [4, n_q - 4]
    got = np.concatenate([ex.ex_idx_host for ex, _ in eng.reco]).tolist()
    assert got == [i for q in range(n_q) for i in [q, q + 1] + ([q + 2] if q % 2 else [])]
    assert np.concatenate([ex.ex_sign_host for ex, _ in eng.reco]).tolist() == [sg for q in range(n_q) for sg in [1, 1] + ([-1] if q % 2 else [])]
    assert all(kw == dict(k=5, strategy="sum_scores", doc_filter=None, exclude_examples=False, mmr_lambda=0.5) for _, kw in eng.reco)
    assert len(sols) == n_q and all(s_.question is None and s_.docs == docs[:4] and len(s_.doc_scores) == 4 for s_ in sols)
    assert all(d == {"recommended": "sum_scores", "mmr_value": 0.25} for s_ in sols for d in s_.doc_metadata)
    eng.reco.clear()
    rag.recommend(like[:1])
    assert eng.reco[0][1]["strategy"] == "best_score" and eng.reco[0][1]["k"] == 20 and eng.reco[0][1]["exclude_examples"] is True
    rag.global_config.recommend_strategy = "average_vector"
    rag.recommend(like[:1], num_to_retrieve=3)
    assert eng.reco[-1][1]["strategy"] == "average_vector"
    for bad, what in (([["no such passage"]], "recommend: unknown document 'no such passage'"), ([docs[0]], "LISTS of documents"),
                      ([[docs[0]] * 33], "33 examples"), ([[]], "holds no example")):
        with pytest.raises(ValueError, match=what):
            rag.recommend(bad)
    with pytest.raises(ValueError, match="strategy='cosine'"):
        rag.recommend(like[:1], strategy="cosine")
    with pytest.raises(ValueError, match="num_to_retrieve=21 exceeds the engine's max_topk=20"):
        rag.recommend(like[:1], num_to_retrieve=21)
    # retrieve(like=, unlike=) blends score rows: the query strategy is refused by name
    with pytest.raises(ValueError, match=r'retrieve\(like=, unlike=\) does not serve RetrievalConfig.recommend_strategy="average_vector"'):
        rag.retrieve(queries, num_to_retrieve=3, like=like, unlike=unlike)
    assert not eng.calls
    rag.global_config.recommend_strategy = "best_score"
    # ... every batch of the pipeline gets its own rows
    sols = rag.retrieve(queries, num_to_retrieve=3, like=like, unlike=unlike)
    assert len(eng.calls) == 2
    for kw, lo in zip(eng.calls, (0, 4)):
        ex = kw["feedback"]
        hi = min(lo + 4, n_q)
        assert isinstance(ex, Examples) and ex.batch == hi - lo and kw["feedback_weight"] == 0.3 and kw["feedback_strategy"] == "best_score"
        assert ex.ex_idx_host.tolist() == [i for q in range(lo, hi) for i in [q, q + 1] + ([q + 2] if q % 2 else [])]
    assert all(d == {"feedback_weight": 0.3} for s_ in sols for d in s_.doc_metadata)
    eng.calls.clear()
    rag.global_config.recommend_strategy = "sum_scores"
    rag.retrieve(queries[:2], num_to_retrieve=3, like=like[:2], feedback_weight=0.5)
    assert eng.calls[0]["feedback_weight"] == 0.5 and eng.calls[0]["feedback_strategy"] == "sum_scores"
    assert eng.calls[0]["feedback"].ex_sign_host.tolist() == [1, 1, 1, 1]
    # weight 0 and no examples: the plain call's arguments
    eng.calls.clear()
    sols = rag.retrieve(queries[:2], num_to_retrieve=3, like=like[:2], feedback_weight=0)
    rag.retrieve(queries[:2], num_to_retrieve=3)
    assert all("feedback" not in kw and "feedback_weight" not in kw for kw in eng.calls) and sols[0].doc_metadata[0] == {}
    # refusals by name
    with pytest.raises(ValueError, match="one list of documents per query expected"):
        rag.retrieve(queries[:2], like=like[:3])
    with pytest.raises(ValueError, match="unknown document"):
        rag.retrieve(queries[:1], like=[["nope"]])
    with pytest.raises(ValueError, match="feedback_weight=2"):
        rag.retrieve(queries[:1], like=like[:1], feedback_weight=2)
    for name in ("like", "unlike"):
        kw = {name: like[:1]}
        with pytest.raises(ValueError, match=f"retrieve_fused does not serve {name}:"):
            rag.retrieve_fused([[queries[0]]], **kw)
        with pytest.raises(ValueError, match=f"retrieve_ircot does not serve {name}:"):
            rag.retrieve_ircot(queries[:1], 1, **kw)
        with pytest.raises(ValueError, match=f"retrieve_dpr does not serve {name}:"):
            rag.retrieve_dpr(queries[:1], **kw)
