"""Engine calls, row shards, the KNN and the mirror at k > 2048: the device ranks any prefix of the documents
(hrag_opts.max_topk above 2048, K4' in csrc/topk.hip), bit for bit what the stable descending argsort of the engine's
own full score rows gives."""

import threading

import numpy as np
import pytest

from oracle.checks import make_case, ranked_parity

pytestmark = pytest.mark.gpu


def _bf16(bits, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)


def _argsort_desc(rows, k):
    idx = np.argsort(rows, axis=1, kind="stable")[:, ::-1][:, :k]
    return idx.astype(np.int32), np.take_along_axis(rows, idx, axis=1)


@pytest.fixture(scope="module")
def case(gpu_device):
    from hipporag_amd.engine import HippoRAGEngine
    kg, pass_bits, fact_bits, index = make_case(24000, 200000, 64, seed=2049)
    assert kg.n_passages > 2048
    eng = HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                         max_batch=300, max_topk=kg.n_passages)
    yield gpu_device, kg, pass_bits, fact_bits, index, eng
    eng.close()


def _inputs(dev, pass_bits, fact_bits, b, seed):
    from hipporag_amd import synth
    qf = _bf16(synth.make_queries_np(fact_bits, b, seed=seed)[0], dev)
    qp = _bf16(synth.make_queries_np(pass_bits, b, seed=seed + 1)[0], dev)
    return qf, qp


@pytest.mark.parametrize("b", [1, 8, 40, 130, 300])
def test_retrieve_ranking_is_its_own_full_scores_argsorted(case, b):
    import torch
    dev, kg, pass_bits, fact_bits, index, eng = case
    qf, qp = _inputs(dev, pass_bits, fact_bits, b, seed=10 + b)
    idx, sc = eng.score_facts(qf, k=5)
    cnt = torch.full((b,), 5, dtype=torch.int32, device=dev)
    cnt[::3] = 0                                           # the DPR fallback rows
    for k in (2049, kg.n_passages):
        out = eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=k)
        full = eng.last_doc_scores(b).cpu().numpy()
        want_idx, want_sc = _argsort_desc(full, k)
        np.testing.assert_array_equal(out.doc_idx.cpu().numpy(), want_idx)
        np.testing.assert_array_equal(out.doc_score.cpu().numpy().view(np.int32), want_sc.view(np.int32))
        small = eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=200)   # today's kernel: the prefix, bit for bit
        np.testing.assert_array_equal(small.doc_idx.cpu().numpy(), want_idx[:, :200])
        np.testing.assert_array_equal(small.doc_score.cpu().numpy().view(np.int32), want_sc[:, :200].view(np.int32))


def test_converged_repeat_path_keeps_the_prefix(case):
    """retrieve_converged under ppr_tol with a short base count (queries flagged NOT_CONVERGED are repeated on the wider
    state): the k = n_passages ranking starts with the k = 200 ranking, bit for bit."""
    import torch
    dev, kg, pass_bits, fact_bits, index, eng = case
    b = 40
    qf, qp = _inputs(dev, pass_bits, fact_bits, b, seed=77)
    idx, sc = eng.score_facts(qf, k=5)
    cnt = torch.full((b,), 5, dtype=torch.int32, device=dev)
    kw = dict(ppr_iters=3, ppr_tol=1.5e-6, ppr_max_iters=200)
    small = eng.retrieve_converged(qp, idx, sc, cnt, k=200, **kw)
    big = eng.retrieve_converged(qp, idx, sc, cnt, k=kg.n_passages, **kw)
    np.testing.assert_array_equal(big.doc_idx.cpu().numpy()[:, :200], small.doc_idx.cpu().numpy())
    np.testing.assert_array_equal(big.doc_score.cpu().numpy()[:, :200], small.doc_score.cpu().numpy())
    assert np.all(big.flags.cpu().numpy() == small.flags.cpu().numpy())


def test_against_the_fp64_oracle(case):
    """The whole 2049-prefix against the fp64 oracle: every returned score within 1e-5 relative of the oracle's score of
    that passage (where the oracle's score is not negligible), the order tie-class-aware (oracle.checks.ranked_parity:
    the window follows the measured error)."""
    import torch
    import oracle
    from hipporag_amd.graph import bf16_bits_to_float
    from hipporag_amd import synth
    dev, kg, pass_bits, fact_bits, index, eng = case
    b = 9
    qf_bits, _ = synth.make_queries_np(fact_bits, b, seed=5)
    qp_bits, _ = synth.make_queries_np(pass_bits, b, seed=6)
    idx, sc = eng.score_facts(_bf16(qf_bits, dev), k=5)
    cnt = torch.full((b,), 5, dtype=torch.int32, device=dev)
    out = eng.retrieve(_bf16(qp_bits, dev), idx, sc, cnt, ppr_iters=20, k=2049)
    got_idx, got_sc = out.doc_idx.cpu().numpy(), out.doc_score.cpu().numpy()
    qf, qp = bf16_bits_to_float(qf_bits), bf16_bits_to_float(qp_bits)
    for q in (0, 4, 8):
        ref = oracle.retrieve_one(index, qf[q], qp[q])
        full = ref.x[kg.passage_vertex]
        want = full[got_idx[q]]
        big = want > 1e-3 * want.max()
        assert (np.abs(got_sc[q][big] - want[big]) / want[big]).max() < 1e-5, q
        rep = ranked_parity(got_idx[q], got_sc[q], ref.sorted_doc_ids, ref.sorted_doc_scores, full, gap_cap=1e-3)
        assert rep["equal"], (q, rep)


def test_dense_and_scored_retrieve(case):
    import torch
    dev, kg, pass_bits, fact_bits, index, eng = case
    b = 24
    qf, qp = _inputs(dev, pass_bits, fact_bits, b, seed=31)
    raw = eng.sim_scores("passages", qp).cpu().numpy()
    mn, mx = raw.min(axis=1, keepdims=True), raw.max(axis=1, keepdims=True)
    norm = np.where(mx - mn == 0, np.float32(1), (raw - mn) / (mx - mn)).astype(np.float32)
    for k in (2049, kg.n_passages):
        want_idx, want_sc = _argsort_desc(raw, k)
        d_idx, d_sc = eng.dense_retrieve(qp, k=k)
        np.testing.assert_array_equal(d_idx.cpu().numpy(), want_idx)
        np.testing.assert_array_equal(d_sc.cpu().numpy(), np.take_along_axis(norm, want_idx.astype(np.int64), axis=1))
    idx, sc = eng.score_facts(qf, k=5)
    cnt = torch.full((b,), 5, dtype=torch.int32, device=dev)
    s = eng.retrieve_scored(torch.from_numpy(raw).to(dev), idx, sc, cnt, ppr_iters=20, k=3000)
    want_idx, want_sc = _argsort_desc(eng.last_doc_scores(b).cpu().numpy(), 3000)
    np.testing.assert_array_equal(s.doc_idx.cpu().numpy(), want_idx)
    np.testing.assert_array_equal(s.doc_score.cpu().numpy(), want_sc)


@pytest.mark.parametrize("native", [False, True])
def test_eight_shards_equal_the_unsharded_engine(gpu_device, native):
    import torch
    from hipporag_amd import dist as hd
    from hipporag_amd.engine import HippoRAGEngine
    world, b, k = 8, 130, 2500
    kg, pass_bits, fact_bits, _ = make_case(24000, 200000, 64, seed=808)
    sidx = hd.shard_index(kg.csr, kg.passage_vertex, world, kg.subj_vertex, kg.obj_vertex, kg.num_chunks)
    qf, qp = _inputs(gpu_device, pass_bits, fact_bits, b, seed=3)
    kw = dict(link_top_k=5, damping=0.5, passage_node_weight=0.05, ppr_iters=20, k=k)
    got = hd.run_local_shards(world, sidx, pass_bits, fact_bits, qf, qp, kw, 2, gpu_device, k, native=native)
    with HippoRAGEngine(sidx.csr, sidx.passage_vertex, pass_bits, fact_bits, sidx.subj_vertex, sidx.obj_vertex,
                        sidx.num_chunks, max_batch=b, max_topk=k) as eng:
        idx, sc = eng.score_facts(qf, k=5)
        cnt = torch.full((b,), 5, dtype=torch.int32, device=gpu_device)
        out = eng.retrieve(qp, idx, sc, cnt, **kw)
        torch.cuda.synchronize()
        assert eng.timings()["slab_width"] == 128
        np.testing.assert_array_equal(got[2], out.doc_idx.cpu().numpy())
        np.testing.assert_array_equal(got[3], out.doc_score.cpu().numpy())
    assert np.all(got[4] == 0)


def test_two_workspaces_of_an_f32_split_engine_on_two_threads(gpu_device):
    """The per-call split-query buffer lives in every workspace (it was allocated once per engine): two handles of an
    f32 engine on two threads and two streams give what sequential calls give, at k = 2049 and k = 200."""
    import torch
    from hipporag_amd import synth
    from hipporag_amd.engine import HippoRAGEngine
    from hipporag_amd.graph import bf16_bits_to_float
    kg, pass_bits, fact_bits, _ = make_case(24000, 200000, 64, seed=99)
    pe, fe = bf16_bits_to_float(pass_bits).astype(np.float32), bf16_bits_to_float(fact_bits).astype(np.float32)
    b = 16
    qs = []
    for seed in (1, 2):
        qs.append(tuple(torch.from_numpy(bf16_bits_to_float(synth.make_queries_np(bits, b, seed=seed + j)[0])
                                         .astype(np.float32)).to(gpu_device) for j, bits in enumerate((fact_bits, pass_bits))))
    with HippoRAGEngine(kg.csr, kg.passage_vertex, pe, fe, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                        max_batch=b, max_topk=2049) as eng:
        def run(h, q, k):
            idx, sc = h.score_facts(q[0], k=5)
            cnt = torch.full((b,), 5, dtype=torch.int32, device=gpu_device)
            out = h.retrieve(q[1], idx, sc, cnt, ppr_iters=20, k=k)
            d_idx, d_sc = h.dense_retrieve(q[1], k=k)
            return [t.clone() for t in (idx, sc, out.doc_idx, out.doc_score, d_idx, d_sc)]

        ref = {(i, k): run(eng, qs[i], k) for i in (0, 1) for k in (2049, 200)}
        torch.cuda.synchronize()
        w = eng.workspace()
        errors = []
        start = threading.Barrier(2)

        def worker(h, i):
            try:
                with torch.cuda.stream(torch.cuda.Stream(device=gpu_device)):
                    start.wait()
                    for _ in range(5):
                        for k in (2049, 200):
                            got = run(h, qs[i], k)
                            torch.cuda.current_stream().synchronize()
                            for g, r in zip(got, ref[(i, k)]):
                                if not torch.equal(g, r):
                                    errors.append((i, k))
            except Exception as exc:   # noqa: BLE001 -- reported below
                errors.append(repr(exc))

        threads = [threading.Thread(target=worker, args=(h, i)) for i, h in enumerate((eng, w))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        w.close()
    assert not errors, errors[:5]


def test_retrieve_knn_beyond_2048(gpu_device):
    from hipporag_amd.knn import retrieve_knn
    from tests.helpers import tie_aware_equal
    rng = np.random.default_rng(4096)
    nk, dim, nq = 50000, 768, 6
    keys = rng.standard_normal((nk, dim)).astype(np.float32)
    q = (keys[rng.integers(0, nk, nq)] + 0.5 * rng.standard_normal((nq, dim))).astype(np.float32)
    idx, sc = retrieve_knn(None, None, q, keys, k=4096, return_arrays=True)
    qn = q / np.linalg.norm(q, axis=1, keepdims=True)
    kn = keys / np.linalg.norm(keys, axis=1, keepdims=True)
    s = qn.astype(np.float64) @ kn.astype(np.float64).T
    order = np.argsort(s, axis=1, kind="stable")[:, ::-1][:, :4096]
    assert idx.shape == (nq, 4096)
    for i in range(nq):
        assert tie_aware_equal(idx[i], order[i], s[i][order[i]], abs_gap=4e-6), i
        np.testing.assert_allclose(sc[i], s[i][idx[i]], rtol=0, atol=3e-6)
    i2, s2 = retrieve_knn(None, None, q, keys, k=2047, return_arrays=True)   # today's path: the same prefix
    np.testing.assert_array_equal(i2, idx[:, :2047])
    np.testing.assert_array_equal(s2, sc[:, :2047])


def test_mirror_ranks_5000_documents_on_the_device(gpu_device, monkeypatch):
    from hipporag_amd import synth
    from hipporag_amd.graph import bf16_bits_to_float
    from hipporag_amd.retriever import HippoRAG, RetrievalConfig

    class Table:
        def __init__(self, t):
            self.t = t

        def batch_encode(self, texts, instruction=None, norm=True):
            return np.stack([self.t["f" if instruction and "fact" in instruction else "p"][x] for x in texts])

    kg, pass_bits, fact_bits, _ = make_case(48000, 300000, 64, seed=5000)
    assert kg.n_passages > 5000
    n = 12
    qf, _ = synth.make_queries_np(fact_bits, n, seed=3)
    qp, _ = synth.make_queries_np(pass_bits, n, seed=4)
    queries = [f"question {i}" for i in range(n)]
    table = {"f": dict(zip(queries, bf16_bits_to_float(qf))), "p": dict(zip(queries, bf16_bits_to_float(qp)))}

    def mirror(top_k):
        return HippoRAG.from_arrays(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex,
                                    kg.num_chunks, global_config=RetrievalConfig(embedding_precision="bf16", max_batch=8,
                                                                                 retrieval_top_k=top_k),
                                    embedding_model=Table(table))

    host = mirror(2048)                       # engine max_topk = 2048: the host ranks beyond it
    want = host.retrieve(queries, num_to_retrieve=5000)
    want_d = host.retrieve_dpr(queries, num_to_retrieve=5000)
    dev = mirror(5000)
    dev.retrieve(queries[:1], num_to_retrieve=10)
    assert dev.engine.max_topk == 5000

    def refuse(*a, **k):
        raise AssertionError("the host ranking path was taken")

    monkeypatch.setattr(dev.engine, "last_doc_scores", refuse)
    monkeypatch.setattr(dev.engine, "sim_scores", refuse)
    got = dev.retrieve(queries, num_to_retrieve=5000)
    got_d = dev.retrieve_dpr(queries, num_to_retrieve=5000)
    # the same scores in the same order; the documents equal except inside runs of EQUAL returned scores (the DPR
    # ranking orders by the raw score, which min-max normalisation can map to one float: the host sorts the
    # normalised value, the device the raw one -- the k <= 2048 kernel does the same)
    for a, b in list(zip(got, want)) + list(zip(got_d, want_d)):
        assert len(a.docs) == 5000 and len(b.docs) == 5000
        sa, sb = np.asarray(a.doc_scores), np.asarray(b.doc_scores)
        np.testing.assert_array_equal(sa, sb)
        start = 0
        while start < len(sa):
            end = start + 1
            while end < len(sa) and sa[end] == sa[start]:
                end += 1
            if end < len(sa):                 # the run cut by the k boundary may hold other members
                assert set(a.docs[start:end]) == set(b.docs[start:end]), (a.question, start)
            start = end
