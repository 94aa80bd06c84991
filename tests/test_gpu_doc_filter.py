"""The doc filter on the device (include/hrag.h hrag_topk_rows_masked, hrag_retrieve_filtered & co.): every selection
path of csrc/topk.hip in its masked form against a numpy restatement, the engine on every PPR state path, the row
shards, the mirror and the convergence repeat -- each held to "the allowed prefix of the unfiltered ranking", bit for
bit."""

import numpy as np
import pytest

from hipporag_amd import synth
from hipporag_amd.engine import pack_mask
from oracle.checks import make_case

pytestmark = pytest.mark.gpu


def _bf16(bits, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)


def _words(m, dev):
    import torch
    return torch.from_numpy(pack_mask(m).view(np.int32)).to(dev)


def expected_masked_topk(x, allowed, k, normalize, idx_offset=0):
    """The filtered ranking restated: per row the first min(k, allowed) entries of np.argsort(x, kind="stable")[::-1]
    that `allowed` admits, -1 / 0 beyond; the row min / max over EVERY element (fminf / fmaxf: NaN skipped)."""
    x = np.asarray(x, np.float32)
    b, n = x.shape
    allowed = np.broadcast_to(allowed, x.shape)
    nan = np.isnan(x)
    mn = np.where(nan, np.float32(np.inf), x).min(axis=1, initial=np.inf).astype(np.float32)
    mx = np.where(nan, np.float32(-np.inf), x).max(axis=1, initial=-np.inf).astype(np.float32)
    idx = np.full((b, k), -1, np.int32)
    val = np.zeros((b, k), np.float32)
    for i in range(b):
        order = np.argsort(x[i], kind="stable")[::-1]
        order = order[allowed[i][order]][:k]
        idx[i, :len(order)] = order + idx_offset
        v = x[i, order]
        if normalize:
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                rng_ = mx[i] - mn[i]
                v = np.float32(1) * np.ones_like(v) if rng_ == 0 else ((v - mn[i]) / rng_).astype(np.float32)
        val[i, :len(order)] = v
    return idx, val, mn, mx


def _rows(b, n, seed):
    """Scores with NaN, +-inf, +-0 and heavy ties."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-50, 50, (b, n)).astype(np.float32) / 8
    for i in range(b):
        at = rng.integers(0, n, 8)
        x[i, at[:2]] = np.nan
        x[i, at[2]] = np.inf
        x[i, at[3]] = -np.inf
        x[i, at[4]] = -0.0
        x[i, at[5]] = 0.0
    return x


def _masks(kind, b, n, k, rng):
    if kind == "all":
        return np.ones((b, n), bool)
    if kind == "none":
        return np.zeros((b, n), bool)
    if kind in ("exactly_k", "fewer_than_k", "one"):
        cnt = {"exactly_k": min(k, n), "fewer_than_k": max(1, min(k, n) // 3), "one": 1}[kind]
        m = np.zeros((b, n), bool)
        for i in range(b):
            m[i, rng.choice(n, cnt, replace=False)] = True
        return m
    p = {"p50": 0.5, "p1": 0.01}[kind]
    return rng.random((b, n)) < p


def _masked(scores, b, n, k, m_words, ld, bit_offset, normalize, ws_bytes):
    import torch
    from hipporag_amd import _lib
    lib = _lib.load()
    dev = scores.device
    idx = torch.empty((b, k), dtype=torch.int32, device=dev)
    val = torch.empty((b, k), dtype=torch.float32, device=dev)
    mn = torch.empty((b,), dtype=torch.float32, device=dev)
    mx = torch.empty((b,), dtype=torch.float32, device=dev)
    ws = torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device=dev)
    _lib.check(lib.hrag_topk_rows_masked(scores.data_ptr(), b, n, scores.shape[1], k, 0, normalize, m_words.data_ptr(),
                                         ld, bit_offset, idx.data_ptr(), val.data_ptr(), mn.data_ptr(), mx.data_ptr(),
                                         ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream))
    return tuple(t.cpu().numpy() for t in (idx, val, mn, mx))


def _unmasked_ws(scores, b, n, k, normalize):
    import torch
    from hipporag_amd import _lib
    lib = _lib.load()
    dev = scores.device
    need = int(lib.hrag_topk_rows_workspace_bytes(b, n, k))
    idx = torch.empty((b, k), dtype=torch.int32, device=dev)
    val = torch.empty((b, k), dtype=torch.float32, device=dev)
    mn = torch.empty((b,), dtype=torch.float32, device=dev)
    mx = torch.empty((b,), dtype=torch.float32, device=dev)
    ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
    _lib.check(lib.hrag_topk_rows_ws(scores.data_ptr(), b, n, scores.shape[1], k, 0, normalize, idx.data_ptr(),
                                     val.data_ptr(), mn.data_ptr(), mx.data_ptr(), ws.data_ptr(), need,
                                     torch.cuda.current_stream().cuda_stream))
    return tuple(t.cpu().numpy() for t in (idx, val, mn, mx))


# (batch, n, k): one workgroup per row; split + merge (batch < 64, n >= 32768, a workspace); large k in LDS;
# large k through tile sort + merge; k = n
PATHS = {"one_wg": (70, 5000, 200), "one_wg_short": (3, 3000, 50), "split": (4, 70001, 300),
         "large_lds": (3, 40000, 5000), "large_tiles": (2, 60000, 20000), "k_eq_n": (3, 2500, 2500)}
MASKS = ["all", "none", "exactly_k", "fewer_than_k", "one", "p50", "p1"]


def _bits_at(m, bit_offset, lead_seed):
    """The rows of m placed at bit bit_offset of a wider mask (random bits in front: they must be ignored)."""
    b, n = m.shape
    rng = np.random.default_rng(lead_seed)
    wide = np.concatenate([rng.random((b, bit_offset)) < 0.5, m, rng.random((b, 40)) < 0.5], axis=1)
    return wide


@pytest.mark.parametrize("path", list(PATHS))
def test_masked_topk_rows_every_path_against_numpy(gpu_device, path):
    import torch
    b, n, k = PATHS[path]
    x = _rows(b, n, seed=list(PATHS).index(path))
    ld_elems = n + 3
    xd = torch.zeros((b, ld_elems), dtype=torch.float32)
    xd[:, :n] = torch.from_numpy(x)
    xd = xd.to(gpu_device)
    from hipporag_amd import _lib
    need = int(_lib.load().hrag_topk_rows_workspace_bytes(b, n, k))
    ws_bytes = max(need, 64 * 4096 * 8 + 64 * 64 * 8)      # >= 2 MiB also lets the k <= 2048 rows split
    rng = np.random.default_rng(7)
    base = _unmasked_ws(xd, b, n, k, 1)
    for kind in MASKS:
        m = _masks(kind, b, n, k, rng)
        for bit_offset in (0, 5, 37):
            wide = _bits_at(m, bit_offset, 3)
            for per_row in (True, False):
                rows = wide if per_row else wide[:1]
                words = _words(rows, gpu_device)
                ld = words.shape[1] if per_row else 0
                for normalize in (0, 1):
                    got = _masked(xd, b, n, k, words if per_row else words[0].contiguous(), ld, bit_offset, normalize,
                                  ws_bytes)
                    want = expected_masked_topk(x, m if per_row else m[:1], k, normalize)
                    msg = f"{path} {kind} offset {bit_offset} per_row {per_row} normalize {normalize}"
                    np.testing.assert_array_equal(got[0], want[0], err_msg=msg)
                    np.testing.assert_array_equal(got[1], want[1], err_msg=msg)      # NaN == NaN, +0 == -0
                    np.testing.assert_array_equal(got[2], want[2], err_msg=msg)
                    np.testing.assert_array_equal(got[3], want[3], err_msg=msg)
                    if kind == "all" and normalize:
                        for g, w in zip(got, base):                      # = hrag_topk_rows_ws, bit for bit
                            np.testing.assert_array_equal(g.view(np.int32), w.view(np.int32), err_msg=msg)


def test_masked_topk_rejects_a_short_row_stride(gpu_device):
    import torch
    from hipporag_amd import _lib
    x = torch.zeros((2, 100), device=gpu_device)
    words = torch.zeros((2, 4), dtype=torch.int32, device=gpu_device)
    with pytest.raises(_lib.HragError):
        _masked(x, 2, 100, 5, words, 3, 0, 0, 0)         # 3 words < ceil(100 / 32)
    with pytest.raises(_lib.HragError):
        _masked(x, 2, 100, 5, words, 4, 40, 0, 0)        # 4 words < ceil(140 / 32)


# ------------------------------------------------------------------ the engine, every PPR state path
@pytest.fixture(scope="module")
def case(gpu_device):
    from hipporag_amd._lib import OPT_NO_F16, OPT_NO_FP8
    from hipporag_amd.engine import HippoRAGEngine
    kg, pass_bits, fact_bits, index = make_case(12000, 100000, 64, seed=4242)
    engines = {}
    for name, flags in (("default", 0), ("f32", OPT_NO_FP8 | OPT_NO_F16)):
        engines[name] = HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex,
                                       kg.num_chunks, max_batch=130, max_topk=kg.n_passages, flags=flags)
    yield gpu_device, kg, pass_bits, fact_bits, engines
    for e in engines.values():
        e.close()


STATES = [("small", "default", 5), ("f16", "default", 40), ("fp8", "default", 130), ("f32", "f32", 40)]


def _state_inputs(dev, kg, pass_bits, fact_bits, eng, b, seed):
    import torch
    qf = _bf16(synth.make_queries_np(fact_bits, b, seed=seed)[0], dev)
    qp = _bf16(synth.make_queries_np(pass_bits, b, seed=seed + 1)[0], dev)
    idx, sc = eng.score_facts(qf, k=5)
    cnt = torch.full((b,), 5, dtype=torch.int32, device=dev)
    cnt[::4] = 0                                            # DPR fallback rows
    return qp, idx, sc, cnt


def _allowed_prefix(full_idx, full_sc, allowed, k):
    b = full_idx.shape[0]
    allowed = np.broadcast_to(allowed, (b, allowed.shape[-1]))
    idx = np.full((b, k), -1, np.int32)
    sc = np.zeros((b, k), np.float32)
    for i in range(b):
        keep = allowed[i][full_idx[i]]
        sel = full_idx[i][keep][:k]
        idx[i, :len(sel)] = sel
        sc[i, :len(sel)] = full_sc[i][keep][:k]
    return idx, sc


def _same(got_idx, got_sc, want_idx, want_sc, msg=""):
    np.testing.assert_array_equal(np.asarray(got_idx), want_idx, err_msg=msg)
    np.testing.assert_array_equal(np.asarray(got_sc, np.float32).view(np.int32), want_sc.view(np.int32), err_msg=msg)


@pytest.mark.parametrize("state,which,b", STATES)
def test_engine_filtered_retrieve_is_the_allowed_prefix_of_the_full_ranking(case, state, which, b):
    import torch
    dev, kg, pass_bits, fact_bits, engines = case
    eng = engines[which]
    n_p = kg.n_passages
    qp, idx, sc, cnt = _state_inputs(dev, kg, pass_bits, fact_bits, eng, b, seed=31 + b)
    full = eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=n_p)
    f_idx, f_sc = full.doc_idx.cpu().numpy(), full.doc_score.cpu().numpy()
    width = eng.timings()["slab_width"]
    assert (state == "fp8") == (width == 128)
    assert (full.flags.cpu().numpy() & 1).any()             # the DPR fallback is in the batch
    # NULL filter: hrag_retrieve bit for bit (the filtered entry point with filter_dev = NULL through the C ABI)
    for k in (10, 200):
        plain = eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=k)
        _same(plain.doc_idx.cpu(), plain.doc_score.cpu().numpy(), f_idx[:, :k], f_sc[:, :k])
    rng = np.random.default_rng(b)
    per_row = rng.random((b, n_p)) < 0.3
    per_row[1] = False                                       # an empty allowed set
    per_row[2] = False
    per_row[2, rng.choice(n_p, 3, replace=False)] = True     # fewer than k
    one = rng.random(n_p) < 0.05
    for k in (10, 200, n_p):
        for m, form in ((per_row, "bool"), (one, "bool"), (per_row, "packed"), (one, "packed")):
            f = torch.from_numpy(m) if form == "bool" else torch.from_numpy(pack_mask(m).view(np.int32))
            out = eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=k, doc_filter=f.to(dev))
            want_idx, want_sc = _allowed_prefix(f_idx, f_sc, m, k)
            msg = f"{state} k={k} {form} {m.shape}"
            _same(out.doc_idx.cpu(), out.doc_score.cpu().numpy(), want_idx, want_sc, msg)
            np.testing.assert_array_equal(out.flags.cpu().numpy(), full.flags.cpu().numpy(), err_msg=msg)
    assert (eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=10,
                         doc_filter=torch.from_numpy(per_row).to(dev)).doc_idx.cpu().numpy()[1] == -1).all()
    # retrieve_scored_filtered: the same with the caller's raw passage scores
    raw = eng.sim_scores("passages", qp)
    full_s = eng.retrieve_scored(raw, idx, sc, cnt, ppr_iters=20, k=n_p)
    out_s = eng.retrieve_scored(raw, idx, sc, cnt, ppr_iters=20, k=200, doc_filter=torch.from_numpy(per_row).to(dev))
    want_idx, want_sc = _allowed_prefix(full_s.doc_idx.cpu().numpy(), full_s.doc_score.cpu().numpy(), per_row, 200)
    _same(out_s.doc_idx.cpu(), out_s.doc_score.cpu().numpy(), want_idx, want_sc, "scored")


def test_engine_filtered_dense_retrieve(case):
    import torch
    dev, kg, pass_bits, fact_bits, engines = case
    eng = engines["default"]
    n_p = kg.n_passages
    for b in (3, 100):
        qp = _bf16(synth.make_queries_np(pass_bits, b, seed=91 + b)[0], dev)
        f_idx, f_sc = (t.cpu().numpy() for t in eng.dense_retrieve(qp, k=n_p))
        p_idx, p_sc = (t.cpu().numpy() for t in eng.dense_retrieve(qp, k=100))
        _same(p_idx, p_sc, f_idx[:, :100], f_sc[:, :100])
        m = np.random.default_rng(b).random((b, n_p)) < 0.1
        m[0] = False
        for k in (100, n_p):
            g_idx, g_sc = (t.cpu().numpy() for t in eng.dense_retrieve(qp, k=k, doc_filter=torch.from_numpy(m).to(dev)))
            want_idx, want_sc = _allowed_prefix(f_idx, f_sc, m, k)   # min-max over ALL passages: scores unchanged
            _same(g_idx, g_sc, want_idx, want_sc, f"dense b={b} k={k}")


def test_engine_rejects_a_short_filter_stride(case):
    import torch
    from hipporag_amd import _lib
    dev, kg, pass_bits, fact_bits, engines = case
    eng = engines["default"]
    qp = _bf16(synth.make_queries_np(pass_bits, 2, seed=1)[0], dev)
    short = torch.zeros((2, (kg.n_passages + 31) // 32 - 1), dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        eng.dense_retrieve(qp, k=10, doc_filter=short)
    lib = _lib.load()
    idx = torch.empty((2, 10), dtype=torch.int32, device=dev)
    sc = torch.empty((2, 10), dtype=torch.float32, device=dev)
    st = lib.hrag_dense_retrieve_filtered(eng._handle, eng._q(qp).data_ptr(), 2, 10, idx.data_ptr(), sc.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream, short.data_ptr(), short.shape[1])
    assert st == _lib.HRAG_EINVAL


# ------------------------------------------------------------------ row shards
@pytest.mark.parametrize("native", [False, True])
def test_row_shards_filtered_equal_the_single_engine(gpu_device, native):
    import torch
    from hipporag_amd import dist as hd
    from hipporag_amd.engine import HippoRAGEngine
    world, b, k = 3, 70, 100
    kg, pass_bits, fact_bits, index = make_case(12000, 120000, 128, seed=777)
    sidx = hd.shard_index(kg.csr, kg.passage_vertex, world, kg.subj_vertex, kg.obj_vertex, kg.num_chunks)
    n_p = len(sidx.passage_vertex)
    qf = _bf16(synth.make_queries_np(fact_bits, b, seed=3)[0], gpu_device)
    qp = _bf16(synth.make_queries_np(pass_bits, b, seed=4)[0], gpu_device)
    rng = np.random.default_rng(5)
    m = rng.random((b, n_p)) < 0.2
    lo, hi = sidx.passages[1]
    assert lo % 32 != 0 or sidx.passages[2][0] % 32 != 0          # a shard's slice starts inside a word
    m[:, lo:hi] = False                                           # shard 1 holds no allowed passage
    m[0] = False
    filt = torch.from_numpy(m).to(gpu_device)
    kw = dict(link_top_k=5, damping=0.5, passage_node_weight=0.05, ppr_iters=20, k=k, doc_filter=filt)
    got = hd.run_local_shards(world, sidx, pass_bits, fact_bits, qf, qp, kw, 2, gpu_device, k, native=native)
    with HippoRAGEngine(sidx.csr, sidx.passage_vertex, pass_bits, fact_bits, sidx.subj_vertex, sidx.obj_vertex,
                        sidx.num_chunks, max_batch=b, max_topk=k) as eng:
        idx, sc = eng.score_facts(qf, k=5)
        cnt = torch.full((b,), 5, dtype=torch.int32, device=gpu_device)
        out = eng.retrieve(qp, idx, sc, cnt, link_top_k=5, damping=0.5, passage_node_weight=0.05, ppr_iters=20, k=k,
                           doc_filter=filt)
        one = (out.doc_idx.cpu().numpy(), out.doc_score.cpu().numpy())
    _same(got[2], got[3], one[0], one[1], f"native={native}")
    assert (got[2][0] == -1).all()
    assert not np.isin(got[2], np.arange(lo, hi)).any()


# ------------------------------------------------------------------ convergence repeat
def test_not_converged_repeat_keeps_each_querys_filter_row(gpu_device):
    import torch
    from hipporag_amd._lib import FLAG_NOT_CONVERGED
    from hipporag_amd.engine import HippoRAGEngine
    from tests.test_gpu_fp8_adversarial import _index, _ring
    n, src, dst, w, pv, pinned = _ring()
    csr, pass_bits, fact_bits, index = _index(n, src, dst, w, pv, 64, seed=11, pinned_facts=pinned)
    n_p, b = len(pv), 130
    qf = _bf16(synth.make_queries_np(fact_bits, b, seed=5)[0], gpu_device)
    qp = _bf16(synth.make_queries_np(pass_bits, b, seed=6)[0], gpu_device)
    m = np.random.default_rng(9).random((b, n_p)) < 0.25
    tol = 1.5e-6
    with HippoRAGEngine(csr, index.passage_vertex, pass_bits, fact_bits, index.subj_vertex, index.obj_vertex,
                        index.num_chunks, max_batch=b, max_topk=n_p) as eng:
        idx, sc = eng.score_facts(qf, k=5)
        cnt = torch.full((b,), 5, dtype=torch.int32, device=gpu_device)
        kw = dict(damping=0.5, ppr_iters=20, ppr_tol=tol, ppr_max_iters=400)
        raw = eng.retrieve(qp, idx, sc, cnt, k=n_p, **kw)
        assert (raw.flags.cpu().numpy() & FLAG_NOT_CONVERGED).any()          # some queries are rerun
        pend = eng.retrieve_converged_start(qp, idx, sc, cnt, k=n_p, **kw)
        full = pend.finish()
        assert pend.repeated
        pend_f = eng.retrieve_converged_start(qp, idx, sc, cnt, k=50, doc_filter=torch.from_numpy(m).to(gpu_device), **kw)
        got = pend_f.finish()
        assert pend_f.repeated
    want_idx, want_sc = _allowed_prefix(full.doc_idx.cpu().numpy(), full.doc_score.cpu().numpy(), m, 50)
    _same(got.doc_idx.cpu(), got.doc_score.cpu().numpy(), want_idx, want_sc, "converged repeat")


# ------------------------------------------------------------------ the mirror
@pytest.fixture(scope="module")
def mirror(gpu_device):
    from hipporag_amd.retriever import Chunk, HippoRAG, RetrievalConfig
    from tests.golden.make_golden import DOCS, QUERIES, TRIPLES, MockEmbeddingModel
    meta = [{"user": ["a", "b", "c"][i % 3], "year": 2020 + i % 4} for i in range(len(DOCS))]
    chunks = [Chunk(d, source_id=f"src{i % 2}", metadata=meta[i]) for i, d in enumerate(DOCS)]
    rag = HippoRAG(RetrievalConfig(max_batch=4, retrieval_top_k=len(DOCS) + 3, embedding_precision="bf16"),
                   embedding_model=MockEmbeddingModel())
    rag.index_from_openie(chunks, TRIPLES)
    return rag, QUERIES, chunks


def _allowed_docs(rag, f):
    keys = rag.passage_node_keys
    out = set()
    for i, key in enumerate(keys):
        md = rag.chunk_metadata.get(key, {})
        if all(kk in md and (md[kk] in v if isinstance(v, list) else md[kk] == v) for kk, v in f.items()):
            out.add(rag.passage_texts[i])
    return out


def _filtered_view(sol, allowed, n):
    keep = [i for i, d in enumerate(sol.docs) if d in allowed][:n]
    return [sol.docs[i] for i in keep], np.asarray(sol.doc_scores)[keep]


def test_mirror_filters_are_the_allowed_prefix_of_its_full_ranking(mirror):
    rag, queries, chunks = mirror
    n_all = len(rag.passage_node_keys)
    filters = [{"user": "a"}, {"user": ["b", "c"], "year": [2021, 2022]}, {"source_id": "src1"}, {"user": "nobody"}]
    for method in ("retrieve", "retrieve_dpr"):
        full = getattr(rag, method)(queries, num_to_retrieve=n_all)
        for f in filters:
            allowed = _allowed_docs(rag, f)
            for n in (2, n_all):
                got = getattr(rag, method)(queries, num_to_retrieve=n, doc_filter=f)
                for g, w in zip(got, full):
                    docs, scores = _filtered_view(w, allowed, n)
                    assert g.docs == docs, (method, f, n)
                    np.testing.assert_array_equal(np.asarray(g.doc_scores, np.float32), scores.astype(np.float32))
                    assert all(rag.chunk_metadata and md == rag.chunk_metadata[rag.passage_node_keys[
                        rag.passage_texts.index(d)]] for d, md in zip(g.docs, g.doc_metadata))
        # per-query filters, and a bool array
        per = [filters[i % len(filters)] for i in range(len(queries))]
        got = getattr(rag, method)(queries, num_to_retrieve=3, doc_filter=per)
        for g, w, f in zip(got, full, per):
            assert g.docs == _filtered_view(w, _allowed_docs(rag, f), 3)[0]
        arr = np.zeros(n_all, bool)
        arr[[0, 4, 7]] = True
        got = getattr(rag, method)(queries, num_to_retrieve=3, doc_filter=arr)
        for g, w in zip(got, full):
            assert g.docs == _filtered_view(w, {rag.passage_texts[i] for i in (0, 4, 7)}, 3)[0]
    assert all(r.docs == [] for r in rag.retrieve(queries, doc_filter={"user": "nobody"}))


def test_mirror_beyond_max_topk_and_ircot_apply_the_filter(mirror):
    rag, queries, chunks = mirror
    n_all = len(rag.passage_node_keys)
    f = {"year": [2020, 2022]}
    allowed = _allowed_docs(rag, f)
    eng = rag.engine
    full = rag.retrieve(queries, num_to_retrieve=n_all)
    full_dpr = rag.retrieve_dpr(queries, num_to_retrieve=n_all)
    saved = eng.max_topk
    try:
        eng.max_topk = 2                                  # num_to_retrieve > max_topk: ranked on the host
        got = rag.retrieve(queries, num_to_retrieve=n_all, doc_filter=f)
        got_dpr = rag.retrieve_dpr(queries, num_to_retrieve=n_all, doc_filter=f)
    finally:
        eng.max_topk = saved
    for g, w in zip(got, full):
        assert g.docs == _filtered_view(w, allowed, n_all)[0]
    for g, w in zip(got_dpr, full_dpr):
        assert g.docs == _filtered_view(w, allowed, n_all)[0]
    ir = rag.retrieve_ircot(queries, max_qa_steps=2, num_to_retrieve=3, doc_filter=f,
                            reason_fn=lambda q, docs, th: "thinking about " + q)
    for r in ir:
        assert r.docs and set(r.docs) <= allowed


def test_mirror_sees_new_and_deleted_chunks(mirror):
    from hipporag_amd.retriever import Chunk
    rag, queries, chunks = mirror
    new = Chunk("George Rankin later became a mayor.", source_id="src9", metadata={"user": "z"})
    rag.index_from_openie([new], [[("George Rankin", "became", "mayor")]])
    try:
        got = rag.retrieve(queries, num_to_retrieve=5, doc_filter={"user": "z"})
        assert all(r.docs == [new.content] for r in got)
        got = rag.retrieve_dpr(queries, num_to_retrieve=5, doc_filter={"source_id": "src9"})
        assert all(r.docs == [new.content] for r in got)
    finally:
        rag.delete([new.content])
    assert all(r.docs == [] for r in rag.retrieve(queries, num_to_retrieve=5, doc_filter={"user": "z"}))
