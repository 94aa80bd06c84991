"""The scoped doc filter on the device (include/hrag.h, "scoped doc filter": hrag_score_facts_scoped,
hrag_retrieve_scoped & co.): tenant isolation on a disjoint union of corpora, phase A and the fact bitset against numpy
restatements, the masked prior held to its definition on every PPR state path, the "every passage allowed" case bit
for bit, edge cases, workspaces and the mirror surface."""

import numpy as np
import pytest

from hipporag_amd import synth
from hipporag_amd.engine import pack_mask
from oracle.checks import make_case, tie_aware_equal

pytestmark = pytest.mark.gpu


def _bf16(bits, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)


def _words(m, dev):
    import torch
    return torch.from_numpy(pack_mask(m).view(np.int32)).to(dev)


def _same(got_idx, got_sc, want_idx, want_sc, msg=""):
    np.testing.assert_array_equal(np.asarray(got_idx), np.asarray(want_idx), err_msg=msg)
    np.testing.assert_array_equal(np.asarray(got_sc, np.float32).view(np.int32),
                                  np.asarray(want_sc, np.float32).view(np.int32), err_msg=msg)


def _np(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------ restatements
def fact_mask_np(doc_allowed, row_ptr, pos):
    """bool [R, F]: fact f allowed when one of its sources is an allowed passage."""
    doc_allowed = np.atleast_2d(doc_allowed)
    n_f = len(row_ptr) - 1
    out = np.zeros((doc_allowed.shape[0], n_f), bool)
    for f in range(n_f):
        src = pos[row_ptr[f]:row_ptr[f + 1]]
        if len(src):
            out[:, f] = doc_allowed[:, src].any(axis=1)
    return out


def scoped_topk_np(x, allowed, k):
    """Phase A of the "seeds" scope: the first min(k, allowed) allowed entries of np.argsort(x, kind="stable")[::-1],
    min-max normalised over the allowed raw scores (fminf / fmaxf: NaN skipped; zero range: 1), -1 / 0 beyond."""
    x = np.asarray(x, np.float32)
    b, n = x.shape
    allowed = np.broadcast_to(allowed, x.shape)
    idx = np.full((b, k), -1, np.int32)
    val = np.zeros((b, k), np.float32)
    for i in range(b):
        a = allowed[i] & ~np.isnan(x[i])
        order = np.argsort(x[i], kind="stable")[::-1]
        order = order[allowed[i][order]][:k]
        if not len(order):
            continue
        mn, mx = (np.float32(x[i][a].min()), np.float32(x[i][a].max())) if a.any() else (np.float32(np.inf),
                                                                                             np.float32(-np.inf))
        v = x[i, order]
        rng_ = np.float32(mx - mn)
        with np.errstate(invalid="ignore"):
            v = np.ones_like(v) if rng_ == 0 else ((v - mn) / rng_).astype(np.float32)
        idx[i, :len(order)] = order
        val[i, :len(order)] = v
    return idx, val


def masked_prior_np(raw, allowed):
    """The prior of the "seeds" scope in fp32: (x - min_A) / (max_A - min_A) on A (zero range: 1), 0 elsewhere."""
    raw = np.asarray(raw, np.float32)
    allowed = np.broadcast_to(allowed, raw.shape)
    out = np.zeros_like(raw)
    for i in range(raw.shape[0]):
        a = allowed[i]
        if not a.any():
            continue
        mn, mx = np.float32(raw[i, a].min()), np.float32(raw[i, a].max())
        rng_ = np.float32(mx - mn)
        out[i, a] = 1.0 if rng_ == 0 else ((raw[i, a] - mn) / rng_).astype(np.float32)
    return out


def rank_prior_np(raw, allowed, k):
    """The dense ranking of the "seeds" scope: the masked prior's values ranked (score desc, larger index first) over A."""
    y = masked_prior_np(raw, allowed)
    allowed = np.broadcast_to(allowed, y.shape)
    idx = np.full((y.shape[0], k), -1, np.int32)
    val = np.zeros((y.shape[0], k), np.float32)
    for i in range(y.shape[0]):
        order = np.argsort(y[i], kind="stable")[::-1]
        order = order[allowed[i][order]][:k]
        idx[i, :len(order)] = order
        val[i, :len(order)] = y[i, order]
    return idx, val


def random_sources(n_f, n_p, rng, unsourced=0.1):
    row_ptr = np.zeros(n_f + 1, np.int64)
    pos = []
    for f in range(n_f):
        c = 0 if rng.random() < unsourced else int(rng.integers(1, 4))
        pos.extend(rng.choice(n_p, c, replace=False).tolist())
        row_ptr[f + 1] = len(pos)
    return row_ptr, np.asarray(pos, np.int32)


# ------------------------------------------------------------------ the fact bitset (hrag_fact_mask_from_docs)
@pytest.mark.parametrize("bit_offset", [0, 5, 31, 37])
def test_fact_mask_from_docs_against_numpy(gpu_device, bit_offset):
    import torch
    from hipporag_amd._lib import check, load
    from hipporag_amd.engine import _stream
    lib = load()
    rng = np.random.default_rng(100 + bit_offset)
    n_p, n_f, rows = 1000, 4099, 5
    row_ptr, pos = random_sources(n_f, n_p, rng)
    allowed = rng.random((rows, n_p)) < 0.05
    allowed[1] = False
    allowed[2] = True
    lead = rng.random((rows, bit_offset)) < 0.5               # bits before the offset must not be read as passages
    words = pack_mask(np.concatenate([lead, allowed], axis=1))
    fw = (n_f + 31) // 32
    d_rp = torch.from_numpy(row_ptr).to(gpu_device)
    d_pos = torch.from_numpy(pos).to(gpu_device)
    for ld in (words.shape[1], 0):
        doc = torch.from_numpy(words.view(np.int32)).to(gpu_device)
        n_rows = rows if ld else 1
        out = torch.empty((n_rows, fw), dtype=torch.int32, device=gpu_device)
        check(lib.hrag_fact_mask_from_docs(doc.data_ptr(), ld, bit_offset, n_p, n_rows, d_rp.data_ptr(), d_pos.data_ptr(),
                                           n_f, out.data_ptr(), _stream()))
        want = fact_mask_np(allowed if ld else allowed[:1], row_ptr, pos)
        np.testing.assert_array_equal(_np(out).view(np.uint32), pack_mask(want), err_msg=f"ld={ld}")
    assert not fact_mask_np(np.ones((1, n_p), bool), row_ptr, pos)[0][np.diff(row_ptr) == 0].any()


# ------------------------------------------------------------------ engines on one connected graph
@pytest.fixture(scope="module")
def case(gpu_device):
    from hipporag_amd._lib import OPT_NO_F16, OPT_NO_FP8
    from hipporag_amd.engine import HippoRAGEngine
    kg, pass_bits, fact_bits, index = make_case(12000, 100000, 64, seed=5151)
    rng = np.random.default_rng(7)
    row_ptr, pos = random_sources(kg.n_facts, kg.n_passages, rng)
    engines = {}
    for name, flags in (("default", 0), ("f32", OPT_NO_FP8 | OPT_NO_F16)):
        e = HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                           max_batch=130, max_topk=kg.n_passages, flags=flags)
        e.set_fact_sources(row_ptr, pos)
        engines[name] = e
    yield gpu_device, kg, pass_bits, fact_bits, engines, (row_ptr, pos)
    for e in engines.values():
        e.close()


@pytest.mark.parametrize("b", [1, 8, 16, 17, 40])
def test_scoped_phase_a_against_numpy(case, b):
    """B <= 16 and B > 16 (where the unscoped call takes the fused path) alike: the numpy restatement bit for bit."""
    import torch
    dev, kg, pass_bits, fact_bits, engines, (row_ptr, pos) = case
    eng = engines["default"]
    n_p = kg.n_passages
    qf = _bf16(synth.make_queries_np(fact_bits, b, seed=60 + b)[0], dev)
    raw = _np(eng.sim_scores("facts", qf))
    rng = np.random.default_rng(b)
    per_row = rng.random((b, n_p)) < 0.02
    per_row[0] = False                                       # no allowed fact
    if b > 2:
        per_row[1] = False
        per_row[1, 0] = True                                 # a single passage: its facts only (or none)
    one = rng.random(n_p) < 0.001
    for k in (1, 5, 16, 64):
        for m in (per_row, one):
            got_idx, got_sc = eng.score_facts(qf, k=k, scope_filter=_words(m, dev))
            allowed_f = fact_mask_np(m if m.ndim == 2 else m[None], row_ptr, pos)
            want_idx, want_sc = scoped_topk_np(raw, allowed_f, k)
            _same(_np(got_idx), _np(got_sc), want_idx, want_sc, f"b={b} k={k} shape={m.shape}")
    assert (_np(eng.score_facts(qf, k=5, scope_filter=_words(per_row, dev))[0])[0] == -1).all()
    # every passage allowed and every fact sourced: hrag_score_facts bit for bit (fused path for B > 16)
    all_src = np.arange(kg.n_facts + 1, dtype=np.int64), (np.arange(kg.n_facts) % n_p).astype(np.int32)
    from hipporag_amd.engine import HippoRAGEngine
    with HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                        max_batch=130, max_topk=64) as e2:
        e2.set_fact_sources(*all_src)
        for k in (5, 16):
            a_idx, a_sc = e2.score_facts(qf, k=k)
            s_idx, s_sc = e2.score_facts(qf, k=k, scope_filter=torch.ones(n_p, dtype=torch.bool))
            _same(_np(s_idx), _np(s_sc), _np(a_idx), _np(a_sc), f"all allowed b={b} k={k}")


STATES = [("small", "default", 5), ("f16", "default", 40), ("fp8", "default", 130), ("f32", "f32", 40)]


def _phase_b_inputs(dev, eng, fact_bits, pass_bits, b, seed, scope_filter):
    import torch
    qf = _bf16(synth.make_queries_np(fact_bits, b, seed=seed)[0], dev)
    qp = _bf16(synth.make_queries_np(pass_bits, b, seed=seed + 1)[0], dev)
    idx, sc = eng.score_facts(qf, k=5, scope_filter=scope_filter)
    cnt = (idx >= 0).sum(dim=1).to(torch.int32)
    cnt[::4] = 0                                            # DPR fallback rows
    return qp, idx, sc, cnt


@pytest.mark.parametrize("state,which,b", STATES)
def test_scoped_prior_is_the_masked_min_max_on_every_state(case, state, which, b):
    """hrag_retrieve_scored_scoped(raw, A) == hrag_retrieve_scored_filtered(prior_A(raw), A) bit for bit, where prior_A
    is the restated masked min-max (its own min / max are then 0 / 1: the unscoped normalisation is identity)."""
    dev, kg, pass_bits, fact_bits, engines, _ = case
    import torch
    eng = engines[which]
    n_p = kg.n_passages
    rng = np.random.default_rng(300 + b)
    per_row = rng.random((b, n_p)) < 0.2
    per_row[-1] = False                                      # an empty allowed set
    one = rng.random(n_p) < 0.3
    for m in (per_row, one):
        w = _words(m, dev)
        qp, idx, sc, cnt = _phase_b_inputs(dev, eng, fact_bits, pass_bits, b, 90 + b, w)
        raw = eng.sim_scores("passages", qp)
        prior = torch.from_numpy(masked_prior_np(_np(raw)[:, :n_p], m)).to(dev)
        for k in (10, 200):
            got = eng.retrieve_scored(raw, idx, sc, cnt, ppr_iters=20, k=k, doc_filter=w, filter_scope="seeds")
            want = eng.retrieve_scored(prior, idx, sc, cnt, ppr_iters=20, k=k, doc_filter=w)
            msg = f"{state} k={k} {m.shape}"
            _same(_np(got.doc_idx), _np(got.doc_score), _np(want.doc_idx), _np(want.doc_score), msg)
            np.testing.assert_array_equal(_np(got.flags), _np(want.flags), err_msg=msg)
            # the q_pass entry point scores the same passages
            got_q = eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=k, doc_filter=w, filter_scope="seeds")
            _same(_np(got_q.doc_idx), _np(got_q.doc_score), _np(got.doc_idx), _np(got.doc_score), msg + " q_pass")
        if m.ndim == 2:
            assert (_np(got.doc_idx)[-1] == -1).all() and (_np(got.doc_score)[-1] == 0).all()


@pytest.mark.parametrize("state,which,b", STATES)
def test_all_allowed_scoped_equals_the_unscoped_call(case, state, which, b):
    """Every passage allowed (and, through score_facts, every sourced fact): the unscoped hrag_retrieve bit for bit, also
    under the convergence contract."""
    import torch
    dev, kg, pass_bits, fact_bits, engines, _ = case
    eng = engines[which]
    allow = torch.ones(kg.n_passages, dtype=torch.bool)
    qp, idx, sc, cnt = _phase_b_inputs(dev, eng, fact_bits, pass_bits, b, 150 + b, None)
    for k in (10, 200):
        plain = eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=k)
        scoped = eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=k, doc_filter=allow, filter_scope="seeds")
        _same(_np(scoped.doc_idx), _np(scoped.doc_score), _np(plain.doc_idx), _np(plain.doc_score), f"{state} k={k}")
    plain = eng.retrieve_converged(qp, idx, sc, cnt, k=50)
    scoped = eng.retrieve_converged(qp, idx, sc, cnt, k=50, doc_filter=allow, filter_scope="seeds")
    _same(_np(scoped.doc_idx), _np(scoped.doc_score), _np(plain.doc_idx), _np(plain.doc_score), f"{state} converged")


def test_scoped_edge_cases_and_dense(case):
    import torch
    dev, kg, pass_bits, fact_bits, engines, (row_ptr, pos) = case
    eng = engines["default"]
    n_p = kg.n_passages
    b = 6
    qp = _bf16(synth.make_queries_np(pass_bits, b, seed=5)[0], dev)
    raw = _np(eng.sim_scores("passages", qp))[:, :n_p]
    m = np.zeros((b, n_p), bool)
    m[0, 17] = True                                          # a single allowed passage
    m[2] = True                                              # all allowed
    m[3, :40] = True
    m[4, [3, 9, 200]] = True
    # row 1: empty; row 5: all-equal allowed scores (three copies of one raw score)
    m[5, [10, 11, 12]] = True
    raw_eq = raw.copy()
    raw_eq[5, [10, 11, 12]] = raw_eq[5, 10]
    for k in (3, 50):
        idx, sc = eng.dense_retrieve(qp, k=k, doc_filter=torch.from_numpy(m), filter_scope="seeds")
        want_idx, want_sc = rank_prior_np(raw, m, k)
        _same(_np(idx), _np(sc), want_idx, want_sc, f"dense k={k}")
        assert _np(sc)[0, 0] == 1.0 and (_np(idx)[1] == -1).all()
    # all-equal allowed scores on the prior path (caller's raw scores): prior 1 on the three, 0 elsewhere
    kept = torch.full((b, 5), -1, dtype=torch.int32)
    ksc = torch.zeros((b, 5), dtype=torch.float32)
    cnt = torch.zeros((b,), dtype=torch.int32)               # every row on the DPR fallback: normalised over A
    out = eng.retrieve_scored(torch.from_numpy(raw_eq).to(dev), kept, ksc, cnt, ppr_iters=20, k=n_p,
                              doc_filter=torch.from_numpy(m), filter_scope="seeds")
    assert (_np(out.flags) & 1).all()
    want_idx, want_sc = rank_prior_np(raw_eq, m, n_p)
    _same(_np(out.doc_idx), _np(out.doc_score), want_idx, want_sc, "fallback over A")
    np.testing.assert_array_equal(_np(out.doc_score)[5, :3], np.ones(3, np.float32))
    last = _np(eng.last_doc_scores(b))[:, :n_p]
    rows = np.array([0, 2, 3, 4, 5])                        # (row 1, the empty set, carries no meaning)
    assert (last[rows][~m[rows]] == 0).all()                 # fallback rows: 0 outside A


def test_scoped_calls_need_sources_and_a_filter(case):
    import torch
    from hipporag_amd import _lib
    from hipporag_amd.engine import HippoRAGEngine
    dev, kg, pass_bits, fact_bits, engines, (row_ptr, pos) = case
    qf = _bf16(synth.make_queries_np(fact_bits, 2, seed=1)[0], dev)
    with HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                        max_batch=4, max_topk=10) as e:
        with pytest.raises(_lib.HragError, match="set_fact_sources"):
            e.score_facts(qf, k=5, scope_filter=torch.ones(kg.n_passages, dtype=torch.bool))
        with pytest.raises(_lib.HragError):
            e.set_fact_sources(row_ptr[:-1], pos)            # wrong fact count
        bad = pos.copy()
        bad[0] = kg.n_passages
        with pytest.raises(_lib.HragError):
            e.set_fact_sources(row_ptr, bad)
        w = e.workspace()
        with pytest.raises(_lib.HragError, match="workspace"):
            e.set_fact_sources(row_ptr, pos)
        w.close()
    with pytest.raises(ValueError):
        engines["default"].retrieve(_bf16(synth.make_queries_np(pass_bits, 2, seed=2)[0], dev),
                                    torch.zeros((2, 5), dtype=torch.int32), torch.zeros((2, 5)),
                                    torch.zeros(2, dtype=torch.int32), filter_scope="seeds")


def test_workspace_scoped_results_match_the_root(case):
    import threading

    import torch
    from hipporag_amd.engine import HippoRAGEngine
    dev, kg, pass_bits, fact_bits, engines, (row_ptr, pos) = case
    root = HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                          max_batch=64, max_topk=100)
    try:
        root.set_fact_sources(row_ptr, pos)
        ws = root.workspace()
        b = 40
        rng = np.random.default_rng(3)
        m = rng.random((b, kg.n_passages)) < 0.1
        qf = _bf16(synth.make_queries_np(fact_bits, b, seed=8)[0], dev)
        qp = _bf16(synth.make_queries_np(pass_bits, b, seed=9)[0], dev)

        def run(e):
            w = _words(m, dev)
            idx, sc = e.score_facts(qf, k=5, scope_filter=w)
            cnt = (idx >= 0).sum(dim=1).to(torch.int32)
            o = e.retrieve(qp, idx, sc, cnt, k=100, doc_filter=w, filter_scope="seeds")
            torch.cuda.current_stream().synchronize()
            return _np(idx), _np(sc), _np(o.doc_idx), _np(o.doc_score)

        want = run(root)
        got = {}

        def worker():
            with torch.cuda.stream(torch.cuda.Stream()):
                got["ws"] = run(ws)

        t = threading.Thread(target=worker)
        t.start()
        got["root"] = run(root)
        t.join()
        for name in ("ws", "root"):
            for g, w_ in zip(got[name], want):
                np.testing.assert_array_equal(g.view(np.int32), w_.view(np.int32), err_msg=name)
    finally:
        root.close()


# ------------------------------------------------------------------ tenant isolation on a disjoint union of corpora
TENANTS = ("alpha", "bravo", "charlie")


def _tenant_corpus(t, n_docs=14, seed=0):
    """Documents + triples of one tenant: entity names made from the tenant's own word, no word shared with another
    tenant's entities."""
    rng = np.random.default_rng(seed + 17 * TENANTS.index(t))
    ents = [f"{t}{w}" for w in ("stone", "river", "tower", "field", "cedar", "harbor", "lantern", "orchard", "meadow",
                                "quarry", "summit", "valley")]
    docs, triples = [], []
    for i in range(n_docs):
        a, b_, c = rng.choice(len(ents), 3, replace=False)
        docs.append(f"{t} note {i}: {ents[a]} borders {ents[b_]}; {ents[b_]} faces {ents[c]}.")
        triples.append([(ents[a], "borders", ents[b_]), (ents[b_], "faces", ents[c])])
    return docs, triples, ents


def _queries(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        t = TENANTS[i % 3]
        _, _, ents = _tenant_corpus(t)
        o = TENANTS[(i + 1) % 3]
        _, _, other = _tenant_corpus(o)
        out.append(f"q{i} where is {ents[int(rng.integers(len(ents)))]} near {other[int(rng.integers(len(other)))]}")
    return out


def _mirror(tenants, prec, accel):
    from hipporag_amd.retriever import Chunk, HippoRAG, RetrievalConfig
    from tests.golden.make_golden import MockEmbeddingModel
    rag = HippoRAG(RetrievalConfig(max_batch=256, retrieval_top_k=64, embedding_precision=prec, ppr_accel=accel),
                   embedding_model=MockEmbeddingModel())
    docs, triples = [], []
    for t in tenants:
        d, tr, _ = _tenant_corpus(t)
        docs += [Chunk(x, metadata={"tenant": t}) for x in d]
        triples += tr
    rag.index_from_openie(docs, triples)
    rag.prepare_retrieval_objects()
    return rag


def _check_equal(got, want, msg):
    assert len(got.docs) == len(want.docs), msg
    w_sc = np.asarray(want.doc_scores, np.float64)
    pos = {d: i for i, d in enumerate(want.docs)}
    assert set(got.docs) == set(want.docs), msg
    assert tie_aware_equal([pos[d] for d in got.docs], list(range(len(want.docs))), w_sc), msg
    np.testing.assert_allclose(np.asarray(got.doc_scores, np.float64), w_sc, rtol=1e-5, atol=1e-12, err_msg=msg)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("accel", [True, False])
def test_tenant_isolation(gpu_device, prec, accel):
    """A "seeds"-scoped query over tenant T of a shared index == the same query on an index of T alone; the "ranking"
    scope does not have this property (checked on the same case, so the test is known to discriminate)."""
    union = _mirror(TENANTS, prec, accel)
    alone = {t: _mirror([t], prec, accel) for t in TENANTS}
    queries = _queries(257, seed=11)
    n_t = 14
    broke = 0
    for b in (1, 8, 32, 257):
        qs = queries[:b]
        for t in TENANTS:
            want = alone[t].retrieve(qs, num_to_retrieve=n_t)
            got = union.retrieve(qs, num_to_retrieve=n_t, doc_filter={"tenant": t}, filter_scope="seeds")
            for i, (g, w) in enumerate(zip(got, want)):
                _check_equal(g, w, f"{prec} accel={accel} b={b} tenant={t} query={i}")
            post = union.retrieve(qs, num_to_retrieve=n_t, doc_filter={"tenant": t}, filter_scope="ranking")
            for g, w in zip(post, want):
                try:
                    _check_equal(g, w, "")
                except AssertionError:
                    broke += 1
        # per-query filters that mix tenants
        ten = [TENANTS[(i * 7) % 3] for i in range(b)]
        got = union.retrieve(qs, num_to_retrieve=n_t, doc_filter=[{"tenant": t} for t in ten], filter_scope="seeds")
        for i, (g, t) in enumerate(zip(got, ten)):
            _check_equal(g, alone[t].retrieve([qs[i]], num_to_retrieve=n_t)[0], f"{prec} per-query b={b} query={i}")
    assert broke > 0, "the post-filter gave the isolated results too: the case does not discriminate"
    # dense retrieval over A is isolated as well
    qs = queries[:8]
    for t in TENANTS:
        got = union.retrieve_dpr(qs, num_to_retrieve=n_t, doc_filter={"tenant": t}, filter_scope="seeds")
        want = alone[t].retrieve_dpr(qs, num_to_retrieve=n_t)
        for g, w in zip(got, want):
            _check_equal(g, w, f"dpr {t}")
    for r in [union] + list(alone.values()):
        r.engine.close()


def test_mirror_surface_with_seeds_scope(gpu_device):
    from hipporag_amd.retriever import QuerySolution
    union = _mirror(TENANTS, "bf16", True)
    qs = _queries(6, seed=3)
    allowed = {d for d, k in zip(union.passage_texts, union.passage_node_keys)
               if union.chunk_metadata[k]["tenant"] == "bravo"}
    f = {"tenant": "bravo"}
    for res in (union.retrieve(qs, num_to_retrieve=5, doc_filter=f, filter_scope="seeds"),
                union.retrieve_dpr(qs, num_to_retrieve=5, doc_filter=f, filter_scope="seeds"),
                union.retrieve_ircot(qs, max_qa_steps=2, num_to_retrieve=5, doc_filter=f, filter_scope="seeds",
                                     reason_fn=lambda q, docs, th: "thinking about " + q)):
        for r in res:
            assert r.docs and set(r.docs) <= allowed
    union.global_config.doc_filter_scope = "seeds"           # the config default
    union.qa_fn = lambda sols: (sols, [], {})
    sols, _, _ = union.rag_qa(qs, doc_filter=f)
    assert all(isinstance(s, QuerySolution) and set(s.docs) <= allowed for s in sols)
    want = union.retrieve(qs, num_to_retrieve=5, doc_filter=f, filter_scope="seeds")
    got = union.retrieve(qs, num_to_retrieve=5, doc_filter=f)
    assert [g.docs for g in got] == [w.docs for w in want]
    # beyond max_topk: ranked on the host from every passage's score, the scope kept
    eng = union.engine
    saved = eng.max_topk
    try:
        eng.max_topk = 2
        got_b = union.retrieve(qs, num_to_retrieve=10, doc_filter=f)
        got_d = union.retrieve_dpr(qs, num_to_retrieve=10, doc_filter=f)
    finally:
        eng.max_topk = saved
    want_b = union.retrieve(qs, num_to_retrieve=10, doc_filter=f)
    want_d = union.retrieve_dpr(qs, num_to_retrieve=10, doc_filter=f)
    for g, w in zip(got_b + got_d, want_b + want_d):
        assert g.docs == w.docs
        np.testing.assert_allclose(g.doc_scores, w.doc_scores, rtol=1e-6)
    eng.close()
