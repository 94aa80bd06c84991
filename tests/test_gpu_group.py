"""Grouped retrieval on the device (include/hrag.h, csrc/group.hip): hrag_group_rows against the numpy restatement of
tests/group_helpers.py bit for bit, the grouped engine calls on every PPR state path against the restatement applied to
hrag_last_doc_scores, their composition with the doc filter / the "seeds" scope / the convergence contract /
HRAG_OPT_ACCEL, workspaces (bf16 and f32 engines), the mirror, and the argument errors."""

import threading

import numpy as np
import pytest

from hipporag_amd import synth
from hipporag_amd.engine import pack_mask
from oracle.checks import make_case
from tests.group_helpers import (canonical, csr_of, dedup_full_ranking, group_rank_np, group_reduce_np, random_groups,
                                 same_bits)

pytestmark = pytest.mark.gpu
AGG = {"max": 0, "sum": 1}


def _bf16(bits, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)


def _np(t):
    return t.cpu().numpy()


def _words(m, dev):
    import torch
    return torch.from_numpy(pack_mask(m).view(np.int32)).to(dev)


def _scores(rng, b, n):
    x = (rng.integers(-40, 40, (b, n)).astype(np.float32) / 8 * rng.random((b, n)).astype(np.float32)).astype(np.float32)
    for i in range(b):
        at = rng.integers(0, n, 6)
        x[i, at[0]] = np.nan
        x[i, at[1]] = np.inf
        x[i, at[2]] = -np.inf
        x[i, at[3]] = -0.0
        x[i, at[4]] = x[i, at[5]]
    return x


def _group_rows(dev, x, ld, g, n_groups, agg, mask=None, per_query=True, bit_offset=0):
    import torch
    from hipporag_amd import _lib
    lib = _lib.load()
    b, n = x.shape
    xd = torch.zeros((b, ld), dtype=torch.float32)
    xd[:, :n] = torch.from_numpy(x)
    xd = xd.to(dev)
    ptr, members = csr_of(g, n_groups)
    ptr_d, mem_d = torch.from_numpy(ptr).to(dev), torch.from_numpy(members).to(dev)
    out_ld = n_groups + 5
    gs = torch.full((b, out_ld), 7.0, dtype=torch.float32, device=dev)
    gb = torch.full((b, out_ld), 7, dtype=torch.int32, device=dev)
    w, wld = None, 0
    if mask is not None:
        rng = np.random.default_rng(bit_offset + 1)
        rows = mask if per_query else mask[:1]
        wide = np.concatenate([rng.random((rows.shape[0], bit_offset)) < 0.5, rows, rng.random((rows.shape[0], 37)) < 0.5], axis=1)
        w = _words(wide, dev)
        wld = w.shape[1] if per_query else 0
    _lib.check(lib.hrag_group_rows(xd.data_ptr(), b, n, ld, ptr_d.data_ptr(), mem_d.data_ptr(), n_groups, AGG[agg],
                                   w.data_ptr() if w is not None else None, wld, bit_offset, gs.data_ptr(), gb.data_ptr(),
                                   out_ld, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    gs, gb = _np(gs), _np(gb)
    assert (gs[:, n_groups:] == 7.0).all() and (gb[:, n_groups:] == 7).all()          # nothing written past n_groups
    return gs[:, :n_groups], gb[:, :n_groups]


SHAPES = [("one", 1000, 1), ("singletons", 777, 8), ("two", 4099, 9), ("contiguous", 5003, 64), ("shuffled", 6001, 65),
          ("power", 3000, 2), ("contiguous", 2048, 256)]


@pytest.mark.parametrize("kind,n,b", SHAPES)
@pytest.mark.parametrize("agg", ["max", "sum"])
def test_group_rows_against_numpy(gpu_device, kind, n, b, agg):
    rng = np.random.default_rng(n + b)
    g = random_groups(rng, n, kind)
    n_groups = int(g.max()) + 1
    x = _scores(rng, b, n)
    mask = rng.random((b, n)) < 0.4
    mask[0] = False
    for m, per_query, off in ((None, True, 0), (mask, True, 0), (mask, True, 13), (mask, False, 45)):
        gs, gb = _group_rows(gpu_device, x, n + 3, g, n_groups, agg, m, per_query, off)
        for i in range(b):
            a = None if m is None else (m[i] if per_query else m[0])
            ws, wb = group_reduce_np(x[i], g, a, n_groups, agg)
            assert gb[i].tolist() == wb.tolist(), (kind, agg, i, off)
            assert same_bits(gs[i], ws), (kind, agg, i, off)


@pytest.mark.parametrize("agg", ["max", "sum"])
def test_group_rows_power_law_with_one_group_beyond_50000_members(gpu_device, agg):
    rng = np.random.default_rng(3)
    n = 70001
    small = random_groups(rng, n - 52000, "power")
    g = np.concatenate([small, np.full(52000, small.max() + 1, np.int32)])
    g = g[rng.permutation(n)]
    n_groups = int(g.max()) + 1
    x = _scores(rng, 3, n)
    x[1] = np.abs(x[1]) * np.float32(1e-5)                   # PPR-like: small positive numbers of mixed size, no NaN
    mask = rng.random((3, n)) < 0.7
    for m in (None, mask):
        gs, gb = _group_rows(gpu_device, x, n + 3, g, n_groups, agg, m)
        for i in range(3):
            ws, wb = group_reduce_np(x[i], g, None if m is None else m[i], n_groups, agg)
            assert gb[i].tolist() == wb.tolist() and same_bits(gs[i], ws), (agg, i)


# ------------------------------------------------------------------ engines
@pytest.fixture(scope="module")
def case(gpu_device):
    from hipporag_amd._lib import OPT_NO_F16, OPT_NO_FP8
    from hipporag_amd.engine import HippoRAGEngine
    kg, pass_bits, fact_bits, index = make_case(24000, 200000, 64, seed=6161)
    rng = np.random.default_rng(1)
    g = random_groups(rng, kg.n_passages, "shuffled")
    engines = {}
    for name, flags in (("default", 0), ("f32", OPT_NO_FP8 | OPT_NO_F16)):
        e = HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                           max_batch=256, max_topk=kg.n_passages, flags=flags)
        engines[name] = e
    yield gpu_device, kg, pass_bits, fact_bits, engines, g
    for e in engines.values():
        e.close()


def _inputs(dev, eng, fact_bits, pass_bits, b, seed):
    import torch
    qf = _bf16(synth.make_queries_np(fact_bits, b, seed=seed)[0], dev)
    qp = _bf16(synth.make_queries_np(pass_bits, b, seed=seed + 1)[0], dev)
    idx, sc = eng.score_facts(qf, k=5)
    cnt = torch.full((b,), 5, dtype=torch.int32, device=dev)
    cnt[::4] = 0                                            # DPR fallback rows
    return qp, idx, sc, cnt


def _check_rows(out, full, g, n_groups, allowed, k, agg, msg):
    gi, gs, rep = _np(out.group_idx), _np(out.group_score), _np(out.best_doc_idx)
    for i in range(full.shape[0]):
        a = None if allowed is None else (allowed if allowed.ndim == 1 else allowed[i])
        e = group_rank_np(full[i], g, a, k, agg, n_groups)
        assert gi[i].tolist() == e[0].tolist() and rep[i].tolist() == e[2].tolist(), (msg, i)
        assert same_bits(gs[i], e[1]), (msg, i)


STATES = [("small1", "default", 1, 4), ("small8", "default", 8, 4), ("f16", "default", 64, 2), ("fp8", "default", 256, 8),
          ("f32", "f32", 40, 1)]


@pytest.mark.parametrize("state,which,b,want_state", STATES)
def test_grouped_retrieve_on_every_state_path(case, state, which, b, want_state):
    dev, kg, pass_bits, fact_bits, engines, g = case
    eng = engines[which]
    n_p, n_groups = kg.n_passages, int(g.max()) + 1
    qp, idx, sc, cnt = _inputs(dev, eng, fact_bits, pass_bits, b, 40 + b)
    eng.set_passage_groups(None)
    before = eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=n_p)
    eng.set_passage_groups(g)
    plain = eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=n_p)
    assert eng.stats()["last_ppr_state"] == want_state
    for a_, b_ in ((plain.doc_idx, before.doc_idx), (plain.doc_score, before.doc_score), (plain.flags, before.flags)):
        assert np.array_equal(_np(a_).view(np.int32), _np(b_).view(np.int32))           # ungrouped calls: unchanged
    assert (_np(plain.flags)[::4] & 1).all()
    skipped = total = 0
    for agg in ("max", "sum"):
        for k in (10, 2500, n_groups + 7):                   # k > 2048: the large-k path; k > G
            out = eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=k, group_agg=agg)
            assert eng.stats()["last_ppr_state"] == want_state
            full = _np(eng.last_doc_scores(b))
            _check_rows(out, full, g, n_groups, None, k, agg, f"{state} {agg} k={k}")
            for a_, b_ in ((out.flags, plain.flags), (out.residual, plain.residual), (out.iters_used, plain.iters_used)):
                assert np.array_equal(_np(a_).view(np.int32), _np(b_).view(np.int32)), (state, agg, k)
            if agg == "max":                                 # == the existing call's full ranking, repeats dropped
                pi, ps = _np(plain.doc_idx), _np(plain.doc_score)
                for i in range(b):
                    total += 1
                    by_pos = np.zeros(n_p, np.float32)
                    by_pos[pi[i]] = ps[i]
                    want = dedup_full_ranking(by_pos, g, None, k)
                    if want is None:
                        skipped += 1
                        continue
                    _, first = np.unique(g[pi[i]], return_index=True)
                    keep = pi[i][np.sort(first)][:k]
                    m = len(keep)
                    assert _np(out.best_doc_idx)[i, :m].tolist() == keep.tolist(), (state, i)
                    assert _np(out.group_idx)[i, :m].tolist() == g[keep].tolist()
                    assert same_bits(_np(out.group_score)[i, :m], by_pos[keep])
    assert skipped <= 0.10 * total, (skipped, total)
    # retrieve_scored: the same rows through the other entry point
    raw = eng.sim_scores("passages", qp)
    a1 = eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=50, group_agg="sum")
    a1 = [_np(t).copy() for t in (a1.group_idx, a1.group_score, a1.best_doc_idx)]
    a2 = eng.retrieve_scored(raw, idx, sc, cnt, ppr_iters=20, k=50, group_agg="sum")
    for x, y in zip(a1, (a2.group_idx, a2.group_score, a2.best_doc_idx)):
        assert np.array_equal(x.view(np.int32), _np(y).view(np.int32))


@pytest.mark.parametrize("state,which,b,want_state", [STATES[1], STATES[2], STATES[3]])
def test_grouped_composes_with_filter_scope_contract_and_accel(case, state, which, b, want_state):
    import torch
    from hipporag_amd._lib import OPT_ACCEL
    dev, kg, pass_bits, fact_bits, engines, g = case
    eng = engines[which]
    eng.set_passage_groups(g)
    n_p, n_groups = kg.n_passages, int(g.max()) + 1
    qp, idx, sc, cnt = _inputs(dev, eng, fact_bits, pass_bits, b, 70 + b)
    rng = np.random.default_rng(b)
    per = rng.random((b, n_p)) < 0.3
    per[-1] = False
    one = rng.random(n_p) < 0.05
    for m in (per, one):
        w = _words(m, dev)
        for agg in ("max", "sum"):
            for scope in ("ranking", "seeds"):
                out = eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=100, doc_filter=w, filter_scope=scope, group_agg=agg)
                full = _np(eng.last_doc_scores(b))
                _check_rows(out, full, g, n_groups, m, 100, agg, f"{state} {agg} {scope} {m.shape}")
                ref = eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=100, doc_filter=w, filter_scope=scope)
                assert np.array_equal(_np(out.flags), _np(ref.flags))
    assert (_np(out.group_idx)[-1] == -1).all() or m.ndim == 1
    # the convergence contract and the accelerated plan: whatever scores they leave, the groups are formed over them
    for setup in ("tol", "accel"):
        if setup == "accel":
            eng.set_flags(OPT_ACCEL, True)
        try:
            kw = dict(ppr_iters=20, ppr_tol=1.5e-6, ppr_max_iters=30) if setup == "tol" else dict(ppr_iters=20)
            out = eng.retrieve(qp, idx, sc, cnt, k=64, group_agg="sum", **kw)
            full = _np(eng.last_doc_scores(b))
            _check_rows(out, full, g, n_groups, None, 64, "sum", f"{state} {setup}")
            ref = eng.retrieve(qp, idx, sc, cnt, k=64, **kw)
            for a_, b_ in ((out.flags, ref.flags), (out.residual, ref.residual), (out.iters_used, ref.iters_used)):
                assert np.array_equal(_np(a_).view(np.int32), _np(b_).view(np.int32)), (state, setup)
        finally:
            if setup == "accel":
                eng.set_flags(OPT_ACCEL, False)


def test_grouped_dense_retrieve(case):
    dev, kg, pass_bits, fact_bits, engines, g = case
    eng = engines["default"]
    eng.set_passage_groups(g)
    n_p, n_groups = kg.n_passages, int(g.max()) + 1
    qp = _bf16(synth.make_queries_np(pass_bits, 33, seed=5)[0], dev)
    pi, ps = (_np(t) for t in eng.dense_retrieve(qp, k=n_p))
    full = np.zeros((33, n_p), np.float32)
    np.put_along_axis(full, pi.astype(np.int64), ps, axis=1)          # the normalised dense scores by position
    m = np.random.default_rng(2).random((33, n_p)) < 0.2
    for agg in ("max", "sum"):
        for mask in (None, m):
            kw = {} if mask is None else {"doc_filter": _words(mask, dev)}
            gi, gs, rep = (_np(t) for t in eng.dense_retrieve(qp, k=40, group_agg=agg, **kw))
            for i in range(33):
                e = group_rank_np(full[i], g, None if mask is None else mask[i], 40, agg, n_groups)
                assert gi[i].tolist() == e[0].tolist() and rep[i].tolist() == e[2].tolist() and same_bits(gs[i], e[1])


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_workspaces_grouped_and_ungrouped_two_threads_bit_identical(gpu_device, precision):
    """Two threads, two streams, one index; on an embedding_precision="f32" engine as well (HRAG_F32_SPLIT: the
    split-query buffer of a workspace), where the ungrouped score_facts / retrieve / dense_retrieve are covered too."""
    import torch
    from hipporag_amd.engine import HippoRAGEngine
    from hipporag_amd.graph import bf16_bits_to_float
    dev = gpu_device
    kg, pass_bits, fact_bits, _ = make_case(6000, 60000, 128, seed=4343)
    pe, fe = (pass_bits, fact_bits) if precision == "bf16" else (bf16_bits_to_float(pass_bits), bf16_bits_to_float(fact_bits))
    g = random_groups(np.random.default_rng(4), kg.n_passages, "contiguous")

    def q(bits, b, seed):
        qb = synth.make_queries_np(bits, b, seed=seed)[0]
        return _bf16(qb, dev) if precision == "bf16" else torch.from_numpy(bf16_bits_to_float(qb)).to(dev)

    def run(h, qf, qp):
        b = qf.shape[0]
        idx, sc = h.score_facts(qf, k=5)
        cnt = torch.full((b,), 5, dtype=torch.int32, device=dev)
        o = h.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=50)
        gm = h.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=50, group_agg="max")
        gsum = h.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=50, group_agg="sum")
        d = h.dense_retrieve(qp, k=50)
        dg = h.dense_retrieve(qp, k=50, group_agg="sum")
        return [idx, sc, o.doc_idx, o.doc_score, o.flags, gm.group_idx, gm.group_score, gm.best_doc_idx, gsum.group_idx,
                gsum.group_score, gsum.best_doc_idx, *d, *dg]

    with HippoRAGEngine(kg.csr, kg.passage_vertex, pe, fe, kg.subj_vertex, kg.obj_vertex, kg.num_chunks, max_batch=130,
                        max_topk=50) as eng:
        ws0 = eng.stats()["workspace_bytes"]
        eng.set_passage_groups(g)
        assert eng.stats()["workspace_bytes"] > ws0                     # the group rows are booked with the workspace half
        for batch in (9, 130):
            qa, qb = (q(fact_bits, batch, 11), q(pass_bits, batch, 12)), (q(fact_bits, batch, 21), q(pass_bits, batch, 22))
            ref_a = [t.clone() for t in run(eng, *qa)]
            ref_b = [t.clone() for t in run(eng, *qb)]
            torch.cuda.synchronize()
            w = eng.workspace()
            assert w.stats()["workspace_bytes"] == eng.stats()["workspace_bytes"]
            errors, start = [], threading.Barrier(2)

            def worker(handle, qq, ref, name):
                try:
                    torch.cuda.set_device(dev)
                    stream = torch.cuda.Stream(device=dev)
                    start.wait()
                    with torch.cuda.stream(stream):
                        for _ in range(5):
                            got = run(handle, *qq)
                            stream.synchronize()
                            for x, r in zip(got, ref):
                                if not torch.equal(x.view(torch.int32), r.view(torch.int32)):
                                    raise AssertionError(f"{name}: result differs from the sequential call")
                except Exception as exc:
                    errors.append((name, repr(exc)))

            ts = [threading.Thread(target=worker, args=(eng, qa, ref_a, "engine")),
                  threading.Thread(target=worker, args=(w, qb, ref_b, "workspace"))]
            for t in ts:
                t.start()
            for t in ts:
                t.join(timeout=300)
            assert not errors, errors
            w.close()


def test_argument_errors_are_checks_before_any_launch(case):
    import torch
    from hipporag_amd import _lib
    from hipporag_amd._lib import HragError
    from hipporag_amd.engine import HippoRAGEngine
    dev, kg, pass_bits, fact_bits, engines, g = case
    eng = engines["default"]
    lib = _lib.load()
    qp, idx, sc, cnt = _inputs(dev, eng, fact_bits, pass_bits, 4, 3)
    eng.set_passage_groups(None)
    with pytest.raises(HragError, match="hrag_engine_set_passage_groups") as ei:
        eng.retrieve(qp, idx, sc, cnt, k=5, group_agg="max")
    assert ei.value.status == _lib.HRAG_EINVAL
    with pytest.raises(HragError):
        eng.dense_retrieve(qp, k=5, group_agg="max")
    bad = g.copy()
    bad[5] = -1
    with pytest.raises(ValueError):
        eng.set_passage_groups(bad)
    arr = np.ascontiguousarray(g, np.int32)
    st = lib.hrag_engine_set_passage_groups(eng._handle, arr.ctypes.data, int(g.max()))       # one id out of range
    assert st == _lib.HRAG_EINVAL and b"outside" in lib.hrag_last_error()
    eng.set_passage_groups(g)
    with pytest.raises(ValueError):
        eng.retrieve(qp, idx, sc, cnt, k=5, group_agg="mean")
    gi = torch.empty((4, 5), dtype=torch.int32, device=dev)
    gs = torch.empty((4, 5), dtype=torch.float32, device=dev)
    st = lib.hrag_dense_retrieve_grouped(eng._handle, qp.data_ptr(), 4, 5, None, None, None, None, 0, 0, 2,
                                         gi.data_ptr(), gs.data_ptr(), gi.data_ptr())
    assert st == _lib.HRAG_EINVAL and b"agg" in lib.hrag_last_error()
    w = eng.workspace()
    try:
        with pytest.raises(ValueError):
            w.set_passage_groups(g)
        st = lib.hrag_engine_set_passage_groups(w._handle, arr.ctypes.data, int(g.max()) + 1)   # a workspace handle
        assert st == _lib.HRAG_EINVAL
        st = lib.hrag_engine_set_passage_groups(eng._handle, arr.ctypes.data, int(g.max()) + 1)  # live workspaces
        assert st in (_lib.HRAG_EINVAL, _lib.HRAG_EBUSY) and b"workspace" in lib.hrag_last_error()
    finally:
        w.close()
    eng.set_passage_groups(g)                                                                   # accepted again
    # a row-shard engine
    from hipporag_amd import dist
    sidx = dist.shard_index(kg.csr, kg.passage_vertex, 2, kg.subj_vertex, kg.obj_vertex, kg.num_chunks)
    sh = dist.build_shard_engine(sidx, pass_bits, fact_bits, 1, max_batch=8, max_topk=10)
    try:
        ga = np.zeros(kg.n_passages, np.int32)
        st = lib.hrag_engine_set_passage_groups(sh._handle, ga.ctypes.data, 1)
        assert st == _lib.HRAG_EINVAL and b"row-shard" in lib.hrag_last_error()
    finally:
        sh.close()


def test_mirror_group_by_equals_grouping_the_full_ranking_on_the_host(gpu_device):
    from hipporag_amd.retriever import HippoRAG, RetrievalConfig, Chunk
    from tools import real2wiki as rw
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "support", "adapter_on_real_reference.py")
    spec = importlib.util.spec_from_file_location("adapter_on_real_reference", path)
    sup = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sup)
    docs, triples = rw.openie_inputs(600)
    chunks = [Chunk(d, source_id=f"src{i // 4}") if i % 50 else Chunk(d) for i, d in enumerate(docs)]
    rag = HippoRAG(RetrievalConfig(embedding_precision="bf16", max_batch=16, retrieval_top_k=len(docs), ppr_tol=0.0,
                                   ppr_accel=False), embedding_model=sup.Bf16Mock())
    rag.index_from_openie(chunks, triples)
    n_p = len(rag.passage_node_keys)
    group_of, values, sizes = rag.group_table("source_id")
    pos = {t: i for i, t in enumerate(rag.passage_texts)}
    queries = [" ".join(triples[i][0]) for i in range(0, 600, 41) if triples[i]][:12]
    for fn in (rag.retrieve, rag.retrieve_dpr):
        full = fn(queries, num_to_retrieve=n_p)
        for agg in ("max", "sum"):
            got = fn(queries, num_to_retrieve=15, group_by="source_id", group_agg=agg)
            for f, gq in zip(full, got):
                by_pos = np.zeros(n_p, np.float32)
                by_pos[[pos[d] for d in f.docs]] = np.asarray(f.doc_scores, np.float32)
                e = group_rank_np(by_pos, group_of, None, 15, agg, len(values))
                assert [pos[d] for d in gq.docs] == e[2].tolist(), (fn.__name__, agg)
                assert same_bits(np.asarray(gq.doc_scores, np.float32), e[1])
                assert [m["group"] for m in gq.doc_metadata] == [values[j] for j in e[0]]
                assert [m["group_size"] for m in gq.doc_metadata] == [int(sizes[j]) for j in e[0]]
