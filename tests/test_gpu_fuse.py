"""Fused retrieval on the device (include/hrag.h "fused retrieval", csrc/fuse.hip): hrag_fuse_rows and hrag_rrf_rows against
the numpy restatement of tests/fuse_helpers.py bit for bit; hrag_last_fused behind Engine.retrieve on the small-batch, the
two-stage fp16 and the e4m3 PPR state paths against the restatement applied to hrag_last_doc_scores; its composition with
the doc filter, grouped retrieval, group hits, the convergence contract and HRAG_OPT_ACCEL; workspaces, argument errors,
and the mirror's retrieve_fused.  No tolerances anywhere."""

import threading

import numpy as np
import pytest

from hipporag_amd import synth
from hipporag_amd.engine import pack_mask
from oracle.checks import make_case
from tests.fuse_helpers import fuse_np, partitions, rank_np, rrf_np
from tests.group_helpers import group_rank_np, random_groups, same_bits
from tests.group_hits_helpers import group_hits_np

pytestmark = pytest.mark.gpu

GUARD = np.float32(-7.25)


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


def _lib():
    from hipporag_amd import _lib
    return _lib.load(), _lib.check


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


SHAPES = [(1000, 1), (777, 8), (4099, 9), (5003, 64), (2048, 256)]


@pytest.mark.parametrize("n,b", SHAPES)
def test_fuse_rows_against_numpy(gpu_device, n, b):
    import torch
    lib, check = _lib()
    rng = np.random.default_rng(n + b)
    x = _scores(rng, b, n)
    w = (rng.random(b) * 4).astype(np.float32)
    w[rng.integers(0, b)] = 0
    ld, tail = n + 3, 64
    w_d = torch.from_numpy(w).to(gpu_device)
    for name, mp in partitions(rng, b).items():
        mp_d = torch.from_numpy(mp).to(gpu_device)
        nq = len(mp) - 1
        for mode, code, weights in (("sum", 0, None), ("sum", 0, w), ("max", 1, None)):
            want = fuse_np(x, mp, mode, weights)
            # the float4 route needs 16-byte rows: ld = n + 3 is not a multiple of 4 for every n here but 2048 + 3 -- run the
            # aligned layout (ld rounded up to 4) as well, with the same guards
            for ld_ in (ld, (n + 3 + 3) // 4 * 4):
                h = np.full(b * ld_ + tail, GUARD, np.float32)                # pad columns and a guard behind the buffer
                h[:b * ld_].reshape(b, ld_)[:, :n] = x
                d = torch.from_numpy(h).to(gpu_device)
                check(lib.hrag_fuse_rows(d.data_ptr(), b, n, ld_, mp_d.data_ptr(), nq,
                                         w_d.data_ptr() if weights is not None else None, code, _stream()))
                got = _np(d)
                rows = got[:b * ld_].reshape(b, ld_)
                assert same_bits(rows[:nq, :n], want), (name, mode, weights is not None, ld_)
                assert (rows[:, n:] == GUARD).all() and (got[b * ld_:] == GUARD).all(), (name, mode, ld_)
                assert (rows[:nq, :n].view(np.uint32)[np.isnan(rows[:nq, :n])] == 0x7fc00000).all()


@pytest.mark.parametrize("n,b", SHAPES)
def test_rrf_rows_against_numpy(gpu_device, n, b):
    import torch
    lib, check = _lib()
    rng = np.random.default_rng(7 * n + b)
    w = (rng.random(b) * 4).astype(np.float32)
    w[rng.integers(0, b)] = 0
    w_d = torch.from_numpy(w).to(gpu_device)
    ld, tail = n + 3, 64
    for name, mp in partitions(rng, b).items():
        mp_d = torch.from_numpy(mp).to(gpu_device)
        nq = len(mp) - 1
        for depth in (1, 200, 2500):
            d_ = min(depth, n)                                             # 2500 is clamped to n
            # every member of a question lists the SAME passages in its own order (heavy ties), with -1 slots
            lists = np.full((b, d_), -1, np.int32)
            for q in range(nq):
                pool = rng.choice(n, d_, replace=False).astype(np.int32)
                for i in range(mp[q], mp[q + 1]):
                    lists[i] = rng.permutation(pool)
            lists[rng.random(lists.shape) < 0.1] = -1
            l_d = torch.from_numpy(lists).to(gpu_device)
            for c in (0, 60):
                for weights in (None, w):
                    out = torch.full((nq * ld + tail,), float(GUARD), dtype=torch.float32, device=gpu_device)
                    check(lib.hrag_rrf_rows(l_d.data_ptr(), b, d_, mp_d.data_ptr(), nq,
                                            w_d.data_ptr() if weights is not None else None, c, out.data_ptr(), n, ld,
                                            _stream()))
                    got = _np(out)
                    rows = got[:nq * ld].reshape(nq, ld)
                    want = rrf_np(lists, mp, n, weights, c)
                    assert np.array_equal(rows[:, :n].view(np.uint32), want.view(np.uint32)), (name, depth, c)
                    assert (rows[:, n:] == GUARD).all() and (got[nq * ld:] == GUARD).all(), (name, depth, c)


# ------------------------------------------------------------------ engines
@pytest.fixture(scope="module")
def case(gpu_device):
    from hipporag_amd.engine import HippoRAGEngine
    kg, pass_bits, fact_bits, _ = make_case(24000, 200000, 64, seed=6262)
    g = random_groups(np.random.default_rng(2), kg.n_passages, "shuffled")
    eng = HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                         max_batch=130, max_topk=kg.n_passages)
    eng.set_passage_groups(g)
    yield gpu_device, kg, pass_bits, fact_bits, eng, g
    eng.close()


def _inputs(dev, eng, fact_bits, pass_bits, b, seed):
    import torch
    qf = _bf16(synth.make_queries_np(fact_bits, b, seed=seed)[0], dev)
    qp = _bf16(synth.make_queries_np(pass_bits, b, seed=seed + 1)[0], dev)
    idx, sc = eng.score_facts(qf, k=5)
    cnt = torch.full((b,), 5, dtype=torch.int32, device=dev)
    cnt[::4] = 0                                            # DPR fallback rows (kept_count 0)
    return qp, idx, sc, cnt


def _check_ranking(out, fused, k, allowed, msg):
    wi, ws = rank_np(fused, k, allowed)
    assert np.array_equal(_np(out.doc_idx), wi), msg
    assert same_bits(_np(out.doc_score), ws), msg
    assert (_np(out.doc_score).view(np.uint32)[_np(out.doc_idx) < 0] == 0).all(), msg


STATES = [("small", 5, 4, {}), ("f16", 40, 2, {}), ("fp8", 130, 8, {}),
          ("fp8-tol", 130, 8, dict(ppr_tol=1.5e-6, ppr_max_iters=30)), ("fp8-accel", 130, 8, "accel")]


@pytest.mark.parametrize("state,b,want_state,setup", STATES)
def test_last_fused_behind_retrieve(case, state, b, want_state, setup):
    from hipporag_amd._lib import OPT_ACCEL
    dev, kg, pass_bits, fact_bits, eng, g = case
    n_p = kg.n_passages
    rng = np.random.default_rng(b)
    qp, idx, sc, cnt = _inputs(dev, eng, fact_bits, pass_bits, b, 30 + b)
    kw = dict(setup) if isinstance(setup, dict) else {}
    w = (rng.random(b) * 4).astype(np.float32)
    w[1] = 0
    if setup == "accel":
        eng.set_flags(OPT_ACCEL, True)
    try:
        def member_rows():
            eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=1, **kw)
            assert eng.stats()["last_ppr_state"] == want_state
            return _np(eng.last_doc_scores(b))

        parts = partitions(rng, b)
        for name, mp in parts.items():
            nq = len(mp) - 1
            per = rng.random((nq, n_p)) < 0.3
            per[-1] = False                                          # a question with no allowed passage
            one = rng.random(n_p) < 0.05
            for mode, weights in (("sum", w), ("sum", None), ("max", None), ("rrf", w), ("rrf", None)):
                for flt in ((None, per, one) if name == "random" else (None,)):
                    for k in ((1, 200, 2500) if flt is None and name in ("random", "one") else (200,)):
                        c, depth = (60, 200) if k != 1 else (0, 7)
                        full = member_rows()                         # every fusion works on the rows of a fresh retrieve
                        out = eng.last_fused(mp, weights=weights, fuse=mode, rrf_c=c, rrf_depth=depth, k=k,
                                             doc_filter=None if flt is None else _words(flt, dev))
                        fused = fuse_np(full, mp, mode, weights, c, depth, flt)
                        msg = f"{state} {name} {mode} w={weights is not None} k={k} flt={None if flt is None else flt.shape}"
                        assert same_bits(_np(eng.last_doc_scores(nq)), fused), msg
                        _check_ranking(out, fused, k, flt, msg)
                        if flt is per:
                            assert (_np(out.doc_idx)[-1] == -1).all() and (_np(out.doc_score)[-1].view(np.uint32) == 0).all()
        # grouped outputs and group hits over the fused rows
        mp = parts["random"]
        nq = len(mp) - 1
        per = rng.random((nq, n_p)) < 0.4
        for mode, agg in (("sum", "sum"), ("max", "max"), ("rrf", "sum")):
            for flt in (None, per):
                full = member_rows()
                out = eng.last_fused(mp, weights=w if mode != "max" else None, fuse=mode, rrf_depth=150, k=40,
                                     doc_filter=None if flt is None else _words(flt, dev), group_agg=agg, group_hits=3)
                fused = fuse_np(full, mp, mode, w if mode != "max" else None, 60, 150, flt)
                assert same_bits(_np(eng.last_doc_scores(nq)), fused)
                gi, gs, rep, hi, hs = (_np(t) for t in (out.group_idx, out.group_score, out.best_doc_idx, out.hit_idx,
                                                        out.hit_score))
                for q in range(nq):
                    a = None if flt is None else flt[q]
                    e = group_rank_np(fused[q], g, a, 40, agg)
                    assert gi[q].tolist() == e[0].tolist() and rep[q].tolist() == e[2].tolist(), (state, mode, q)
                    assert same_bits(gs[q], e[1]), (state, mode, q)
                    h = group_hits_np(fused[q], g, a, gi[q], 3)
                    assert hi[q].tolist() == h[0].tolist() and same_bits(hs[q], h[1]), (state, mode, q)
    finally:
        if setup == "accel":
            eng.set_flags(OPT_ACCEL, False)


def test_both_output_sets_and_a_second_fusion_above_the_new_batch(case):
    import torch
    from hipporag_amd import _lib
    dev, kg, pass_bits, fact_bits, eng, g = case
    lib = _lib.load()
    n_p, b = kg.n_passages, 12
    qp, idx, sc, cnt = _inputs(dev, eng, fact_bits, pass_bits, b, 5)
    eng.retrieve(qp, idx, sc, cnt, k=1)
    full = _np(eng.last_doc_scores(b))
    mp = np.array([0, 3, 4, 12], np.int32)
    ws = torch.empty((int(lib.hrag_fuse_workspace_bytes(b, n_p, 0, 0, 0)),), dtype=torch.uint8, device=dev)
    di, gi, bi = (torch.empty((3, 9), dtype=torch.int32, device=dev) for _ in range(3))
    ds, gs = (torch.empty((3, 9), dtype=torch.float32, device=dev) for _ in range(2))

    def call(batch, ptr, nq):
        return lib.hrag_last_fused(eng._handle, batch, ptr.ctypes.data, nq, None, 0, 0, 0, 9, None, 0, 1, di.data_ptr(),
                                   ds.data_ptr(), gi.data_ptr(), gs.data_ptr(), bi.data_ptr(), ws.data_ptr(), ws.numel(),
                                   _stream())

    assert call(b, mp, 3) == _lib.HRAG_OK
    fused = fuse_np(full, mp, "sum")
    wi, wsc = rank_np(fused, 9)
    assert np.array_equal(_np(di), wi) and same_bits(_np(ds), wsc)
    for q in range(3):
        e = group_rank_np(fused[q], g, None, 9, "sum")
        assert _np(gi)[q].tolist() == e[0].tolist() and _np(bi)[q].tolist() == e[2].tolist() and same_bits(_np(gs)[q], e[1])
    # the rows are a batch of 3 now: a fusion of 3 rows works, one of 4 is refused
    assert call(4, np.array([0, 4], np.int32), 1) == _lib.HRAG_EINVAL and b"exceeds" in lib.hrag_last_error()
    assert call(3, np.array([0, 1, 3], np.int32), 2) == _lib.HRAG_OK
    assert same_bits(_np(eng.last_doc_scores(2)), fuse_np(fused, [0, 1, 3], "sum"))


def test_workspace_handle_on_a_second_thread_gives_identical_bits(case):
    import torch
    dev, kg, pass_bits, fact_bits, eng, g = case
    b = 40
    mp = partitions(np.random.default_rng(9), b)["random"]
    w = (np.random.default_rng(10).random(b) * 4).astype(np.float32)

    def run(h, inputs):
        outs = []
        for mode in ("sum", "max", "rrf"):
            h.retrieve(*inputs, k=1)
            o = h.last_fused(mp, weights=None if mode == "max" else w, fuse=mode, rrf_depth=100, k=50, group_agg="sum",
                             group_hits=2)
            outs += [o.group_idx, o.group_score, o.best_doc_idx, o.hit_idx, o.hit_score, h.last_doc_scores(len(mp) - 1)]
        return outs

    in_a, in_b = _inputs(dev, eng, fact_bits, pass_bits, b, 11), _inputs(dev, eng, fact_bits, pass_bits, b, 21)
    ref_a, ref_b = [t.clone() for t in run(eng, in_a)], [t.clone() for t in run(eng, in_b)]
    torch.cuda.synchronize()
    wk = eng.workspace()
    errors, start = [], threading.Barrier(2)

    def worker(handle, inputs, ref, name):
        try:
            torch.cuda.set_device(dev)
            stream = torch.cuda.Stream(device=dev)
            start.wait()
            with torch.cuda.stream(stream):
                for _ in range(3):
                    got = run(handle, inputs)
                    stream.synchronize()
                    for x, r in zip(got, ref):
                        if not torch.equal(x.view(torch.int32), r.view(torch.int32)):
                            raise AssertionError(f"{name}: result differs from the sequential call")
        except Exception as exc:
            errors.append((name, repr(exc)))

    ts = [threading.Thread(target=worker, args=(eng, in_a, ref_a, "engine")),
          threading.Thread(target=worker, args=(wk, in_b, ref_b, "workspace"))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    wk.close()
    assert not errors, errors


def test_argument_errors_leave_the_handle_usable(case):
    import torch
    from hipporag_amd import _lib, dist
    from hipporag_amd.engine import HippoRAGEngine
    dev, kg, pass_bits, fact_bits, eng, g = case
    lib = _lib.load()
    n_p, b = kg.n_passages, 6
    qp, idx, sc, cnt = _inputs(dev, eng, fact_bits, pass_bits, b, 3)
    eng.retrieve(qp, idx, sc, cnt, k=1)
    full = _np(eng.last_doc_scores(b))
    ws = torch.empty((int(lib.hrag_fuse_workspace_bytes(b, n_p, 2, 50, 1)) + 16,), dtype=torch.uint8, device=dev)
    di = torch.full((b, 5), 7, dtype=torch.int32, device=dev)
    ds = torch.full((b, 5), 7.0, dtype=torch.float32, device=dev)
    good = np.array([0, 2, 6], np.int32)
    ones = np.ones(b, np.float32)
    short = torch.zeros((2, 3), dtype=torch.int32, device=dev)

    def call(e=eng, batch=b, ptr=good, nq=2, w=None, mode=0, c=60, depth=50, k=5, fw=None, fld=0, agg=-1, ws_ptr=None,
             ws_bytes=None, di_ptr=di.data_ptr()):
        return lib.hrag_last_fused(e._handle, batch, ptr.ctypes.data if ptr is not None else None, nq,
                                   w.ctypes.data if w is not None else None, mode, c, depth, k, fw, fld, agg, di_ptr,
                                   ds.data_ptr(), None, None, None, ws.data_ptr() if ws_ptr is None else ws_ptr,
                                   ws.numel() - 16 if ws_bytes is None else ws_bytes, _stream())

    def bad_w(v):
        x = ones.copy()
        x[3] = v
        return x

    bad = [dict(ptr=np.array([0, 2, 2], np.int32)), dict(ptr=np.array([0, 3, 2, 6], np.int32), nq=3),
           dict(ptr=np.array([1, 2, 6], np.int32)), dict(ptr=np.array([0, 2, 5], np.int32)), dict(ptr=None), dict(nq=0),
           dict(nq=7, ptr=np.arange(8, dtype=np.int32)), dict(mode=3), dict(mode=-1),
           dict(mode=1, w=ones), dict(w=bad_w(-1.0)), dict(w=bad_w(np.nan)), dict(w=bad_w(np.inf)),
           dict(mode=2, depth=0), dict(mode=2, depth=n_p + 1), dict(mode=2, c=-1), dict(k=0), dict(k=n_p + 1),
           dict(fw=short.data_ptr(), fld=3), dict(agg=2), dict(ws_bytes=8), dict(ws_ptr=ws.data_ptr() + 4),
           dict(di_ptr=None)]
    for kw in bad:
        assert call(**kw) == _lib.HRAG_EINVAL, kw
        torch.cuda.synchronize()
        assert bool((di == 7).all()) and bool((ds == 7.0).all()), kw
        assert same_bits(_np(eng.last_doc_scores(b)), full), kw            # the rows and their batch are what they were
    assert call(batch=0) == _lib.HRAG_ECAPACITY and call(batch=131) == _lib.HRAG_ECAPACITY
    assert call(mode=2, w=ones) == _lib.HRAG_OK                            # and the good call still works
    fused = fuse_np(full, good, "rrf", ones, 60, 50)
    wi, wsc = rank_np(fused, 5)
    assert np.array_equal(_np(di)[:2], wi) and same_bits(_np(ds)[:2], wsc)
    with pytest.raises(ValueError):
        eng.last_fused([0, 2, 2], fuse="sum")
    # a fresh handle has no rows; an ungrouped dense call writes none
    wk = eng.workspace()
    try:
        assert call(e=wk) == _lib.HRAG_EINVAL and b"no score rows" in lib.hrag_last_error()
        wk.dense_retrieve(qp, k=5)
        assert call(e=wk) == _lib.HRAG_EINVAL and b"no score rows" in lib.hrag_last_error()
        wk.retrieve(qp, idx, sc, cnt, k=1)
        assert call(e=wk) == _lib.HRAG_OK
        torch.cuda.synchronize()
    finally:
        wk.close()
    # grouping outputs without a group table; a row-shard engine
    bare = HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                          max_batch=8, max_topk=10)
    try:
        bare.retrieve(qp, idx, sc, cnt, k=1)
        with pytest.raises(_lib.HragError, match="hrag_engine_set_passage_groups"):
            bare.last_fused(good, fuse="sum", k=5, group_agg="max")
        assert _np(bare.last_fused(good, fuse="sum", k=5).doc_idx).shape == (2, 5)
    finally:
        bare.close()
    sidx = dist.shard_index(kg.csr, kg.passage_vertex, 2, kg.subj_vertex, kg.obj_vertex, kg.num_chunks)
    sh = dist.build_shard_engine(sidx, pass_bits, fact_bits, 1, max_batch=8, max_topk=10)
    try:
        assert call(e=sh) == _lib.HRAG_EINVAL and b"row-shard" in lib.hrag_last_error()
    finally:
        sh.close()
    # the engine-free calls
    x = torch.zeros((4, 100), dtype=torch.float32, device=dev)
    ptr = torch.tensor([0, 4], dtype=torch.int32, device=dev)
    lists = torch.zeros((4, 10), dtype=torch.int32, device=dev)
    wd = torch.ones((4,), dtype=torch.float32, device=dev)
    s = _stream()
    for args in ((None, 4, 100, 100, ptr.data_ptr(), 1, None, 0), (x.data_ptr(), 0, 100, 100, ptr.data_ptr(), 1, None, 0),
                 (x.data_ptr(), 4, 100, 99, ptr.data_ptr(), 1, None, 0), (x.data_ptr(), 4, 0, 100, ptr.data_ptr(), 1, None, 0),
                 (x.data_ptr(), 4, 100, 100, None, 1, None, 0), (x.data_ptr(), 4, 100, 100, ptr.data_ptr(), 5, None, 0),
                 (x.data_ptr(), 4, 100, 100, ptr.data_ptr(), 0, None, 0), (x.data_ptr(), 4, 100, 100, ptr.data_ptr(), 1, None, 2),
                 (x.data_ptr(), 4, 100, 100, ptr.data_ptr(), 1, wd.data_ptr(), 1)):
        assert lib.hrag_fuse_rows(*args, s) == _lib.HRAG_EINVAL, args
    for args in ((None, 4, 10, ptr.data_ptr(), 1, None, 60, x.data_ptr(), 100, 100),
                 (lists.data_ptr(), 4, 0, ptr.data_ptr(), 1, None, 60, x.data_ptr(), 100, 100),
                 (lists.data_ptr(), 4, 10, ptr.data_ptr(), 1, None, -1, x.data_ptr(), 100, 100),
                 (lists.data_ptr(), 4, 10, ptr.data_ptr(), 1, None, 60, None, 100, 100),
                 (lists.data_ptr(), 4, 10, ptr.data_ptr(), 1, None, 60, x.data_ptr(), 100, 99)):
        assert lib.hrag_rrf_rows(*args, s) == _lib.HRAG_EINVAL, args
    assert lib.hrag_fuse_rows(x.data_ptr(), 4, 100, 100, ptr.data_ptr(), 1, wd.data_ptr(), 0, s) == _lib.HRAG_OK
    torch.cuda.synchronize()


def test_mirror_retrieve_fused(gpu_device):
    from hipporag_amd.retriever import HippoRAG, RetrievalConfig, Chunk
    from tools import real2wiki as rw
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "support", "adapter_on_real_reference.py")
    spec = importlib.util.spec_from_file_location("adapter_on_real_reference", path)
    sup = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sup)
    docs, triples = rw.openie_inputs(600)
    chunks = [Chunk(d, source_id=f"src{i // 4}") for i, d in enumerate(docs)]
    rag = HippoRAG(RetrievalConfig(embedding_precision="bf16", max_batch=16, retrieval_top_k=len(docs), ppr_tol=0.0,
                                   ppr_accel=False), embedding_model=sup.Bf16Mock())
    rag.index_from_openie(chunks, triples)
    n_p = len(rag.passage_node_keys)
    pos = {t: i for i, t in enumerate(rag.passage_texts)}
    queries = [" ".join(triples[i][0]) for i in range(0, 600, 13) if triples[i]][:20]
    plain = rag.retrieve(queries, num_to_retrieve=n_p)
    # one-member questions under "max": exactly what retrieve() returns (two device batches of max_batch = 16)
    single = rag.retrieve_fused([[q] for q in queries], fuse="max", num_to_retrieve=25)
    for q, p, f in zip(queries, plain, single):
        assert f.question == q and f.docs == p.docs[:25]
        assert np.array_equal(np.asarray(f.doc_scores, np.float32).view(np.uint32),
                              np.asarray(p.doc_scores[:25], np.float32).view(np.uint32))

    def by_pos(r):
        row = np.zeros(n_p, np.float32)
        row[[pos[d] for d in r.docs]] = np.asarray(r.doc_scores, np.float32)
        return row

    # a two-paraphrase question under "rrf": the restatement over the two retrieve() score rows; a filter; weights
    # (the member rows of that call are a batch of three: the same three queries through retrieve() give the same bits)
    rows = np.stack([by_pos(r) for r in rag.retrieve(queries[:3], num_to_retrieve=n_p)])
    allowed = np.arange(n_p) % 3 != 0
    for kw, flt, w in ((dict(), None, None), (dict(rrf_c=10, rrf_depth=30), allowed, [[2.0, 0.5], [1.0]])):
        got = rag.retrieve_fused([queries[:2], [queries[2]]], fuse="rrf", num_to_retrieve=20, doc_filter=flt, weights=w, **kw)
        fused = fuse_np(rows, [0, 2, 3], "rrf", None if w is None else np.concatenate(w), kw.get("rrf_c", 60),
                        kw.get("rrf_depth", 20), flt)
        wi, ws = rank_np(fused, 20, flt)
        assert got[0].question == queries[0] and got[1].question == queries[2]
        for q in range(2):
            assert got[q].docs == [rag.passage_texts[p] for p in wi[q]]
            assert same_bits(np.asarray(got[q].doc_scores, np.float32), ws[q])
    # "sum" grouped by source, and the host form beyond the engine's max_topk agrees with the device form
    small = HippoRAG(RetrievalConfig(embedding_precision="bf16", max_batch=16, retrieval_top_k=5, ppr_tol=0.0,
                                     ppr_accel=False), embedding_model=sup.Bf16Mock())
    small.index_from_openie(chunks, triples)
    qs = [queries[:3], queries[3:5]]
    for kw in (dict(fuse="sum", weights=[[1, 2, 0.5], [1, 1]]), dict(fuse="max"), dict(fuse="rrf", rrf_depth=5),
               dict(fuse="sum", group_by="source_id", group_agg="sum", group_hits=2)):
        a = rag.retrieve_fused(qs, num_to_retrieve=15, **kw)
        b = small.retrieve_fused(qs, num_to_retrieve=15, **kw)
        for x, y in zip(a, b):
            assert x.docs == y.docs and len(x.docs) == 15
            assert same_bits(np.asarray(x.doc_scores, np.float32), np.asarray(y.doc_scores, np.float32))
            assert [m.get("group_hits") for m in x.doc_metadata] == [m.get("group_hits") for m in y.doc_metadata]
    with pytest.raises(ValueError, match="max_batch"):
        rag.retrieve_fused([queries[:17]], fuse="sum")
