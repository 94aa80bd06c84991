"""The doc filter's "seeds" scope on the multi-GPU paths (include/hrag.h: hrag_shard_score_facts_scoped,
hrag_shard_passage_scores_scoped, hrag_shard_mask_prior, hrag_shard_score_facts_all_scoped, hrag_shard_retrieve_scoped;
hipporag_amd/dist.py): row shards as threads on one device (dist.LocalComm), the hybrid mode, and two processes over gloo.
Every scoped result must be BIT-IDENTICAL to HippoRAGEngine.score_facts(scope_filter=) + retrieve(filter_scope="seeds")
of the unsharded engine on the same index and filter -- the bar the unscoped shard paths meet against the unscoped
engine (tests/test_gpu_shard.py)."""

import os
import socket

import numpy as np
import pytest

from hipporag_amd import synth
from tests.helpers import make_case, tie_aware_equal

pytestmark = pytest.mark.gpu

KW = dict(link_top_k=5, damping=0.5, passage_node_weight=0.05, ppr_iters=20)


def _bf16(bits, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)


def _fact_sources(n_f, n_p, seed):
    """fact -> 1 or 2 source passages among the first 90 % of the passages (the rest source no fact)."""
    rng = np.random.default_rng(seed)
    counts = 1 + (rng.random(n_f) < 0.3)
    row_ptr = np.zeros(n_f + 1, np.int64)
    np.cumsum(counts, out=row_ptr[1:])
    return row_ptr, rng.integers(0, int(n_p * 0.9), row_ptr[-1]).astype(np.int32)


def _case(world, b, seed, dev):
    import torch
    from hipporag_amd import dist as hd
    kg, pass_bits, fact_bits, _ = make_case(12000, 120000, 128, seed=seed, power_law=(world == 3))
    sidx = hd.shard_index(kg.csr, kg.passage_vertex, world, kg.subj_vertex, kg.obj_vertex, kg.num_chunks)
    n_p, n_f = len(kg.passage_vertex), len(kg.subj_vertex)
    fsrc = _fact_sources(n_f, n_p, seed)
    qp_bits = synth.make_queries_np(pass_bits, b, seed=4)[0]
    if b > 7:
        qp_bits[7] = 0                                          # every passage score 0: a tied prior
    qf, qp = _bf16(synth.make_queries_np(fact_bits, b, seed=3)[0], dev), _bf16(qp_bits, dev)
    return kg, pass_bits, fact_bits, sidx, fsrc, qf, qp


def _tenant_rows(sidx, fsrc, b, world, seed):
    """Per-query rows mixing tenants (two halves of the index, 10 % of each) and every edge case."""
    rng = np.random.default_rng(seed)
    n_p = len(sidx.passage_vertex)
    row_ptr, pos = fsrc
    tenant = np.arange(n_p) % 2
    m = (rng.random((b, n_p)) < 0.1) & (tenant[None, :] == (np.arange(b) % 2)[:, None])
    if world > 1:
        lo1, hi1 = sidx.passages[1]
        m[:, lo1:hi1] = False                                  # shard 1 holds no allowed passage
    edge = {}
    if b > 9:
        m[3] = False                                           # empty A
        edge["empty"] = 3
        m[6] = False
        m[6, pos[0]] = True                                    # a single allowed passage
        m[7] = True                                            # all allowed, tied scores
        f_lo, f_hi = sidx.facts[world - 1]                     # no fact of the last shard allowed
        src = np.zeros(n_p, bool)
        src[pos[row_ptr[f_lo]:row_ptr[f_hi]]] = True
        m[8] = (rng.random(n_p) < 0.3) & ~src
        m[9] = False
        m[9, int(n_p * 0.9):] = True                           # passages without facts: the DPR fallback
        edge["dpr"] = 9
    return m, edge


def _engine(sidx, pass_bits, fact_bits, fsrc, b, k, **kw):
    from hipporag_amd.engine import HippoRAGEngine
    eng = HippoRAGEngine(sidx.csr, sidx.passage_vertex, pass_bits, fact_bits, sidx.subj_vertex, sidx.obj_vertex,
                         sidx.num_chunks, max_batch=max(b, 65), max_topk=k, **kw)
    eng.set_fact_sources(*fsrc)
    return eng


def _single(eng, qf, qp, filt, k, **kw):
    import torch
    idx, sc = eng.score_facts(qf, k=5, scope_filter=filt)
    cnt = (idx >= 0).sum(1).to(torch.int32)
    out = eng.retrieve(qp, idx, sc, cnt, k=k, doc_filter=filt, filter_scope="seeds", **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (idx, sc, out.doc_idx, out.doc_score, out.flags, out.residual, out.iters_used)
            if t is not None]


def _cnt_from_ids(idx, sc):
    return idx, sc, (idx >= 0).sum(1).to(idx.dtype)


def _bits_equal(got, want, what):
    for g, w, name in zip(got, want, ("fact ids", "fact scores", "doc ids", "doc scores", "flags")):
        g, w = np.asarray(g), np.asarray(w)
        if g.dtype == np.float32:
            g, w = g.view(np.int32), w.view(np.int32)
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


@pytest.mark.parametrize("world,b,groups,native,one_row", [
    (1, 70, 1, False, False), (2, 257, 2, True, True), (3, 70, 0, False, False), (3, 70, 2, True, False),
    (8, 257, 2, False, False), (8, 1, 1, True, True), (2, 1, 2, False, False)])
def test_scoped_shards_are_bit_identical_to_the_single_engine(gpu_device, world, b, groups, native, one_row):
    import torch
    from hipporag_amd import dist as hd
    kg, pass_bits, fact_bits, sidx, fsrc, qf, qp = _case(world, b, 820 + world, gpu_device)
    m, edge = _tenant_rows(sidx, fsrc, b, world, 5)
    if world > 1:
        assert any(lo % 32 for lo, _ in sidx.passages[1:])    # a shard's slice starts inside a word
    filt = torch.from_numpy(m[min(1, b - 1)] if one_row else m).to(gpu_device)
    kw = dict(KW, k=100, doc_filter=filt, filter_scope="seeds")
    got = hd.run_local_shards(world, sidx, pass_bits, fact_bits, qf, qp, kw, groups, gpu_device, 100,
                              filter_fn=_cnt_from_ids, native=native, fact_sources=fsrc)
    with _engine(sidx, pass_bits, fact_bits, fsrc, b, 100) as eng:
        one = _single(eng, qf, qp, filt, 100, **KW)
    _bits_equal(got[:2], one[:2], "phase A")
    if b > 64:                        # the single engine's staged fp8 PPR (the one the shards run) serves batch > 64
        _bits_equal(got, one, f"world {world}")
        if "empty" in edge and not one_row:
            assert (got[2][edge["empty"]] == -1).all() and (got[3][edge["empty"]] == 0).all()
            assert got[4][edge["dpr"]] & 1
            assert (got[2][edge["dpr"]] >= 0).any()
    else:
        # batch 1: the single engine runs its small-batch PPR there, the shards their fp8 state -- the Python host loop
        # and the one-call driver on the same shards agree bit for bit, the single engine within the parity bar
        other = hd.run_local_shards(world, sidx, pass_bits, fact_bits, qf, qp, kw, groups, gpu_device, 100,
                                    filter_fn=_cnt_from_ids, native=not native, fact_sources=fsrc)
        _bits_equal(got, other, f"world {world} native vs Python loop")
        n = int((one[2][0] >= 0).sum())
        assert n == int((got[2][0] >= 0).sum()) > 0
        assert tie_aware_equal(got[2][0][:n], one[2][0][:n], one[3][0][:n], rel_gap=2e-5)
        np.testing.assert_allclose(got[3][0][:n], one[3][0][:n], rtol=1e-5)


def test_all_allowed_equals_the_unscoped_shards_and_ranking_differs(gpu_device):
    """Every passage allowed: the scoped shards give the unscoped shards' result bit for bit.  A real filter: the
    "ranking" scope (the post-filter) gives a different answer for some query -- the scope is not a no-op."""
    import torch
    from hipporag_amd import dist as hd
    world, b = 2, 70
    kg, pass_bits, fact_bits, sidx, fsrc, qf, qp = _case(world, b, 851, gpu_device)
    n_p = len(sidx.passage_vertex)
    every = torch.ones((n_p,), dtype=torch.bool, device=gpu_device)
    run = lambda kw, **x: hd.run_local_shards(world, sidx, pass_bits, fact_bits, qf, qp, kw, 2, gpu_device, 100,
                                              filter_fn=_cnt_from_ids, fact_sources=fsrc, **x)
    plain = run(dict(KW, k=100))
    scoped = run(dict(KW, k=100, doc_filter=every, filter_scope="seeds"))
    _bits_equal(scoped, plain, "all allowed")
    m, _ = _tenant_rows(sidx, fsrc, b, world, 6)
    filt = torch.from_numpy(m).to(gpu_device)
    seeds = run(dict(KW, k=100, doc_filter=filt, filter_scope="seeds"))
    ranking = run(dict(KW, k=100, doc_filter=filt))
    assert not np.array_equal(seeds[0], ranking[0])
    assert not np.array_equal(seeds[2], ranking[2])


@pytest.mark.parametrize("native", [False, True])
def test_scoped_convergence_contract_on_shards(gpu_device, native):
    """ppr_tol > 0: residual and sweeps used equal the single engine's scoped call, bit for bit."""
    import threading
    import torch
    from hipporag_amd import dist as hd
    from hipporag_amd.engine import ShardStages
    world, b, tol = 4, 130, 1e-7
    kg, pass_bits, fact_bits, sidx, fsrc, qf, qp = _case(world, b, 861, gpu_device)
    m, _ = _tenant_rows(sidx, fsrc, b, world, 7)
    filt = torch.from_numpy(m).to(gpu_device)
    kw = dict(KW, k=100, ppr_tol=tol, ppr_max_iters=29)
    shared, results, errors = {}, [None] * world, []

    def worker(rank):
        try:
            torch.cuda.set_device(gpu_device)
            eng = hd.build_shard_engine(sidx, pass_bits, fact_bits, rank, max_batch=b, max_topk=100, sell_seg_len=64,
                                        fact_sources=fsrc)
            cls = hd.NativeShardedRetriever if native else hd.ShardedRetriever
            rs = cls(ShardStages(eng), hd.LocalComm(rank, world, shared), groups=2)
            idx, sc = rs.score_facts(qf, k=5, scope_filter=filt)
            out = rs.retrieve(qp, idx, sc, (idx >= 0).sum(1).to(torch.int32), doc_filter=filt, filter_scope="seeds", **kw)
            torch.cuda.synchronize()
            results[rank] = [t.cpu().numpy() for t in (idx, sc) + tuple(out)]
            shared["_barrier"].wait()
            eng.close()
        except Exception as exc:
            errors.append((rank, exc))
            try:
                shared["_barrier"].abort()
            except Exception:
                pass

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    assert not errors, errors
    for r in range(1, world):
        for a, w in zip(results[r], results[0]):
            np.testing.assert_array_equal(a, w)
    with _engine(sidx, pass_bits, fact_bits, fsrc, b, 100, sell_seg_len=64) as eng:
        one = _single(eng, qf, qp, filt, 100, **dict(KW, ppr_tol=tol, ppr_max_iters=29))
    _bits_equal(results[0][:5], one[:5], "contract")
    np.testing.assert_array_equal(results[0][5].view(np.int32), one[5].view(np.int32))    # residual
    np.testing.assert_array_equal(results[0][6], one[6])                                  # sweeps used
    assert int(one[6].max()) > 20


def test_scoped_shards_k3000_through_the_large_merge(gpu_device):
    import torch
    from hipporag_amd import dist as hd
    world, b, k = 2, 70, 3000
    kg, pass_bits, fact_bits, sidx, fsrc, qf, qp = _case(world, b, 871, gpu_device)
    m, _ = _tenant_rows(sidx, fsrc, b, world, 8)
    m[11] = True
    filt = torch.from_numpy(m).to(gpu_device)
    for native in (False, True):
        got = hd.run_local_shards(world, sidx, pass_bits, fact_bits, qf, qp,
                                  dict(KW, k=k, doc_filter=filt, filter_scope="seeds"), 2, gpu_device, k,
                                  filter_fn=_cnt_from_ids, native=native, fact_sources=fsrc)
        with _engine(sidx, pass_bits, fact_bits, fsrc, b, k) as eng:
            one = _single(eng, qf, qp, filt, k, **KW)
        _bits_equal(got, one, f"k={k} native={native}")


@pytest.mark.parametrize("world,b", [(2, 70), (4, 260)])
def test_scoped_hybrid_is_bit_identical_to_the_single_engine(gpu_device, world, b):
    import torch
    from hipporag_amd import dist as hd
    from hipporag_amd.engine import HippoRAGEngine
    kg, pass_bits, fact_bits, sidx, fsrc, qf, qp = _case(world, b, 880 + world, gpu_device)
    m, _ = _tenant_rows(sidx, fsrc, b, world, 9)
    filt = torch.from_numpy(m).to(gpu_device)
    arrays = dict(csr=kg.csr, passage_vertex=kg.passage_vertex, subj_vertex=kg.subj_vertex, obj_vertex=kg.obj_vertex,
                  num_chunks=kg.num_chunks)
    kw = dict(KW, k=100, doc_filter=filt, filter_scope="seeds")
    f_idx, f_sc, d_idx, d_sc, flags = hd.run_local_hybrid(world, arrays, sidx, pass_bits, fact_bits, qf, qp, kw,
                                                          gpu_device, 100, fact_sources=fsrc)
    bn = b // world
    with HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex,
                        kg.num_chunks, max_batch=b, max_topk=100) as eng:
        eng.set_fact_sources(*fsrc)
        idx, sc = eng.score_facts(qf, k=5, scope_filter=filt)
        _bits_equal((f_idx, f_sc), (idx.cpu().numpy(), sc.cpu().numpy()), "hybrid phase A")
        cnt = (idx >= 0).sum(1).to(torch.int32)                 # what run_local_hybrid keeps in the scope
        for r in range(world):
            sl = slice(r * bn, (r + 1) * bn)
            one = eng.retrieve(qp[sl], idx[sl], sc[sl], cnt[sl], k=100, doc_filter=filt[sl], filter_scope="seeds", **KW)
            _bits_equal((d_idx[sl], d_sc[sl], flags[sl]),
                        tuple(t.cpu().numpy() for t in (one.doc_idx, one.doc_score, one.flags)), f"hybrid rank {r}")


def test_single_engine_scoped_calls_refuse_a_row_shard(gpu_device):
    import torch
    from hipporag_amd import dist as hd
    from hipporag_amd._lib import HragError
    from hipporag_amd.engine import doc_filter_words
    world, b = 2, 8
    kg, pass_bits, fact_bits, sidx, fsrc, qf, qp = _case(world, b, 891, gpu_device)
    eng = hd.build_shard_engine(sidx, pass_bits, fact_bits, 1, max_batch=b, max_topk=10, fact_sources=fsrc)
    try:
        assert eng.has_fact_sources
        filt = torch.ones((len(sidx.passage_vertex),), dtype=torch.bool, device=gpu_device)
        with pytest.raises(HragError, match="hrag_shard_score_facts_scoped"):
            eng.score_facts(qf, k=5, scope_filter=filt)
        # the shard steps: a NULL filter is refused
        from hipporag_amd import _lib
        lib = _lib.load()
        t = torch.empty((b,), dtype=torch.float32, device=gpu_device)
        st = lib.hrag_shard_mask_prior(eng._handle, t.data_ptr(), t.data_ptr(), b, t.data_ptr(), t.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream, None, 0)
        assert st == _lib.HRAG_EINVAL
        fw, _ = doc_filter_words(filt, len(sidx.passage_vertex), b, gpu_device)
        assert fw.numel() > 0
    finally:
        eng.close()


# ------------------------------------------------------------------ two processes over gloo
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gloo_worker(rank, world, port, ret):
    import torch
    import torch.distributed as dist
    from hipporag_amd import dist as hd
    from hipporag_amd.engine import ShardStages
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        b = 257
        kg, pass_bits, fact_bits, sidx, fsrc, qf, qp = _case(world, b, 901, dev)
        m, _ = _tenant_rows(sidx, fsrc, b, world, 10)
        filt = torch.from_numpy(m).to(dev)
        seng = hd.build_shard_engine(sidx, pass_bits, fact_bits, rank, max_batch=b, max_topk=100, sell_seg_len=64,
                                     fact_sources=fsrc)
        outs = []
        for cls in (hd.ShardedRetriever, hd.NativeShardedRetriever):
            rs = cls(ShardStages(seng), hd.HostStagedComm(rank, world), groups=2)
            idx, sc = rs.score_facts(qf, k=5, scope_filter=filt)
            out = rs.retrieve(qp, idx, sc, (idx >= 0).sum(1).to(torch.int32), k=100, doc_filter=filt,
                              filter_scope="seeds", **KW)
            torch.cuda.synchronize()
            outs.append([t.cpu().numpy() for t in (idx, sc) + tuple(out)])
        with _engine(sidx, pass_bits, fact_bits, fsrc, b, 100, sell_seg_len=64) as eng:
            one = _single(eng, qf, qp, filt, 100, **KW)
        for o in outs:
            _bits_equal(o, one, f"gloo rank {rank}")
        seng.close()
        ret[rank] = 1
    finally:
        dist.destroy_process_group()


def test_two_processes_over_gloo_scoped_match_the_single_engine():
    import torch.multiprocessing as mp
    ret = mp.Manager().dict()
    mp.spawn(_gloo_worker, args=(2, _free_port(), ret), nprocs=2, join=True)
    assert dict(ret) == {0: 1, 1: 1}
