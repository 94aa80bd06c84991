"""The first true residual of the e4m3-state PPR, stored or recomputed (csrc/ppr8.hip modes B0N / B1).

By default the first sweep does not store the fp32 R_1 and the boundary that closes stage 2 forms it again in registers
from c_0 -- the same loads and the same fp32 operations in the same order as the first sweep.  HRAG_OPT_STORE_R1 keeps
the stored form.  Nothing a caller can see may depend on the choice: ranked passages, scores, flags, the contract's
residual and the sweep count are compared with np.array_equal, flag off against flag on, over the shapes that pick
different kernels and plans (slab pairs, an odd last slab, partly filled slabs, long rows, the accelerated and the
tolerance plan, sweep counts that the fp8 state does not serve at all) and against the 8-shard emulated run."""

import numpy as np
import pytest

from hipporag_amd import synth
from hipporag_amd._lib import OPT_ACCEL, OPT_STORE_R1
from tests.helpers import make_case

pytestmark = pytest.mark.gpu

FIELDS = ("doc_idx", "doc_score", "flags", "residual", "iters_used")


def _bf16(bits, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(device).view(torch.bfloat16)


def _both(eng, qp, idx, sc, cnt, **kw):
    """The same call with R_1 recomputed (the default) and stored; returns the two outputs as dicts of numpy arrays.
    recomputed: whether the default is expected to take modes B0N / B1 (hrag_stats.ppr8_r1_long_rows >= 0: the plan's own
    word, so a plan condition that stopped matching cannot pass as stored-against-stored); None: the e4m3 state does not
    serve the call at all."""
    import torch
    recomputed = kw.pop("recomputed", True)
    outs = []
    for store in (False, True):
        eng.set_flags(OPT_STORE_R1, store)
        out = eng.retrieve(qp, idx, sc, cnt, **kw)
        torch.cuda.synchronize()
        outs.append({f: getattr(out, f).cpu().numpy() for f in FIELDS})
        if recomputed is not None:
            path = eng.stats()["ppr8_r1_long_rows"]
            assert (path >= 0) == (recomputed and not store), (store, path)
    eng.set_flags(OPT_STORE_R1, False)
    return outs


def _assert_same(got, want, what):
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f)


def _engine(kg, pass_bits, fact_bits, b, k, **kw):
    from hipporag_amd.engine import HippoRAGEngine
    return HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                          max_batch=b, max_topk=k, **kw)


def _queries(pass_bits, fact_bits, b, device, eng):
    import torch
    qf = _bf16(synth.make_queries_np(fact_bits, b, seed=3)[0], device)
    qp = _bf16(synth.make_queries_np(pass_bits, b, seed=4)[0], device)
    idx, sc = eng.score_facts(qf, k=5)
    cnt = torch.full((b,), 5, dtype=torch.int32, device=device)
    return qp, idx, sc, cnt


@pytest.mark.parametrize("b", [65, 128, 200, 256, 384])
def test_recomputed_first_residual_is_bit_identical_over_batch_shapes(gpu_device, b):
    """65 / 128: one slab (the one-slab kernel); 200 / 256: one slab pair, the second slab partly filled at 200;
    384: a pair and an odd last slab."""
    kg, pass_bits, fact_bits, _ = make_case(12000, 120000, 64, seed=900 + b)
    with _engine(kg, pass_bits, fact_bits, b, 100) as eng:
        qp, idx, sc, cnt = _queries(pass_bits, fact_bits, b, gpu_device, eng)
        new, old = _both(eng, qp, idx, sc, cnt, ppr_iters=20, k=100)
        assert eng.timings()["slab_width"] == 128
        assert int(new["iters_used"].max()) == 20 and not np.any(new["flags"] & 8)
        _assert_same(new, old, b)


@pytest.mark.parametrize("b", [130, 384])
def test_long_rows_keep_the_stored_first_residual(gpu_device, b):
    """A power-law graph at sell_seg_len = 64: the hubs are cut into segments, their rows are finished by the
    last-arriving wavefront and keep the stored R_1 next to the recomputed one of every other row."""
    kg, pass_bits, fact_bits, _ = make_case(16000, 160000, 64, seed=41, power_law=True)
    assert int(np.diff(kg.csr.row_ptr).max()) > 4 * 64          # there are long rows
    with _engine(kg, pass_bits, fact_bits, b, 100, sell_seg_len=64) as eng:
        qp, idx, sc, cnt = _queries(pass_bits, fact_bits, b, gpu_device, eng)
        new, old = _both(eng, qp, idx, sc, cnt, ppr_iters=20, k=100)
        assert eng.timings()["slab_width"] == 128
        eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=100)
        assert eng.stats()["ppr8_r1_long_rows"] > 0             # the engine's matrix has long rows, and they kept R_1
        _assert_same(new, old, b)


def test_filtered_seeds_and_zero_passage_weight(gpu_device):
    """Queries whose facts were all filtered out (DPR ranking, no teleport mass from seeds), queries with a single seed,
    and a batch with passage_node_weight = 0 (c_0 lives on the seed rows alone)."""
    import torch
    b = 200
    kg, pass_bits, fact_bits, _ = make_case(9000, 90000, 64, seed=515)
    with _engine(kg, pass_bits, fact_bits, b, 60) as eng:
        qp, idx, sc, cnt = _queries(pass_bits, fact_bits, b, gpu_device, eng)
        keep = np.full(b, 5, dtype=np.int32)
        keep[[0, 7, 127, 128, 199]] = 0
        keep[[1, 129]] = 1
        cnt = torch.from_numpy(keep).to(gpu_device)
        new, old = _both(eng, qp, idx, sc, cnt, ppr_iters=20, k=60)
        assert np.all((new["flags"][[0, 7, 127, 128, 199]] & 1) == 1) and not (new["flags"][2] & 1)
        _assert_same(new, old, "filtered seeds")
        new, old = _both(eng, qp, idx, sc, cnt, ppr_iters=20, k=60, passage_node_weight=0.0)
        _assert_same(new, old, "zero passage weight")


def test_accelerated_and_tolerance_plans(gpu_device):
    """HRAG_OPT_ACCEL with and without a tolerance (measured stage scales: 1 / cs_0 comes from the device table), and a
    tolerance on the plain plan that is low enough for extension stages to run."""
    b = 130
    kg, pass_bits, fact_bits, _ = make_case(12000, 120000, 128, seed=611)
    with _engine(kg, pass_bits, fact_bits, b, 100) as eng:
        qp, idx, sc, cnt = _queries(pass_bits, fact_bits, b, gpu_device, eng)
        new, old = _both(eng, qp, idx, sc, cnt, ppr_iters=20, k=100, ppr_tol=1e-7, ppr_max_iters=29)
        assert int(new["iters_used"].max()) > 20                 # at least one extension stage ran
        _assert_same(new, old, "tolerance")
        eng.set_flags(OPT_ACCEL, True)
        try:
            # fixed count: 1, 3, 3, ... -- the 3-sweep stage 2 needs all three buffers, R_1 stays stored
            new, old = _both(eng, qp, idx, sc, cnt, ppr_iters=20, k=100, recomputed=False)
            _assert_same(new, old, "accel")
            new, old = _both(eng, qp, idx, sc, cnt, ppr_iters=20, k=100, ppr_tol=1.5e-6, ppr_max_iters=30)
            _assert_same(new, old, "accel + tolerance")
        finally:
            eng.set_flags(OPT_ACCEL, False)


@pytest.mark.parametrize("iters", [1, 2, 3, 20])
def test_sweep_counts(gpu_device, iters):
    """1, 2, 3 sweeps never reach the staged e4m3 state (it serves 16 .. 30): the flag must not matter there either."""
    b = 130
    kg, pass_bits, fact_bits, _ = make_case(6000, 60000, 64, seed=4343)
    with _engine(kg, pass_bits, fact_bits, b, 50) as eng:
        qp, idx, sc, cnt = _queries(pass_bits, fact_bits, b, gpu_device, eng)
        new, old = _both(eng, qp, idx, sc, cnt, ppr_iters=iters, k=50, recomputed=True if iters == 20 else None)
        _assert_same(new, old, iters)


def test_eight_shards_against_the_single_engine(gpu_device):
    """The row shards share the plan (their replicated c_0 survives the exchanges: buffer 0 is exchanged once before the
    first sweep and not written before stage 3): the 8-shard emulated run equals the single engine with R_1 recomputed
    and with R_1 stored."""
    import torch
    from hipporag_amd import dist as hd
    from hipporag_amd.engine import HippoRAGEngine
    world, b, groups = 8, 130, 2
    kg, pass_bits, fact_bits, _ = make_case(12000, 120000, 128, seed=508)
    sidx = hd.shard_index(kg.csr, kg.passage_vertex, world, kg.subj_vertex, kg.obj_vertex, kg.num_chunks)
    qf = _bf16(synth.make_queries_np(fact_bits, b, seed=3)[0], gpu_device)
    qp = _bf16(synth.make_queries_np(pass_bits, b, seed=4)[0], gpu_device)
    kw = dict(link_top_k=5, damping=0.5, passage_node_weight=0.05, ppr_iters=20, k=100)
    got = hd.run_local_shards(world, sidx, pass_bits, fact_bits, qf, qp, kw, groups, gpu_device, 100)
    with HippoRAGEngine(sidx.csr, sidx.passage_vertex, pass_bits, fact_bits, sidx.subj_vertex, sidx.obj_vertex,
                        sidx.num_chunks, max_batch=b, max_topk=100) as eng:
        idx, sc = eng.score_facts(qf, k=5)
        cnt = torch.full((b,), 5, dtype=torch.int32, device=gpu_device)
        new, old = _both(eng, qp, idx, sc, cnt, **kw)
    _assert_same(new, old, "single engine")
    for name, one in (("recomputed", new), ("stored", old)):
        assert np.array_equal(got[2], one["doc_idx"]), name
        assert np.array_equal(got[3], one["doc_score"]), name
        assert np.array_equal(got[4], one["flags"]), name


def test_two_shards_with_nan_and_poisoned_inputs(gpu_device):
    """Row shards at world 2 (shared state buffers, dist.LocalComm) on an index with NaN fact and passage rows, with
    negative, zero and NaN kept scores: bit-identical to the single engine with R_1 recomputed and stored.  The poisoned
    scores are fixed once, under a lock, before any shard uses them: both shard threads call the filter."""
    import threading
    import torch
    from hipporag_amd import dist as hd
    from hipporag_amd.engine import HippoRAGEngine
    world, b, k = 2, 70, 50
    kg, pass_bits, fact_bits, _ = make_case(3000, 30000, 64, seed=811)
    fact_bits, pass_bits = fact_bits.copy(), pass_bits.copy()
    fact_bits[[11, kg.n_facts // 3], 0] = np.array([0x7FC0, 0xFFC0], np.uint16)
    pass_bits[[5, kg.n_passages - 2], 2] = np.uint16(0x7FC0)
    sidx = hd.shard_index(kg.csr, kg.passage_vertex, world, kg.subj_vertex, kg.obj_vertex, kg.num_chunks)
    qf = _bf16(synth.make_queries_np(fact_bits, b, seed=21)[0], gpu_device)
    qp = _bf16(synth.make_queries_np(pass_bits, b, seed=22)[0], gpu_device)
    kw = dict(link_top_k=5, damping=0.5, passage_node_weight=0.05, ppr_iters=20, k=k)
    lock, poison = threading.Lock(), {}

    def poisoned(sc):
        with lock:
            if "sc" not in poison:
                s = sc.cpu().numpy().copy()
                rng = np.random.default_rng(77)
                for q in range(b):
                    s[q, rng.integers(2, 5)] = [-0.3, 0.0, -0.0][q % 3]
                    if q % 4 == 0:
                        s[q, 4] = np.nan
                    if q % 5 == 1:
                        s[q, 3] = -1.0
                poison["sc"] = s
        return torch.from_numpy(poison["sc"]).to(sc.device)

    def filt(idx, sc):
        return idx, poisoned(sc), torch.full((b,), 5, dtype=torch.int32, device=sc.device)

    got = hd.run_local_shards(world, sidx, pass_bits, fact_bits, qf, qp, kw, 0, gpu_device, k, filt)
    with HippoRAGEngine(sidx.csr, sidx.passage_vertex, pass_bits, fact_bits, sidx.subj_vertex, sidx.obj_vertex,
                        sidx.num_chunks, max_batch=b, max_topk=k) as eng:
        idx, sc = eng.score_facts(qf, k=5)
        cnt = torch.full((b,), 5, dtype=torch.int32, device=gpu_device)
        new, old = _both(eng, qp, idx, poisoned(sc), cnt, **kw)
    _assert_same(new, old, "single engine")
    assert np.isfinite(got[3]).all()
    for name, one in (("recomputed", new), ("stored", old)):
        assert np.array_equal(got[2], one["doc_idx"]), name
        assert np.array_equal(got[3], one["doc_score"]), name
        assert np.array_equal(got[4], one["flags"]), name
