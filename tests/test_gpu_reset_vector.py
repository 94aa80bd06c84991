"""The reset vector ("personalization") that phase B hands to the PPR solve, held to its numpy restatement on every
state path (include/hrag.h, hrag_stage_seeds / the passage prior):
  a. hrag_stage_seeds against tests/helpers.py seeds_np bit for bit, on poisoned output buffers, at the extremes of
     the seed rule (repeats, ties, absent / out-of-range ids, NaN / inf / subnormal / signed-zero scores, odd batches);
  b. the prior of hrag_stage_teleport against prior_np bit for bit, and on every state path the identity
     "NaN at passages P == the row's minimum at P" (both give P a prior of exactly 0) bit for bit;
  c. end to end with NaN fact rows, NaN / negative / zero kept scores and NaN / +-inf passage scores: finite, within
     the 1e-5 bar of the oracle on the restated, sanitised reset vector, reproducible over stale seed buffers, and the
     row shards and the hybrid mode bit-identical to the single engine."""

import numpy as np
import pytest

import oracle
from hipporag_amd import synth
from tests.helpers import expected_topk, make_case, prior_np, seeds_np, tie_aware_equal

pytestmark = pytest.mark.gpu

K = 50
KW = dict(link_top_k=5, damping=0.5, passage_node_weight=0.05, ppr_iters=20, k=K)
SENTINEL = 0x5EED


def _bf16(bits, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(device).view(torch.bfloat16)


def _t(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


@pytest.fixture(scope="module")
def case():
    kg, pass_bits, fact_bits, index = make_case(3000, 30000, 64, seed=811)
    return dict(kg=kg, pass_bits=pass_bits, fact_bits=fact_bits, index=index)


# ----------------------------------------------------------------------------- a. hrag_stage_seeds
SCORE_PALETTE = np.array([0.0, -0.0, 1e-40, -1e-40, 0.5, 0.5, 0.25, -0.75, 3.0, np.inf, -np.inf, np.nan, np.nan,
                          0.1, 1.0], np.float32)


def _fact_table(rng, n_facts, v):
    """subject / object ids with -1 and ids >= V (out of range: skipped), facts 0-3 on vertex 5 on both sides, facts
    4-7 with subject == object, num_chunks 0 / small / huge"""
    subj = rng.integers(-1, v + 4, n_facts).astype(np.int32)
    obj = rng.integers(-1, v + 4, n_facts).astype(np.int32)
    subj[:4] = obj[:4] = 5
    obj[4:8] = subj[4:8]
    nch = rng.integers(0, 4, v).astype(np.int32)
    nch[rng.integers(0, v, 8)] = 1 << 30
    nch[5] = 3
    return subj, obj, nch


def _seed_batch(rng, b, kf, n_facts, link_top_k):
    kept_idx = rng.integers(0, n_facts, (b, kf)).astype(np.int32)
    odd = rng.random((b, kf))
    kept_idx[odd < 0.08] = -1
    kept_idx[(odd >= 0.08) & (odd < 0.12)] = n_facts + 7                 # out-of-range fact ids
    sc = rng.random((b, kf)).astype(np.float32)
    pick = rng.random((b, kf)) < 0.35
    sc[pick] = SCORE_PALETTE[rng.integers(0, SCORE_PALETTE.size, int(pick.sum()))]
    sc[rng.random((b, kf)) < 0.15] = np.float32(0.5)                       # exact ties between different facts
    cnt = rng.integers(0, kf + 1, b).astype(np.int32)
    special = rng.random(b)
    cnt[special < 0.05] = -3
    cnt[(special >= 0.05) & (special < 0.1)] = kf + 4
    if b >= 3:                                                             # one vertex in every entry, several NaNs
        kept_idx[0, :] = rng.integers(0, 4, kf)
        cnt[0] = kf
        kept_idx[1, :] = np.arange(kf) + 8
        sc[1, ::2] = np.nan
        cnt[1] = kf
        cnt[2] = 0
    return kept_idx, sc, cnt


def _stage_seeds(stages, kept_idx, sc, cnt, link_top_k, out, device):
    import torch
    stages.seeds(_t(kept_idx, device), _t(sc, device), _t(cnt, device), link_top_k, out=out)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _check_seeds(got, want, flags_before, msg):
    vtx, w, cnt, flags = got
    w_vtx, w_w, w_cnt, w_flags, _ = want
    np.testing.assert_array_equal(cnt, w_cnt, err_msg=f"seed_cnt {msg}")
    np.testing.assert_array_equal(flags & 5, w_flags, err_msg=f"flags {msg}")
    np.testing.assert_array_equal(flags & ~5, flags_before & ~5, err_msg=f"other flag bits {msg}")
    slot = np.arange(32)[None, :] < w_cnt[:, None]
    np.testing.assert_array_equal(np.where(slot, vtx, -1), np.where(slot, w_vtx, -1), err_msg=f"seed_vtx {msg}")
    np.testing.assert_array_equal(np.where(slot, w.view(np.int32), 0), np.where(slot, w_w.view(np.int32), 0),
                                  err_msg=f"seed_w bits {msg}")


@pytest.mark.parametrize("kf", [1, 5, 16])
def test_stage_seeds_matches_numpy_bit_for_bit(gpu_device, case, kf):
    """Every slot below seed_cnt equals seeds_np: buffers poisoned before the call (a sentinel vertex, NaN weights,
    random flag bits), then the same buffers overwritten by a second batch -- an unwritten slot shows either way."""
    import torch
    from hipporag_amd.engine import EngineStages, HippoRAGEngine
    kg = case["kg"]
    v = kg.num_vertices
    rng = np.random.default_rng(kf)
    n_facts = kg.n_facts
    subj, obj, nch = _fact_table(rng, n_facts, v)
    with HippoRAGEngine(kg.csr, kg.passage_vertex, case["pass_bits"], case["fact_bits"], subj, obj, nch,
                        max_batch=8, max_topk=8) as eng:
        st = EngineStages(eng)
        for b in (1, 2, 3, 63, 64, 65, 1025):
            for link_top_k in sorted({0, 1, 3, kf, 2 * kf + 1, 32}):
                out = (torch.full((b, 32), SENTINEL, dtype=torch.int32, device=gpu_device),
                       torch.full((b, 32), float("nan"), dtype=torch.float32, device=gpu_device),
                       torch.full((b,), -7, dtype=torch.int32, device=gpu_device),
                       _t(rng.integers(0, 1 << 12, b).astype(np.int32), gpu_device))
                for rep in range(2):        # rep 1: over the seeds rep 0 left in the same buffers
                    kept_idx, sc, cnt = _seed_batch(rng, b, kf, n_facts, link_top_k)
                    flags_before = out[3].cpu().numpy()
                    got = _stage_seeds(st, kept_idx, sc, cnt, link_top_k, out, gpu_device)
                    want = seeds_np(kept_idx, sc, cnt, link_top_k, subj, obj, nch)
                    _check_seeds(got, want, flags_before, f"b={b} kf={kf} link_top_k={link_top_k} rep={rep}")
                    assert not np.signbit(got[1][np.arange(32)[None, :] < got[2][:, None]]).any()


# ----------------------------------------------------------------------------- b. the passage prior
def _score_rows(rng, b, n):
    s = rng.standard_normal((b, n)).astype(np.float32)
    s[0] = 1.0                                                            # range 0: a prior of 1 * weight everywhere
    if b > 4:
        s[1, rng.integers(0, n, 5)] = np.nan
        s[2, rng.integers(0, n, 3)] = np.inf
        s[3, rng.integers(0, n, 3)] = -np.inf
        s[4] = np.nan                                                     # no number at all
        s[5, :3] = [np.nan, np.inf, -np.inf]
    return s


@pytest.mark.parametrize("slab_width,pad", [(16, 5), (32, 0), (64, 3)])
def test_stage_teleport_prior_matches_numpy_bit_for_bit(gpu_device, case, slab_width, pad):
    """hrag_row_minmax + hrag_stage_teleport == prior_np in every column of every (partial) slab, DPR-flagged rows 0,
    the columns past the batch 0; scores with ld > n."""
    import torch
    from hipporag_amd.engine import EngineStages, HippoRAGEngine
    kg = case["kg"]
    n = kg.n_passages
    b = 70
    rng = np.random.default_rng(slab_width)
    with HippoRAGEngine(kg.csr, kg.passage_vertex, case["pass_bits"], case["fact_bits"], kg.subj_vertex,
                        kg.obj_vertex, kg.num_chunks, max_batch=b, max_topk=8, slab_width=slab_width) as eng:
        st = EngineStages(eng)
        s = _score_rows(rng, b, n)
        full = np.full((b, n + pad), np.nan, np.float32)
        full[:, :n] = s
        flags = np.zeros(b, np.int32)
        flags[rng.integers(0, b, 6)] |= 1
        flags[9] |= 4                                                     # only bit 0 zeroes a row
        scores_t = _t(full, gpu_device)
        mn, mx = st.row_minmax(scores_t[:, :n].contiguous())
        tele = st.teleport(scores_t, mn, mx, 0.05, _t(flags, gpu_device))
        torch.cuda.synchronize()
        bc, ns = eng.layout(b)
        assert bc == slab_width and ns * bc > b
        _, _, _, w_mn, w_mx = expected_topk(s, 1)
        np.testing.assert_array_equal(mn.cpu().numpy(), w_mn)
        np.testing.assert_array_equal(mx.cpu().numpy(), w_mx)
        want = prior_np(s, 0.05, w_mn, w_mx)
        want[(flags & 1) == 1] = 0
        got = tele.cpu().numpy().transpose(0, 2, 1).reshape(ns * bc, n)
        np.testing.assert_array_equal(got[:b].view(np.int32), want.view(np.int32))
        assert np.all(got[b:] == 0)
        assert np.all(want[4] == 0) and np.all(want[0][(flags[0] & 1) == 0] == np.float32(0.05))


def _kept_from_phase_a(eng, qf_bits, device, b):
    import torch
    idx, sc = eng.score_facts(_bf16(qf_bits[:b], device), k=5)
    return idx, sc, torch.full((b,), 5, dtype=torch.int32, device=device)


def _with_nan_and_min(rng, s, allowed=None):
    """(raw with NaN at some passages P of every row, raw' = the same with the row minimum over its numbers at P --
    over the allowed passages in the "seeds" scope)"""
    raw = s.copy()
    b, n = raw.shape
    raw2 = raw.copy()
    for q in range(b):
        p = rng.choice(n, size=int(rng.integers(1, 6)), replace=False)
        keep = np.ones(n, bool) if allowed is None else allowed[q].copy()
        keep[p] = False
        if not keep.any():
            continue
        raw[q, p] = np.nan
        raw2[q, p] = raw[q, keep].min()
    return raw, raw2


def _same(a, b, msg):
    for x, y, what in zip(a, b, ("doc_idx", "doc_score", "flags")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what} {msg}")


@pytest.mark.parametrize("path,b", [("sv", 1), ("sv", 2), ("sv", 5), ("sv", 8), ("f16", 40), ("f8", 130),
                                    ("f8-accel", 130), ("pair", 300), ("f32", 40), ("f8-seeds-scope", 130)])
def test_nan_passage_score_equals_the_row_minimum_on_every_state_path(gpu_device, case, path, b):
    """retrieve_scored(raw with NaN at P) == retrieve_scored(raw' with the row minimum at P), bit for bit: the same
    min / max, a prior of exactly 0 on P on both sides -- and so the same fp16 / fp8 scales and masses."""
    import torch
    from hipporag_amd._lib import OPT_ACCEL, OPT_F32_STATE
    from hipporag_amd.engine import HippoRAGEngine
    kg = case["kg"]
    n = kg.n_passages
    rng = np.random.default_rng(b + len(path))
    flags = OPT_F32_STATE if path == "f32" else 0
    qf_bits, _ = synth.make_queries_np(case["fact_bits"], b, seed=b)
    qp_bits, _ = synth.make_queries_np(case["pass_bits"], b, seed=b + 1)
    with HippoRAGEngine(kg.csr, kg.passage_vertex, case["pass_bits"], case["fact_bits"], kg.subj_vertex,
                        kg.obj_vertex, kg.num_chunks, max_batch=max(b, 8), max_topk=K, flags=flags) as eng:
        if path == "f8-accel":
            eng.set_flags(OPT_ACCEL, True)
        idx, sc, cnt = _kept_from_phase_a(eng, qf_bits, gpu_device, b)
        s = eng.sim_scores("passages", _bf16(qp_bits, gpu_device)).cpu().numpy()
        kw = dict(KW)
        allowed = None
        if path == "f8-seeds-scope":
            allowed = rng.random((b, n)) < 0.6
            kw.update(doc_filter=_t(allowed, gpu_device), filter_scope="seeds")
        raw, raw2 = _with_nan_and_min(rng, s, allowed)
        outs = []
        for r in (raw, raw2):
            o = eng.retrieve_scored(_t(r, gpu_device), idx, sc, cnt, **kw)
            torch.cuda.synchronize()
            outs.append((o.doc_idx.cpu().numpy(), o.doc_score.cpu().numpy(), o.flags.cpu().numpy()))
        width = eng.timings()["slab_width"]
    _same(outs[0], outs[1], f"{path} b={b} slab width {width}")
    assert np.isfinite(outs[0][1]).all() and np.all(outs[0][2] & ~4 == 0), np.unique(outs[0][2])


@pytest.mark.parametrize("b", [2, 40, 130])
def test_nan_passage_rows_through_retrieve_equal_the_row_minimum(gpu_device, case, b):
    """retrieve(q_pass) on an index whose passage embeddings hold NaN rows (bf16 NaNs of both signs) ==
    retrieve_scored(the same scores with the row minimum at those passages), bit for bit."""
    import torch
    from hipporag_amd.engine import HippoRAGEngine
    kg = case["kg"]
    pass_bits = case["pass_bits"].copy()
    nan_rows = np.array([3, kg.n_passages // 2, kg.n_passages - 1])
    pass_bits[nan_rows, 1] = np.array([0x7FC0, 0xFFC1, 0x7F81], np.uint16)
    qf_bits, _ = synth.make_queries_np(case["fact_bits"], b, seed=b + 5)
    qp_bits, _ = synth.make_queries_np(case["pass_bits"], b, seed=b + 6)
    with HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, case["fact_bits"], kg.subj_vertex, kg.obj_vertex,
                        kg.num_chunks, max_batch=max(b, 8), max_topk=K) as eng:
        idx, sc, cnt = _kept_from_phase_a(eng, qf_bits, gpu_device, b)
        qp = _bf16(qp_bits, gpu_device)
        s = eng.sim_scores("passages", qp).cpu().numpy()
        assert np.isnan(s[:, nan_rows]).all() and not np.isnan(np.delete(s, nan_rows, axis=1)).any()
        s2 = s.copy()
        s2[:, nan_rows] = np.nanmin(s, axis=1)[:, None]
        a = eng.retrieve(qp, idx, sc, cnt, **KW)
        bb = eng.retrieve_scored(_t(s2, gpu_device), idx, sc, cnt, **KW)
        torch.cuda.synchronize()
        outs = [(o.doc_idx.cpu().numpy(), o.doc_score.cpu().numpy(), o.flags.cpu().numpy()) for o in (a, bb)]
    _same(outs[0], outs[1], f"b={b}")
    assert np.isfinite(outs[0][1]).all()


# ----------------------------------------------------------------------------- c. end to end
def _nan_index(case):
    """the case with NaN fact rows (phase A ranks them first in every query, NaN score) and NaN passage rows"""
    fact_bits, pass_bits = case["fact_bits"].copy(), case["pass_bits"].copy()
    nan_facts = np.array([11, case["kg"].n_facts // 3])
    fact_bits[nan_facts, 0] = np.array([0x7FC0, 0xFFC0], np.uint16)
    nan_pass = np.array([5, case["kg"].n_passages - 2])
    pass_bits[nan_pass, 2] = np.uint16(0x7FC0)
    return fact_bits, pass_bits, nan_facts, nan_pass


def _poison_kept(rng, sc):
    """negative and zero scores next to the phase-A NaNs; every query keeps at least one positive score"""
    sc = sc.copy()
    b = sc.shape[0]
    for q in range(b):
        r = rng.integers(2, 5)
        sc[q, r] = [-0.3, 0.0, -0.0][q % 3]
        if q % 4 == 0:
            sc[q, 4] = np.nan
        if q % 5 == 1:
            sc[q, 3] = -1.0
    return sc


def _reset_np(kg, kept_idx, kept_sc, cnt, s, weight=0.05):
    vtx, w, n, flags, _ = seeds_np(kept_idx, kept_sc, cnt, 5, kg.subj_vertex, kg.obj_vertex, kg.num_chunks)
    prior = prior_np(s, weight)
    resets = []
    for q in range(kept_idx.shape[0]):
        r = np.zeros(kg.num_vertices)
        r[kg.passage_vertex] = prior[q]
        np.add.at(r, vtx[q, :n[q]], w[q, :n[q]].astype(np.float64))
        resets.append(r)
    return resets, flags


@pytest.mark.parametrize("path,b", [("sv", 3), ("f16", 40), ("f8", 130), ("f8-accel", 130), ("pair", 300),
                                    ("f32", 40)])
def test_nan_inputs_end_to_end_against_the_oracle(gpu_device, case, path, b):
    import torch
    from hipporag_amd._lib import OPT_ACCEL, OPT_F32_STATE
    from hipporag_amd.engine import HippoRAGEngine
    kg, index = case["kg"], case["index"]
    fact_bits, pass_bits, nan_facts, nan_pass = _nan_index(case)
    rng = np.random.default_rng(3 * b + len(path))
    qf_bits, _ = synth.make_queries_np(case["fact_bits"], b, seed=b + 11)
    qp_bits, _ = synth.make_queries_np(case["pass_bits"], b, seed=b + 12)
    with HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex,
                        kg.num_chunks, max_batch=max(b, 8), max_topk=K,
                        flags=OPT_F32_STATE if path == "f32" else 0) as eng:
        if path == "f8-accel":
            eng.set_flags(OPT_ACCEL, True)
        idx, sc, cnt = _kept_from_phase_a(eng, qf_bits, gpu_device, b)
        idx_h, sc_h = idx.cpu().numpy(), sc.cpu().numpy()
        assert np.isin(idx_h[:, :2], nan_facts).all() and np.isnan(sc_h[:, :2]).all()   # the NaN facts come first
        sc_h = _poison_kept(rng, sc_h)
        s = eng.sim_scores("passages", _bf16(qp_bits, gpu_device)).cpu().numpy()
        s[1 % b, rng.integers(0, kg.n_passages, 3)] = np.inf                 # +-inf: the whole prior is 0
        if b > 2:
            s[2, rng.integers(0, kg.n_passages, 2)] = -np.inf
        s_t, sc_t = _t(s, gpu_device), _t(sc_h, gpu_device)
        first = eng.retrieve_scored(s_t, idx, sc_t, cnt, **KW)
        torch.cuda.synchronize()
        first = (first.doc_idx.cpu().numpy(), first.doc_score.cpu().numpy(), first.flags.cpu().numpy())
        # another call leaves other seeds (more of them, other counts) in the engine's buffers, then the same again
        other_sc = rng.random(sc_h.shape).astype(np.float32)
        eng.retrieve_scored(s_t, idx, _t(other_sc, gpu_device), cnt, link_top_k=10, ppr_iters=20, k=K)
        again = eng.retrieve_scored(s_t, idx, sc_t, cnt, **KW)
        torch.cuda.synchronize()
        again = (again.doc_idx.cpu().numpy(), again.doc_score.cpu().numpy(), again.flags.cpu().numpy())
    _same(first, again, f"{path} b={b}: the same call over stale seed buffers")
    got_idx, got_sc, flags = first
    assert np.isfinite(got_sc).all(), path
    resets, w_flags = _reset_np(kg, idx_h, sc_h, cnt.cpu().numpy(), s)
    np.testing.assert_array_equal(flags, w_flags, err_msg=path)
    pv = kg.passage_vertex
    for q in sorted(set(range(0, b, max(1, b // 8))) | {0, 1, min(2, b - 1), b - 1}):
        want_ids, want_sc, x = oracle.run_ppr(index, resets[q])
        assert tie_aware_equal(got_idx[q], want_ids[:K], want_sc[:K], rel_gap=2e-5), (path, q)
        want = x[pv][got_idx[q]]
        rel = float((np.abs(got_sc[q] - want) / want).max())
        assert rel < 1e-5, (path, q, rel)


def test_nan_inputs_on_row_shards_and_the_hybrid_mode_are_bit_identical_to_the_single_engine(gpu_device, case):
    """Row shards (world 2, dist.LocalComm) with NaN / negative / zero kept scores on an index with NaN fact and
    passage rows, and the hybrid mode on the same index: bit-identical to the single engine."""
    import torch
    from hipporag_amd import dist as hd
    from hipporag_amd.engine import HippoRAGEngine
    kg = case["kg"]
    fact_bits, pass_bits, _, _ = _nan_index(case)
    world, b = 2, 70
    rng = np.random.default_rng(77)
    sidx = hd.shard_index(kg.csr, kg.passage_vertex, world, kg.subj_vertex, kg.obj_vertex, kg.num_chunks)
    qf_bits, _ = synth.make_queries_np(case["fact_bits"], b, seed=21)
    qp_bits, _ = synth.make_queries_np(case["pass_bits"], b, seed=22)
    qf_t, qp_t = _bf16(qf_bits, gpu_device), _bf16(qp_bits, gpu_device)
    poison = {}

    def filter_fn(idx, sc):
        if "sc" not in poison:
            poison["sc"] = _poison_kept(rng, sc.cpu().numpy())
        return idx, _t(poison["sc"], sc.device), torch.full((b,), 5, dtype=torch.int32, device=sc.device)

    got = hd.run_local_shards(world, sidx, pass_bits, fact_bits, qf_t, qp_t, KW, 0, gpu_device, K, filter_fn)
    with HippoRAGEngine(sidx.csr, sidx.passage_vertex, pass_bits, fact_bits, sidx.subj_vertex, sidx.obj_vertex,
                        sidx.num_chunks, max_batch=b, max_topk=K) as eng:
        idx, sc, cnt = _kept_from_phase_a(eng, qf_bits, gpu_device, b)
        one = eng.retrieve(qp_t, idx, _t(poison["sc"], gpu_device), cnt, **KW)
        torch.cuda.synchronize()
        one = tuple(t.cpu().numpy() for t in (idx, one.doc_idx, one.doc_score, one.flags))
    np.testing.assert_array_equal(got[0], one[0])
    _same(got[2:], one[1:], "row shards")
    assert np.isfinite(got[3]).all()
    # the hybrid mode: phase A's own NaN candidates, NaN passage rows
    arrays = dict(csr=kg.csr, passage_vertex=kg.passage_vertex, subj_vertex=kg.subj_vertex, obj_vertex=kg.obj_vertex,
                  num_chunks=kg.num_chunks)
    f_idx, f_sc, d_idx, d_sc, flags = hd.run_local_hybrid(world, arrays, sidx, pass_bits, fact_bits, qf_t, qp_t, KW,
                                                          gpu_device, K)
    bn = b // world
    with HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex,
                        kg.num_chunks, max_batch=b, max_topk=K) as eng:
        idx, sc, cnt = _kept_from_phase_a(eng, qf_bits, gpu_device, b)
        np.testing.assert_array_equal(f_idx, idx.cpu().numpy())
        for r in range(world):
            sl = slice(r * bn, (r + 1) * bn)
            o = eng.retrieve(qp_t[sl], idx[sl], sc[sl], cnt[sl], **KW)
            torch.cuda.synchronize()
            _same((d_idx[sl], d_sc[sl], flags[sl]), (o.doc_idx.cpu().numpy(), o.doc_score.cpu().numpy(),
                                                     o.flags.cpu().numpy()), f"hybrid rank {r}")
    assert np.isfinite(d_sc).all()
