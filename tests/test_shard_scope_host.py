"""CPU tests of the doc filter's "seeds" scope on the row-sharded orchestration (hipporag_amd/dist.py ShardedRetriever with
the scoped shard steps of include/hrag.h: hrag_shard_score_facts_scoped, hrag_shard_passage_scores_scoped,
hrag_shard_mask_prior), over dist.LocalComm (4 shards in one process) and gloo (world 2).

The shard compute is the numpy stand-in of tests/test_shard_orchestration.py, extended with the scoped steps.  Under test
is what dist.py adds for the scope -- the allowed min / max all-reduced, the owned rows rewritten with them, the min / max
of the rewritten rows all-reduced again, the scoped candidates merged -- against a numpy restatement of the scope on the
whole index (retriever.masked_minmax_rows, the fact rule "a fact is allowed when one of its sources is", the oracle PPR)."""

import os
import threading

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import oracle
from hipporag_amd import dist as hd
from hipporag_amd import synth
from hipporag_amd.graph import bf16_bits_to_float
from hipporag_amd.retriever import masked_minmax_rows
from tests.helpers import make_case
from tests.test_shard_orchestration import FakeShardStages, _free_port

K = 40
ITERS = 20


def fact_mask_np(allowed, row_ptr, pos):
    """bool [R, F]: fact f is allowed in row r when one of its source passages is."""
    allowed = np.atleast_2d(allowed)
    out = np.zeros((allowed.shape[0], len(row_ptr) - 1), bool)
    for f in range(len(row_ptr) - 1):
        src = pos[row_ptr[f]:row_ptr[f + 1]]
        if len(src):
            out[:, f] = allowed[:, src].any(axis=1)
    return out


def _minmax_allowed(s, a):
    mn = np.where(a.any(1), np.where(a, s, np.inf).min(1), np.inf).astype(np.float32)
    mx = np.where(a.any(1), np.where(a, s, -np.inf).max(1), -np.inf).astype(np.float32)
    return torch.from_numpy(mn), torch.from_numpy(mx)


def _masked_topk(s, a, k, idx_offset):
    """oracle.topk_desc among the allowed entries of every row: -1 / 0 beyond them."""
    b = s.shape[0]
    idx = np.full((b, k), -1, np.int32)
    val = np.zeros((b, k), np.float32)
    for r in range(b):
        cand = np.flatnonzero(a[r])
        if not len(cand):
            continue
        o = cand[oracle.topk_desc(s[r][cand], k)]
        idx[r, :len(o)] = o + idx_offset
        val[r, :len(o)] = s[r][o]
    return torch.from_numpy(idx), torch.from_numpy(val)


class ScopedFakeShardStages(FakeShardStages):
    """The stand-in with the scoped shard steps: the fact -> source table is the GLOBAL one (global fact order and
    passage positions); the shard reads the rows of its own facts, the doc filter is the global one."""

    has_fact_sources = True

    def __init__(self, sidx, index, rank, fact_sources):
        super().__init__(sidx, index, rank)
        self.row_ptr, self.pos = fact_sources

    def _allowed(self, scope_filter, b):
        a = np.asarray(scope_filter.cpu().numpy(), bool)
        return np.broadcast_to(np.atleast_2d(a), (b, a.shape[-1]))

    def shard_score_facts(self, q, k, scope_filter=None):
        if scope_filter is None:
            return super().shard_score_facts(q, k)
        s = (q.double().numpy() @ self.fe.T).astype(np.float32)
        allowed = self._allowed(scope_filter, s.shape[0])
        fm = fact_mask_np(allowed, self.row_ptr, self.pos)[:, self.f_lo:self.f_hi]
        idx, val = _masked_topk(s, fm, k, self.f_lo)
        return (idx, val) + _minmax_allowed(s, fm)

    def shard_passage_scores(self, q, scope_filter=None):
        mn, mx = super().shard_passage_scores(q)
        if scope_filter is None:
            return mn, mx
        self.own_allowed = self._allowed(scope_filter, self.s_local.shape[0])[:, self.p_lo:self.p_hi]
        return _minmax_allowed(self.s_local, self.own_allowed)

    def shard_mask_prior(self, mn, mx, scope_filter):
        a = self._allowed(scope_filter, self.s_local.shape[0])[:, self.p_lo:self.p_hi]
        lo, hi = mn.numpy()[:, None], mx.numpy()[:, None]
        rng = (hi - lo).astype(np.float32)
        with np.errstate(invalid="ignore", divide="ignore"):
            norm = np.where(rng == 0, np.float32(1), (self.s_local - lo) / rng).astype(np.float32)
        self.s_local = np.where(a, norm, np.float32(0)).astype(np.float32)
        if self.s_local.shape[1] == 0:
            b = self.s_local.shape[0]
            return torch.full((b,), np.inf), torch.full((b,), -np.inf)
        return torch.from_numpy(self.s_local.min(1)), torch.from_numpy(self.s_local.max(1))

    def shard_finish(self, mn, mx, flags, k, doc_filter=None):
        b = self.b
        doc = np.zeros((b, self.p_hi - self.p_lo), np.float32)
        fl = flags.numpy()
        for q in range(b):
            if fl[q] & 1:
                rng = float(mx[q] - mn[q])
                doc[q] = np.ones_like(self.s_local[q]) if rng == 0 else (self.s_local[q] - float(mn[q])) / np.float32(rng)
            elif self.mass[q] > 0:
                doc[q] = (self.x_final[self.pv_local, q] / self.mass[q]).astype(np.float32)
            else:
                fl[q] |= 2
        a = np.ones_like(doc, bool) if doc_filter is None else self._allowed(doc_filter, b)[:, self.p_lo:self.p_hi]
        return _masked_topk(doc, a, k, self.p_lo)


def _problem(world):
    kg, pass_bits, fact_bits, index = make_case(1500, 12000, 32, seed=21, power_law=True)
    sidx = hd.shard_index(kg.csr, kg.passage_vertex, world, kg.subj_vertex, kg.obj_vertex, kg.num_chunks)
    n_p, n_f = len(kg.passage_vertex), len(kg.subj_vertex)
    rng = np.random.default_rng(3)
    # fact -> sources: one or two passages among the first 90 %; the last 10 % source no fact
    sourced = int(n_p * 0.9)
    counts = 1 + (rng.random(n_f) < 0.3)
    row_ptr = np.zeros(n_f + 1, np.int64)
    np.cumsum(counts, out=row_ptr[1:])
    pos = rng.integers(0, sourced, row_ptr[-1]).astype(np.int32)
    b = 70
    qf = torch.from_numpy(bf16_bits_to_float(synth.make_queries_np(fact_bits, b, 1)[0]))
    qp = torch.from_numpy(bf16_bits_to_float(synth.make_queries_np(pass_bits, b, 2)[0]))
    qp[7] = 0                                                         # every passage score 0: tied
    allowed = rng.random((b, n_p)) < 0.1
    lo1, hi1 = sidx.passages[1]
    allowed[:, lo1:hi1] = False                                      # shard 1 holds no allowed passage in any row
    allowed[3] = False                                               # empty A
    allowed[6] = False
    one = pos[np.flatnonzero((pos < lo1) | (pos >= hi1))[0]]
    allowed[6, one] = True                                           # a single allowed passage (it sources a fact)
    allowed[7] = True                                                # all allowed and tied
    f_lo, f_hi = sidx.facts[world - 1]                               # no fact of the last shard is allowed
    mine = np.zeros(n_p, bool)
    mine[pos[row_ptr[f_lo]:row_ptr[f_hi]]] = True
    allowed[8] &= ~mine
    allowed[8, lo1:hi1] = False
    assert allowed[8].any()
    allowed[9] = False                                               # passages without a fact: the DPR fallback
    allowed[9, sourced:] = True
    return kg, index, sidx, (row_ptr, pos), qf, qp, b, torch.from_numpy(allowed)


def _run_rank(rs, qf, qp, b, allowed):
    idx, sc = rs.score_facts(qf, k=5, scope_filter=allowed)
    cnt = (idx >= 0).sum(1).to(torch.int32)
    return (idx, sc) + tuple(rs.retrieve(qp, idx, sc, cnt, ppr_iters=ITERS, k=K, doc_filter=allowed,
                                         filter_scope="seeds"))


def _check(index, fact_sources, qf, qp, b, allowed, idx, sc, doc_idx, doc_val, flags):
    a = allowed.numpy()
    row_ptr, pos = fact_sources
    fm = fact_mask_np(a, row_ptr, pos)
    s_f = (qf.double().numpy() @ index.fact_emb.astype(np.float64).T).astype(np.float32)
    s_p = (qp.double().numpy() @ index.passage_emb.astype(np.float64).T).astype(np.float32)
    # phase A: the top 5 among the allowed facts, normalised over them
    want_idx, raw = _masked_topk(s_f, fm, 5, 0)
    mn, mx = _minmax_allowed(s_f, fm)
    rng = (mx - mn).unsqueeze(1)
    want_sc = torch.where(want_idx < 0, torch.zeros_like(raw),
                          torch.where(rng == 0, torch.ones_like(raw), (raw - mn.unsqueeze(1)) / rng))
    np.testing.assert_array_equal(idx.numpy(), want_idx.numpy())
    np.testing.assert_allclose(sc.numpy(), want_sc.numpy(), rtol=0, atol=1e-6)
    # phase B: the prior normalised over A (0 elsewhere), PPR over the whole graph, the ranking post-filtered by A
    prior = masked_minmax_rows(s_p, a)
    seen = set()
    for q in range(b):
        n = int((idx[q] >= 0).sum())
        if not a[q].any():
            seen.add("empty A")
            assert (doc_idx[q].numpy() == -1).all() and (doc_val[q].numpy() == 0).all(), q
            continue
        if n == 0:
            seen.add("dpr")
            assert flags[q] & 1, q
            by_p = oracle.min_max_normalize(prior[q])
            ids = np.flatnonzero(a[q])
            ids = ids[oracle.topk_desc(by_p[ids], K)]
            want_ids, want_sc = ids, by_p[ids]
        else:
            assert not flags[q] & 1, q
            fs = np.zeros(len(index.subj_vertex), np.float32)
            kept = idx[q, :n].numpy()
            fs[kept] = sc[q, :n].numpy()
            sid, sw = oracle.seed_weights(index, fs, kept.tolist(), 5)
            ids, scores, _ = oracle.run_ppr(index, oracle.reset_vector(index, sid, sw, prior[q]), 0.5, "power", ITERS)
            keep = a[q][ids]
            want_ids, want_sc = ids[keep][:K], scores[keep][:K]
        m = len(want_ids)
        np.testing.assert_array_equal(doc_idx[q, :m].numpy(), want_ids, err_msg=str(q))
        np.testing.assert_allclose(doc_val[q, :m].numpy(), want_sc, rtol=3e-6, atol=1e-7, err_msg=str(q))
        assert (doc_idx[q, m:].numpy() == -1).all(), q
    assert seen == {"empty A", "dpr"}


def test_scoped_problem_has_every_edge_case():
    world = 4
    kg, index, sidx, fsrc, qf, qp, b, allowed = _problem(world)
    a = allowed.numpy()
    row_ptr, pos = fsrc
    fm = fact_mask_np(a, row_ptr, pos)
    lo1, hi1 = sidx.passages[1]
    assert not a[np.arange(b) != 7][:, lo1:hi1].any()                # a shard with no allowed passage
    f_lo, f_hi = sidx.facts[world - 1]
    assert not fm[8, f_lo:f_hi].any() and fm[8].any()               # a shard with no allowed fact
    assert not a[3].any() and a[6].sum() == 1 and a[7].all()        # empty A, one passage, all allowed
    assert a[9].any() and not fm[9].any()                           # allowed passages, no allowed fact: DPR
    assert any(lo % 32 for lo, _ in sidx.passages[1:])               # a shard's slice starts inside a word


def test_scoped_sharded_retriever_four_local_shards_match_numpy():
    world = 4
    kg, index, sidx, fsrc, qf, qp, b, allowed = _problem(world)
    shared, results, errors = {}, [None] * world, []

    def worker(rank):
        try:
            rs = hd.ShardedRetriever(ScopedFakeShardStages(sidx, index, rank, fsrc), hd.LocalComm(rank, world, shared),
                                     groups=2)
            results[rank] = _run_rank(rs, qf, qp, b, allowed)
        except Exception as exc:
            errors.append((rank, repr(exc)))
            shared["_barrier"].abort()

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, errors
    _check(index, fsrc, qf, qp, b, allowed, *results[0])
    for r in range(1, world):
        for g, w in zip(results[r], results[0]):
            assert torch.equal(g, w)


def test_scoped_and_ranking_scopes_differ_on_the_same_case():
    """The "seeds" scope is not the post-filter: on the same case the "ranking" scope answers differently."""
    world = 2
    kg, index, sidx, fsrc, qf, qp, b, allowed = _problem(world)
    shared, results, errors = {}, [None] * world, []

    def worker(rank):
        try:
            rs = hd.ShardedRetriever(ScopedFakeShardStages(sidx, index, rank, fsrc), hd.LocalComm(rank, world, shared),
                                     groups=1)
            seeds = _run_rank(rs, qf, qp, b, allowed)
            idx, sc = rs.score_facts(qf, k=5)
            cnt = torch.full((b,), 5, dtype=torch.int32)
            ranking = (idx, sc) + tuple(rs.retrieve(qp, idx, sc, cnt, ppr_iters=ITERS, k=K, doc_filter=allowed))
            results[rank] = (seeds, ranking)
        except Exception as exc:
            errors.append((rank, repr(exc)))
            shared["_barrier"].abort()

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, errors
    seeds, ranking = results[0]
    assert not torch.equal(seeds[0], ranking[0])
    assert not torch.equal(seeds[2], ranking[2])


def _gloo_worker(rank, world, port, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        kg, index, sidx, fsrc, qf, qp, b, allowed = _problem(world)
        rs = hd.ShardedRetriever(ScopedFakeShardStages(sidx, index, rank, fsrc), hd.TorchComm(rank, world), groups=2)
        out = _run_rank(rs, qf, qp, b, allowed)
        if rank == 0:
            _check(index, fsrc, qf, qp, b, allowed, *out)
        gathered = [torch.empty_like(out[2]) for _ in range(world)]
        dist.all_gather(gathered, out[2])
        for g in gathered:
            assert torch.equal(g, out[2])
        ret[rank] = 1
    finally:
        dist.destroy_process_group()


def test_scoped_sharded_retriever_world2_gloo_matches_numpy():
    world = 2
    ret = mp.Manager().dict()
    mp.spawn(_gloo_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    assert dict(ret) == {0: 1, 1: 1}


def test_retrievers_without_fact_sources_still_refuse():
    """A shard engine without the table refuses exactly as before; one with it serves the scope."""
    st = FakeShardStages.__new__(FakeShardStages)
    with pytest.raises(ValueError, match="not supported"):
        hd.serve_seeds_scope(st, "seeds")
    with pytest.raises(ValueError, match="not supported"):
        hd.serve_seeds_scope(st, scope_filter=object())
    assert hd.serve_seeds_scope(st, "ranking") is False
    sc = ScopedFakeShardStages.__new__(ScopedFakeShardStages)
    assert hd.serve_seeds_scope(sc, "seeds") is True and hd.serve_seeds_scope(sc, "ranking") is False
    assert hd.serve_seeds_scope(sc, scope_filter=object()) is True
    with pytest.raises(ValueError, match="filter_scope"):
        hd.serve_seeds_scope(sc, "tenant")


def test_shard_index_keeps_passage_and_fact_order():
    """build_shard_engine(fact_sources=) applies the GLOBAL table unchanged: shard_index relabels vertices only --
    passage positions and fact ids keep their order, and shard g's passages / facts are contiguous ranges in it."""
    kg = synth.make_kg(3000, 30000, seed=9, power_law=True)
    for world in (1, 2, 3, 8):
        s = hd.shard_index(kg.csr, kg.passage_vertex, world, kg.subj_vertex, kg.obj_vertex, kg.num_chunks)
        np.testing.assert_array_equal(s.passage_vertex, s.perm[kg.passage_vertex])    # passage p stays passage p
        np.testing.assert_array_equal(s.subj_vertex, s.perm[kg.subj_vertex])          # fact f stays fact f
        np.testing.assert_array_equal(s.obj_vertex, s.perm[kg.obj_vertex])
        for parts, n in ((s.passages, len(kg.passage_vertex)), (s.facts, len(kg.subj_vertex))):
            assert parts[0][0] == 0 and parts[-1][1] == n
            assert all(parts[g][1] == parts[g + 1][0] for g in range(world - 1))
