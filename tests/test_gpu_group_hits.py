"""Group hits on the device (include/hrag.h "group hits", csrc/group.hip group_hits_kernel): hrag_group_hits_rows against
the numpy restatement of tests/group_hits_helpers.py bit for bit; hrag_last_group_hits behind the grouped engine calls on
every PPR state path against the restatement applied to hrag_last_doc_scores and against hrag_retrieve_filtered under the
filter (allowed AND member of the group); the composition with the doc filter / the "seeds" scope / the convergence
contract / HRAG_OPT_ACCEL; the dense call, workspaces, the tiled route, the mirror and the argument errors."""

import threading

import numpy as np
import pytest

from hipporag_amd import synth
from hipporag_amd.engine import pack_mask
from oracle.checks import make_case
from tests.group_helpers import csr_of, random_groups, same_bits
from tests.group_hits_helpers import group_hits_np, random_group_ids

pytestmark = pytest.mark.gpu


def _bf16(bits, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)


def _np(t):
    return t.cpu().numpy()


def _words(m, dev):
    import torch
    return torch.from_numpy(pack_mask(m).view(np.int32)).to(dev)


def _bits_equal(a, b):
    a, b = _np(a), _np(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


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


class _Rows:
    """hrag_group_hits_rows over one uploaded set of score rows and one group table."""

    def __init__(self, dev, x, ld, g, n_groups):
        import torch
        from hipporag_amd import _lib
        self.lib, self.check, self.dev = _lib.load(), _lib.check, dev
        self.b, self.n = x.shape
        self.ld, self.n_groups = ld, n_groups
        xd = torch.zeros((self.b, ld), dtype=torch.float32)
        xd[:, :self.n] = torch.from_numpy(x)
        self.xd = xd.to(dev)
        ptr, members = csr_of(g, n_groups)
        self.ptr, self.mem = torch.from_numpy(ptr).to(dev), torch.from_numpy(members).to(dev)

    def mask(self, mask, per_query, bit_offset):
        """The filter as device words, the rows of interest starting at bit_offset of rows with random bits around them."""
        if mask is None:
            return None, 0, 0
        rng = np.random.default_rng(bit_offset + 1)
        rows = mask if per_query else mask[:1]
        wide = np.concatenate([rng.random((rows.shape[0], bit_offset)) < 0.5, rows, rng.random((rows.shape[0], 37)) < 0.5], axis=1)
        w = _words(wide, self.dev)
        return w, (w.shape[1] if per_query else 0), bit_offset

    def __call__(self, ids, m, w=None, wld=0, off=0):
        import torch
        k = ids.shape[1]
        gi = torch.from_numpy(ids).to(self.dev)
        size = self.b * k * m
        hi = torch.full((size + 64,), 7, dtype=torch.int32, device=self.dev)            # a guard behind the [b, k, m] arrays
        hs = torch.full((size + 64,), 7.0, dtype=torch.float32, device=self.dev)
        self.check(self.lib.hrag_group_hits_rows(self.xd.data_ptr(), self.b, self.n, self.ld, self.ptr.data_ptr(),
                                                 self.mem.data_ptr(), self.n_groups, gi.data_ptr(), k, m,
                                                 w.data_ptr() if w is not None else None, wld, off, hi.data_ptr(),
                                                 hs.data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        hi, hs = _np(hi), _np(hs)
        assert (hi[size:] == 7).all() and (hs[size:] == 7.0).all()                      # nothing written past the arrays
        return hi[:size].reshape(self.b, k, m), hs[:size].reshape(self.b, k, m)


def _check_against_np(hits, x, g, masks, ids, m, msg):
    hi, hs = hits
    for i in range(x.shape[0]):
        e = group_hits_np(x[i], g, None if masks is None else masks[i], ids[i], m)
        assert hi[i].tolist() == e[0].tolist(), (msg, i)
        assert same_bits(hs[i], e[1]), (msg, i)
        assert (hs[i].view(np.uint32)[hi[i] < 0] == 0).all(), (msg, i)


SHAPES = [("one", 1000, 1), ("singletons", 777, 8), ("two", 4099, 9), ("contiguous", 5003, 64), ("shuffled", 6001, 65),
          ("power", 3000, 2), ("contiguous", 2048, 256)]


@pytest.mark.parametrize("kind,n,b", SHAPES)
def test_group_hits_rows_against_numpy(gpu_device, kind, n, b):
    rng = np.random.default_rng(n + b)
    g = random_groups(rng, n, kind)
    n_groups = int(g.max()) + 1
    x = _scores(rng, b, n)
    mask = rng.random((b, n)) < 0.4
    mask[0] = False
    rows = _Rows(gpu_device, x, n + 3, g, n_groups)
    for k in (1, 200, 2500):
        ids = random_group_ids(rng, n_groups, b, k)
        for m_, per_query, off in ((None, True, 0), (mask, True, 0), (mask, True, 13), (mask, False, 45)):
            w, wld, o = rows.mask(m_, per_query, off)
            masks = None if m_ is None else (m_ if per_query else np.broadcast_to(m_[0], m_.shape))
            want = [group_hits_np(x[i], g, None if masks is None else masks[i], ids[i], 64) for i in range(b)]
            want_i, want_s = np.stack([w_[0] for w_ in want]), np.stack([w_[1] for w_ in want])
            for m in (1, 2, 8, 64):                           # the first m of a row's 64 are its m: one restatement run
                hi, hs = rows(ids, m, w, wld, o)
                assert np.array_equal(hi, want_i[:, :, :m]), (kind, k, m, off)
                assert same_bits(hs, want_s[:, :, :m]), (kind, k, m, off)
                assert (hs.view(np.uint32)[hi < 0] == 0).all()


def test_group_hits_rows_long_group_equal_scores_and_nan_rows(gpu_device):
    """The power-law table with one group beyond 50 000 members; a row of all-equal scores (the order is the position's
    alone), a row with many NaN (ranked first, by position), a PPR-like row."""
    rng = np.random.default_rng(3)
    n = 70001
    small = random_groups(rng, n - 52000, "power")
    big = int(small.max()) + 1
    g = np.concatenate([small, np.full(52000, big, np.int32)])
    g = g[rng.permutation(n)]
    n_groups = big + 1
    x = _scores(rng, 4, n)
    x[1] = np.float32(0.25)
    x[2, rng.random(n) < 0.3] = np.nan
    x[3] = np.abs(x[3]) * np.float32(1e-5)
    mask = rng.random((4, n)) < 0.7
    rows = _Rows(gpu_device, x, n + 3, g, n_groups)
    ids = random_group_ids(rng, n_groups, 4, 200)
    ids[:, 0] = big
    ids[:, 5] = big
    for m_, off in ((None, 0), (mask, 0), (mask, 13)):
        w, wld, o = rows.mask(m_, True, off)
        for m in (1, 2, 8, 64):
            _check_against_np(rows(ids, m, w, wld, o), x, g, m_, ids, m, f"long m={m} off={off}")


# ------------------------------------------------------------------ engines
@pytest.fixture(scope="module")
def case(gpu_device):
    from hipporag_amd._lib import OPT_NO_F16, OPT_NO_FP8
    from hipporag_amd.engine import HippoRAGEngine
    kg, pass_bits, fact_bits, index = make_case(24000, 200000, 64, seed=6161)
    g = random_groups(np.random.default_rng(1), kg.n_passages, "shuffled")
    engines = {}
    for name, flags in (("default", 0), ("f32", OPT_NO_FP8 | OPT_NO_F16)):
        e = HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                           max_batch=257, max_topk=kg.n_passages, flags=flags)
        e.set_passage_groups(g)
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
    cnt[::4] = 0                                            # DPR fallback rows (kept_count 0)
    return qp, idx, sc, cnt


def _same_call(out, ref, msg):
    """Every output of the grouped call is what the call without group_hits returns."""
    for name in ("group_idx", "doc_idx", "doc_score", "flags", "residual", "iters_used"):
        a, b = getattr(out, name), getattr(ref, name)
        assert (a is None) == (b is None) and (a is None or _bits_equal(a, b)), (msg, name)


def _check_hits(out, full, g, allowed, m, agg, msg):
    hi, hs, gi = _np(out.hit_idx), _np(out.hit_score), _np(out.group_idx)
    assert hi.shape == gi.shape + (m,) and hi.dtype == np.int32 and hs.dtype == np.float32
    for i in range(full.shape[0]):
        a = None if allowed is None else (allowed if allowed.ndim == 1 else allowed[i])
        e = group_hits_np(full[i], g, a, gi[i], m)
        assert hi[i].tolist() == e[0].tolist(), (msg, i)
        assert same_bits(hs[i], e[1]), (msg, i)
    assert np.array_equal(hi[:, :, 0], _np(out.best_doc_idx)), msg                  # consequence 1
    if agg == "max":
        assert np.array_equal(hs[:, :, 0].view(np.uint32), _np(out.group_score).view(np.uint32)), msg


STATES = [("small1", "default", 1, 4), ("small8", "default", 8, 4), ("f16", "default", 64, 2), ("fp8", "default", 257, 8),
          ("f32-1", "f32", 1, None), ("f32-8", "f32", 8, None), ("f32-64", "f32", 64, None), ("f32-257", "f32", 257, None)]


@pytest.mark.parametrize("state,which,b,want_state", STATES)
def test_hits_behind_the_grouped_retrieve_on_every_state_path(case, state, which, b, want_state):
    import torch
    dev, kg, pass_bits, fact_bits, engines, g = case
    eng = engines[which]
    n_p = kg.n_passages
    qp, idx, sc, cnt = _inputs(dev, eng, fact_bits, pass_bits, b, 40 + b)
    member = None
    for agg, k, m in (("max", 10, 3), ("max", 200, 8), ("sum", 50, 3), ("sum", 7, 64)):
        ref = eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=k, group_agg=agg)
        out = eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=k, group_agg=agg, group_hits=m)
        if want_state is not None:
            assert eng.stats()["last_ppr_state"] == want_state
        else:
            assert eng.stats()["last_ppr_state"] not in (2, 8)              # neither the fp16 nor the fp8 state
        assert (_np(out.flags)[::4] & 1).all()
        _same_call(out, ref, f"{state} {agg} k={k}")
        full = _np(eng.last_doc_scores(b))
        _check_hits(out, full, g, None, m, agg, f"{state} {agg} k={k} m={m}")
        if member is None:
            # consequence 2: for one (query, ranked group) pair per query, the existing filtered ranking under the filter
            # "member of that group" -- a second full PPR per pair, which the hits spare the caller
            gi, hi, hs = _np(out.group_idx), _np(out.hit_idx), _np(out.hit_score)
            slot = np.arange(b) % k
            member = g[None, :] == gi[np.arange(b), slot][:, None]
            flt = eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=m, doc_filter=_words(member, dev))
            assert np.array_equal(_np(flt.doc_idx), hi[np.arange(b), slot]), state
            assert np.array_equal(_np(flt.doc_score).view(np.uint32), hs[np.arange(b), slot].view(np.uint32)), state
    # retrieve_scored: the same rows through the other entry point
    raw = eng.sim_scores("passages", qp)
    a1 = eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=50, group_agg="sum", group_hits=5)
    a1 = [_np(t).copy() for t in (a1.group_idx, a1.hit_idx, a1.hit_score)]
    a2 = eng.retrieve_scored(raw, idx, sc, cnt, ppr_iters=20, k=50, group_agg="sum", group_hits=5)
    for x, y in zip(a1, (a2.group_idx, a2.hit_idx, a2.hit_score)):
        assert np.array_equal(x.view(np.int32), _np(y).view(np.int32))
    # ids that did not come from the grouped call: any [B, k] ids in [-1, n_groups), an id outside treated as -1
    n_groups = int(g.max()) + 1
    ids = random_group_ids(np.random.default_rng(b), n_groups, b, 9)
    ids[:, 3] = n_groups + 5
    hi, hs = eng.last_group_hits(torch.from_numpy(ids), 4)
    full = _np(eng.last_doc_scores(b))
    seen = np.where(ids >= n_groups, -1, ids)
    for i in range(b):
        e = group_hits_np(full[i], g, None, seen[i], 4)
        assert _np(hi)[i].tolist() == e[0].tolist() and same_bits(_np(hs)[i], e[1]), (state, i)


@pytest.mark.parametrize("state,which,b", [("f16", "default", 64), ("fp8", "default", 257), ("f32", "f32", 8)])
def test_hits_compose_with_filter_scope_contract_and_accel(case, state, which, b):
    from hipporag_amd._lib import OPT_ACCEL
    dev, kg, pass_bits, fact_bits, engines, g = case
    eng = engines[which]
    n_p = kg.n_passages
    qp, idx, sc, cnt = _inputs(dev, eng, fact_bits, pass_bits, b, 70 + b)
    rng = np.random.default_rng(b)
    per = rng.random((b, n_p)) < 0.3
    per[-1] = False
    one = rng.random(n_p) < 0.05
    for m_ in (per, one):
        w = _words(m_, dev)
        for agg in ("max", "sum"):
            for scope in ("ranking", "seeds"):
                kw = dict(ppr_iters=20, k=60, doc_filter=w, filter_scope=scope, group_agg=agg)
                ref = eng.retrieve(qp, idx, sc, cnt, **kw)
                out = eng.retrieve(qp, idx, sc, cnt, group_hits=4, **kw)
                _same_call(out, ref, f"{state} {agg} {scope} {m_.shape}")
                full = _np(eng.last_doc_scores(b))
                _check_hits(out, full, g, m_, 4, agg, f"{state} {agg} {scope} {m_.shape}")
                if m_.ndim == 2:
                    assert (_np(out.hit_idx)[-1] == -1).all()                       # a filter that allows nothing
    for setup in ("tol", "accel"):
        if setup == "accel":
            eng.set_flags(OPT_ACCEL, True)
        try:
            kw = dict(ppr_iters=20, ppr_tol=1.5e-6, ppr_max_iters=30) if setup == "tol" else dict(ppr_iters=20)
            ref = eng.retrieve(qp, idx, sc, cnt, k=64, group_agg="sum", **kw)
            out = eng.retrieve(qp, idx, sc, cnt, k=64, group_agg="sum", group_hits=6, **kw)
            _same_call(out, ref, f"{state} {setup}")
            full = _np(eng.last_doc_scores(b))
            _check_hits(out, full, g, None, 6, "sum", f"{state} {setup}")
        finally:
            if setup == "accel":
                eng.set_flags(OPT_ACCEL, False)


def test_hits_behind_the_grouped_dense_retrieve(case):
    dev, kg, pass_bits, fact_bits, engines, g = case
    eng = engines["default"]
    n_p = kg.n_passages
    qp = _bf16(synth.make_queries_np(pass_bits, 33, seed=5)[0], dev)
    pi, ps = (_np(t) for t in eng.dense_retrieve(qp, k=n_p))
    full = np.zeros((33, n_p), np.float32)
    np.put_along_axis(full, pi.astype(np.int64), ps, axis=1)          # the normalised dense scores by position
    mask = np.random.default_rng(2).random((33, n_p)) < 0.2
    for agg in ("max", "sum"):
        for m_ in (None, mask):
            kw = {} if m_ is None else {"doc_filter": _words(m_, dev)}
            ref = eng.dense_retrieve(qp, k=40, group_agg=agg, **kw)
            got = eng.dense_retrieve(qp, k=40, group_agg=agg, group_hits=5, **kw)
            assert len(ref) == 3 and len(got) == 5
            for a, b_ in zip(ref, got):
                assert _bits_equal(a, b_)
            gi, gs, rep, hi, hs = (_np(t) for t in got)
            for i in range(33):
                e = group_hits_np(full[i], g, None if m_ is None else m_[i], gi[i], 5)
                assert hi[i].tolist() == e[0].tolist() and same_bits(hs[i], e[1]), (agg, i)
            assert np.array_equal(hi[:, :, 0], rep)
            if agg == "max":
                assert np.array_equal(hs[:, :, 0].view(np.uint32), gs.view(np.uint32))


def test_workspaces_two_threads_with_hits_bit_identical(gpu_device):
    import torch
    from hipporag_amd.engine import HippoRAGEngine
    dev = gpu_device
    kg, pass_bits, fact_bits, _ = make_case(6000, 60000, 128, seed=4343)
    g = random_groups(np.random.default_rng(4), kg.n_passages, "contiguous")

    def q(bits, b, seed):
        return _bf16(synth.make_queries_np(bits, b, seed=seed)[0], dev)

    def run(h, qf, qp):
        b = qf.shape[0]
        idx, sc = h.score_facts(qf, k=5)
        cnt = torch.full((b,), 5, dtype=torch.int32, device=dev)
        gm = h.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=50, group_agg="max", group_hits=3)
        gsum = h.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=50, group_agg="sum", group_hits=8)
        dg = h.dense_retrieve(qp, k=50, group_agg="sum", group_hits=2)
        return [gm.group_idx, gm.group_score, gm.best_doc_idx, gm.hit_idx, gm.hit_score, gsum.group_idx, gsum.group_score,
                gsum.hit_idx, gsum.hit_score, *dg]

    with HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                        max_batch=130, max_topk=50) as eng:
        eng.set_passage_groups(g)
        for batch in (9, 130):
            qa, qb = (q(fact_bits, batch, 11), q(pass_bits, batch, 12)), (q(fact_bits, batch, 21), q(pass_bits, batch, 22))
            ref_a = [t.clone() for t in run(eng, *qa)]
            ref_b = [t.clone() for t in run(eng, *qb)]
            torch.cuda.synchronize()
            w = eng.workspace()
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


def test_argument_errors_leave_the_outputs_untouched(case):
    import torch
    from hipporag_amd import _lib
    from hipporag_amd.engine import HippoRAGEngine
    dev, kg, pass_bits, fact_bits, engines, g = case
    eng = engines["default"]
    lib = _lib.load()
    n_p, n_groups = kg.n_passages, int(g.max()) + 1
    qp, idx, sc, cnt = _inputs(dev, eng, fact_bits, pass_bits, 4, 3)
    out = eng.retrieve(qp, idx, sc, cnt, k=5, group_agg="max")
    stream = torch.cuda.current_stream().cuda_stream
    hi = torch.full((4, 5, 64), 7, dtype=torch.int32, device=dev)
    hs = torch.full((4, 5, 64), 7.0, dtype=torch.float32, device=dev)
    gi = out.group_idx

    def untouched():
        torch.cuda.synchronize()
        return bool((hi == 7).all()) and bool((hs == 7.0).all())

    def last(e, batch, k, m, gi_ptr=gi.data_ptr(), hi_ptr=hi.data_ptr(), hs_ptr=hs.data_ptr(), fw=None, fld=0):
        return lib.hrag_last_group_hits(e._handle, batch, gi_ptr, k, m, fw, fld, hi_ptr, hs_ptr, stream)

    for m in (0, 65, -3):
        assert last(eng, 4, 5, m) == _lib.HRAG_EINVAL and b"hits" in lib.hrag_last_error()
        assert untouched()
    assert last(eng, 4, 0, 3) == _lib.HRAG_EINVAL and untouched()
    assert last(eng, 4, 5, 3, gi_ptr=None) == _lib.HRAG_EINVAL and untouched()
    assert last(eng, 4, 5, 3, hi_ptr=None) == _lib.HRAG_EINVAL and untouched()
    assert last(eng, 5, 5, 3) == _lib.HRAG_EINVAL and b"exceeds" in lib.hrag_last_error()   # the rows are a batch of 4
    assert untouched()
    short = torch.zeros((4, 3), dtype=torch.int32, device=dev)
    assert last(eng, 4, 5, 3, fw=short.data_ptr(), fld=3) == _lib.HRAG_EINVAL and untouched()   # filter rows too short
    assert last(eng, 4, 5, 3) == _lib.HRAG_OK                                                # and the good call still works
    torch.cuda.synchronize()
    e0 = group_hits_np(_np(eng.last_doc_scores(4))[0], g, None, _np(gi)[0], 3)
    assert _np(hi).reshape(-1)[:15].reshape(5, 3).tolist() == e0[0].tolist()
    hi.fill_(7)
    hs.fill_(7.0)
    # Python: the checks of the keyword
    for bad in (0, 65):
        with pytest.raises(ValueError):
            eng.retrieve(qp, idx, sc, cnt, k=5, group_agg="max", group_hits=bad)
    with pytest.raises(ValueError, match="group_agg"):
        eng.retrieve(qp, idx, sc, cnt, k=5, group_hits=3)
    with pytest.raises(ValueError, match="group_agg"):
        eng.dense_retrieve(qp, k=5, group_hits=3)
    # a fresh handle has no rows; an ungrouped dense call writes none; a grouped dense call does
    w = eng.workspace()
    try:
        assert last(w, 4, 5, 3) == _lib.HRAG_EINVAL and b"no score rows" in lib.hrag_last_error()
        w.dense_retrieve(qp, k=5)
        assert last(w, 4, 5, 3) == _lib.HRAG_EINVAL and b"no score rows" in lib.hrag_last_error()
        assert untouched()
        w.dense_retrieve(qp[:2], k=5, group_agg="max")
        assert last(w, 2, 5, 3) == _lib.HRAG_OK
        assert last(w, 3, 5, 3) == _lib.HRAG_EINVAL
        torch.cuda.synchronize()
    finally:
        w.close()
    hi.fill_(7)
    hs.fill_(7.0)
    # the engine-free call: the checks of hrag_group_rows plus hits and k
    x = torch.zeros((2, 100), dtype=torch.float32, device=dev)
    ptr, members = csr_of(np.zeros(100, np.int32), 1)
    ptr_d, mem_d = torch.from_numpy(ptr).to(dev), torch.from_numpy(members).to(dev)
    ids = torch.zeros((2, 5), dtype=torch.int32, device=dev)

    def rows(batch=2, n=100, ld=100, n_groups=1, k=5, m=3, fw=None, fld=0, off=0):
        return lib.hrag_group_hits_rows(x.data_ptr(), batch, n, ld, ptr_d.data_ptr(), mem_d.data_ptr(), n_groups,
                                        ids.data_ptr(), k, m, fw, fld, off, hi.data_ptr(), hs.data_ptr(), stream)

    for kw in (dict(m=0), dict(m=65), dict(k=0), dict(batch=0), dict(ld=99), dict(n_groups=0), dict(n_groups=101),
               dict(fw=short.data_ptr(), fld=3), dict(fw=short.data_ptr(), fld=0, off=-1)):
        assert rows(**kw) == _lib.HRAG_EINVAL, kw
        assert untouched(), kw
    assert rows() == _lib.HRAG_OK
    torch.cuda.synchronize()
    # without a group table, and on a row-shard engine
    bare = HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                          max_batch=4, max_topk=10)
    try:
        bare.retrieve(qp, idx, sc, cnt, k=5)
        hi.fill_(7)
        hs.fill_(7.0)
        assert last(bare, 4, 5, 3) == _lib.HRAG_EINVAL and b"hrag_engine_set_passage_groups" in lib.hrag_last_error()
        assert untouched()
    finally:
        bare.close()
    from hipporag_amd import dist
    sidx = dist.shard_index(kg.csr, kg.passage_vertex, 2, kg.subj_vertex, kg.obj_vertex, kg.num_chunks)
    sh = dist.build_shard_engine(sidx, pass_bits, fact_bits, 1, max_batch=8, max_topk=10)
    try:
        assert last(sh, 4, 5, 3) == _lib.HRAG_EINVAL and b"row-shard" in lib.hrag_last_error()
        assert untouched()
    finally:
        sh.close()


def test_mirror_group_hits_equal_grouping_the_full_ranking_and_the_tiled_route(gpu_device):
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
    queries = [" ".join(triples[i][0]) for i in range(0, 600, 13) if triples[i]][:40]      # three tiles of max_batch = 16
    assert len(queries) > 2 * 16
    for fn in (rag.retrieve, rag.retrieve_dpr):
        full = fn(queries, num_to_retrieve=n_p)
        for agg in ("max", "sum"):
            plain = fn(queries, num_to_retrieve=15, group_by="source_id", group_agg=agg)
            got = fn(queries, num_to_retrieve=15, group_by="source_id", group_agg=agg, group_hits=3)
            tiles = [r for lo in range(0, len(queries), 16)
                     for r in fn(queries[lo: lo + 16], num_to_retrieve=15, group_by="source_id", group_agg=agg, group_hits=3)]
            for f, p, gq, tq in zip(full, plain, got, tiles):
                assert gq.docs == p.docs                                                    # docs and scores unchanged
                assert np.array_equal(np.asarray(gq.doc_scores, np.float32).view(np.uint32),
                                      np.asarray(p.doc_scores, np.float32).view(np.uint32))
                assert "group_hits" not in p.doc_metadata[0]
                by_pos = np.zeros(n_p, np.float32)
                by_pos[[pos[d] for d in f.docs]] = np.asarray(f.doc_scores, np.float32)
                gids = [values.index(m["group"]) if m["group"] is not None else int(group_of[pos[d]])
                        for m, d in zip(gq.doc_metadata, gq.docs)]
                e = group_hits_np(by_pos, group_of, None, gids, 3)
                for j, md in enumerate(gq.doc_metadata):
                    hits = md["group_hits"]
                    keep = e[0][j] >= 0
                    assert [h["position"] for h in hits] == e[0][j][keep].tolist(), (fn.__name__, agg, j)
                    assert [h["doc"] for h in hits] == [rag.passage_texts[p_] for p_ in e[0][j][keep]]
                    assert same_bits(np.asarray([h["score"] for h in hits], np.float32), e[1][j][keep])
                    assert hits[0]["doc"] == gq.docs[j] and len(hits) == min(3, md["group_size"])
                assert [m["group_hits"] for m in tq.doc_metadata] == [m["group_hits"] for m in gq.doc_metadata]
                assert tq.docs == gq.docs
    # beyond the engine's max_topk the host form serves the same call: both routes agree
    small = HippoRAG(RetrievalConfig(embedding_precision="bf16", max_batch=16, retrieval_top_k=5, ppr_tol=0.0,
                                     ppr_accel=False), embedding_model=sup.Bf16Mock())
    small.index_from_openie(chunks, triples)
    a = rag.retrieve(queries[:16], num_to_retrieve=15, group_by="source_id", group_hits=3)
    b = small.retrieve(queries[:16], num_to_retrieve=15, group_by="source_id", group_hits=3)
    for x, y in zip(a, b):
        assert x.docs == y.docs
        assert [m["group_hits"] for m in x.doc_metadata] == [m["group_hits"] for m in y.doc_metadata]
