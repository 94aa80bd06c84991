"""The stage-level operators of include/hrag.h composed by hand, and on row shards.

  h. "hrag_retrieve() is exactly the composition of these": on an HRAG_OPT_F32_STATE engine
     row_minmax -> seeds -> teleport -> ppr_init -> K x ppr_step -> colsum -> doc_scores -> topk on caller-owned buffers
     gives the bits of retrieve_scored on the same engine -- all passage scores, flags, ranked ids and scores.  The
     engine's own path (csrc/engine.hip retrieve_impl, the fp32-state branch) launches the same kernels with the same
     arguments, so nothing but equality is acceptable.
  i. "on the rows this engine owns": engines created on contiguous row windows of the same graph (one of them empty,
     every cut inside the passage vertices' range, the hub graph's first window owning multi-segment rows) write their
     ppr_init / ppr_step into ONE shared state pair; after every sweep it equals the unsharded engine's bit for bit,
     every shard having touched its own rows only (which also means a seed outside a shard's window is ignored by it
     and applied exactly once overall); the shards' colsums add up to the unsharded one; doc_scores on any shard
     engine equals the unsharded engine's.
  j. the argument checks the header states: status, a message, nothing launched."""

import numpy as np
import pytest

from tests import stage_helpers as sh
from tests.test_gpu_csr_sweep import SENTINEL_BITS, _hub, bits, dev, make_engine, sentinel

pytestmark = pytest.mark.gpu

K = 50


@pytest.fixture(scope="module")
def graphs():
    return {"edge": sh.edge_graph(), "hub": _hub()}


def _inputs(rng, g, b, device):
    """raw passage scores and kept facts; queries 1 and b - 1 keep nothing (the DPR fallback)"""
    n_p, n_f = len(g["passage_vertex"]), len(g["subj"])
    scores = rng.standard_normal((b, n_p)).astype(np.float32)
    kept_idx = rng.integers(0, n_f, (b, 5)).astype(np.int32)
    kept_idx[:, 0] = rng.integers(0, 32, b)                # facts whose subject is a hub / threshold / isolated row
    kept_score = (rng.random((b, 5)) + 0.05).astype(np.float32)
    kept_count = np.full(b, 5, np.int32)
    kept_count[[1, b - 1]] = 0
    kept_count[2] = 3
    return tuple(dev(a, device) for a in (scores, kept_idx, kept_score, kept_count))


def _compose(st, scores, kept_idx, kept_score, kept_count, b, damping, iters, device):
    sv, sw, sc, flags = st.seeds(kept_idx, kept_score, kept_count, 5)
    mn, mx = st.row_minmax(scores)
    tele = st.teleport(scores, mn, mx, 0.05, flags)
    bc, ns = st.layout(b)
    x, y = (sentinel((ns, st.e.num_vertices, bc), device) for _ in range(2))
    st.ppr_init(tele, (sv, sw, sc), b, x)
    for _ in range(iters):
        st.ppr_step(tele, (sv, sw, sc), b, damping, x, y)
        x, y = y, x
    sums = st.colsum(x, b)
    doc = st.doc_scores(x, sums, b, scores, mn, mx, flags)
    idx, val, _, _ = st.topk(doc, K)
    return doc, flags, idx, val


# ----------------------------------------------------------------------------- h. the header's promise
@pytest.mark.parametrize("width", [16, 32, 64])
@pytest.mark.parametrize("graph", ["edge", "hub"])
def test_retrieve_is_exactly_the_composition_of_the_stage_operators(gpu_device, graphs, graph, width):
    import torch
    from hipporag_amd._lib import PPR_STATE_F32
    from hipporag_amd.engine import EngineStages
    g = graphs[graph]
    rng = np.random.default_rng(width + len(graph))
    with make_engine(g, width, 70) as eng:
        st = EngineStages(eng)
        for b in (5, 40, 70):
            scores, kept_idx, kept_score, kept_count = _inputs(rng, g, b, gpu_device)
            for iters in (1, 12, 20):
                for damping in (0.5, 0.85):
                    what = f"{graph} width={width} b={b} iters={iters} damping={damping}"
                    out = eng.retrieve_scored(scores, kept_idx, kept_score, kept_count, link_top_k=5, damping=damping,
                                              passage_node_weight=0.05, ppr_iters=iters, k=K)
                    want_doc = eng.last_doc_scores(b)
                    torch.cuda.synchronize()
                    # (batches <= 8 too: an fp32-state engine has no small-batch kernels)
                    assert eng.timings()["slab_width"] == eng.layout(b)[0], what
                    assert eng.stats()["last_ppr_state"] == PPR_STATE_F32, what
                    doc, flags, idx, val = _compose(st, scores, kept_idx, kept_score, kept_count, b, damping, iters,
                                                    gpu_device)
                    torch.cuda.synchronize()
                    flags_h = flags.cpu().numpy()
                    np.testing.assert_array_equal(flags_h, out.flags.cpu().numpy(), err_msg=f"flags {what}")
                    assert (flags_h[[1, b - 1]] & 1).all() and not (flags_h[0] & 1), what
                    np.testing.assert_array_equal(bits(doc.cpu().numpy()), bits(want_doc.cpu().numpy()),
                                                  err_msg=f"all passage scores {what}")
                    np.testing.assert_array_equal(idx.cpu().numpy(), out.doc_idx.cpu().numpy(), err_msg=f"ranked ids {what}")
                    np.testing.assert_array_equal(bits(val.cpu().numpy()), bits(out.doc_score.cpu().numpy()),
                                                  err_msg=f"ranked scores {what}")
                    assert np.isfinite(val.cpu().numpy()).all(), what


# ----------------------------------------------------------------------------- i. row shards
def _cuts(v, split):
    return {"2": [0, (3 * v) // 8 + 3, v], "3": [0, v // 7 + 1, (2 * v) // 3 + 5, v],
            "3-one-empty": [0, v // 5 + 2, v // 5 + 2, v]}[split]


def _outside_untouched(after, before, lo, hi, what):
    import torch
    a, b_ = after.view(torch.int32), before.view(torch.int32)
    assert torch.equal(a[:, :lo], b_[:, :lo]) and torch.equal(a[:, hi:], b_[:, hi:]), f"{what}: wrote outside rows [{lo}, {hi})"


@pytest.mark.parametrize("split", ["2", "3", "3-one-empty"])
@pytest.mark.parametrize("graph,width,b", [("edge", 16, 21), ("hub", 32, 40), ("edge", 64, 70)])
def test_row_shards_share_one_state(gpu_device, graphs, graph, width, b, split):
    import torch
    from hipporag_amd.engine import EngineStages
    g = graphs[graph]
    csr, pv = g["csr"], g["passage_vertex"]
    v = csr.num_vertices
    cuts = _cuts(v, split)
    windows = list(zip(cuts[:-1], cuts[1:]))
    assert any(lo == hi for lo, hi in windows) == (split == "3-one-empty")
    pv_sorted = np.sort(pv)
    assert all(pv_sorted[0] < lo < pv_sorted[-1] for lo, _ in windows[1:])    # every cut lies among the passage vertices
    if graph == "hub":
        assert int((np.diff(csr.row_ptr)[:windows[0][1]] > 512).sum()) >= 48    # the first window owns the hubs
    rng = np.random.default_rng(width + len(split))
    seg = 128 if graph == "edge" else 0
    lay = (width, -(-b // width))
    with make_engine(g, width, b, segment_nnz=seg) as full:
        shards = [make_engine(dict(g, csr=csr.rows(lo, hi)), width, b, segment_nnz=seg, row_offset=lo) for lo, hi in windows]
        try:
            st0, sts = EngineStages(full), [EngineStages(e) for e in shards]
            assert all(s.layout(b) == lay for s in [st0] + sts)
            assert [(e.row_offset, e.n_rows) for e in shards] == [(lo, hi - lo) for lo, hi in windows]
            tele32 = sh.random_tele(rng, b, len(pv))
            seeds = sh.random_seeds(rng, b, v, g["seed_pool"])
            tele = dev(sh.to_slab(tele32, width), gpu_device)
            seeds_d = tuple(dev(a, gpu_device) for a in seeds)
            shape = (lay[1], v, width)

            def on_shards(call, what):
                out = sentinel(shape, gpu_device)
                for (lo, hi), s in zip(windows, sts):
                    before = out.clone()
                    call(s, out)
                    torch.cuda.synchronize()
                    _outside_untouched(out, before, lo, hi, what)
                return out

            x_full = sentinel(shape, gpu_device)
            st0.ppr_init(tele, seeds_d, b, x_full)
            x_sh = on_shards(lambda s, out: s.ppr_init(tele, seeds_d, b, out), "ppr_init")
            assert torch.equal(x_sh.view(torch.int32), x_full.view(torch.int32)), "ppr_init"
            want0 = sh.init_np(tele32, g["r2t"], seeds, v)
            np.testing.assert_array_equal(bits(sh.from_slab(x_sh.cpu().numpy(), b)), bits(want0))
            for sweep in range(5):
                y_full = sentinel(shape, gpu_device)
                st0.ppr_step(tele, seeds_d, b, 0.5, x_full, y_full)
                y_sh = on_shards(lambda s, out: s.ppr_step(tele, seeds_d, b, 0.5, x_sh, out), f"ppr_step {sweep}")
                same = y_sh.view(torch.int32) == y_full.view(torch.int32)
                assert bool(same.all()), f"sweep {sweep}: {int((~same).sum())} elements differ from the unsharded engine"
                assert not bool(torch.isnan(y_sh).any()), f"sweep {sweep}"
                x_full, x_sh = y_full, y_sh
            # colsum: the shards' sums add up
            total = st0.colsum(x_full, b).cpu().numpy()
            parts = [s.colsum(x_sh, b).cpu().numpy() for s in sts]
            x_h = sh.from_slab(x_sh.cpu().numpy(), b)
            for (lo, hi), part in zip(windows, parts):
                want = sh.colsum_np(x_h, lo, hi)
                assert np.all(np.abs(part - want) <= max(hi - lo, 1) * 2.0 ** -52 * want), (lo, hi)
            assert np.all(np.abs(sum(parts) - total) <= v * 2.0 ** -52 * total)
            assert np.all(total > 0)
            # doc_scores from the completed state: any shard engine gives the unsharded engine's bits
            scores = dev(rng.standard_normal((b, len(pv))).astype(np.float32), gpu_device)
            mn, mx = st0.row_minmax(scores)
            flags_h = (np.arange(b) % 4 == 1).astype(np.int32)
            sums = dev(total, gpu_device)
            want_doc = st0.doc_scores(x_full, sums, b, scores, mn, mx, dev(flags_h, gpu_device)).cpu().numpy()
            for s in sts:
                got = s.doc_scores(x_sh, sums, b, scores, mn, mx, dev(flags_h, gpu_device)).cpu().numpy()
                np.testing.assert_array_equal(bits(got), bits(want_doc))
        finally:
            for e in shards:
                e.close()


# ----------------------------------------------------------------------------- j. argument checks
def test_stage_argument_checks(gpu_device, graphs):
    import torch
    from hipporag_amd._lib import HRAG_ECAPACITY, HRAG_EINVAL, HragError, check
    from hipporag_amd.engine import EngineStages, _stream
    g = graphs["edge"]
    v, n_p, b = g["csr"].num_vertices, len(g["passage_vertex"]), 6
    rng = np.random.default_rng(0)
    with make_engine(g, 32, 8) as eng:
        st = EngineStages(eng)
        bc, ns = st.layout(b)
        tele = dev(sh.to_slab(sh.random_tele(rng, b, n_p), bc), gpu_device)
        seeds = tuple(dev(a, gpu_device) for a in sh.random_seeds(rng, b, v))
        x = dev(sh.to_slab(sh.random_state(rng, b, v), bc), gpu_device)
        x_before = x.clone()
        y = sentinel((ns, v, bc), gpu_device)
        scores = dev(rng.standard_normal((b, n_p)).astype(np.float32), gpu_device)
        mn, mx = st.row_minmax(scores)
        flags = torch.zeros((b,), dtype=torch.int32, device=gpu_device)
        sums = torch.ones((b,), dtype=torch.float64, device=gpu_device)
        out = sentinel((b, n_p), gpu_device)
        tele_out = sentinel((ns, n_p, bc), gpu_device)
        ws = sentinel((ns * 256 * bc,), gpu_device, torch.float64)
        sums_out = sentinel((b,), gpu_device, torch.float64)

        def refused(status, fn):
            with pytest.raises(HragError) as err:
                fn()
            assert err.value.status == status, err.value
            assert len(str(err.value).split(":", 1)[1].strip()) > 0        # a message comes with the status

        def doc_scores(batch, out_ld):
            return st.lib.hrag_stage_doc_scores(st.h, x.data_ptr(), sums.data_ptr(), batch, scores.data_ptr(), n_p,
                                                mn.data_ptr(), mx.data_ptr(), flags.data_ptr(), out.data_ptr(), out_ld,
                                                _stream())

        def teleport(batch, ld):
            return st.lib.hrag_stage_teleport(st.h, scores.data_ptr(), ld, mn.data_ptr(), mx.data_ptr(), 0.05,
                                              flags.data_ptr(), batch, tele_out.data_ptr(), _stream())

        def colsum(batch):
            return st.lib.hrag_stage_colsum(st.h, x.data_ptr(), batch, ws.data_ptr(), sums_out.data_ptr(), _stream())

        refused(HRAG_EINVAL, lambda: st.ppr_step(tele, seeds, b, 0.5, x, x))                 # x == y
        refused(HRAG_EINVAL, lambda: check(doc_scores(b, n_p - 1)))                           # out_ld < n_passages
        refused(HRAG_EINVAL, lambda: check(teleport(b, n_p - 1)))                             # ld < n_passages
        for batch in (0, eng.max_batch + 1):
            refused(HRAG_ECAPACITY, lambda: st.ppr_init(tele, seeds, batch, y))
            refused(HRAG_ECAPACITY, lambda: st.ppr_step(tele, seeds, batch, 0.5, x, y))
            refused(HRAG_ECAPACITY, lambda: check(colsum(batch)))
            refused(HRAG_ECAPACITY, lambda: check(doc_scores(batch, n_p)))
            refused(HRAG_ECAPACITY, lambda: check(teleport(batch, n_p)))
            refused(HRAG_ECAPACITY, lambda: st.layout(batch))
        assert st.lib.hrag_colsum_workspace_bytes(st.h, 0) == 0
        torch.cuda.synchronize()
        assert torch.equal(x.view(torch.int32), x_before.view(torch.int32))
        for t in (y, out, tele_out):
            assert bool((t.view(torch.int32) == SENTINEL_BITS).all())
        for t in (ws, sums_out):
            assert bool(torch.isnan(t).all())
        assert int(flags.sum()) == 0
        # and the same calls with legal arguments go through
        st.ppr_step(tele, seeds, b, 0.5, x, y)
        check(doc_scores(b, n_p))
        check(teleport(b, n_p))
        check(colsum(b))
        torch.cuda.synchronize()
        assert not bool(torch.isnan(y).any()) and not bool(torch.isnan(out).any())
        assert not bool(torch.isnan(tele_out).any()) and not bool(torch.isnan(sums_out).any())
