"""The fp32 CSR sweep (csrc/ppr_spmm.hip) and the stage operators around it, one call at a time, at every slab width.

What hrag_ppr runs, what hrag_retrieve runs on an HRAG_OPT_F32_STATE engine and what every unconverged query is repeated
on is ppr_spmm_kernel<G> / ppr_spmm_seg_kernel<G> / ppr_spmm_reduce_kernel<G> with G = slab width / 4 in {1, 2, 4, 8, 16};
the end-to-end tests reach G = 8 only, after 20 contracting sweeps, at a 1e-5 bar.  Here every instantiation runs ONE
operator on caller-owned buffers (engine.EngineStages) and is compared with the fp64 restatement of
tests/stage_helpers.py (pinned against the oracle in tests/test_stage_helpers_host.py):

  a. ppr_init: bit for bit (the teleport entry or 0, plus one fp32 add of the seed);
  b. ppr_step from a random state: |y - y64| <= gamma(deg + 5) * mag per entry -- deg FMAs into the accumulator in
     whatever order lanes, segments and the reduce kernel take them, the beta * t product, the final FMA, the seed's
     product and add (Higham's gamma over the fp32 unit roundoff, tests/helpers.py).  Derived, not measured: the
     observed worst err / bound goes to the "csr_sweep" test report (helpers.write_test_report) for the record only.  Rows without
     entries and without a seed are exactly fl32(beta * t); no row keeps the NaN the output was filled with;
  c. NaN in the padding columns (q >= batch) of x changes no valid column of y, of colsum, of doc_scores;
  d. three runs are bit-identical, and so are engines created with HRAG_OPT_NT_CSR, HRAG_OPT_NT_STORE, both, and
     HRAG_OPT_NATURAL_ROW_ORDER (a row's accumulation order does not depend on the wavefront that owns it);
  e. colsum within n_rows * 2^-52 (fp64 accumulation of exact conversions, any order) in a workspace of exactly
     hrag_colsum_workspace_bytes with a guard region behind it;
  f. doc_scores bit for bit, out_ld > n_passages, fallback / zero-mass / normal queries mixed in one batch;
  g. hrag_ppr (dense reset vector: the row_to_tele == NULL branch) for 0, 1 and 7 sweeps under the per-sweep bound
     propagated in numpy.

Graphs: stage_helpers.edge_graph (rows on every short / long / segment threshold, rows without entries, a degree-1
tail) and the 48-hub graph of test_gpu_long_rows.py (multi-segment rows of up to 40 segments at the default
thresholds)."""

import time

import numpy as np
import pytest

from hipporag_amd.graph import build_csr
from tests import stage_helpers as sh
from tests.helpers import U32, gamma, write_test_report

pytestmark = pytest.mark.gpu

WIDTHS = (4, 8, 16, 32, 64)
# one full slab, a partial last slab, more than one slab -- and every batch large enough that auto_slab_width picks
# the engine's own width
BATCHES = {4: (1, 4, 7), 8: (5, 8, 13), 16: (9, 16, 37), 32: (17, 32, 70), 64: (64, 70, 130)}
SEGMENT_NNZ = {4: 64, 8: 64, 16: 128, 32: 128, 64: 128}     # edge graph; the hub graph keeps the default (512)
DAMPINGS = (0.5, 0.85, 0.3)
SENTINEL_BITS = 0x7FC0BEEF                                   # a quiet NaN with a payload
SENTINEL_BITS64 = 0x7FF8BEEF0000ABCD                         # the same as a double
K_COLSUM_BLOCKS = 256                                        # kColsumBlocks, csrc/common.h

_REPORT = {"ratio": {}, "seconds": {}}


def _record(kind, key, ratio, t0):
    _REPORT["ratio"].setdefault(kind, {})
    _REPORT["ratio"][kind][key] = max(_REPORT["ratio"][kind].get(key, 0.0), float(ratio))
    _REPORT["seconds"][f"{kind}:{key}"] = round(_REPORT["seconds"].get(f"{kind}:{key}", 0.0) + time.time() - t0, 2)
    write_test_report("csr_sweep", _REPORT)


def _hub():
    from tests.test_gpu_long_rows import _hub_graph
    n, src, dst, w, pv = _hub_graph()
    rng = np.random.default_rng(41)
    csr = build_csr(n, src, dst, w)
    pv = np.asarray(pv, np.int32)
    r2t = np.full(n, -1, np.int32)
    r2t[pv] = np.arange(len(pv), dtype=np.int32)
    is_p = np.zeros(n, bool)
    is_p[pv] = True
    ents = np.flatnonzero(~is_p)
    subj = ents[rng.integers(0, len(ents), 4000)]
    obj = ents[rng.integers(0, len(ents), 4000)]
    subj[:40] = ents[:40]                                    # the hubs that are not passages
    num_chunks = np.zeros(n, np.int32)
    num_chunks[ents] = rng.integers(0, 4, len(ents))
    assert int((np.diff(csr.row_ptr) > 512).sum()) >= 48
    return dict(csr=csr, passage_vertex=pv, r2t=r2t, subj=subj.astype(np.int32), obj=obj.astype(np.int32),
                num_chunks=num_chunks, seed_pool=np.arange(48))


@pytest.fixture(scope="module")
def graphs():
    return {"edge": sh.edge_graph(), "hub": _hub()}


def make_engine(g, width, max_batch, flags=0, segment_nnz=0, **kw):
    """a scores-only fp32-state engine (no embeddings, no SELL-8 build) on the graph dict g"""
    from hipporag_amd._lib import OPT_F32_STATE
    from hipporag_amd.engine import HippoRAGEngine
    return HippoRAGEngine(g["csr"], g["passage_vertex"], None, None, g["subj"], g["obj"], g["num_chunks"], dim=64,
                          max_batch=max_batch, max_topk=64, slab_width=width, flags=OPT_F32_STATE | flags,
                          segment_nnz=segment_nnz, **kw)


def dev(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def sentinel(shape, device, dtype=None):
    """a buffer of NaNs with a payload (as float32 / float64), so that an unwritten element shows bit for bit"""
    import torch
    if dtype == torch.float64:
        return torch.full(shape, SENTINEL_BITS64, dtype=torch.int64, device=device).view(torch.float64)
    return torch.full(shape, SENTINEL_BITS, dtype=torch.int32, device=device).view(torch.float32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def nan_padded_slab(rows, bc):
    """to_slab with NaN instead of 0 in the padding columns"""
    b, n = rows.shape
    ns = -(-b // bc)
    pad = np.full((ns * bc, n), np.nan, np.float32)
    pad[:b] = rows
    return np.ascontiguousarray(pad.reshape(ns, bc, n).transpose(0, 2, 1))


def row_class(deg, short_thresh, seg_len):
    return ("zero-degree" if deg == 0 else "short" if deg <= short_thresh else "single-segment" if deg <= seg_len
            else "multi-segment")


def assert_within(got, y64, mag, deg, what, short_thresh, seg_len):
    """|got - y64| <= gamma(deg + 5) * mag per entry; -> the worst err / bound"""
    assert not np.isnan(got).any(), f"{what}: {int(np.isnan(got).sum())} entries were not written (or are NaN)"
    bound = gamma(deg + 5)[None, :] * mag
    err = np.abs(got.astype(np.float64) - y64)
    bad = err > bound
    if bad.any():
        q, i = np.argwhere(bad)[0]
        classes = sorted({row_class(int(deg[j]), short_thresh, seg_len) for j in np.unique(np.argwhere(bad)[:, 1])})
        raise AssertionError(f"{what}: {int(bad.sum())} entries in {len(np.unique(np.argwhere(bad)[:, 1]))} rows beyond the "
                             f"bound, row classes {classes}; first: query {q} row {i} (degree {int(deg[i])}) got "
                             f"{got[q, i]!r} want {y64[q, i]!r} err {err[q, i]:.3e} bound {bound[q, i]:.3e}")
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


class Case:
    """random inputs of one batch on one engine, on the host and on the device"""

    def __init__(self, st, g, b, want_layout, rng, device):
        assert st.layout(b) == want_layout, (b, st.layout(b), want_layout)
        self.b, (self.bc, self.ns) = b, want_layout
        csr, pv = g["csr"], g["passage_vertex"]
        self.v, self.n_p = csr.num_vertices, len(pv)
        self.tele32 = sh.random_tele(rng, b, self.n_p)
        self.seeds = sh.random_seeds(rng, b, self.v, g["seed_pool"])
        self.x32 = sh.random_state(rng, b, self.v)
        self.tele_d = dev(sh.to_slab(self.tele32, self.bc), device)
        self.seeds_d = tuple(dev(a, device) for a in self.seeds)
        self.x_d = dev(sh.to_slab(self.x32, self.bc), device)
        self.device = device

    def state(self):
        return sentinel((self.ns, self.v, self.bc), self.device)


def check_init_and_step(st, g, b, want_layout, rng, device, short_thresh, seg_len, dampings=DAMPINGS):
    """(a), (b) and the repeat of (d) for one batch; -> worst err / bound of the steps"""
    import torch
    c = Case(st, g, b, want_layout, rng, device)
    csr, r2t = g["csr"], g["r2t"]
    x0 = c.state()
    st.ppr_init(c.tele_d, c.seeds_d, b, x0)
    torch.cuda.synchronize()
    got0 = sh.from_slab(x0.cpu().numpy(), b)
    want0 = sh.init_np(c.tele32, r2t, c.seeds, c.v)
    np.testing.assert_array_equal(bits(got0), bits(want0), err_msg=f"ppr_init b={b} layout={want_layout}")
    sd = sh.seed_dense(c.seeds, b, c.v)
    t32 = sh._tele_rows(c.tele32, r2t, 0, c.v)
    worst = 0.0
    for damping in dampings:
        what = f"ppr_step b={b} layout={want_layout} damping={damping}"
        y = c.state()
        st.ppr_step(c.tele_d, c.seeds_d, b, damping, c.x_d, y)
        torch.cuda.synchronize()
        y_h = y.cpu().numpy()
        for rep in range(2):
            y2 = c.state()
            st.ppr_step(c.tele_d, c.seeds_d, b, damping, c.x_d, y2)
            torch.cuda.synchronize()
            assert np.array_equal(bits(y2.cpu().numpy()), bits(y_h)), f"{what}: run {rep + 2} differs from run 1"
        got = sh.from_slab(y_h, b)
        y64, mag, deg = sh.step_np(csr, c.x32.astype(np.float64), c.tele32.astype(np.float64), r2t, c.seeds,
                                   np.float32(damping))
        worst = max(worst, assert_within(got, y64, mag, deg, what, short_thresh, seg_len))
        # rows without entries and without a seed: fmaf(alpha, 0, beta * t) = fl32(beta * t) exactly
        beta = np.float32(np.float32(1) - np.float32(damping))
        plain = (deg == 0)[None, :] & (sd == 0)
        assert plain.sum() >= b or not (deg == 0).any()           # (the hub graph has no row without entries)
        np.testing.assert_array_equal(bits(got[plain]), bits((beta * t32).astype(np.float32)[plain]), err_msg=what)
    return worst


# ----------------------------------------------------------------------------- a, b, d (repeat)
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("graph", ["edge", "hub"])
def test_init_and_one_sweep_match_fp64_at_every_width(gpu_device, graphs, graph, width):
    from hipporag_amd.engine import EngineStages
    t0 = time.time()
    g = graphs[graph]
    seg = SEGMENT_NNZ[width] if graph == "edge" else 0
    rng = np.random.default_rng(100 * width + len(graph))
    worst = 0.0
    with make_engine(g, width, max(BATCHES[width]), segment_nnz=seg) as eng:
        st = EngineStages(eng)
        for b in BATCHES[width]:
            worst = max(worst, check_init_and_step(st, g, b, (width, -(-b // width)), rng, gpu_device, 2 * width,
                                                   seg or 512, DAMPINGS if graph == "edge" else (0.5, 0.85)))
    _record("step_" + graph, str(width), worst, t0)


@pytest.mark.parametrize("b,bc", [(1, 4), (3, 4), (6, 8), (12, 16), (20, 32)])
def test_small_batches_on_a_wide_engine_take_the_narrower_kernels(gpu_device, graphs, b, bc):
    """auto_slab_width: a width-64 engine (short-row threshold 128, 128-entry segments) runs a batch of b queries on the
    narrowest kernel that holds it -- G = 1 lanes then walk rows of up to 128 entries"""
    from hipporag_amd.engine import EngineStages
    t0 = time.time()
    g = graphs["edge"]
    rng = np.random.default_rng(b)
    with make_engine(g, 64, 32, segment_nnz=128) as eng:
        worst = check_init_and_step(EngineStages(eng), g, b, (bc, 1), rng, gpu_device, 128, 128)
    _record("step_auto_width", f"{bc} (b={b})", worst, t0)


# ----------------------------------------------------------------------------- c. padding
@pytest.mark.parametrize("width", WIDTHS)
def test_nan_in_the_padding_columns_cannot_leak(gpu_device, graphs, width):
    import torch
    from hipporag_amd.engine import EngineStages
    g = graphs["edge"]
    b = BATCHES[width][2]
    ns = -(-b // width)
    assert ns * width > b
    rng = np.random.default_rng(width)
    with make_engine(g, width, b, segment_nnz=SEGMENT_NNZ[width]) as eng:
        st = EngineStages(eng)
        c = Case(st, g, b, (width, ns), rng, gpu_device)
        x_nan = dev(nan_padded_slab(c.x32, width), gpu_device)
        assert int(torch.isnan(x_nan).sum()) == (ns * width - b) * c.v
        scores = dev(rng.standard_normal((b, c.n_p)).astype(np.float32), gpu_device)
        mn, mx = st.row_minmax(scores)
        flags_h = (np.arange(b) % 3 == 1).astype(np.int32)
        outs = []
        for x in (c.x_d, x_nan):
            y = c.state()
            st.ppr_step(c.tele_d, c.seeds_d, b, 0.5, x, y)
            sums = st.colsum(x, b)
            flags = dev(flags_h, gpu_device)
            doc = st.doc_scores(x, sums, b, scores, mn, mx, flags)
            torch.cuda.synchronize()
            outs.append((sh.from_slab(y.cpu().numpy(), b), sums.cpu().numpy(), doc.cpu().numpy(), flags.cpu().numpy()))
    for a, bb, what in zip(outs[0], outs[1], ("y", "colsum", "doc_scores", "flags")):
        assert not np.isnan(a.astype(np.float64)).any(), what
        np.testing.assert_array_equal(bits(a) if a.dtype.kind == "f" else a, bits(bb) if bb.dtype.kind == "f" else bb,
                                      err_msg=what)


# ----------------------------------------------------------------------------- d. option flags
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("graph", ["edge", "hub"])
def test_option_flags_change_no_bit(gpu_device, graphs, graph, width):
    """HRAG_OPT_NT_CSR / NT_STORE are cache hints; HRAG_OPT_NATURAL_ROW_ORDER only changes which wavefront owns a short
    row, and a row's entries are walked by its own G lanes in the same order wherever it sits"""
    import torch
    from hipporag_amd._lib import OPT_NATURAL_ROW_ORDER, OPT_NT_CSR, OPT_NT_STORE
    from hipporag_amd.engine import EngineStages
    g = graphs[graph]
    seg = SEGMENT_NNZ[width] if graph == "edge" else 0
    b = BATCHES[width][1 if graph == "hub" else 2]
    lay = (width, -(-b // width))
    results = {}
    for name, flags in (("plain", 0), ("nt_csr", OPT_NT_CSR), ("nt_store", OPT_NT_STORE),
                        ("nt_both", OPT_NT_CSR | OPT_NT_STORE), ("natural_order", OPT_NATURAL_ROW_ORDER)):
        rng = np.random.default_rng(width)                    # the same inputs on every engine
        with make_engine(g, width, b, flags=flags, segment_nnz=seg) as eng:
            st = EngineStages(eng)
            c = Case(st, g, b, lay, rng, gpu_device)
            x0, y = c.state(), c.state()
            st.ppr_init(c.tele_d, c.seeds_d, b, x0)
            st.ppr_step(c.tele_d, c.seeds_d, b, 0.85, c.x_d, y)
            torch.cuda.synchronize()
            results[name] = (x0.cpu().numpy(), y.cpu().numpy())
    for name, (x0, y) in results.items():
        assert np.array_equal(bits(x0), bits(results["plain"][0])), f"ppr_init, {name}"
        same = bits(y) == bits(results["plain"][1])
        assert same.all(), f"ppr_step, {name}: {int((~same).sum())} elements differ from the plain engine"


# ----------------------------------------------------------------------------- e, f. colsum and doc_scores
@pytest.mark.parametrize("width", WIDTHS)
def test_colsum_and_doc_scores(gpu_device, graphs, width):
    import torch
    from hipporag_amd._lib import check
    from hipporag_amd.engine import EngineStages, _stream
    t0 = time.time()
    g = graphs["edge"]
    pv = g["passage_vertex"]
    rng = np.random.default_rng(7 * width)
    worst = 0.0
    with make_engine(g, width, max(BATCHES[width]), segment_nnz=SEGMENT_NNZ[width]) as eng:
        st = EngineStages(eng)
        for b in BATCHES[width]:
            c = Case(st, g, b, (width, -(-b // width)), rng, gpu_device)
            what = f"b={b} width={width}"
            # roles by query: 0 / 4 normal, 1 fallback, 2 zero mass, 3 fallback with equal scores and zero mass
            role = np.arange(b) % 5
            x32 = c.x32.copy()
            x32[(role == 2) | (role == 3)] = 0
            x_d = dev(sh.to_slab(x32, width), gpu_device)
            # e. workspace of exactly the reported size, a guard behind it
            nbytes = int(st.lib.hrag_colsum_workspace_bytes(st.h, b))
            assert nbytes == c.ns * K_COLSUM_BLOCKS * width * 8, what
            guard = 4096
            ws = sentinel((nbytes // 8 + guard,), gpu_device, torch.float64)
            sums = sentinel((b + 8,), gpu_device, torch.float64)
            guard_before = bits(ws[nbytes // 8:].cpu().numpy()).copy()
            check(st.lib.hrag_stage_colsum(st.h, x_d.data_ptr(), b, ws.data_ptr(), sums.data_ptr(), _stream()))
            torch.cuda.synchronize()
            assert np.array_equal(bits(ws[nbytes // 8:].cpu().numpy()), guard_before), f"colsum wrote past its workspace, {what}"
            assert not torch.isnan(ws[:nbytes // 8]).any(), f"colsum left part of its workspace unwritten, {what}"
            sums_h = sums.cpu().numpy()
            assert np.all(bits(sums_h[b:]) == SENTINEL_BITS64), what
            want = sh.colsum_np(x32)
            tol = c.v * 2.0 ** -52 * want
            assert np.all(np.abs(sums_h[:b] - want) <= tol), (what, sums_h[:b], want)
            assert np.all(sums_h[:b][(role == 2) | (role == 3)] == 0)
            worst = max(worst, float((np.abs(sums_h[:b] - want)[want > 0] / tol[want > 0]).max()))
            # f. doc_scores from the device's own sums
            n_p, out_ld = c.n_p, c.n_p + 5
            scores = rng.standard_normal((b, n_p + 3)).astype(np.float32)
            scores[role == 3] = np.float32(0.625)
            mn, mx = scores[:, :n_p].min(axis=1), scores[:, :n_p].max(axis=1)
            flags_h = (np.where((role == 1) | (role == 3), 1, 0) | np.where(np.arange(b) % 2 == 0, 4, 0)).astype(np.int32)
            flags = dev(flags_h, gpu_device)
            out = sentinel((b, out_ld), gpu_device)
            sums_b = sums[:b].contiguous()
            scores_d, mn_d, mx_d = dev(scores, gpu_device), dev(mn, gpu_device), dev(mx, gpu_device)
            check(st.lib.hrag_stage_doc_scores(st.h, x_d.data_ptr(), sums_b.data_ptr(), b, scores_d.data_ptr(),
                                               scores.shape[1], mn_d.data_ptr(), mx_d.data_ptr(), flags.data_ptr(),
                                               out.data_ptr(), out_ld, _stream()))
            torch.cuda.synchronize()
            out_h = out.cpu().numpy()
            want_out, want_flags = sh.doc_scores_np(x32, sums_h[:b], pv, flags_h, scores, mn, mx)
            np.testing.assert_array_equal(bits(out_h[:, :n_p]), bits(want_out), err_msg=f"doc_scores {what}")
            assert np.all(bits(out_h[:, n_p:]) == SENTINEL_BITS), f"doc_scores wrote past n_passages, {what}"
            np.testing.assert_array_equal(flags.cpu().numpy(), want_flags, err_msg=f"flags {what}")
            assert np.all(want_flags[role == 2] & 2) and not np.any(want_flags[role != 2] & 2)
            assert np.all(out_h[:, :n_p][role == 3] == 1) and np.all(out_h[:, :n_p][role == 2] == 0)
    _record("colsum", str(width), worst, t0)


# ----------------------------------------------------------------------------- g. hrag_ppr
def ppr_reference(csr, reset32, damping, iters):
    """iters sweeps of step_np from the sanitised dense reset vector, with the bound of every sweep carried along:
        E_k = a P E_(k-1) + gamma(deg + 5) * (mag_k + a P E_(k-1))
    (the device's iterate is within E_(k-1) of the fp64 one, so its own sweep's magnitudes are within a P E_(k-1) of
    mag_k), then the normalisation x / sum(x) in fp64 rounded once to fp32:
        |x_dev / S_dev - x / S| <= E / (S - dS) + x dS / (S (S - dS)) + U32 x / S,  dS = sum(E) + V 2^-52 S
    -> (want [B, V], bound [B, V], zero-mass rows)"""
    r = np.where(np.isnan(reset32) | (reset32 < 0), np.float32(0), reset32).astype(np.float64)
    p = sh.csr_matrix64(csr)
    a = float(np.float32(damping))
    x, err = r.copy(), np.zeros_like(r)
    for _ in range(iters):
        pe = a * (p @ err.T).T
        y, mag, deg = sh.step_np(csr, x, r, None, None, np.float32(damping))
        err = pe + gamma(deg + 5)[None, :] * (mag + pe)
        x = y
    s = x.sum(axis=1)
    zero = ~(s > 0)
    s1 = np.where(zero, 1.0, s)
    ds = err.sum(axis=1) + csr.num_vertices * 2.0 ** -52 * s1
    want = x / s1[:, None]
    bound = (err / (s1 - ds)[:, None] + x * (ds / (s1 * (s1 - ds)))[:, None] + U32 * want)
    want[zero], bound[zero] = 0, 0
    return want, bound, zero


def dense_resets(rng, g, b):
    """reset vectors as the pipeline forms them (a prior on the passages, a few seeds) with NaN and negative entries
    sprinkled in, an all-zero row and a row without a positive entry"""
    v = g["csr"].num_vertices
    r = np.zeros((b, v), np.float32)
    r[:, g["passage_vertex"]] = sh.random_tele(rng, b, len(g["passage_vertex"]))
    r += sh.seed_dense(sh.random_seeds(rng, b, v, g["seed_pool"]), b, v)
    r[rng.random((b, v)) < 0.01] = np.nan
    r[rng.random((b, v)) < 0.01] *= -1
    if b >= 3:
        r[1] = 0
        r[2] = -np.abs(r[2])
        r[2, ::7] = np.nan
    return r


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("graph", ["edge", "hub"])
def test_hrag_ppr_dense_reset(gpu_device, graphs, graph, width):
    """Batches <= 8 included: an HRAG_OPT_F32_STATE engine has no small-batch kernels (hrag_engine_stats.ppr_states is
    the fp32 state alone), so hrag_ppr -- which leaves no timings behind -- runs the CSR sweep at every batch size."""
    import torch
    from hipporag_amd._lib import PPR_STATE_F32
    t0 = time.time()
    g = graphs[graph]
    csr = g["csr"]
    v = csr.num_vertices
    seg = SEGMENT_NNZ[width] if graph == "edge" else 0
    rng = np.random.default_rng(width + 1000)
    worst = 0.0
    batches = BATCHES[width] if graph == "edge" else BATCHES[width][1:2]
    dampings = DAMPINGS if graph == "edge" else (0.85,)
    with make_engine(g, width, max(batches), segment_nnz=seg) as eng:
        assert eng.stats()["ppr_states"] == PPR_STATE_F32
        for b in batches:
            assert eng.layout(b) == (width, -(-b // width))
            reset = dense_resets(rng, g, b)
            reset_d = dev(reset, gpu_device)
            for damping in dampings:
                for iters in (0, 1, 7):
                    what = f"hrag_ppr {graph} width={width} b={b} damping={damping} iters={iters}"
                    x, flags = eng.ppr(reset_d, damping=damping, iters=iters)
                    torch.cuda.synchronize()
                    got, flags = x.cpu().numpy(), flags.cpu().numpy()
                    want, bound, zero = ppr_reference(csr, reset, damping, iters)
                    assert not np.isnan(got).any(), what
                    err = np.abs(got.astype(np.float64) - want)
                    bad = err > bound
                    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[0], float(err[bad].max()))
                    pos = bound > 0
                    worst = max(worst, float((err[pos] / bound[pos]).max()))
                    np.testing.assert_array_equal(flags, np.where(zero, 2, 0), err_msg=what)
                    assert np.all(got[zero] == 0), what
                    total = got[~zero].astype(np.float64).sum(axis=1)
                    assert np.all(np.abs(total - 1) <= v * 2.0 ** -23), (what, total)
                    if b >= 3:
                        assert zero[1] and zero[2] and not zero[0]
    _record("hrag_ppr_" + graph, str(width), worst, t0)
