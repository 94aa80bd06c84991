"""Facets on the device (include/hrag.h, "facets"; csrc/facet.hip): hrag_payload_facet and hrag_payload_facet_ids held count
for count to the numpy restatement of tests/facet_helpers.py, the host validation, the engine's and the mirror's calls.
Equality is exact and integer: there is no tolerance in this file."""

import ctypes as C
import time

import numpy as np
import pytest

from hipporag_amd import synth
from hipporag_amd._lib import FACET_MAX_BINS, PAY_TILE
from hipporag_amd.engine import pack_mask
from oracle.checks import make_case
from tests.facet_helpers import (GONE_COL, SKEW_CODE, SKEW_COL, WINDOW, Spec, codes, edges_i64, facet_bins_np,
                                 facet_columns, facet_counts_np, facet_ids_np, random_spec, special_specs)
from tests.payload_helpers import cols_for_restatement, payload_filter_np

pytestmark = pytest.mark.gpu

T = PAY_TILE
SIZES = [1, 31, 32, 33, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]          # the payload suite's
GUARD = np.int32(-0x5A5A5A5B)
PAD = 3


def _L():
    from hipporag_amd import _lib
    return _lib, _lib.load()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _np(t):
    return t.cpu().numpy()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _index(cols):
    from hipporag_amd.payload import PayloadColumns, PayloadIndex
    pc = PayloadColumns(len(cols[0][1]))
    for i, (typ, values, present) in enumerate(cols):
        pc._add(f"c{i}", typ, values, present)
    return PayloadIndex(pc)


def _desc(spec):
    """(hrag_facet_spec, the tensor that keeps its edges alive)"""
    L, _ = _L()
    e = _dev(spec.edges) if spec.edges is not None and len(spec.edges) else None
    return L.FacetSpecDesc(spec.col, spec.kind, spec.n_bins, spec.lo, e.data_ptr() if e is not None else None,
                           0 if spec.edges is None else len(spec.edges)), e


def _splits(ix, n_bins, b):
    from hipporag_amd.facet import facet_splits
    return facet_splits(ix, n_bins, b)


def _facet(ix, spec, b, words=None, ld_w=0):
    """hrag_payload_facet into a guard-filled [b, n_bins + 2 + PAD] buffer -> int32 [b, n_bins + 2 + PAD]"""
    import torch
    L, lib = _L()
    d, keep = _desc(spec)
    out = _dev(np.full((b, spec.n_bins + 2 + PAD), GUARD, np.int32))
    need = C.c_int64(-1)
    L.check(lib.hrag_payload_facet_ws_bytes(ix._handle, spec.n_bins, b, C.byref(need)))
    ws = torch.full((need.value // 4 + 1,), 0x7F7F7F7F, dtype=torch.int32, device="cuda")      # junk: the call needs no memset
    L.check(lib.hrag_payload_facet(ix._handle, C.byref(d), words.data_ptr() if words is not None else None, ld_w, b,
                                   out.data_ptr(), spec.n_bins + 2 + PAD, ws.data_ptr(), need.value, _stream()))
    torch.cuda.synchronize()
    return _np(out)


def _facet_ids(ix, spec, ids):
    import torch
    L, lib = _L()
    d, keep = _desc(spec)
    b, k = ids.shape
    out = _dev(np.full((b, spec.n_bins + 2 + PAD), GUARD, np.int32))
    di = _dev(np.concatenate([ids, np.full((b, 2), 0, np.int32)], axis=1))                     # ld_i > k: the tail is not read
    L.check(lib.hrag_payload_facet_ids(ix._handle, C.byref(d), di.data_ptr(), k + 2, k, b, out.data_ptr(),
                                       spec.n_bins + 2 + PAD, _stream()))
    torch.cuda.synchronize()
    return _np(out)


def _count_rows(words, ld, n, b):
    import torch
    L, lib = _L()
    cnt = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    L.check(lib.hrag_bitset_count_rows(words.data_ptr(), ld, n, b, cnt.data_ptr(), _stream()))
    return _np(cnt)


def _word_forms(rng, n, b):
    """(name, allowed bool [b, n], device words or None, ld_w): NULL, one broadcast row, and per-query rows with a stride
    of their own, junk words behind W and junk bits above n in the last word."""
    w = (n + 31) // 32
    rows = rng.random((b, n)) < 0.7
    yield "NULL", np.ones((b, n), bool), None, 0
    one = pack_mask(rows[0])
    yield "broadcast", np.repeat(rows[:1], b, axis=0), _dev(one), 0
    per = np.concatenate([pack_mask(rows), rng.integers(0, 2 ** 32, (b, 2), dtype=np.uint32)], axis=1)
    if n % 32:
        per[:, w - 1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)                      # every bit above n set
    yield "per query", rows, _dev(per), w + 2


def _check(got, want, spec, what):
    nb = spec.n_bins
    assert (got[:, nb + 2:] == GUARD).all(), f"{what}: the entries beyond n_bins + 2 are not touched"
    np.testing.assert_array_equal(got[:, :nb + 2], want, err_msg=what)


@pytest.fixture(scope="module")
def indexes(gpu_device):
    """One index per passage count, with its host columns: built once, shared by the batch sizes."""
    made = {}
    for n in SIZES + [16 * T]:
        cols = facet_columns(np.random.default_rng(n), n)
        made[n] = (cols, _index(cols))
    yield made
    for _, ix in made.values():
        ix.close()


# ---------------------------------------------------------------------------------- hrag_payload_facet
@pytest.mark.parametrize("b", [1, 3, 65])
@pytest.mark.parametrize("n", SIZES)
def test_facet_matches_the_restatement_count_for_count(indexes, n, b):
    """Every special spec of facet_helpers (1 bin, lo at the int64 extremes, no edges, equal and infinite edges, n_bins at
    WINDOW - 1 / WINDOW / WINDOW + 1 / 2 WINDOW + 5, edge lists at the LDS cap and one above, the skewed and the all-missing
    column) and random ones, each under NULL
    words, a broadcast row and per-query rows; columns with and without presence words; into rows wider than n_bins + 2."""
    cols, ix = indexes[n]
    rng = np.random.default_rng(1000 * b + n)
    forms = list(_word_forms(rng, n, b))
    sums = [np.full(b, n, np.int32) if w is None else _count_rows(w, ld, n, b) for _, _, w, ld in forms]
    for (_, allowed, _, _), s in zip(forms, sums):
        np.testing.assert_array_equal(s, allowed.sum(1))
    specs = list(special_specs().items()) + [(f"random {i}", random_spec(rng)) for i in range(6)]
    for name, spec in specs:
        bins = facet_bins_np(n, cols, spec)                      # the reference: once per spec, shared by the word forms
        for (form, allowed, words, ld), s in zip(forms, sums):
            got = _facet(ix, spec, b, words, ld)
            what = f"n={n} b={b} spec={name} words={form} splits={_splits(ix, spec.n_bins, b)}"
            _check(got, facet_counts_np(n, cols, spec, allowed, bins), spec, what)
            np.testing.assert_array_equal(got[:, :spec.n_bins + 2].sum(1), s, err_msg=what)      # hrag_bitset_count_rows


def test_a_split_launch_gives_the_one_split_counts(indexes):
    """The split count is a pure function of (n_passages, n_bins, batch), read off hrag_payload_facet_ws_bytes
    (facet.facet_splits): at 16 T passages a single query is split 16 ways -- one tile each --, 256 queries 4 ways and 1024
    queries not at all.  The same words counted each way give the same rows."""
    n = 16 * T
    cols, ix = indexes[n]
    rng = np.random.default_rng(99)
    allowed = rng.random(n) < 0.5
    words = _dev(pack_mask(allowed))
    for name in ("skewed", "WINDOW + 1", "12 edges", "all missing", "2 * WINDOW + 5"):
        spec = special_specs()[name]
        assert _splits(ix, spec.n_bins, 1) == 16 and _splits(ix, spec.n_bins, 1024) == 1, name
        assert _splits(ix, spec.n_bins, 256) == (4 if spec.n_bins <= WINDOW else 2), name
        want = facet_counts_np(n, cols, spec, allowed)
        for b in (1, 256, 1024):
            got = _facet(ix, spec, b, words, 0)
            _check(got, np.repeat(want, b, axis=0), spec, f"{name} b={b} splits={_splits(ix, spec.n_bins, b)}")
    L, lib = _L()
    need = C.c_int64(-1)
    L.check(lib.hrag_payload_facet_ws_bytes(ix._handle, 300, 1, C.byref(need)))
    assert need.value == 4 * 1 * 16 * 302
    L.check(lib.hrag_payload_facet_ws_bytes(ix._handle, 300, 256, C.byref(need)))
    assert need.value == 4 * 256 * 4 * 302
    L.check(lib.hrag_payload_facet_ws_bytes(ix._handle, 300, 1024, C.byref(need)))
    assert need.value == 0


@pytest.mark.parametrize("n", [T + 1, 3 * T + 17])
def test_the_skewed_and_the_all_missing_column(indexes, n):
    """One code holds a third of the passages (the ballot step of facet.hip counts its lanes in a register), and a column no
    passage has a value in (every lane lands on "missing")."""
    cols, ix = indexes[n]
    rng = np.random.default_rng(n)
    for b in (1, 65):
        forms = list(_word_forms(rng, n, b))
        for name in ("skewed", "all missing", "all missing, edges"):
            spec = special_specs()[name]
            for form, allowed, words, ld in forms:
                want = facet_counts_np(n, cols, spec, allowed)
                _check(_facet(ix, spec, b, words, ld), want, spec, f"n={n} b={b} {name} {form}")
                if name == "skewed" and form == "NULL":
                    assert want[0, SKEW_CODE] > n // 4 and want[0, SKEW_CODE] == want[0, :-2].max()
                if spec.col == GONE_COL:
                    assert (want[:, :-1] == 0).all() and (want[:, -1] == allowed.sum(1)).all()
    # the hot code on the second window, and a hot "other"
    for spec in (codes(SKEW_COL, SKEW_CODE - WINDOW - 3, 2 * WINDOW), codes(SKEW_COL, SKEW_CODE + 1, 5)):
        _check(_facet(ix, spec, 3), facet_counts_np(n, cols, spec, np.ones((3, n), bool)), spec, str(spec))


# ---------------------------------------------------------------------------------- hrag_payload_facet_ids
@pytest.mark.parametrize("k", [1, 64, 65, 200, 2049])
def test_facet_ids_matches_the_restatement_and_the_words_form(indexes, k):
    n = 3 * T + 17
    cols, ix = indexes[n]
    rng = np.random.default_rng(k)
    b = 5
    ids = rng.integers(0, n, (b, k)).astype(np.int32)
    ids[rng.random((b, k)) < 0.15] = -1                                        # the padding
    ids[rng.random((b, k)) < 0.05] = n                                         # out of range, both ways
    ids[rng.random((b, k)) < 0.05] = -7
    ids[rng.random((b, k)) < 0.02] = np.iinfo(np.int32).max
    ids[0] = ids[0, 0]                                                         # one id repeated k times
    ids[1, : k // 2] = ids[1, k - k // 2:]                                     # repeats
    ids[2] = -1                                                                # nothing to count
    distinct = np.zeros((b, n), bool)
    for q in range(b):
        r = ids[q][(ids[q] >= 0) & (ids[q] < n)]
        distinct[q, r] = True
    uniq = np.full((b, k), -1, np.int32)                                       # rows without repeats, for the words form
    for q in range(b):
        r = np.flatnonzero(distinct[q])[:k]
        uniq[q, : len(r)] = rng.permutation(r)
    words = _dev(pack_mask(distinct))
    w = (n + 31) // 32
    for name in ("1000 codes", "skewed", "lo = INT64_MAX", "equal neighbouring edges", "edges at the infinities",
                 "i64 edges at the extremes", "all missing", "WINDOW + 1", "2 * WINDOW + 5", "m = 0"):
        spec = special_specs()[name]
        bins = facet_bins_np(n, cols, spec)
        want = facet_ids_np(n, cols, spec, ids, bins)
        _check(_facet_ids(ix, spec, ids), want, spec, f"k={k} {name}")
        assert (want.sum(1) == ((ids >= 0) & (ids < n)).sum(1)).all() and want[2].sum() == 0
        # distinct ids: the ids form equals the words form under a mask of exactly those ids
        by_ids = _facet_ids(ix, spec, uniq)
        by_words = _facet(ix, spec, b, words, w)
        _check(by_ids, by_words[:, :spec.n_bins + 2], spec, f"k={k} {name}: ids against words")
        _check(by_words, facet_counts_np(n, cols, spec, distinct, bins), spec, f"k={k} {name}: words")


# ---------------------------------------------------------------------------------- the host checks
def test_every_host_rejection_names_its_argument(indexes):
    import torch
    from hipporag_amd._lib import HRAG_EINVAL
    L, lib = _L()
    n = 65
    cols, ix = indexes[n]
    w = (n + 31) // 32
    edges = _dev(np.arange(4, dtype=np.int64))
    out = torch.zeros((2, 16), dtype=torch.int32, device="cuda")
    words = torch.zeros((2, w + 1), dtype=torch.int32, device="cuda")
    ids = torch.zeros((2, 8), dtype=torch.int32, device="cuda")
    ws = torch.zeros((64,), dtype=torch.int32, device="cuda")

    def spec(column=2, kind=0, n_bins=10, lo=0, e=None, m=0):
        return L.FacetSpecDesc(column, kind, n_bins, lo, e, m)

    def call(handle=ix._handle, s=spec(), wd=words.data_ptr(), ld_w=w + 1, batch=2, o=out.data_ptr(), ld_c=16, wsp=ws.data_ptr(),
             ws_bytes=256):
        return lib.hrag_payload_facet(handle, C.byref(s) if s is not None else None, wd, ld_w, batch, o, ld_c, wsp, ws_bytes,
                                      _stream())

    def call_ids(handle=ix._handle, s=spec(), i=ids.data_ptr(), ld_i=8, k=8, batch=2, o=out.data_ptr(), ld_c=16):
        return lib.hrag_payload_facet_ids(handle, C.byref(s) if s is not None else None, i, ld_i, k, batch, o, ld_c, _stream())
    e5 = spec(kind=1, n_bins=5, e=edges.data_ptr(), m=4)
    assert call() == 0 and call(ld_w=0) == 0 and call(wd=None) == 0 and call(s=e5) == 0 and call(ld_c=12) == 0
    assert call(s=spec(column=1, kind=1, n_bins=1)) == 0 and call(wsp=None, ws_bytes=0) == 0       # m = 0; one split: no workspace
    assert call_ids() == 0 and call_ids(s=e5, k=1) == 0 and call_ids(ld_i=9) == 0
    bad = {
        "a NULL handle": (dict(handle=None), "payload index"), "a NULL spec": (dict(s=None), "spec"),
        "a NULL output": (dict(o=None), "counts_out_dev"), "batch 0": (dict(batch=0), "batch"),
        "batch 65536": (dict(batch=65536), "batch"), "a negative column": (dict(s=spec(column=-1)), "spec.column"),
        "a column outside the index": (dict(s=spec(column=len(cols))), "spec.column"),
        "an unknown kind": (dict(s=spec(kind=2)), "spec.kind"), "a negative kind": (dict(s=spec(kind=-1)), "spec.kind"),
        "CODES on an F64 column": (dict(s=spec(column=1)), "F64 column"),
        "n_bins 0": (dict(s=spec(n_bins=0)), "spec.n_bins"),
        "n_bins above the cap": (dict(s=spec(n_bins=FACET_MAX_BINS + 1), ld_c=FACET_MAX_BINS + 3), "spec.n_bins"),
        "EDGES with n_bins != m + 1": (dict(s=spec(kind=1, n_bins=4, e=edges.data_ptr(), m=4)), "spec.n_edges"),
        "EDGES with a negative m": (dict(s=spec(kind=1, n_bins=1, e=edges.data_ptr(), m=-1)), "spec.n_edges"),
        "EDGES without edges": (dict(s=spec(kind=1, n_bins=5, e=None, m=4)), "spec.edges_dev"),
        "unaligned edges": (dict(s=spec(kind=1, n_bins=4, e=edges.data_ptr() + 4, m=3)), "spec.edges_dev"),
        "ld_c too small": (dict(ld_c=11), "ld_c"), "an unaligned output": (dict(o=out.data_ptr() + 2), "counts_out_dev"),
    }
    only_words = {
        "ld_w below W": (dict(ld_w=w - 1), "ld_w"), "a negative ld_w": (dict(ld_w=-1), "ld_w"),
        "unaligned words": (dict(wd=words.data_ptr() + 1), "words_dev"),
    }
    only_ids = {
        "NULL ids": (dict(i=None), "idx_dev"), "k 0": (dict(k=0), "k="), "a negative k": (dict(k=-3), "k="),
        "ld_i below k": (dict(ld_i=7), "ld_i"), "unaligned ids": (dict(i=ids.data_ptr() + 2), "idx_dev"),
    }
    for fn, table in ((call, {**bad, **only_words}), (call_ids, {**bad, **only_ids})):
        for what, (kw, names) in table.items():
            assert fn(**kw) == HRAG_EINVAL, what
            assert names in lib.hrag_last_error().decode(), (what, lib.hrag_last_error())
    # the workspace: a launch that splits needs what the query call returns
    big_cols, big = indexes[3 * T + 17]
    need = C.c_int64(-1)
    L.check(lib.hrag_payload_facet_ws_bytes(big._handle, 10, 2, C.byref(need)))
    assert need.value == 4 * 2 * 4 * 12 and _splits(big, 10, 2) == 4
    buf = torch.zeros((need.value // 4,), dtype=torch.int32, device="cuda")
    assert call(handle=big._handle, wd=None, wsp=buf.data_ptr(), ws_bytes=need.value) == 0
    for what, kw, names in (("ws_bytes too small", dict(wsp=buf.data_ptr(), ws_bytes=need.value - 1), "ws_bytes"),
                            ("a NULL workspace", dict(wsp=None, ws_bytes=need.value), "ws_dev"),
                            ("an unaligned workspace", dict(wsp=buf.data_ptr() + 1, ws_bytes=need.value), "ws_dev")):
        assert call(handle=big._handle, wd=None, **kw) == HRAG_EINVAL, what
        assert names in lib.hrag_last_error().decode(), (what, lib.hrag_last_error())
    for what, args, names in (("a NULL handle", (None, 10, 2, C.byref(need)), "payload index"), ("a NULL out", (ix._handle, 10, 2, None), "out"),
                              ("n_bins 0", (ix._handle, 0, 2, C.byref(need)), "n_bins"),
                              ("n_bins above the cap", (ix._handle, FACET_MAX_BINS + 1, 2, C.byref(need)), "n_bins"),
                              ("batch 0", (ix._handle, 10, 0, C.byref(need)), "batch")):
        assert lib.hrag_payload_facet_ws_bytes(*args) == HRAG_EINVAL, what
        assert names in lib.hrag_last_error().decode(), (what, lib.hrag_last_error())
    torch.cuda.synchronize()
    # the Python side
    from hipporag_amd.facet import compile_facet
    from hipporag_amd.payload import PayloadIndex
    small = PayloadIndex.from_columns({"a": [1, 2, None], "s": ["x", None, "x"]}, 3)
    sp = compile_facet(small, "s")
    with pytest.raises(ValueError, match="another index"):
        ix.facet(sp)
    with pytest.raises(TypeError, match="FacetSpec"):
        small.facet("s")
    with pytest.raises(ValueError, match="words or ids, not both"):
        small.facet(sp, torch.ones(3, dtype=torch.bool), ids=torch.zeros((1, 2), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="ids: an int32 device tensor"):
        small.facet(sp, ids=torch.zeros((1, 2), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="out"):
        small.facet(sp, out=torch.zeros((1, 2), dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError, match="words"):
        small.facet(sp, {"a": 1})
    fc = small.facet(sp)
    assert _np(fc.counts).tolist() == [[2]] and _np(fc.other).tolist() == [0] and _np(fc.missing).tolist() == [1]
    assert fc.top() == [[("x", 2)]] and fc.labels == ["x"]
    mine = torch.full((2, 5), 9, dtype=torch.int32, device="cuda")
    fc = small.facet(compile_facet(small, "a", lo=2, n_values=1), torch.tensor([[True, True, False], [False, True, True]]), out=mine)
    assert _np(mine).tolist() == [[1, 1, 0, 9, 9], [1, 0, 1, 9, 9]] and fc.raw.data_ptr() == mine.data_ptr()
    assert _np(small.facet(sp, ids=torch.tensor([[2, 2, -1, 3, 1]], dtype=torch.int32, device="cuda")).raw).tolist() == [[2, 0, 1]]
    small.close()
    with pytest.raises(ValueError, match="closed"):
        small.facet(sp)


# ---------------------------------------------------------------------------------- the engine
def test_the_engine_counts_under_a_payload_filter_and_over_retrieved_ids(gpu_device):
    import torch
    from hipporag_amd.engine import HippoRAGEngine, compile_facet
    from hipporag_amd.payload import PayloadIndex, compile_filters, encode_columns
    kg, pass_bits, fact_bits, _ = make_case(3000, 24000, 64, seed=4141)
    n_p = kg.n_passages
    rng = np.random.default_rng(5)
    columns = {"source": [None if rng.random() < 0.2 else f"s{int(rng.integers(0, 40))}" for _ in range(n_p)],
               "year": [None if rng.random() < 0.1 else int(rng.integers(2000, 2024)) for _ in range(n_p)],
               "score": rng.standard_normal(n_p)}
    host = encode_columns(columns, n_p)
    cols = cols_for_restatement(host)
    eng = HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                         max_batch=16, max_topk=min(200, n_p))
    ix = PayloadIndex(host)
    ws = None
    try:
        with pytest.raises(ValueError, match="facet needs a payload index"):
            eng.facet("source")
        eng.set_payload_index(ix)
        ws = eng.workspace()
        filters = [{"year": {"$gte": 2015}}, {"source": ["s3", "s7"]}, None, {"score": {"$lt": -5.0}}, {"$not": {"year": 2020}}]
        pf = compile_filters(ix, filters)
        allowed = payload_filter_np(n_p, cols, pf.arrays(), pf.batch)
        src = Spec(host.column_id("source"), 0, len(host.vocab["source"]), 0, None)
        want = facet_counts_np(n_p, cols, src, allowed)
        assert want[3].sum() == 0 and want[2].sum() == n_p
        for handle in (eng, ws):
            fc = handle.facet("source", doc_filter=pf)
            np.testing.assert_array_equal(_np(fc.raw), want)
            assert fc.labels == sorted(host.vocab["source"]) and fc.top(3)[0][0][1] == want[0, :-2].max()
            np.testing.assert_array_equal(_np(fc.other), 0)
            np.testing.assert_array_equal(_np(fc.missing), want[:, -1])
        one = compile_filters(ix, filters[0])                                     # a broadcast filter: one row
        np.testing.assert_array_equal(_np(eng.facet("source", doc_filter=one).raw), want[:1])
        np.testing.assert_array_equal(_np(eng.facet("source").raw), facet_counts_np(n_p, cols, src, np.ones(n_p, bool)))
        mask = torch.from_numpy(allowed).cuda()
        np.testing.assert_array_equal(_np(eng.facet("source", doc_filter=mask).raw), want)
        yr = compile_facet(ix, "year", edges=[2005, 2010, 2020])
        np.testing.assert_array_equal(_np(ws.facet(yr, doc_filter=pf).raw),
                                      facet_counts_np(n_p, cols, edges_i64(host.column_id("year"), [2005, 2010, 2020]), allowed))
        # the ids a retrieve call returned, padding included (query 3's filter allows nothing)
        b, k = pf.batch, 50
        bf16 = lambda bits_: torch.from_numpy(np.ascontiguousarray(bits_).view(np.int16)).cuda().view(torch.bfloat16)
        qf = bf16(synth.make_queries_np(fact_bits, b, seed=300)[0])
        qp = bf16(synth.make_queries_np(pass_bits, b, seed=301)[0])
        idx, sc = eng.score_facts(qf, k=5)
        cnt = torch.full((b,), 5, dtype=torch.int32, device="cuda")
        got = eng.retrieve(qp, idx, sc, cnt, k=k, doc_filter=pf)
        ids = _np(got.doc_idx)
        assert (ids[3] == -1).all() and (ids[0] >= 0).all()
        want_ids = facet_ids_np(n_p, cols, src, ids)
        for handle in (eng, ws):
            np.testing.assert_array_equal(_np(handle.facet("source", ids=got.doc_idx).raw), want_ids)
        assert want_ids.sum(1).tolist() == (ids >= 0).sum(1).tolist()
        with pytest.raises(ValueError, match="doc_filter or ids, not both"):
            eng.facet("source", doc_filter=pf, ids=got.doc_idx)
        with pytest.raises(ValueError, match="unknown field 'nope'"):
            eng.facet("nope")
    finally:
        if ws is not None:
            ws.close()
        eng.close()
        ix.close()


# ---------------------------------------------------------------------------------- the mirror
META = [("s1", {"user": "alice", "year": 2020}), ("s2", {"user": "bob", "year": 2021}), ("s1", {"user": "alice", "year": 2021}),
        (None, {"year": 2022}), ("s3", {"user": "carol"})]        # the metadata of tests/test_gpu_payload.py's mirror


def test_the_mirror_counts_what_the_python_metadata_holds(gpu_device):
    from hipporag_amd.retriever import Chunk, HippoRAG, RetrievalConfig
    from tests.golden.make_golden import DOCS, TRIPLES, MockEmbeddingModel
    chunks = [Chunk(d, source_id=META[i % 5][0], metadata=dict(META[i % 5][1], page=i)) for i, d in enumerate(DOCS)]
    rag = HippoRAG(RetrievalConfig(max_batch=4, retrieval_top_k=len(DOCS) + 3, embedding_precision="bf16", payload_index=True),
                   embedding_model=MockEmbeddingModel())
    rag.index_from_openie(chunks, TRIPLES)
    metas = [rag.chunk_metadata.get(key, {}) for key in rag.passage_node_keys]

    def count(pred, key):
        vals = [m.get(key) for m in metas if pred(m)]
        tally = {}
        for v in vals:
            if v is not None:
                tally[v] = tally.get(v, 0) + 1
        order = sorted(tally.items(), key=lambda kv: (-kv[1], kv[0]))              # count descending, then label = code order
        return {"values": order, "other": 0, "missing": sum(v is None for v in vals), "total": len(vals)}
    cases = [({"year": {"$gte": 2021}}, lambda m: "year" in m and m["year"] >= 2021), (None, lambda m: True),
             ({"user": "alice"}, lambda m: m.get("user") == "alice"), ({"user": "nobody"}, lambda m: False)]
    for f, pred in cases:
        got = rag.facets(["source_id", "user"], doc_filter=f)
        assert len(got) == 1 and got[0] == {"source_id": count(pred, "source_id"), "user": count(pred, "user")}, f
    per = rag.facets("source_id", doc_filter=[c[0] if c[0] is not None else {} for c in cases], limit=2)
    for q, (f, pred) in enumerate(cases):
        want = count(pred, "source_id")
        want["values"] = want["values"][:2]
        assert per[q] == {"source_id": want}, f
    years = rag.facets("year", edges=[2021, 2022])[0]["year"]
    ys = [m.get("year") for m in metas]
    buckets = [((None, 2021), ys.count(2020)), ((2021, 2022), ys.count(2021)), ((2022, None), ys.count(2022))]
    assert years["values"] == [lv for lv in sorted(buckets, key=lambda lv: -lv[1]) if lv[1]]         # (sorted is stable)
    assert years["missing"] == ys.count(None) and years["other"] == 0 and years["total"] == len(metas)
    with pytest.raises(ValueError, match="unknown field 'colour'"):
        rag.facets("colour")


# ---------------------------------------------------------------------------------- a seeded slice
def test_a_seeded_five_second_slice_of_random_cases(gpu_device):
    seed = 20240607
    print(f"facet slice: seed {seed}")
    rng = np.random.default_rng(seed)
    t0, cases = time.monotonic(), 0
    while time.monotonic() - t0 < 5.0:
        n = int(rng.choice([int(rng.integers(1, 130)), int(rng.integers(T - 40, T + 40)), int(rng.integers(1, 16 * T + 1))]))
        b = int(rng.choice([1, 2, 3, 17, 65]))
        cols = facet_columns(rng, n)
        ix = _index(cols)
        try:
            forms = list(_word_forms(rng, n, b))
            for _ in range(4):
                spec = random_spec(rng)
                bins = facet_bins_np(n, cols, spec)
                form, allowed, words, ld = forms[int(rng.integers(0, 3))]
                what = f"seed={seed} case={cases} n={n} b={b} spec={spec} words={form}"
                _check(_facet(ix, spec, b, words, ld), facet_counts_np(n, cols, spec, allowed, bins), spec, what)
                k = int(rng.integers(1, 600))
                ids = rng.integers(-3, n + 3, (b, k)).astype(np.int32)
                _check(_facet_ids(ix, spec, ids), facet_ids_np(n, cols, spec, ids, bins), spec, what + f" ids k={k}")
                cases += 1
        finally:
            ix.close()
    print(f"facet slice: {cases} cases in {time.monotonic() - t0:.1f} s")
    assert cases >= 4
