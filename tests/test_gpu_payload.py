"""Payload filters on the device (include/hrag.h, "payload filters"; csrc/payload.hip): hrag_payload_filter and
hrag_bitset_count_rows held word for word to the numpy restatement of tests/payload_helpers.py, the host validation, the
engine's doc_filter=PayloadFilter held bit for bit to the same call with the restatement's words, and the mirror on the toy
corpus."""

import ctypes as C

import numpy as np
import pytest

from hipporag_amd import synth
from hipporag_amd._lib import PAY_MAX_COLS, PAY_TILE
from hipporag_amd.engine import pack_mask
from oracle.checks import make_case
from tests.payload_helpers import (assemble, cols_for_restatement, host_arrays, make_columns, make_programs,
                                   payload_filter_np, payload_words_np, popcount_rows_np, special_programs)

pytestmark = pytest.mark.gpu

T = PAY_TILE
SIZES = [1, 31, 32, 33, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]
GUARD = np.uint32(0xA5A5A5A5)


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


def _filter(ix, prog, b, base=None, ld_a=None, pad=3, n_clauses=None, set_nnz=None):
    """hrag_payload_filter into a guard-filled [b, W + pad] buffer -> uint32 words [b, W + pad]"""
    import torch
    L, lib = _L()
    d = [_dev(a) for a in prog]
    nc = len(prog[1]) if n_clauses is None else n_clauses
    nnz = len(prog[6]) if set_nnz is None else set_nnz
    w = (ix.n_passages + 31) // 32
    out = _dev(np.full((b, w + pad), GUARD, np.uint32))
    aw = None if base is None else _dev(base)
    if ld_a is None:
        ld_a = 0 if base is None or base.ndim == 1 else base.shape[1]
    L.check(lib.hrag_payload_filter(ix._handle, d[0].data_ptr(), *(t.data_ptr() if len(prog[1]) else None for t in d[1:5]),
                                    d[5].data_ptr(), d[6].data_ptr() if len(prog[6]) else None, nc, nnz, b,
                                    aw.data_ptr() if aw is not None else None, ld_a, out.data_ptr(), w + pad, _stream()))
    torch.cuda.synchronize()
    return _np(out).view(np.uint32)


# ---------------------------------------------------------------------------------- hrag_payload_filter
@pytest.fixture(scope="module")
def indexes(gpu_device):
    """One index per passage count, with its host columns: built once, shared by the batch sizes."""
    made = {}
    for n in SIZES:
        cols = make_columns(np.random.default_rng(n), n)
        made[n] = (cols, _index(cols))
    yield made
    for _, ix in made.values():
        ix.close()


@pytest.mark.parametrize("b", [1, 3, 65])
@pytest.mark.parametrize("n", SIZES)
def test_payload_filter_matches_the_restatement_word_for_word(indexes, n, b):
    """b = 65 walks every special program of payload_helpers (each role alone and together, 64 and 65 clauses, the empty /
    one-value / 1000-value sets, lo > hi, the full range, bad columns, kinds and roles); b = 1 is the query at exactly the
    cap; each under a NULL base, a broadcast row and per-query rows, into rows wider than W."""
    cols, ix = indexes[n]
    rng = np.random.default_rng(1000 * b + n)
    progs = make_programs(rng, b)
    prog = assemble(progs)
    w = (n + 31) // 32
    base_rows = rng.random((b, n)) < 0.7
    for base in (None, base_rows[0], base_rows):
        base_words = None if base is None else pack_mask(base)
        if base is not None and base.ndim == 2:          # per-query rows with a stride of their own and junk behind W
            base_words = np.concatenate([base_words, rng.integers(0, 2 ** 32, (b, 2), dtype=np.uint32)], axis=1)
        got = _filter(ix, prog, b, base_words)
        want = payload_words_np(n, cols, prog, b, base)
        assert (got[:, w:] == GUARD).all(), "the words beyond W are not touched"
        np.testing.assert_array_equal(got[:, :w], want, err_msg=f"n={n} b={b} base={None if base is None else base.shape}")
        if n % 32:
            assert (got[:, w - 1] >> np.uint32(n % 32) == 0).all(), "the tail bits of the last word are zero"
    if b == 65:
        names = list(special_programs())
        row = lambda name: payload_filter_np(n, cols, prog, b)[names.index(name)]
        assert row("empty").all() and not row("lo > hi").any() and not row("unknown role").any()
        np.testing.assert_array_equal(row("65 clauses"), row("full range"))          # the 65th clause is ignored


def test_clamped_pointers_read_nothing_outside_the_arrays(indexes):
    """A device-side f_ptr / c_set_ptr cannot be checked on the host: descending or negative entries are clamped, and only
    the clauses [0, n_clauses) and the values [0, set_nnz) are read."""
    n = T + 1
    cols, ix = indexes[n]
    sp = special_programs()
    prog = list(assemble([sp["must"], sp["should"], sp["one value"], sp["1000 values"]]))
    good = payload_words_np(n, cols, prog, 4)
    w = (n + 31) // 32
    # f_ptr: negative, descending and far beyond the end
    wild = list(prog)
    wild[0] = np.array([-7, 1, 0, 2 ** 31 - 1, -1], np.int32)     # [0, 1), empty, [0, 5) i.e. every clause, empty
    got = _filter(ix, wild, 4)
    want = payload_words_np(n, cols, wild, 4)
    np.testing.assert_array_equal(got[:, :w], want)
    np.testing.assert_array_equal(want[0], good[0])
    assert (want[1] == pack_mask(np.ones(n, bool))).all() and (want[3] == want[1]).all()
    # c_set_ptr: descending / negative / beyond set_nnz -- clamped slices (each still ascending, as the definition asks):
    # [0, 2) of the small set, an empty slice at the end, [4, set_nnz) = the 1000 values
    wild = list(prog)
    wild[5] = np.array([5, -3, 2, 2 ** 31 - 1, 4, 4000], np.int32)
    np.testing.assert_array_equal(_filter(ix, wild, 4)[:, :w], payload_words_np(n, cols, wild, 4))
    # smaller counts than the arrays hold: the clauses / values behind them are never used
    for nc, nnz in ((2, len(prog[6])), (len(prog[1]), 500), (0, 0)):
        cut = [prog[0], prog[1][:nc], prog[2][:nc], prog[3][:nc], prog[4][:nc], prog[5][:nc + 1], prog[6][:nnz]]
        want = payload_words_np(n, cols, cut, 4)
        np.testing.assert_array_equal(_filter(ix, prog, 4, n_clauses=nc, set_nnz=nnz)[:, :w], want, err_msg=str((nc, nnz)))


def test_filter_and_create_reject_bad_arguments(indexes):
    import torch
    from hipporag_amd._lib import HRAG_EINVAL, HragError
    L, lib = _L()
    n = 65
    cols, ix = indexes[n]
    w = (n + 31) // 32
    prog = assemble([special_programs()["must"]] * 2)           # two queries: f_ptr covers batch = 2
    d = [_dev(a) for a in prog]
    out = torch.zeros((2, w + 1), dtype=torch.int32, device="cuda")
    base = torch.zeros((2, w), dtype=torch.int32, device="cuda")

    def call(handle=ix._handle, f_ptr=d[0].data_ptr(), n_clauses=2, set_nnz=0, batch=1, aw=None, ld_a=0, o=out.data_ptr(),
             ld_o=w + 1, set_vals=None):
        return lib.hrag_payload_filter(handle, f_ptr, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                                       d[5].data_ptr(), set_vals, n_clauses, set_nnz, batch, aw, ld_a, o, ld_o, _stream())
    assert call() == 0 and call(aw=base.data_ptr(), ld_a=w, batch=2) == 0 and call(aw=base.data_ptr(), ld_a=0, batch=2) == 0
    assert call(ld_o=w) == 0 and call(n_clauses=0, f_ptr=None) == 0
    bad = {"a NULL handle": dict(handle=None), "a NULL output": dict(o=None), "batch 0": dict(batch=0),
           "batch 65536": dict(batch=65536), "ld_o below W": dict(ld_o=w - 1), "ld_a below W": dict(aw=base.data_ptr(), ld_a=w - 1),
           "a negative ld_a": dict(aw=base.data_ptr(), ld_a=-1), "negative n_clauses": dict(n_clauses=-1),
           "negative set_nnz": dict(set_nnz=-1), "set values missing": dict(set_nnz=3), "clauses missing": dict(f_ptr=None)}
    for what, kw in bad.items():
        assert call(**kw) == HRAG_EINVAL, what
        assert lib.hrag_last_error()
    torch.cuda.synchronize()
    # create: everything is checked on the host before anything is allocated
    types, values, present = host_arrays(cols)

    def create(n_passages=n, n_cols=len(cols), t=types, v=values, p=present):
        h = C.c_void_p(0)
        tv = (C.c_int32 * max(len(t), 1))(*[int(x) for x in t])
        vv = (C.c_void_p * max(len(v), 1))(*[None if a is None else a.ctypes.data for a in v])
        pv = (C.c_void_p * max(len(p), 1))(*[None if a is None else a.ctypes.data for a in p]) if p is not None else None
        st = lib.hrag_payload_create(n_passages, n_cols, tv, vv, pv, C.byref(h))
        if st == 0:
            assert h.value and lib.hrag_payload_destroy(h) == 0
        else:
            assert not h.value
        return st
    assert create() == 0 and create(p=None) == 0 and create(n_cols=0) == 0
    many = PAY_MAX_COLS + 1
    for what, kw in {"n_passages 0": dict(n_passages=0), "n_passages 2^31": dict(n_passages=2 ** 31),
                     "negative n_cols": dict(n_cols=-1), "an unknown type": dict(t=[0, 1, 2, 1]),
                     "too many columns": dict(n_cols=many, t=[0] * many, v=[values[0]] * many, p=None),
                     "a NULL value pointer": dict(v=[values[0], None, values[2], values[3]])}.items():
        assert create(**kw) == HRAG_EINVAL, what
    assert lib.hrag_payload_create(n, 0, None, None, None, None) == HRAG_EINVAL               # a NULL out
    assert lib.hrag_payload_destroy(None) == 0
    # the Python side
    from hipporag_amd.payload import PayloadIndex, compile_filters
    small = PayloadIndex.from_columns({"a": [1, 2, None]}, 3)
    pf = compile_filters(small, {"a": 1})
    with pytest.raises(ValueError, match="another index"):
        ix.evaluate(pf)
    with pytest.raises(TypeError, match="PayloadFilter"):
        small.evaluate({"a": 1})
    with pytest.raises(ValueError, match="out"):
        small.evaluate(pf, out=torch.zeros((1, 1), dtype=torch.int64, device="cuda"))
    assert _np(small.evaluate(pf)).view(np.uint32).tolist() == [1] and small.columns == {"a": "i64"}
    assert _np(small.evaluate(pf, and_with=torch.tensor([False, True, True]))).tolist() == [0]
    small.close()
    small.close()                                                                             # idempotent
    with pytest.raises(ValueError, match="closed"):
        small.evaluate(pf)
    with pytest.raises(HragError):
        PayloadIndex.from_columns({}, 2 ** 31)


# ---------------------------------------------------------------------------------- hrag_bitset_count_rows
@pytest.mark.parametrize("n", SIZES)
def test_count_rows_is_the_popcount_of_the_first_n_bits(gpu_device, n):
    import torch
    from hipporag_amd._lib import HRAG_EINVAL
    from hipporag_amd.payload import count_rows
    L, lib = _L()
    rng = np.random.default_rng(n)
    w = (n + 31) // 32
    for b in (1, 3, 65):
        words = rng.integers(0, 2 ** 32, (b, w + 2), dtype=np.uint32)          # ld > W; bits beyond n are set too
        words[0, :w] = 0xFFFFFFFF
        if b > 1:
            words[1, :w] = 0
        d = _dev(words)
        cnt = torch.full((b,), -1, dtype=torch.int32, device="cuda")
        L.check(lib.hrag_bitset_count_rows(d.data_ptr(), w + 2, n, b, cnt.data_ptr(), _stream()))
        want = popcount_rows_np(words, n)
        np.testing.assert_array_equal(_np(cnt), want)
        assert want[0] == n
        np.testing.assert_array_equal(_np(count_rows(d, n)), want)
        np.testing.assert_array_equal(_np(count_rows(d[0], n)), want[:1])
        L.check(lib.hrag_bitset_count_rows(d.data_ptr(), 0, n, b, cnt.data_ptr(), _stream()))      # one row for all
        assert (_np(cnt) == n).all()
    for kw in (dict(ld=w - 1), dict(n=0), dict(batch=0), dict(words=None), dict(out=None)):
        a = dict(words=d.data_ptr(), ld=w + 2, n=n, batch=1, out=cnt.data_ptr())
        a.update(kw)
        if a["ld"] == 0:
            continue                                                                              # (w == 1: 0 is the broadcast)
        assert lib.hrag_bitset_count_rows(a["words"], a["ld"], a["n"], a["batch"], a["out"], _stream()) == HRAG_EINVAL, kw


# ---------------------------------------------------------------------------------- the engine calls
def _random_sources(n_f, n_p, rng, unsourced=0.1):
    row_ptr = np.zeros(n_f + 1, np.int64)
    pos = []
    for f in range(n_f):
        c = 0 if rng.random() < unsourced else int(rng.integers(1, 4))
        pos.extend(rng.choice(n_p, c, replace=False).tolist())
        row_ptr[f + 1] = len(pos)
    return row_ptr, np.asarray(pos, np.int32)


FILTERS = [{"year": {"$gte": 2015}}, {"tag": ["t3", "t7", "t9"], "$not": {"year": 2020}},
           {"$any": {"score": {"$lt": -1.0}, "tag": "t1"}, "year": {"$exists": True}}, {"rare": 1}, {"tag": "nope"}, None,
           {"score": {"$gt": -0.5, "$lte": 0.5}, "$not": {"tag": {"$exists": False}}}]


@pytest.fixture(scope="module")
def case(gpu_device):
    """The smallest case the lexical tests use to reach the small-batch (B = 1), fp16 (B = 9) and e4m3 (B = 65) states."""
    from hipporag_amd.engine import HippoRAGEngine, LexicalIndex
    from hipporag_amd.payload import PayloadIndex, encode_columns
    from tests.group_helpers import random_groups
    from tests.lex_helpers import make_index
    kg, pass_bits, fact_bits, _ = make_case(3000, 24000, 64, seed=4141)
    n_p = kg.n_passages
    rng = np.random.default_rng(5)
    eng = HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                         max_batch=130, max_topk=min(200, n_p))
    eng.set_passage_groups(random_groups(np.random.default_rng(2), n_p, "shuffled"))
    eng.set_fact_sources(*_random_sources(kg.n_facts, n_p, rng))
    lex = LexicalIndex.from_postings(n_p, *make_index(np.random.default_rng(77), n_p))
    eng.set_lexical_index(lex)
    rare = [None] * n_p
    for p in rng.choice(n_p, 5, replace=False):
        rare[int(p)] = 1
    columns = {"year": [None if rng.random() < 0.1 else int(rng.integers(2000, 2024)) for _ in range(n_p)],
               "tag": [None if rng.random() < 0.3 else f"t{int(rng.integers(0, 50))}" for _ in range(n_p)],
               "score": rng.standard_normal(n_p), "rare": rare}
    host = encode_columns(columns, n_p)
    ix = PayloadIndex(host)
    eng.set_payload_index(ix)
    yield gpu_device, kg, pass_bits, fact_bits, eng, ix, host
    eng.close()
    ix.close()
    lex.close()


def _bf16(bits, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)


def _compiled(ix, host, filters, dev):
    """(PayloadFilter, the restatement's words of the same program as a device tensor, allowed bool [B, n])"""
    import torch
    from hipporag_amd.payload import compile_filters
    pf = compile_filters(ix, filters)
    allowed = payload_filter_np(host.n_passages, cols_for_restatement(host), pf.arrays(), pf.batch)
    words = torch.from_numpy(pack_mask(allowed[0] if pf.broadcast else allowed).view(np.int32)).to(dev)
    return pf, words, allowed


def _same_output(a, b, what):
    import torch
    for name in ("doc_idx", "doc_score", "flags", "residual", "iters_used", "group_idx", "hit_idx", "hit_score", "mmr_value"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), (what, name)
        if x is not None:                                    # bit for bit: floats compared through their words
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                               y.view(torch.int32) if y.dtype == torch.float32 else y), (what, name)


@pytest.mark.parametrize("b,want_state", [(1, 4), (9, 2), (65, 8)])
def test_a_payload_filter_is_the_same_call_with_the_restated_words(case, b, want_state):
    import torch
    from tests.lex_helpers import make_queries
    dev, kg, pass_bits, fact_bits, eng, ix, host = case
    n_p, k = kg.n_passages, 20
    filters = [FILTERS[(i + (0 if b > 1 else 1)) % len(FILTERS)] for i in range(b)]
    pf, words, allowed = _compiled(ix, host, filters, dev)
    assert torch.equal(ix.evaluate(pf), words)
    np.testing.assert_array_equal(_np(ix.count(words)), allowed.sum(1))
    if b > 1:
        assert 0 < allowed[3].sum() < k and allowed[4].sum() == 0 and allowed[5].all()       # fewer than k; none; None
    qf = _bf16(synth.make_queries_np(fact_bits, b, seed=300 + b)[0], dev)
    qp = _bf16(synth.make_queries_np(pass_bits, b, seed=301 + b)[0], dev)
    idx, sc = eng.score_facts(qf, k=5)
    cnt = torch.full((b,), 5, dtype=torch.int32, device=dev)
    cnt[::4] = 0                                              # DPR fallback rows
    lex_q = make_queries(np.random.default_rng(b), b)
    for what, kw in (("plain", {}), ("groups", dict(group_agg="max", group_hits=2)), ("sum groups", dict(group_agg="sum")),
                     ("mmr", dict(mmr_lambda=0.5, mmr_candidates=40)), ("lexical", dict(lexical=lex_q, lexical_weight=0.3))):
        want = eng.retrieve(qp, idx, sc, cnt, k=k, doc_filter=words, **kw)
        if what == "plain":
            assert eng.stats()["last_ppr_state"] == want_state
        _same_output(eng.retrieve(qp, idx, sc, cnt, k=k, doc_filter=pf, **kw), want, (b, what))
    if b > 1:
        wi = _np(want.doc_idx)
        assert (wi[4] == -1).all() and (wi[3] >= 0).sum() == allowed[3].sum()
    # the "seeds" scope: phase A under the filter, then the scoped phase B
    s_idx, s_sc = eng.score_facts(qf, k=5, scope_filter=words)
    g_idx, g_sc = eng.score_facts(qf, k=5, scope_filter=pf)
    assert torch.equal(g_idx, s_idx) and torch.equal(g_sc.view(torch.int32), s_sc.view(torch.int32))
    s_cnt = (s_idx >= 0).sum(dim=1).to(torch.int32)
    for kw in ({}, dict(group_agg="max", group_hits=2)):
        want = eng.retrieve(qp, s_idx, s_sc, s_cnt, k=k, doc_filter=words, filter_scope="seeds", **kw)
        _same_output(eng.retrieve(qp, s_idx, s_sc, s_cnt, k=k, doc_filter=pf, filter_scope="seeds", **kw), want, (b, "seeds", kw))
    # retrieve_scored, dense_retrieve, lexical_retrieve, the convergence contract
    rows = eng.sim_scores("passages", qp)
    _same_output(eng.retrieve_scored(rows, idx, sc, cnt, k=k, doc_filter=pf),
                 eng.retrieve_scored(rows, idx, sc, cnt, k=k, doc_filter=words), (b, "scored"))
    for scope in ("ranking", "seeds"):
        for x, y in zip(eng.dense_retrieve(qp, k=k, doc_filter=pf, filter_scope=scope),
                        eng.dense_retrieve(qp, k=k, doc_filter=words, filter_scope=scope)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (b, "dense", scope)
    for x, y in zip(eng.lexical_retrieve(lex_q, k, doc_filter=pf), eng.lexical_retrieve(lex_q, k, doc_filter=words)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (b, "lexical_retrieve")
    want_p = eng.retrieve_converged_start(qp, idx, sc, cnt, k=k, ppr_tol=1.5e-6, ppr_max_iters=60, doc_filter=words)
    want = want_p.finish()
    got_p = eng.retrieve_converged_start(qp, idx, sc, cnt, k=k, ppr_tol=1.5e-6, ppr_max_iters=60, doc_filter=pf)
    eng.retrieve(qp, idx, sc, cnt, k=k, doc_filter=_compiled(ix, host, {"tag": "t1"}, dev)[0])    # another filtered call between
    got = got_p.finish()
    assert got_p.repeated == want_p.repeated
    _same_output(got, want, (b, "contract"))
    # one dict for the whole batch: a broadcast row
    pf1, words1, _ = _compiled(ix, host, FILTERS[1], dev)
    assert pf1.broadcast and words1.dim() == 1
    _same_output(eng.retrieve(qp, idx, sc, cnt, k=k, doc_filter=pf1), eng.retrieve(qp, idx, sc, cnt, k=k, doc_filter=words1),
                 (b, "broadcast"))
    # a following fusion: the filter of the fused ranking is a PayloadFilter of Q queries
    if b == 9:
        pf2, words2, _ = _compiled(ix, host, [FILTERS[0], FILTERS[3]], dev)
        for fuse in ("sum", "rrf"):
            eng.retrieve(qp, idx, sc, cnt, k=1)              # (a fusion replaces the member rows by the fused ones)
            want_f = eng.last_fused([0, 4, 9], fuse=fuse, k=k, doc_filter=words2)
            eng.retrieve(qp, idx, sc, cnt, k=1)
            _same_output(eng.last_fused([0, 4, 9], fuse=fuse, k=k, doc_filter=pf2), want_f, (b, "fused", fuse))


def test_a_workspace_shares_the_roots_index_and_errors_name_the_argument(case):
    import torch
    from hipporag_amd.payload import PayloadIndex, compile_filters
    dev, kg, pass_bits, fact_bits, eng, ix, host = case
    b, k = 9, 20
    filters = [FILTERS[i % len(FILTERS)] for i in range(b)]
    pf, words, _ = _compiled(ix, host, filters, dev)
    qf = _bf16(synth.make_queries_np(fact_bits, b, seed=77)[0], dev)
    qp = _bf16(synth.make_queries_np(pass_bits, b, seed=78)[0], dev)
    idx, sc = eng.score_facts(qf, k=5)
    cnt = torch.full((b,), 5, dtype=torch.int32, device=dev)
    want = eng.retrieve(qp, idx, sc, cnt, k=k, doc_filter=words)
    ws = eng.workspace()
    try:
        _same_output(ws.retrieve(qp, idx, sc, cnt, k=k, doc_filter=pf), want, "workspace")
        _same_output(eng.retrieve(qp, idx, sc, cnt, k=k, doc_filter=pf), want, "root")
        assert ws._pay_words is not eng._pay_words and ws._pay_words.shape == (eng.max_batch, ix.words)
    finally:
        ws.close()
    with pytest.raises(ValueError, match="doc_filter: the PayloadFilter holds 9 queries, the call 4"):
        eng.retrieve(qp[:4], idx[:4], sc[:4], cnt[:4], k=k, doc_filter=pf)
    with pytest.raises(ValueError, match="scope_filter: the PayloadFilter holds 9 queries"):
        eng.score_facts(qf[:4], k=5, scope_filter=pf)
    other = PayloadIndex.from_columns({"year": [1, 2, 3]}, 3)
    try:
        with pytest.raises(ValueError, match="doc_filter: the PayloadFilter was compiled for 3 passages"):
            eng.dense_retrieve(qp, k=k, doc_filter=compile_filters(other, {"year": 1}))
        with pytest.raises(ValueError, match="passages"):
            eng.set_payload_index(other)
    finally:
        other.close()
    with pytest.raises(TypeError, match="torch tensor"):
        eng.shard_finish(torch.zeros(b, device=dev), torch.zeros(b, device=dev), torch.zeros(b, dtype=torch.int32, device=dev),
                         k, doc_filter=pf)                  # the row-shard methods keep taking tensors only
    eng.set_payload_index(None)
    try:
        with pytest.raises(ValueError, match="doc_filter: a PayloadFilter needs a payload index"):
            eng.retrieve(qp, idx, sc, cnt, k=k, doc_filter=pf)
    finally:
        eng.set_payload_index(ix)


# ---------------------------------------------------------------------------------- the mirror
META = [("s1", {"user": "alice", "year": 2020}), ("s2", {"user": "bob", "year": 2021}), ("s1", {"user": "alice", "year": 2021}),
        (None, {"year": 2022}), ("s3", {"user": "carol"})]        # the metadata of tests/test_doc_filter_host.py's CHUNKS


def _mirror(payload_index):
    from hipporag_amd.retriever import Chunk, HippoRAG, RetrievalConfig
    from tests.golden.make_golden import DOCS, TRIPLES, MockEmbeddingModel
    chunks = [Chunk(d, source_id=META[i % 5][0], metadata=dict(META[i % 5][1], page=i)) for i, d in enumerate(DOCS)]
    rag = HippoRAG(RetrievalConfig(max_batch=4, retrieval_top_k=len(DOCS) + 3, embedding_precision="bf16",
                                   payload_index=payload_index), embedding_model=MockEmbeddingModel())
    rag.index_from_openie(chunks, TRIPLES)
    return rag


def _selected(rag, pred):
    return {rag.passage_texts[i] for i, key in enumerate(rag.passage_node_keys) if pred(rag.chunk_metadata.get(key, {}))}


def test_the_mirror_evaluates_the_richer_dicts_on_the_device(gpu_device):
    from hipporag_amd.retriever import Chunk
    from tests.golden.make_golden import QUERIES
    on, off = _mirror(True), _mirror(False)
    n = len(on.passage_node_keys)
    assert off.payload_index is None
    full = on.retrieve(QUERIES, num_to_retrieve=n)
    assert on.payload_index.columns == {"user": "keyword", "year": "i64", "page": "i64", "source_id": "keyword"}
    cases = [({"year": {"$gte": 2021}}, lambda m: "year" in m and m["year"] >= 2021),
             ({"user": {"$exists": False}}, lambda m: "user" not in m),
             ({"$not": {"user": "bob"}}, lambda m: m.get("user") != "bob"),
             ({"$any": {"user": "carol", "year": 2020}}, lambda m: m.get("user") == "carol" or m.get("year") == 2020),
             ({"year": {"$gt": 2020, "$lt": 2022}, "$not": {"source_id": "s2"}, "page": {"$lte": 7.5}},
              lambda m: m.get("year") == 2021 and m.get("source_id") != "s2" and m["page"] <= 7)]
    for f, pred in cases:
        allowed = _selected(on, pred)
        assert 0 < len(allowed) < n, f
        for method in ("retrieve", "retrieve_dpr"):
            ref = full if method == "retrieve" else on.retrieve_dpr(QUERIES, num_to_retrieve=n)
            got = getattr(on, method)(QUERIES, num_to_retrieve=n, doc_filter=f)
            for g, w in zip(got, ref):
                assert g.docs == [d for d in w.docs if d in allowed], (method, f)
                assert set(g.docs) == allowed
        with pytest.raises(ValueError, match="payload_index"):
            off.retrieve(QUERIES, num_to_retrieve=n, doc_filter=f)
    # equality dicts: the same results with the option on and off; per-query lists with None and a bool array
    arr = np.zeros(n, bool)
    arr[[0, 4, 7]] = True
    eq = [{"user": "alice"}, {"user": ["bob", "carol"], "year": [2021, 2022]}, {"source_id": "s1", "year": 2021}, {"user": "nobody"},
          {"colour": "red"}, {"year": 2021.0, "page": [1, 2, 6, True]}, {}]
    for f in eq + [[eq[i % len(eq)] for i in range(len(QUERIES))], [arr if i % 2 else eq[0] for i in range(len(QUERIES))]]:
        a, b = on.retrieve(QUERIES, num_to_retrieve=5, doc_filter=f), off.retrieve(QUERIES, num_to_retrieve=5, doc_filter=f)
        for x, y in zip(a, b):
            assert x.docs == y.docs, f
            np.testing.assert_array_equal(np.asarray(x.doc_scores, np.float32), np.asarray(y.doc_scores, np.float32))
    # a key the index does not hold keeps the host path (equality only) and goes in as the base row
    odd = next(i for i, key in enumerate(on.passage_node_keys) if "year" in on.chunk_metadata[key])
    on.chunk_metadata[on.passage_node_keys[odd]]["odd"] = [1, 2]             # unhashable: not a column
    on._filter_cache = {}
    on.ready_to_retrieve = False
    got = on.retrieve(QUERIES, num_to_retrieve=n, doc_filter={"odd": [[1, 2]], "year": {"$gte": 2000}})
    assert "odd" not in on.payload_index.columns and all(r.docs == [on.passage_texts[odd]] for r in got)
    with pytest.raises(ValueError, match="payload_index"):
        on.retrieve(QUERIES, doc_filter={"odd": {"$exists": True}})
    # after delete and a second index the filters see the new passage list
    first = on.payload_index
    gone = on.passage_texts[1]
    on.delete([gone])
    new = Chunk("George Rankin later became a mayor.", source_id="s9", metadata={"user": "zed", "year": 2030})
    on.index_from_openie([new], [[("George Rankin", "became", "mayor")]])
    got = on.retrieve(QUERIES, num_to_retrieve=n, doc_filter={"year": {"$gt": 2022}})
    assert all(r.docs == [new.content] for r in got)
    assert on.payload_index is not first and not first._handle.value and on.payload_index.n_passages == n
    allowed = _selected(on, lambda m: m.get("user") != "bob")
    got = on.retrieve(QUERIES, num_to_retrieve=n, doc_filter={"$not": {"user": "bob"}})
    assert gone not in allowed and new.content in allowed and all(set(r.docs) == allowed for r in got)
