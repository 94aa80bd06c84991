"""Late-interaction reranking on the device (include/hrag.h, "late-interaction reranking"; csrc/late.hip): the MaxSim
kernel held to the fp64 restatement bit for bit on exact inputs -- every tile edge, both masks, every needle position, the
last passage of the allocation -- and to the derived accumulation bound on realistic ones; the ranking kernel held to
late_rank_np; Engine.retrieve(late=) and its siblings to the restatement over the plain call's own ranking; the mirror on
the planted corpus."""

import numpy as np
import pytest

from hipporag_amd import synth
from oracle.checks import make_case
from tests.helpers import rounded_score_bound, sim_reference
from tests.late_helpers import exact_tokens, late_rank_np, late_scores_np, planted_late_corpus, ragged
from tests.mmr_helpers import mmr_batch_np, same_bits

pytestmark = pytest.mark.gpu

GUARD = -7.25
P_LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 129, 200]
Q_LENGTHS = [0, 1, 15, 16, 17, 33, 64]


def _L():
    from hipporag_amd import _lib
    return _lib, _lib.load()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _np(t):
    return t.cpu().numpy()


def _ids(rng, b, c, n):
    """candidate ids with repeats, -1 slots and ids outside [0, n)"""
    ids = rng.integers(0, n, (b, c)).astype(np.int32)
    if c >= 2:
        ids[:, 1] = ids[:, 0]                              # a repeated id
    m = rng.random((b, c))
    ids[m < 0.08] = -1
    ids[(m >= 0.08) & (m < 0.12)] = n + 5
    ids[(m >= 0.12) & (m < 0.14)] = 2 ** 31 - 1
    return ids


def _scores(ix, lq, ids, ld=None, pad=0):
    """hrag_late_scores -> (the [B, c] view, the whole guard-filled buffer)"""
    import torch
    L, lib = _L()
    b, c = ids.shape
    ld = c if ld is None else ld
    buf = torch.full((b * ld + pad,), GUARD, dtype=torch.float32, device="cuda")
    idd = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).cuda()
    L.check(lib.hrag_late_scores(ix._handle, lq.q_ptr.ctypes.data, lq.q_ptr_dev.data_ptr(),
                                 lq.q_tok.data_ptr() if lq.n_tokens else None, b, idd.data_ptr(), c, buf.data_ptr(), ld,
                                 _stream()))
    torch.cuda.synchronize()
    return buf[:b * ld].view(b, ld), buf


def _pair(p_tokens, q_tokens, dtype):
    from hipporag_amd.late import LateQueries, TokenIndex
    return TokenIndex.from_ragged(p_tokens, dtype), LateQueries.from_ragged(q_tokens, dtype)


def _mixed_lengths(rng, n, pool):
    lens = list(pool) + [int(x) for x in rng.choice(pool, max(0, n - len(pool)))]
    rng.shuffle(lens)
    return lens[:n] if n < len(pool) else lens


# (dim, B, c): together every dim, B and c of the issue's lists; every passage and query length is in every case
EXACT = [(8, 1, 1), (24, 3, 5), (32, 65, 64), (40, 3, 65), (64, 1, 1024), (128, 65, 5), (136, 3, 64), (256, 3, 1024)]


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("dim,b,c", EXACT)
def test_exact_inputs_are_exact(gpu_device, dim, b, c, dtype, negative):
    """negative: every query token in the negative orthant of every passage token -- every s_ij < 0, so a zero-filled row
    (or column) instead of the -inf mask (or the count) would change the result."""
    rng = np.random.default_rng(dim * 1000 + b * 10 + c + negative)
    n = 24
    p_len = _mixed_lengths(rng, n, P_LENGTHS)
    q_len = [Q_LENGTHS[(i + dim) % len(Q_LENGTHS)] for i in range(b)] if b < 7 else _mixed_lengths(rng, b, Q_LENGTHS)
    if b == 1:
        q_len = [Q_LENGTHS[(dim // 8) % (len(Q_LENGTHS) - 1) + 1]]
    p_tok = exact_tokens(rng, p_len, dim, -1 if negative else None)
    q_tok = exact_tokens(rng, q_len, dim, +1 if negative else None)
    ids = _ids(rng, b, c, n)
    ix, lq = _pair(p_tok, q_tok, dtype)
    with ix:
        ld = c + 3
        got, buf = _scores(ix, lq, ids, ld=ld, pad=64)
        got = _np(got)
    want = late_scores_np(*ragged(p_tok, dim), *ragged(q_tok, dim), ids)
    assert np.array_equal(got[:, :c], want), (dim, b, c, dtype, negative)
    assert (got[:, c:] == GUARD).all() and bool((buf[b * ld:] == GUARD).all())
    if negative:
        live = (ids >= 0) & (ids < n)
        has = live & (np.asarray(p_len)[np.where(live, ids, 0)] > 0) & (np.asarray(q_len)[:, None] > 0)
        assert (want[has] < 0).all() and has.any()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_needle_at_every_position(gpu_device, dtype):
    """Passage j of 130 tokens scores low at every token except token j: the score follows j exactly -- a dropped row of
    a tail tile or a dropped lane group shows as the base score."""
    dim, t = 40, 130
    rng = np.random.default_rng(3)
    base = np.full((t, dim), -3 / 8)
    p_tok = []
    for j in range(t):
        a = base.copy()
        a[j] = -1 / 8
        a[j, j % dim] = (1 + j % 3) / 8
        p_tok.append(a)
    q_tok = [rng.integers(1, 4, size=(m, dim)) / 8 for m in (1, 17, 64)]
    ids = np.tile(np.arange(t, dtype=np.int32), (3, 1))
    ix, lq = _pair(p_tok, q_tok, dtype)
    with ix:
        got = _np(_scores(ix, lq, ids)[0])
    want = late_scores_np(*ragged(p_tok, dim), *ragged(q_tok, dim), ids)
    assert np.array_equal(got, want)
    low = late_scores_np(*ragged([base], dim), *ragged(q_tok, dim), np.zeros((3, 1), np.int32))
    assert (want > low).all()


@pytest.mark.parametrize("last", [1, 17])
def test_last_passage_ends_the_allocation(gpu_device, last):
    import torch
    from hipporag_amd.late import LateQueries, TokenIndex
    dim = 136
    rng = np.random.default_rng(last)
    p_tok = exact_tokens(rng, [5, 64, last], dim)
    q_tok = exact_tokens(rng, [17, 64], dim)
    ptr, rows = ragged(p_tok, dim)
    emb = torch.from_numpy(rows).to(torch.bfloat16).cuda()
    assert emb.shape[0] == ptr[-1] and emb.untyped_storage().nbytes() == ptr[-1] * dim * 2     # the last row ends the tensor
    ids = np.array([[2, 1, 0, 2], [0, 2, 2, 1]], np.int32)
    with TokenIndex.from_csr(ptr, emb, "bf16") as ix:
        got = _np(_scores(ix, LateQueries.from_ragged(q_tok, "bf16"), ids)[0])
    assert np.array_equal(got, late_scores_np(ptr, rows, *ragged(q_tok, dim), ids))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_realistic_inputs_within_the_derived_bound(gpu_device, dtype):
    """|score - fp64| <= sum_i max_j bound_ij + 2^-24 (|want| + that sum): each m_i is off by at most the largest
    accumulation bound among its passage's s_ij (rounded_score_bound), the fp64 sum adds nothing visible, and the one
    rounding to fp32 at most 2^-24 of the rounded value."""
    import torch
    dim, nq, n, b = 128, 32, 20, 4
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    td = torch.bfloat16 if dtype == "bf16" else torch.float16
    lens = [100 + 3 * i for i in range(n)]
    unit = lambda x: x / x.norm(dim=1, keepdim=True)
    p_tok = [unit(torch.randn((t, dim), generator=g, device="cuda")).to(td) for t in lens]
    q_tok = [unit(torch.randn((nq, dim), generator=g, device="cuda")).to(td) for _ in range(b)]
    ids = np.tile(np.arange(n, dtype=np.int32), (b, 1))
    ix, lq = _pair(p_tok, q_tok, dtype)
    with ix:
        got = _scores(ix, lq, ids)[0].double()
    worst = 0.0
    for q in range(b):
        for p in range(n):
            s = sim_reference(p_tok[p], q_tok[q])                        # [nq, t] fp64
            bound = rounded_score_bound(p_tok[p], q_tok[q], dim).max(dim=1).values.sum()
            want = s.max(dim=1).values.sum()
            tol = bound + 2.0 ** -24 * (want.abs() + bound)
            worst = max(worst, float((got[q, p] - want).abs() / tol))
    assert worst <= 1.0, (dtype, worst)


def test_position_independence(gpu_device):
    """The same (query, passage) pair at B = 1, inside a batch of 65, at another slot and twice in one row: the same bits."""
    import torch
    dim, n = 128, 30
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    p_tok = [torch.randn((40 + 7 * i, dim), generator=g, device="cuda") for i in range(n)]
    q_tok = [torch.randn((1 + i % 64, dim), generator=g, device="cuda") for i in range(65)]
    from hipporag_amd.late import LateQueries, TokenIndex
    with TokenIndex.from_ragged(p_tok, "bf16") as ix:
        one = _scores(ix, LateQueries.from_ragged([q_tok[40]], "bf16"), np.array([[17]], np.int32))[0]
        rng = np.random.default_rng(0)
        ids = rng.integers(0, n, (65, 9)).astype(np.int32)
        ids[40, 2] = ids[40, 7] = 17
        many = _scores(ix, LateQueries.from_ragged(q_tok, "bf16"), ids)[0]
        sub = _scores(ix, LateQueries.from_ragged(q_tok, "bf16").select([3, 40]), ids[[3, 40]])[0]
    bits = lambda t: t.view(torch.int32)
    assert bits(many[40, 2]) == bits(one[0, 0]) and bits(many[40, 7]) == bits(one[0, 0])
    assert torch.equal(bits(sub), bits(many[[3, 40]]))


def _rank_rows(score, ids, n_ids, k, ld_pad=3):
    import torch
    L, lib = _L()
    b, c = ids.shape
    sd = torch.full((b, c + ld_pad), GUARD, device="cuda")
    sd[:, :c] = torch.from_numpy(score).cuda()
    idd = torch.from_numpy(ids).cuda()
    sel, idx = (torch.full((b, k), 77, dtype=torch.int32, device="cuda") for _ in range(2))
    sc = torch.full((b, k), GUARD, device="cuda")
    L.check(lib.hrag_late_rank_rows(sd.data_ptr(), sd.stride(0), idd.data_ptr(), n_ids, b, c, k, sel.data_ptr(),
                                    idx.data_ptr(), sc.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return _np(sel), _np(idx), _np(sc)


@pytest.mark.parametrize("c", [1, 64, 65, 1024])
def test_ranking_matches_the_restatement(gpu_device, c):
    rng = np.random.default_rng(c)
    b, n = 6, 3 * c + 4
    s = (rng.integers(-6, 7, (b, c)) / 4).astype(np.float32)           # few values: ties everywhere
    specials = [np.nan, np.inf, -np.inf, -0.0, 0.0, np.nan, np.inf, -np.inf]
    if c >= 16:
        for q in range(b):
            at = rng.permutation(c)[:len(specials)]
            s[q, at] = specials
    else:
        s[:, 0] = specials[:b]
    ids = _ids(rng, b, c, n)
    if b > 1 and c > 1:
        ids[1, :] = -1                                                  # a query without live slots
    for k in sorted({1, c}):
        for n_ids in (n, 0):
            got = _rank_rows(s, ids, n_ids, k)
            want = late_rank_np(s, ids, n_ids, k)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (c, k, n_ids)
            assert same_bits(got[2], np.where(np.isnan(want[2]), np.float32(np.nan), want[2])), (c, k, n_ids)


def test_c_abi_refuses_by_code(gpu_device):
    import ctypes as C
    import torch
    from hipporag_amd.late import LateQueries, TokenIndex
    L, lib = _L()
    ptr = np.array([0, 2, 3], np.int64)
    emb = torch.zeros((3, 264), dtype=torch.bfloat16, device="cuda")
    h = C.c_void_p(0)
    for dim, what in ((12, "multiple of 8"), (264, "HRAG_LATE_MAX_DIM")):
        assert lib.hrag_late_create(2, ptr.ctypes.data, emb.data_ptr(), dim, 0, C.byref(h)) == L.HRAG_EINVAL
        assert what in lib.hrag_last_error().decode() and not h.value
    bad = np.array([0, 3, 2], np.int64)
    assert lib.hrag_late_create(2, bad.ctypes.data, emb.data_ptr(), 8, 0, C.byref(h)) == L.HRAG_EINVAL
    assert "tok_ptr" in lib.hrag_last_error().decode()
    rng = np.random.default_rng(0)
    with TokenIndex.from_ragged(exact_tokens(rng, [2, 1], 8), "bf16") as ix:
        lq = LateQueries.from_ragged(exact_tokens(rng, [3, 2], 8), "bf16")
        ids = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
        out = torch.full((2, 4), GUARD, device="cuda")
        big = torch.zeros((80, 8), dtype=torch.bfloat16, device="cuda")

        def scores(qp, c=4, ld=4, tok=lq.q_tok):
            qp = np.asarray(qp, np.int32)
            return lib.hrag_late_scores(ix._handle, qp.ctypes.data, lq.q_ptr_dev.data_ptr(), tok.data_ptr(), 2, ids.data_ptr(),
                                        c, out.data_ptr(), ld, _stream())
        for args, what in ((([0, 3, 2],), "q_ptr decreases"), (([0, 70, 75], 4, 4, big), "HRAG_LATE_MAX_QUERY_TOKENS"),
                           (([0, 3, 5], 0), "c=0"), (([0, 3, 5], 1025), "c=1025"), (([0, 3, 5], 4, 3), "ld=3")):
            assert scores(*args) == L.HRAG_EINVAL and what in lib.hrag_last_error().decode(), what
        sel = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
        for k in (0, 5):
            assert lib.hrag_late_rank_rows(out.data_ptr(), 4, ids.data_ptr(), 2, 2, 4, k, sel.data_ptr(), sel.data_ptr(),
                                           out.data_ptr(), _stream()) == L.HRAG_EINVAL
            assert f"k={k}" in lib.hrag_last_error().decode()
        assert lib.hrag_late_workspace_bytes(2, 1025) < 0 and lib.hrag_late_workspace_bytes(3, 5) == 3 * 8 * 4
        torch.cuda.synchronize()
        assert bool((out == GUARD).all())                                # nothing was enqueued


# ---------------------------------------------------------------------------------- the engine
TOK_DIM = 32


@pytest.fixture(scope="module")
def case(gpu_device):
    from hipporag_amd.engine import HippoRAGEngine, LexicalIndex
    from hipporag_amd.late import TokenIndex
    from hipporag_amd.payload import PayloadIndex, encode_columns
    from tests.lex_helpers import make_index
    kg, pass_bits, fact_bits, _ = make_case(3000, 24000, 64, seed=4141)
    n_p = kg.n_passages
    rng = np.random.default_rng(8)
    eng = HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                         max_batch=70, max_topk=min(200, n_p))
    p_tok = exact_tokens(rng, rng.integers(1, 20, n_p), TOK_DIM)
    tix = TokenIndex.from_ragged(p_tok, "bf16")
    eng.set_token_index(tix)
    lex = LexicalIndex.from_postings(n_p, *make_index(np.random.default_rng(77), n_p))
    eng.set_lexical_index(lex)
    host = encode_columns({"year": [int(rng.integers(2000, 2024)) for _ in range(n_p)], "score": rng.standard_normal(n_p)}, n_p)
    pix = PayloadIndex(host)
    eng.set_payload_index(pix)
    yield gpu_device, kg, pass_bits, fact_bits, eng, ragged(p_tok, TOK_DIM)
    eng.close()
    for x in (tix, lex, pix):
        x.close()


def _bf16(bits, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)


def _inputs(dev, eng, fact_bits, pass_bits, b, seed):
    import torch
    qf = _bf16(synth.make_queries_np(fact_bits, b, seed=seed)[0], dev)
    qp = _bf16(synth.make_queries_np(pass_bits, b, seed=seed + 1)[0], dev)
    idx, sc = eng.score_facts(qf, k=5)
    cnt = torch.full((b,), 5, dtype=torch.int32, device=dev)
    cnt[::4] = 0
    return qp, idx, sc, cnt


def _late_queries(b, seed):
    from hipporag_amd.late import LateQueries
    rng = np.random.default_rng(seed)
    q_tok = exact_tokens(rng, [(3 * i) % 20 for i in range(b)], TOK_DIM)          # (query 0 has no tokens)
    return LateQueries.from_ragged(q_tok, "bf16"), ragged(q_tok, TOK_DIM)


def _want(tok, qry, plain_idx, plain_score, n_p, k):
    """-> (idx, late score, first score) of the restatement over a plain call's ranking"""
    ids, first = _np(plain_idx), _np(plain_score)
    sc = late_scores_np(*tok, *qry, ids)
    sel, idx, out = late_rank_np(sc, ids, n_p, k)
    fs = np.where(sel >= 0, np.take_along_axis(first, np.maximum(sel, 0).astype(np.int64), axis=1), np.float32(0))
    return idx, out, fs, sc


def _check(got_idx, got_score, got_first, want, what):
    assert np.array_equal(_np(got_idx), want[0]), what
    assert same_bits(_np(got_score), want[1]), what
    assert same_bits(_np(got_first), want[2]), what


def test_retrieve_with_late_is_the_restatement_over_its_own_ranking(case):
    import torch
    dev, kg, pass_bits, fact_bits, eng, tok = case
    n_p, b, c, k = kg.n_passages, 9, 50, 10
    qp, idx, sc, cnt = _inputs(dev, eng, fact_bits, pass_bits, b, 70)
    lq, qry = _late_queries(b, 1)
    before = eng.retrieve(qp, idx, sc, cnt, k=k)
    plain = eng.retrieve(qp, idx, sc, cnt, k=c)
    wk = eng.workspace()
    for handle in (eng, wk):
        out = handle.retrieve(qp, idx, sc, cnt, k=k, late=lq, late_candidates=c)
        torch.cuda.synchronize()
        w = _want(tok, qry, plain.doc_idx, plain.doc_score, n_p, k)
        _check(out.doc_idx, out.doc_score, out.first_score, w, "retrieve")
        assert torch.equal(out.flags, plain.flags) and out.mmr_value is None
        # the two public seams give the same bits
        assert same_bits(_np(handle.late_scores(plain.doc_idx, lq)), w[3])
        ri, rs, rsel = handle.late_rerank(plain.doc_idx, lq, k, return_sel=True)
        assert torch.equal(ri, out.doc_idx) and same_bits(_np(rs), _np(out.doc_score))
    wk.close()
    assert not np.array_equal(_np(out.doc_idx), _np(before.doc_idx))                      # (the stage does something)
    # late_candidates None: the k ranked entries in late order
    out = eng.retrieve(qp, idx, sc, cnt, k=k, late=lq)
    _check(out.doc_idx, out.doc_score, out.first_score, _want(tok, qry, before.doc_idx, before.doc_score, n_p, k), "c = k")
    # without late: the call that never heard of it
    after = eng.retrieve(qp, idx, sc, cnt, k=k)
    assert after.first_score is None and torch.equal(after.doc_idx, before.doc_idx)
    assert same_bits(_np(after.doc_score), _np(before.doc_score)) and torch.equal(after.flags, before.flags)


def test_late_composes_with_every_option_before_the_ranking(case):
    import torch
    from hipporag_amd.boost import compile_boosts
    from tests.lex_helpers import make_queries
    dev, kg, pass_bits, fact_bits, eng, tok = case
    n_p, b, c, k = kg.n_passages, 12, 40, 8
    qp, idx, sc, cnt = _inputs(dev, eng, fact_bits, pass_bits, b, 9)
    lq, qry = _late_queries(b, 2)
    kept = (idx, sc, cnt)
    allowed = torch.from_numpy(np.arange(n_p) % 3 != 0).to(dev)
    few = torch.zeros(n_p, dtype=torch.bool, device=dev)
    few[:5] = True                                                      # fewer allowed passages than k: -1 slots
    lex_q = make_queries(np.random.default_rng(3), b)
    prog = compile_boosts(eng._payload_ix("test"), [{"if": {"year": {"$gte": 2012}}, "add": 0.5}, {"mul": 1.25}])
    for what, kw in (("filter", dict(doc_filter=allowed)), ("seeds scope", dict(doc_filter=allowed, filter_scope="seeds")),
                     ("few allowed", dict(doc_filter=few)), ("boost", dict(boost=prog)),
                     ("lexical", dict(lexical=lex_q, lexical_weight=0.3))):
        plain = eng.retrieve(qp, *kept, k=c, **kw)
        out = eng.retrieve(qp, *kept, k=k, late=lq, late_candidates=c, **kw)
        _check(out.doc_idx, out.doc_score, out.first_score, _want(tok, qry, plain.doc_idx, plain.doc_score, n_p, k), what)
        none = eng.retrieve(qp, *kept, k=c, late=None, **kw)
        assert torch.equal(none.doc_idx, plain.doc_idx) and same_bits(_np(none.doc_score), _np(plain.doc_score)), what
        assert none.first_score is None
    # retrieve_scored
    dense = eng.sim_scores("passages", qp)
    plain = eng.retrieve_scored(dense, *kept, k=c)
    out = eng.retrieve_scored(dense, *kept, k=k, late=lq, late_candidates=c)
    _check(out.doc_idx, out.doc_score, out.first_score, _want(tok, qry, plain.doc_idx, plain.doc_score, n_p, k), "scored")
    # dense: one trailing entry
    di, ds = eng.dense_retrieve(qp, k=c)
    got = eng.dense_retrieve(qp, k=k, late=lq, late_candidates=c)
    assert len(got) == 3
    _check(*got, _want(tok, qry, di, ds, n_p, k), "dense")
    assert len(eng.dense_retrieve(qp, k=k)) == 2
    # fusion: one late query per question
    mp = [0, 3, 4, 12]
    fq, fqry = _late_queries(3, 5)
    eng.retrieve(qp, *kept, k=1)
    plain = eng.last_fused(mp, fuse="sum", k=c)
    eng.retrieve(qp, *kept, k=1)
    out = eng.last_fused(mp, fuse="sum", k=k, late=fq, late_candidates=c)
    _check(out.doc_idx, out.doc_score, out.first_score, _want(tok, fqry, plain.doc_idx, plain.doc_score, n_p, k), "fused")
    # MMR picks its k among the c rescored entries, the late scores as relevance
    plain = eng.retrieve(qp, *kept, k=c)
    out = eng.retrieve(qp, *kept, k=k, late=lq, late_candidates=c, mmr_lambda=0.5)
    li, ls, lf, _ = _want(tok, qry, plain.doc_idx, plain.doc_score, n_p, c)
    L, lib = _L()
    pass_dev = _bf16(pass_bits, dev).contiguous()
    lid = torch.from_numpy(li).to(dev)
    g = torch.zeros((b, c, c), dtype=torch.float32, device=dev)
    L.check(lib.hrag_gram_rows(pass_dev.data_ptr(), n_p, pass_bits.shape[1], 0, 0, lid.data_ptr(), b, c, g.data_ptr(), c,
                               _stream()))
    w = mmr_batch_np(ls, li, _np(g), k, 0.5, True, n_p)
    assert np.array_equal(_np(out.doc_idx), w[1]) and same_bits(_np(out.doc_score), w[2]) and same_bits(_np(out.mmr_value), w[3])
    wf = np.where(w[0] >= 0, np.take_along_axis(lf, np.maximum(w[0], 0).astype(np.int64), axis=1), np.float32(0))
    assert same_bits(_np(out.first_score), wf)
    # what the engine refuses, by name, before anything is enqueued
    for kw, name in ((dict(group_agg="max"), "group_agg"), (dict(late_candidates=eng.max_topk + 1), "late_candidates"),
                     (dict(mmr_lambda=0.5, mmr_candidates=c + 1), "mmr_candidates")):
        with pytest.raises(ValueError, match=name):
            eng.retrieve(qp, *kept, k=k, **{"late": lq, "late_candidates": c, **kw})
    with pytest.raises(ValueError, match="late_candidates needs late"):
        eng.retrieve(qp, *kept, k=k, late_candidates=c)
    with pytest.raises(ValueError, match="late: it holds 3 queries"):
        eng.retrieve(qp, *kept, k=k, late=fq)
    from hipporag_amd.engine import CapturedPipeline
    with pytest.raises(NotImplementedError, match="late"):
        CapturedPipeline(eng, 4, late=lq)


@pytest.mark.parametrize("b,want_state", [(9, 2), (65, 8)])
def test_the_contract_repeats_keep_each_rows_own_late_query(gpu_device, b, want_state):
    """retrieve_converged(late=) when finish() repeats SOME rows (the ring of tests/test_gpu_boost.py): the repeat runs a
    strict subset of the batch and must rescore it by the late queries of exactly those rows (LateQueries.select)."""
    import torch
    from hipporag_amd._lib import FLAG_NOT_CONVERGED
    from hipporag_amd.engine import HippoRAGEngine
    from hipporag_amd.late import LateQueries, TokenIndex
    from tests.test_gpu_fp8_adversarial import CASES, _index
    make, damping, _ = CASES["ring"]
    n_v, src, dst, w, pv, pinned = make()
    csr, pass_bits, fact_bits, index = _index(n_v, src, dst, w, pv, 64, seed=11, pinned_facts=pinned)
    n, k, c, tol, iters = len(pv), 10, 30, 1.5e-6, (12 if b <= 64 else 20)
    rng = np.random.default_rng(31 + b)
    p_tok = exact_tokens(rng, rng.integers(1, 12, n), TOK_DIM)
    q_tok = exact_tokens(rng, [1 + q % 9 for q in range(b)], TOK_DIM)
    tok, qry = ragged(p_tok, TOK_DIM), ragged(q_tok, TOK_DIM)
    qf = _bf16(synth.make_queries_np(fact_bits, b, seed=5)[0], gpu_device)
    qp = _bf16(synth.make_queries_np(pass_bits, b, seed=6)[0], gpu_device)
    with TokenIndex.from_ragged(p_tok, "bf16") as tix, \
            HippoRAGEngine(csr, index.passage_vertex, pass_bits, fact_bits, index.subj_vertex, index.obj_vertex,
                           index.num_chunks, max_batch=b, max_topk=n) as eng:
        eng.set_token_index(tix)
        lq = LateQueries.from_ragged(q_tok, "bf16")
        idx, sc = eng.score_facts(qf, k=5)
        cnt = torch.full((b,), 5, dtype=torch.int32, device=gpu_device)
        cnt[::4] = 0                                          # DPR fallback rows
        kw = dict(damping=damping, ppr_iters=iters, ppr_tol=tol, ppr_max_iters=400)
        first = eng.retrieve(qp, idx, sc, cnt, k=1, **kw)
        assert eng.stats()["last_ppr_state"] == want_state
        slow = (_np(first.flags) & FLAG_NOT_CONVERGED) != 0   # what finish() will repeat: some rows, not all
        assert slow.any() and not slow.all()
        plain = eng.retrieve_converged(qp, idx, sc, cnt, k=c, **kw)
        pend = eng.retrieve_converged_start(qp, idx, sc, cnt, k=k, late=lq, late_candidates=c, **kw)
        out = pend.finish()
        torch.cuda.synchronize()
        assert pend.repeated and torch.equal(out.flags, plain.flags) and torch.equal(out.iters_used, plain.iters_used)
        want = _want(tok, qry, plain.doc_idx, plain.doc_score, n, k)
        _check(out.doc_idx, out.doc_score, out.first_score, want, b)
        # a row rescored by a neighbour's query would differ
        rolled = ragged([q_tok[(q + 1) % b] for q in range(b)], TOK_DIM)
        other = _want(tok, rolled, plain.doc_idx, plain.doc_score, n, k)
        assert all(not np.array_equal(other[1][q], want[1][q]) for q in np.flatnonzero(slow))


# ---------------------------------------------------------------------------------- the mirror
def test_the_mirror_finds_the_planted_passage_only_with_late(gpu_device):
    from hipporag_amd.retriever import HippoRAG, RetrievalConfig
    from tests.late_helpers import PlantedEmbedder, PlantedTokenEncoder, planted_texts
    corpus = planted_late_corpus(5)
    docs, triples, queries = planted_texts(corpus)
    enc = PlantedTokenEncoder(corpus)
    rag = HippoRAG(RetrievalConfig(max_batch=2), embedding_model=PlantedEmbedder(corpus), token_encoder=enc)
    rag.index_from_openie(docs, triples)
    plain = rag.retrieve(queries, num_to_retrieve=3)
    late = rag.retrieve(queries, num_to_retrieve=3, late_candidates=20)       # three pipelined batches of two queries
    for q, (sol_p, sol_l) in enumerate(zip(plain, late)):
        right = docs[int(corpus["right"][q])]
        assert sol_p.docs[0] != right, q
        assert "late_score" not in sol_p.doc_metadata[0]
        assert sol_l.docs[0] == right, q
        meta = sol_l.doc_metadata[0]
        assert meta["late_score"] == float(len(corpus["q_tokens"][q])) == float(sol_l.doc_scores[0]), q
        assert meta["first_score"] <= float(sol_p.doc_scores[0]), q         # not above the plain call's first entry
    # the passages were encoded once, every batch encoded its own query strings
    assert [t for texts, is_q in enc.calls if not is_q for t in texts] == docs
    assert [texts for texts, is_q in enc.calls if is_q] == [queries[0:2], queries[2:4], queries[4:6]]
    # pipelined equals serial, bit for bit
    serial = [s_ for lo in range(0, len(queries), 2) for s_ in rag.retrieve(queries[lo:lo + 2], num_to_retrieve=3, late_candidates=20)]
    for a, b_ in zip(serial, late):
        assert a.docs == b_.docs and same_bits(np.asarray(a.doc_scores, np.float32), np.asarray(b_.doc_scores, np.float32))
        assert a.doc_metadata == b_.doc_metadata
    # the dense path serves it too
    dpr = rag.retrieve_dpr(queries, num_to_retrieve=3, late_candidates=20)
    assert all(s_.docs[0] == docs[int(corpus["right"][q])] and "first_score" in s_.doc_metadata[0] for q, s_ in enumerate(dpr))
    rag.engine.close()
