"""Lexical retrieval on the device (include/hrag.h, "lexical retrieval"; csrc/lex.hip): hrag_lex_scores and
hrag_lex_blend_rows held bit for bit to the numpy restatement of tests/lex_helpers.py, hrag_lex_create's host validation,
Engine.retrieve(lexical=) held to Engine.retrieve_scored over rows blended in numpy, and the mirror on the toy corpus."""

import math

import numpy as np
import pytest

from hipporag_amd import synth
from oracle.checks import make_case
from tests.lex_helpers import (LEX_MAX_QUERY_TERMS, LEX_TILE, blend_np, lex_scores_np, make_index, make_queries, rank_np,
                               row_minmax_np, same_bits)

pytestmark = pytest.mark.gpu

T = LEX_TILE
GUARD = -7.25


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
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _lex_scores(ix, q, b, ld, want_minmax=True):
    """hrag_lex_scores into a guard-filled [b, ld] buffer -> (rows, mn, mx)"""
    import torch
    L, lib = _L()
    qp, qt, qw = (_dev(a) for a in q)
    out = torch.full((b, ld), GUARD, dtype=torch.float32, device="cuda")
    mn, mx = (torch.full((b,), GUARD, dtype=torch.float32, device="cuda") for _ in range(2))
    nnz = int(q[1].shape[0])
    L.check(lib.hrag_lex_scores(ix._handle, qp.data_ptr(), qt.data_ptr() if nnz else None, qw.data_ptr() if nnz else None,
                                nnz, b, out.data_ptr(), ld, mn.data_ptr() if want_minmax else None,
                                mx.data_ptr() if want_minmax else None, _stream()))
    return out, mn, mx


# ---------------------------------------------------------------------------------- hrag_lex_scores
@pytest.fixture(scope="module")
def indexes(gpu_device):
    """One index per passage count, with its host arrays: built once, shared by the batch sizes."""
    from hipporag_amd.engine import LexicalIndex
    made = {}
    for n in (1, T - 1, T, T + 1, 3 * T + 17):
        host = make_index(np.random.default_rng(n), n)
        made[n] = (host, LexicalIndex.from_postings(n, *host))
    yield made
    for _, ix in made.values():
        ix.close()


@pytest.mark.parametrize("b", [1, 3, 65])
@pytest.mark.parametrize("n", [1, T - 1, T, T + 1, 3 * T + 17])
def test_lex_scores_match_the_restatement_bit_for_bit(indexes, n, b):
    """b = 65 walks every special query of make_queries; b = 1 is the query at exactly the cap; b = 3 takes the scalar
    store path (an odd row stride), the others the float4 one."""
    import torch
    from hipporag_amd.engine import row_minmax
    (ptr, doc, pw), ix = indexes[n]
    assert ix.n_passages == n and ix.n_terms == 40 and ix.nnz == len(doc)
    q = make_queries(np.random.default_rng(1000 * b + n), b)
    assert np.diff(q[0]).max() == LEX_MAX_QUERY_TERMS and (b < 11 or np.isnan(q[2]).any())
    ld = n + 5 if b == 3 else n + (-n) % 4 + 4
    out, mn, mx = _lex_scores(ix, q, b, ld)
    torch.cuda.synchronize()
    got = _np(out)
    want = lex_scores_np(n, ptr, doc, pw, *q)
    assert (got[:, n:] == GUARD).all(), "the columns beyond n_passages are not touched"
    assert not (got[:, :n] == GUARD).any(), "every column is written"
    assert same_bits(got[:, :n], want), (n, b, np.flatnonzero((got[:, :n].view(np.uint32) != want.view(np.uint32)).any(1))[:5])
    rmn, rmx = row_minmax(out, n)
    assert same_bits(_np(mn), _np(rmn)) and same_bits(_np(mx), _np(rmx))
    wmn, wmx = row_minmax_np(want)
    assert same_bits(_np(mn), wmn) and same_bits(_np(mx), wmx)
    if b == 65:
        assert same_bits(got[1, :n], np.zeros(n)) and same_bits(got[7, :n], np.zeros(n))      # empty query; empty list
        assert same_bits(got[5, :n], np.zeros(n)), "2 * 1.5 - 1 * 3.0 cancels to +0.0"
        assert np.isnan(got[6, :n]).all() and not np.isfinite(got[10, :n]).any()      # a NaN / an inf query weight
    # without the min / max outputs: the same rows
    out2, mn2, _ = _lex_scores(ix, q, b, ld, want_minmax=False)
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32)) and bool((mn2 == GUARD).all())


def test_terms_beyond_the_cap_are_ignored_and_nothing_else_is_touched(indexes):
    """A device-side q_ptr cannot be checked on the host: a list longer than the cap scores its first
    HRAG_LEX_MAX_QUERY_TERMS terms, and a q_ptr that points outside q_term reads nothing beyond q_nnz."""
    import torch
    n = T + 1
    (ptr, doc, pw), ix = indexes[n]
    rng = np.random.default_rng(3)
    m = LEX_MAX_QUERY_TERMS + 40
    q = (np.array([0, m, m + 2], np.int32), rng.integers(0, 40, m + 2).astype(np.int32),
         (rng.integers(-8, 9, m + 2) / 4).astype(np.float32))
    out, _, _ = _lex_scores(ix, q, 2, n)
    assert same_bits(_np(out), lex_scores_np(n, ptr, doc, pw, *q))
    wild = (np.array([-5, 3, 2 ** 31 - 1], np.int32), q[1][:4], q[2][:4])        # clamped to [0, 4): rows 0 and 1 of 4 terms
    out, _, _ = _lex_scores(ix, wild, 2, n + 3)
    torch.cuda.synchronize()
    want = lex_scores_np(n, ptr, doc, pw, np.array([0, 3, 4], np.int32), wild[1], wild[2])
    assert same_bits(_np(out)[:, :n], want) and (_np(out)[:, n:] == GUARD).all()


def test_lex_create_rejects_malformed_postings(gpu_device):
    from hipporag_amd._lib import HRAG_EINVAL, HragError
    from hipporag_amd.engine import LexicalIndex
    good = ([0, 2, 2, 5], [0, 3, 1, 2, 4], [1.0, -2.0, 0.5, 0.0, 3.0])
    LexicalIndex.from_postings(5, *good).close()
    LexicalIndex.from_postings(5, [0, 0], [], []).close()                                    # no postings at all
    bad = {
        "descending docs": ([0, 2, 2, 5], [3, 0, 1, 2, 4], good[2]),
        "a duplicate doc": ([0, 2, 2, 5], [0, 3, 1, 1, 4], good[2]),
        "an id out of range": ([0, 2, 2, 5], [0, 5, 1, 2, 4], good[2]),
        "a negative id": ([0, 2, 2, 5], [-1, 3, 1, 2, 4], good[2]),
        "an inf weight": (good[0], good[1], [1.0, np.inf, 0.5, 0.0, 3.0]),
        "a NaN weight": (good[0], good[1], [1.0, -2.0, np.nan, 0.0, 3.0]),
        "a decreasing term_ptr": ([0, 3, 2, 5], good[1], good[2]),
        "term_ptr[0] != 0": ([1, 2, 2, 5], good[1], good[2]),
    }
    for what, (ptr, doc, w) in bad.items():
        with pytest.raises(HragError) as err:
            LexicalIndex.from_postings(5, ptr, doc, w)
        assert err.value.status == HRAG_EINVAL, what
    with pytest.raises(HragError):
        LexicalIndex.from_postings(0, [0, 0], [], [])
    # from_csr: the passage-major form, inverted on the host; a term repeated within a passage is rejected there
    ix = LexicalIndex.from_csr([0, 2, 3], [1, 0, 1], [1.0, 2.0, 3.0])
    assert (ix.n_passages, ix.n_terms, ix.nnz) == (2, 2, 3)
    ix.close()
    ix.close()                                                                               # idempotent
    with pytest.raises(ValueError, match="repeated within passage 0"):
        LexicalIndex.from_csr([0, 2, 3], [1, 1, 0], [1.0, 2.0, 3.0])


# ---------------------------------------------------------------------------------- hrag_lex_blend_rows
def _blend(dense, lex, alpha, ld=None, alias=False):
    import torch
    from hipporag_amd.engine import row_minmax
    L, lib = _L()
    b, n = dense.shape
    ld = n if ld is None else ld
    d = torch.full((b, ld), GUARD, dtype=torch.float32, device="cuda")
    l = torch.full((b, ld + 4), GUARD, dtype=torch.float32, device="cuda")
    d[:, :n], l[:, :n] = _dev(dense), _dev(lex)
    mn_d, mx_d = row_minmax(d, n)
    mn_l, mx_l = row_minmax(l, n)
    out = d if alias else torch.full((b, ld), GUARD, dtype=torch.float32, device="cuda")
    L.check(lib.hrag_lex_blend_rows(d.data_ptr(), ld, l.data_ptr(), ld + 4, b, n, mn_d.data_ptr(), mx_d.data_ptr(),
                                    mn_l.data_ptr(), mx_l.data_ptr(), alpha, out.data_ptr(), ld, _stream()))
    torch.cuda.synchronize()
    got = _np(out)
    assert (got[:, n:] == GUARD).all()
    if not alias:
        assert same_bits(_np(d)[:, :n], dense), "the dense rows are only read"
    return got[:, :n]


def _blend_case(n, seed):
    rng = np.random.default_rng(seed)
    dense = rng.standard_normal((8, n)).astype(np.float32)
    lex = (rng.integers(0, 40, (8, n)) / 8).astype(np.float32) * (rng.random((8, n)) < 0.3)
    lex = lex.astype(np.float32)
    lex[1] = 0.0                                     # a lexical row of all zeros: no range
    lex[2] = np.nan                                  # a NaN-only lexical row: no number
    dense[3] = 0.375                                 # a constant dense row: range 0 -> 1
    lex[4] = 2.5                                     # a constant non-zero lexical row: no range either
    if n > 3:
        dense[5, 1], lex[5, 2] = np.nan, np.nan      # NaNs are skipped by the min / max and propagate element-wise
        dense[6, 0], dense[6, 2] = -0.0, np.inf
        lex[7, n - 1] = -3.0                         # a negative weight sets the lexical minimum
    return dense, lex


@pytest.mark.parametrize("n,ld", [(1, 1), (3, 4), (1029, 1029), (1029, 1032), (T + 4, T + 4)])
def test_blend_rows_match_the_restatement_bit_for_bit(gpu_device, n, ld):
    dense, lex = _blend_case(n, n + ld)
    for alpha in (0.0, 0.3, 1.0):
        want = blend_np(dense, lex, alpha)
        got = _blend(dense, lex, alpha, ld)
        assert same_bits(got, want), (n, ld, alpha)
        for r in ((0, 1, 2, 3, 4, 5, 6, 7) if alpha == 0 else (1, 2, 4)):
            assert same_bits(got[r], dense[r]), "a row without a lexical range is the dense row bit for bit"
        assert same_bits(_blend(dense, lex, alpha, ld, alias=True), want), "out aliased to dense"


def test_blend_rows_reject_a_bad_alpha(gpu_device):
    from hipporag_amd._lib import HRAG_EINVAL, HragError
    dense, lex = _blend_case(16, 1)
    for alpha in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(HragError) as err:
            _blend(dense, lex, alpha)
        assert err.value.status == HRAG_EINVAL


# ---------------------------------------------------------------------------------- the engine calls
@pytest.fixture(scope="module")
def case(gpu_device):
    from hipporag_amd.engine import HippoRAGEngine, LexicalIndex
    from tests.group_helpers import random_groups
    kg, pass_bits, fact_bits, _ = make_case(3000, 24000, 64, seed=4141)
    n_p = kg.n_passages
    grp = random_groups(np.random.default_rng(2), n_p, "shuffled")
    eng = HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                         max_batch=130, max_topk=min(200, n_p))
    eng.set_passage_groups(grp)
    host = make_index(np.random.default_rng(77), n_p)
    ix = LexicalIndex.from_postings(n_p, *host)
    eng.set_lexical_index(ix)
    yield gpu_device, kg, pass_bits, fact_bits, eng, host
    eng.close()
    ix.close()


def _bf16(bits, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)


def _inputs(dev, eng, fact_bits, pass_bits, b, seed):
    import torch
    qf = _bf16(synth.make_queries_np(fact_bits, b, seed=seed)[0], dev)
    qp = _bf16(synth.make_queries_np(pass_bits, b, seed=seed + 1)[0], dev)
    idx, sc = eng.score_facts(qf, k=5)
    cnt = torch.full((b,), 5, dtype=torch.int32, device=dev)
    cnt[::4] = 0                                      # the DPR fallback ranks the blended rows too
    return qp, idx, sc, cnt


def _same_output(a, b, what):
    import torch
    for name in ("doc_idx", "flags", "iters_used", "group_idx", "hit_idx"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), (what, name)
    for name in ("doc_score", "residual", "hit_score", "mmr_value"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None) and (x is None or same_bits(_np(x), _np(y))), (what, name)


@pytest.mark.parametrize("b,want_state", [(1, 4), (9, 2), (65, 8)])
def test_retrieve_with_lexical_is_retrieve_scored_over_the_blended_rows(case, b, want_state):
    import torch
    dev, kg, pass_bits, fact_bits, eng, (ptr, doc, pw) = case
    n_p, k = kg.n_passages, 20
    qp, idx, sc, cnt = _inputs(dev, eng, fact_bits, pass_bits, b, 300 + b)
    q = make_queries(np.random.default_rng(b), b)
    lex_rows = lex_scores_np(n_p, ptr, doc, pw, *q)
    assert same_bits(_np(eng.lexical_scores(*q)), lex_rows)
    rows, mn, mx = eng.lexical_scores(*q, want_minmax=True)
    assert same_bits(_np(mn), row_minmax_np(lex_rows)[0]) and same_bits(_np(mx), row_minmax_np(lex_rows)[1])
    dense = _np(eng.sim_scores("passages", qp))
    blended = torch.from_numpy(blend_np(dense, lex_rows, 0.3)).to(dev)
    allowed = torch.from_numpy(np.arange(n_p) % 3 != 0).to(dev)
    for what, kw in (("plain", {}), ("doc_filter", dict(doc_filter=allowed)),
                     ("groups", dict(group_agg="max", group_hits=2)), ("mmr", dict(mmr_lambda=0.5, mmr_candidates=40))):
        want = eng.retrieve_scored(blended, idx, sc, cnt, k=k, **kw)
        if what == "plain":
            assert eng.stats()["last_ppr_state"] == want_state
        got = eng.retrieve(qp, idx, sc, cnt, k=k, lexical=q, lexical_weight=0.3, **kw)
        _same_output(got, want, (b, what))
        # the caller's rows blended the same way; they are left as they were
        mine = torch.from_numpy(dense).to(dev)
        got = eng.retrieve_scored(mine, idx, sc, cnt, k=k, lexical=q, lexical_weight=0.3, **kw)
        _same_output(got, want, (b, what, "scored"))
        assert same_bits(_np(mine), dense)
    assert int((want.flags & 1).sum()) >= 1 or b == 1
    # a following fusion works on the rows the lexical call left
    if b == 9:
        eng.retrieve_scored(blended, idx, sc, cnt, k=1)
        want_f = eng.last_fused([0, 4, 9], fuse="sum", k=k)
        eng.retrieve(qp, idx, sc, cnt, k=1, lexical=q, lexical_weight=0.3)
        got_f = eng.last_fused([0, 4, 9], fuse="sum", k=k)
        assert torch.equal(got_f.doc_idx, want_f.doc_idx) and same_bits(_np(got_f.doc_score), _np(want_f.doc_score))
    # the contract's two halves serve it through the same blended rows
    want = eng.retrieve_scored(blended, idx, sc, cnt, k=k, ppr_tol=1.5e-6, ppr_max_iters=60)
    pending = eng.retrieve_converged_start(qp, idx, sc, cnt, k=k, ppr_tol=1.5e-6, ppr_max_iters=60, lexical=q,
                                           lexical_weight=0.3)
    got = pending.finish()
    if not pending.repeated:            # (a repeat reruns rows on a wider state: another computation by design)
        _same_output(got, want, (b, "contract"))


@pytest.mark.parametrize("b", [1, 9, 65])
def test_all_empty_queries_leave_retrieve_bit_identical(case, b):
    """No term matches anything: every lexical row is all +0.0, has no range, and the dense rows go through untouched --
    the whole call is the plain one, whatever the weight."""
    dev, kg, pass_bits, fact_bits, eng, _ = case
    qp, idx, sc, cnt = _inputs(dev, eng, fact_bits, pass_bits, b, 500 + b)
    empty = (np.zeros(b + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    nomatch = (np.arange(b + 1, dtype=np.int32), np.zeros(b, np.int32), np.ones(b, np.float32))    # term 0: no postings
    plain = eng.retrieve(qp, idx, sc, cnt, k=20)
    for q, w in ((empty, 0.3), (nomatch, 1.0), (make_queries(np.random.default_rng(b), b), 0.0)):
        _same_output(eng.retrieve(qp, idx, sc, cnt, k=20, lexical=q, lexical_weight=w), plain, (b, w))
    _same_output(eng.retrieve(qp, idx, sc, cnt, k=20), plain, "lexical=None")


def test_dense_and_lexical_retrieve_rank_the_restated_rows(case):
    import torch
    from tests.lex_helpers import minmax_np
    dev, kg, pass_bits, fact_bits, eng, (ptr, doc, pw) = case
    n_p, b, k = kg.n_passages, 12, 25
    qp, idx, sc, cnt = _inputs(dev, eng, fact_bits, pass_bits, b, 41)
    q = make_queries(np.random.default_rng(12), b)
    assert not np.isfinite(q[2]).all()
    q = (q[0], q[1], np.where(np.isfinite(q[2]), q[2], 1.0).astype(np.float32))     # finite rows: the normalised scores below
    lex_rows = lex_scores_np(n_p, ptr, doc, pw, *q)
    blended = blend_np(_np(eng.sim_scores("passages", qp)), lex_rows, 0.3)
    allowed = np.arange(n_p) % 3 != 0
    allowed_d = torch.from_numpy(allowed).to(dev)
    for flt, flt_d in ((None, None), (allowed, allowed_d)):
        gi, gs = eng.lexical_retrieve(q, k, doc_filter=flt_d)
        wi, ws = rank_np(lex_rows, k, flt)
        assert np.array_equal(_np(gi), wi) and same_bits(_np(gs), ws)
        gi, gs = eng.dense_retrieve(qp, k=k, doc_filter=flt_d, lexical=q, lexical_weight=0.3)
        wi, _ = rank_np(blended, k, flt)
        assert np.array_equal(_np(gi), wi)
        norm = np.stack([minmax_np(r, *[v[0] for v in row_minmax_np(r[None])]) for r in blended])   # over EVERY element
        assert same_bits(_np(gs), np.take_along_axis(norm, wi.astype(np.int64), axis=1) + np.float32(0))
    # more entries than there are allowed passages: -1 / 0 behind them
    few = torch.zeros(n_p, dtype=torch.bool, device=dev)
    few[[5, 9]] = True
    gi, gs = eng.lexical_retrieve(q, 4, doc_filter=few)
    assert (_np(gi)[:, 2:] == -1).all() and (_np(gs)[:, 2:] == 0).all() and set(_np(gi)[:, :2].ravel().tolist()) == {5, 9}


def test_a_workspace_sharing_the_index_gives_the_same_bits(case):
    dev, kg, pass_bits, fact_bits, eng, _ = case
    b = 9
    qp, idx, sc, cnt = _inputs(dev, eng, fact_bits, pass_bits, b, 77)
    q = make_queries(np.random.default_rng(4), b)
    want = eng.retrieve(qp, idx, sc, cnt, k=20, lexical=q, lexical_weight=0.3)
    ws = eng.workspace()
    try:
        _same_output(ws.retrieve(qp, idx, sc, cnt, k=20, lexical=q, lexical_weight=0.3), want, "workspace")
        assert same_bits(_np(ws.lexical_scores(*q)), _np(eng.lexical_scores(*q)))
    finally:
        ws.close()
    with pytest.raises(ValueError, match="passages"):
        from hipporag_amd.engine import LexicalIndex
        small = LexicalIndex.from_postings(3, [0, 1], [2], [1.0])
        try:
            eng.set_lexical_index(small)
        finally:
            small.close()


# ---------------------------------------------------------------------------------- the mirror
TOKEN = "zx9"      # two letters and a digit: a word of its own for the \w+ tokenizer


def _blind_model():
    from tests.golden.make_golden import MockEmbeddingModel

    class Blind(MockEmbeddingModel):
        """The toy embedding model, blind to TOKEN: the text is encoded as if the token were not there."""

        def batch_encode(self, texts, instruction=None, norm=True):
            if isinstance(texts, str):
                texts = [texts]
            return super().batch_encode([" ".join(w for w in t.split() if w != TOKEN) for t in texts], instruction, norm)

    return Blind()


def _idf(n, df):
    return math.log(1.0 + (n - df + 0.5) / (df + 0.5))


def test_mirror_finds_the_passage_that_holds_the_literal_token(gpu_device):
    """Document 3 of the toy corpus gets a token the embedding model does not see; the query is that token alone.  The
    plain ranking misses the passage because the query's embedding is the embedding of an empty string -- unrelated to
    every passage -- so the dense scores rank the passages in an arbitrary order in which document 3 is not first (the
    test asserts that order, it does not assume it).  The recognition filter keeps no fact here, so the ranking IS the
    min-max of the passage scores (the DPR fallback): with lexical_weight = 0.5 document 3 is the only passage with a
    lexical score, its blended score is 0.5 * nd + 0.5 against at most 0.5 for every other passage, and it ranks first."""
    from tests.golden.make_golden import DOCS, TRIPLES
    from hipporag_amd import HippoRAG, RetrievalConfig
    docs = list(DOCS)
    target = docs[3] = DOCS[3] + " " + TOKEN
    cfg = RetrievalConfig(embedding_precision="bf16", max_batch=4, ppr_iters=40, ppr_tol=0.0)
    rag = HippoRAG(cfg, embedding_model=_blind_model(), rerank_filter=lambda q, items, idx, len_after_rerank=None: ([], [], {}))
    rag.index_from_openie(docs, TRIPLES)
    n = len(docs)
    plain = rag.retrieve([TOKEN], num_to_retrieve=n)[0]
    assert plain.docs[0] != target and rag.lexical_model is None and "lexical_weight" not in plain.doc_metadata[0]
    lex = rag.retrieve([TOKEN], num_to_retrieve=n, lexical_weight=0.5)[0]
    assert lex.docs[0] == target and sorted(lex.docs) == sorted(plain.docs)
    assert all(md["lexical_weight"] == 0.5 for md in lex.doc_metadata)
    assert rag.retrieve_dpr([TOKEN], num_to_retrieve=n)[0].docs[0] != target
    dpr = rag.retrieve_dpr([TOKEN], num_to_retrieve=n, lexical_weight=0.5)[0]
    assert dpr.docs[0] == target and dpr.doc_metadata[0]["lexical_weight"] == 0.5
    assert rag.retrieve_ircot([TOKEN], 1, num_to_retrieve=n, lexical_weight=0.5)[0].docs[0] == target
    again = rag.retrieve([TOKEN], num_to_retrieve=n)[0]                  # weight 0 again: the plain call
    assert again.docs == plain.docs and same_bits(again.doc_scores, plain.doc_scores)
    # the model behind it: BM25 over the passages the mirror holds
    m = rag.lexical_model
    tok = m.tokenize
    word = tok(DOCS[0])[0]
    df_word = sum(word in tok(d) for d in docs)
    assert m.n_passages == n and m.idf[m.vocab.id_of[TOKEN]] == _idf(n, 1) and m.idf[m.vocab.id_of[word]] == _idf(n, df_word)
    assert rag.lexical_index.n_passages == n and rag.lexical_index.n_terms == len(m.vocab)
    for call, name in ((lambda: rag.retrieve([TOKEN], lexical_weight=1.5), "lexical_weight"),
                       (lambda: rag.retrieve_dpr([TOKEN], lexical_weight=0.5, mmr_lambda=0.5), "lexical_weight")):
        with pytest.raises(ValueError, match=name):
            call()
    # the config value: built with the engine, rebuilt after delete() and after index_from_openie()
    on = HippoRAG(RetrievalConfig(embedding_precision="bf16", max_batch=4, ppr_iters=40, ppr_tol=0.0, lexical_weight=0.5),
                  embedding_model=_blind_model(), rerank_filter=rag.rerank_filter)
    on.index_from_openie(docs, TRIPLES)
    assert on.retrieve([TOKEN], num_to_retrieve=n)[0].docs[0] == target
    first_index = on.lexical_index
    on.delete([target])
    rest = on.retrieve([TOKEN], num_to_retrieve=n)[0]                    # the token is unknown now: the plain ranking
    assert target not in rest.docs and len(rest.docs) == n - 1
    m = on.lexical_model
    left = [d for d in docs if d != target]
    df_word = sum(word in tok(d) for d in left)
    assert TOKEN not in m.vocab and m.n_passages == n - 1 and m.idf[m.vocab.id_of[word]] == _idf(n - 1, df_word)
    assert on.lexical_index is not first_index and not first_index._handle.value and on.lexical_index.n_passages == n - 1
    new_doc = f"A new page that repeats {TOKEN} and {word}"
    on.index_from_openie([new_doc], [[["new page", "repeats", word]]])
    back = on.retrieve([TOKEN], num_to_retrieve=n)[0]
    m = on.lexical_model
    assert back.docs[0] == new_doc and m.n_passages == n
    assert m.idf[m.vocab.id_of[TOKEN]] == _idf(n, 1) and m.idf[m.vocab.id_of[word]] == _idf(n, df_word + 1)
    with pytest.raises(ValueError, match="retrieve_fused does not serve lexical_weight"):
        on.retrieve_fused([[TOKEN]])
