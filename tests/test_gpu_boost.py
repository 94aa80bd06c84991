"""Boosted retrieval on the device (include/hrag.h, "boosted retrieval"; csrc/boost.hip): hrag_boost_rows held bit for bit to
the numpy restatement of tests/boost_helpers.py, the host validation, retrieve(boost=) and its relatives held bit for bit to
tests/option_helpers.expected_outputs over the restated boosted rows, the convergence contract's repeats held row by row to
each query's own program, and the mirror on the toy corpus.  (boost composed with every other option on every entry:
tests/test_gpu_option_matrix.py and the option slices of tests/test_gpu_soak_slices.py.)"""

import ctypes as C

import numpy as np
import pytest

from hipporag_amd import synth
from hipporag_amd._lib import (BOOST_ADD, BOOST_CONST, BOOST_DECAY, BOOST_EXP, BOOST_FIELD, BOOST_GAUSS, BOOST_LINEAR,
                               BOOST_MUL, BOOST_SQRT, PAY_MUST, PAY_RANGE, PAY_TILE)
from oracle.checks import make_case
from tests import option_helpers as oh
from tests.boost_helpers import (assemble_boost, boost_columns, boost_rows_np, decay_c, make_boosts, special_boosts, term)
from tests.payload_helpers import bits, cols_for_restatement, op

pytestmark = pytest.mark.gpu

T = PAY_TILE
SIZES = [1, 31, 33, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17]
GUARD = np.float32(-12345.5)
F32_SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-39, 3.4e38], np.float32)


def _L():
    from hipporag_amd import _lib
    return _lib, _lib.load()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _np(t):
    return None if t is None else t.cpu().numpy()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    v = (lambda a: a.view(np.uint32)) if got.dtype == np.float32 else (lambda a: a)
    if not np.array_equal(v(got), v(want)):
        at = np.argwhere(v(got) != v(want))
        raise AssertionError(f"{what}: {len(at)} entries differ, first at {tuple(at[0])}: got {got[tuple(at[0])]!r}, "
                             f"want {want[tuple(at[0])]!r}")


def _index(cols):
    from hipporag_amd.payload import PayloadColumns, PayloadIndex
    pc = PayloadColumns(len(cols[0][1]))
    for i, (typ, values, present) in enumerate(cols):
        pc._add(f"c{i}", typ, values, present)
    return PayloadIndex(pc)


def _desc(prog, counts=None):
    """(BoostProgramDesc, the device tensors that back it); counts: (n_terms, n_clauses, set_nnz) instead of the arrays'."""
    L, _ = _L()
    ts = [_dev(a) for a in prog]
    n = (len(prog[1]), len(prog[5]), len(prog[10])) if counts is None else counts
    return L.BoostProgramDesc(*(t.data_ptr() if t.numel() else None for t in ts), *n), ts


def _boost(ix, prog, rows, broadcast=False, mn=None, mx=None, pad=3, shift=0, counts=None):
    """hrag_boost_rows over a copy of rows [b, n] placed in a guard-filled [b, n + pad] buffer that starts `shift` floats
    into its allocation -> the buffer afterwards."""
    import torch
    L, lib = _L()
    b, n = rows.shape
    host = np.full((b, n + pad), GUARD, np.float32)
    host[:, :n] = rows
    flat = torch.empty(b * (n + pad) + shift + 4, dtype=torch.float32, device="cuda")
    buf = flat[shift: shift + b * (n + pad)].view(b, n + pad)
    buf.copy_(torch.from_numpy(host))
    d, keep = _desc(prog, counts)
    dmn, dmx = (None, None) if mn is None else (_dev(np.asarray(mn, np.float32)), _dev(np.asarray(mx, np.float32)))
    L.check(lib.hrag_boost_rows(ix._handle, buf.data_ptr(), n + pad, b, None if mn is None else dmn.data_ptr(),
                                None if mn is None else dmx.data_ptr(), C.byref(d), 1 if broadcast else 0, _stream()))
    torch.cuda.synchronize()
    return _np(buf)


def make_rows(rng, b, n):
    rows = rng.standard_normal((b, n)).astype(np.float32)
    sp = rng.random((b, n)) < 0.15
    rows[sp] = F32_SPECIALS[rng.integers(0, len(F32_SPECIALS), int(sp.sum()))]
    u = rows.view(np.uint32)
    u[0, 0] = 0x7FA00001 if n > 0 else u[0, 0]          # a NaN with a payload
    return rows


@pytest.fixture(scope="module")
def indexes(gpu_device):
    made = {}
    for n in SIZES:
        cols = boost_columns(np.random.default_rng(n), n)
        made[n] = (cols, _index(cols))
    yield made
    for _, ix in made.values():
        ix.close()


# ---------------------------------------------------------------------------------- hrag_boost_rows
@pytest.mark.parametrize("b", [1, 3, 65])
@pytest.mark.parametrize("n", SIZES)
def test_boost_rows_matches_the_restatement_bit_for_bit(indexes, n, b):
    """b = 65 walks every special program (each kind, mode, modifier and decay shape alone and mixed, conditions of every
    role, 0 / 1 / 32 / 33 terms, 64 / 65 clauses, holes with and without `missing`, int64 beyond 2^53, d at 0, inside the
    offset, at c and far beyond, zero and negative weights, sqrt below zero, ill-formed terms and clauses) over rows with NaN
    payloads, +-inf, +-0.0 and denormals; per query and broadcast; rows 16-byte aligned and not; the guard columns n .. ld
    and the rows of queries without terms keep their bits."""
    cols, ix = indexes[n]
    rng = np.random.default_rng(1000 * b + n)
    per = make_boosts(rng, b)
    prog = assemble_boost(per)
    rows = make_rows(rng, b, n)
    want = boost_rows_np(rows, n, cols, prog)
    for shift in (0, 1):
        got = _boost(ix, prog, rows, shift=shift)
        assert (got[:, n:] == GUARD).all(), "the columns beyond n are not touched"
        _same(got[:, :n], want, f"n={n} b={b} shift={shift}")
    untouched = [q for q, terms in enumerate(per) if not terms]
    if untouched:
        _same(got[untouched, :n], rows[untouched], "a query without terms")
    # one list for the batch: every query runs the terms of query 0 (b = 65: "no terms" -- nothing is touched)
    for q0 in (0, min(1, b - 1)):
        one = assemble_boost([per[q0]])
        got = _boost(ix, one, rows, broadcast=True)
        _same(got[:, :n], boost_rows_np(rows, n, cols, one, broadcast=True), f"broadcast n={n} b={b}")
        if not per[q0]:
            _same(got[:, :n], rows, "a broadcast program without terms")
    if b == 65:          # what the definition says of the caps and of ill-formed terms, on the restatement itself
        names = list(special_boosts())
        alone = lambda name, terms: (want[names.index(name)],
                                     boost_rows_np(rows[names.index(name)][None], n, cols, assemble_boost([terms]))[0], name)
        _same(*alone("33 terms", [term(BOOST_CONST, BOOST_ADD, w=0.5)] * 32))           # the 33rd term is ignored
        full = [(0, op(PAY_MUST, PAY_RANGE), np.iinfo(np.int64).min, np.iinfo(np.int64).max, None)]
        _same(*alone("65 clauses", [term(BOOST_CONST, BOOST_MUL, w=2.0, clauses=full), term(BOOST_CONST, BOOST_ADD, w=1.0, clauses=full),
                                    term(BOOST_CONST, BOOST_ADD, w=7.0)]))        # the 65th and 66th clauses are ignored
        for name, left in (("bad kind", term(BOOST_CONST, BOOST_ADD, w=1.0)), ("bad mode", term(BOOST_CONST, BOOST_MUL, w=2.0)),
                           ("bad sub", term(BOOST_CONST, BOOST_ADD, w=0.5)), ("high op bits", term(BOOST_CONST, BOOST_ADD, w=0.5)),
                           ("bad column", term(BOOST_CONST, BOOST_ADD, w=1.0))):
            _same(*alone(name, [left]))                                                  # an ill-formed term is neutral


def test_clamped_pointers_read_nothing_outside_the_arrays(indexes):
    """Device-side t_ptr / t_cl_ptr / c_set_ptr cannot be checked on the host: descending or negative entries are clamped,
    and only the terms [0, n_terms), the clauses [0, n_clauses) and the values [0, set_nnz) are read."""
    n = T + 1
    cols, ix = indexes[n]
    sp = special_boosts()
    per = [sp["const all roles"], sp["decay under a condition"], sp["mixed"], sp["const should"]]
    prog = list(assemble_boost(per))
    rows = make_rows(np.random.default_rng(3), 4, n)
    nt, nc, nnz = len(prog[1]), len(prog[5]), len(prog[10])
    wild = list(prog)
    wild[0] = np.array([-7, 1, 0, 2 ** 31 - 1, -1], np.int32)         # [0, 1), empty, every term (capped), empty
    _same(_boost(ix, wild, rows)[:, :n], boost_rows_np(rows, n, cols, wild), "t_ptr")
    _same(boost_rows_np(rows, n, cols, wild)[[1, 3]], rows[[1, 3]], "empty ranges touch nothing")
    wild = list(prog)
    wild[4] = np.array([3, -2, 2 ** 31 - 1, 0, 5, nc + 40, 1, 2, 2][:nt + 1], np.int32)
    assert len(wild[4]) == nt + 1
    _same(_boost(ix, wild, rows)[:, :n], boost_rows_np(rows, n, cols, wild), "t_cl_ptr")
    wild = list(prog)
    # c_set_ptr: negative, descending and beyond set_nnz -- clamped slices, each still ascending as the definition asks
    assert prog[9].tolist() == [0, 0, 3, 3, 3, 1003, 1004, 1004, 1007, 1007]
    wild[9] = np.array([0, -5, 3, 3, 3, 1003, 1004, 1004, 4000, -1], np.int32)
    _same(_boost(ix, wild, rows)[:, :n], boost_rows_np(rows, n, cols, wild), "c_set_ptr")
    for cnt in ((2, nc, nnz), (nt, 3, nnz), (nt, nc, 500), (nt, 0, 0), (0, 0, 0)):
        a, c, s = cnt
        cut = [prog[0], prog[1][:a], prog[2][:a], prog[3][:a], prog[4][:a + 1], prog[5][:c], prog[6][:c], prog[7][:c], prog[8][:c],
               prog[9][:c + 1], prog[10][:s]]
        _same(_boost(ix, prog, rows, counts=cnt)[:, :n], boost_rows_np(rows, n, cols, cut), str(cnt))


@pytest.mark.parametrize("shape", [BOOST_LINEAR, BOOST_EXP, BOOST_GAUSS])
def test_every_fp64_operation_is_rounded_on_its_own(indexes, shape):
    """3T + 17 random doubles with full mantissas through each decay shape, with weights, origins and offsets that have full
    mantissas too, as MUL and as ADD: a contracted multiply-add anywhere -- in the Horner steps, in the range reduction, in
    w * v, in s * M + A -- shows as a last-bit difference in some of the 6161 entries of a row."""
    n = 3 * T + 17
    cols, ix = indexes[n]
    rng = np.random.default_rng(50 + shape)
    per = []
    for q in range(3):
        scale, decay = float(rng.uniform(5, 80)), float(rng.uniform(0.1, 0.9))
        p = (float(rng.standard_normal() * 10), float(rng.uniform(0, 3)), decay_c(shape, scale, decay))
        per.append([term(BOOST_DECAY, BOOST_MUL, shape, col=4, w=float(rng.uniform(0.5, 2)), p=p),
                    term(BOOST_DECAY, BOOST_ADD, shape, col=3, w=float(rng.standard_normal()), p=(p[0] / 40, 0.0, decay_c(shape, 1.3, decay))),
                    term(BOOST_FIELD, BOOST_ADD, BOOST_SQRT, col=4, w=float(rng.uniform(0.01, 0.02)),
                         clauses=[(4, op(PAY_MUST, PAY_RANGE), int(bits(0.0)), int(bits(np.inf)), None)])])
    prog = assemble_boost(per)
    rows = rng.standard_normal((3, n)).astype(np.float32)
    want = boost_rows_np(rows, n, cols, prog)
    assert (want != rows).mean() > 0.9 and np.isfinite(want).all()
    _same(_boost(ix, prog, rows)[:, :n], want, f"shape {shape}")


def _midpoint_case(shape, n, seed):
    """A decay term (MUL) over random doubles and a FIELD term (ADD) over a column built so that s * M + x lands EXACTLY on
    the midpoint of two neighbouring floats, for every passage: the fp32 result is then decided by round-half-to-even, and a
    last-bit difference in ANY fp64 operation before it -- a contracted multiply-add in the Horner steps, the range
    reduction, w * v or s * M + A -- moves the sum off the midpoint and, half of the time, the result to the other
    neighbour.  (Random inputs do not show this: a last-bit fp64 difference survives the rounding to fp32 about once in
    2^29 entries.)  -> (columns, program, rows, M)."""
    from hipporag_amd._lib import PAY_F64
    from tests.boost_helpers import _pos, exp_dec_np
    rng = np.random.default_rng(seed)
    z = rng.standard_normal(n) * 50.0
    w, origin, offset = float(rng.uniform(1.1, 1.9)), float(rng.standard_normal()), float(rng.uniform(0, 1))
    c = decay_c(shape, float(rng.uniform(150, 200)), float(rng.uniform(0.4, 0.6)))
    d = _pos(np.abs(z - origin) - offset)
    v = _pos((c - d) / c) if shape == BOOST_LINEAR else exp_dec_np(c * d) if shape == BOOST_EXP else exp_dec_np(c * (d * d))
    M = w * v
    rows = rng.uniform(1.0, 2.0, (1, n)).astype(np.float32)
    p_hi = rows[0].astype(np.float64) * M
    lower = np.where(np.arange(n) % 2 == 0, 2.0 ** -10, 2.0 ** -10 * (1 + 2.0 ** -23))       # an even and an odd lower neighbour
    mid = lower + 2.0 ** -34
    x = mid - p_hi
    assert (p_hi > 2.0 ** -8).all() and (p_hi + x == mid).all()                              # the cancellation is exact
    cols = [(PAY_F64, bits(z), None), (PAY_F64, bits(x), None)]
    prog = assemble_boost([[term(BOOST_DECAY, BOOST_MUL, shape, col=0, w=w, p=(origin, offset, c)),
                            term(BOOST_FIELD, BOOST_ADD, col=1, w=1.0)]])
    return cols, prog, rows, M, x


@pytest.mark.parametrize("shape", [BOOST_LINEAR, BOOST_EXP, BOOST_GAUSS])
def test_a_last_bit_of_any_fp64_operation_would_show_in_the_fp32_result(gpu_device, shape):
    n = 3 * T + 17
    cols, prog, rows, M, x = _midpoint_case(shape, n, 70 + shape)
    want = boost_rows_np(rows, n, cols, prog)
    even = np.arange(n) % 2 == 0
    assert (want[0, even] == np.float32(2.0 ** -10)).all() and (want[0, ~even] == np.float32(2.0 ** -10 * (1 + 2.0 ** -22))).all()
    # the design works: M one ulp up or down changes most results; so does a fused s * M + x (the exact sum is off the midpoint)
    s64 = rows[0].astype(np.float64)
    moved = np.zeros(n, bool)
    for other in (np.nextafter(M, np.inf), np.nextafter(M, -np.inf)):
        moved |= ((s64 * other) + x).astype(np.float32) != want[0]
    assert moved.mean() > 0.5
    ix = _index(cols)
    try:
        _same(_boost(ix, prog, rows)[:, :n], want, f"shape {shape}")
    finally:
        ix.close()


def test_the_min_max_form_reads_the_normalised_entry(indexes):
    """With mn / mx the kernel boosts minmax(s) = (s - mn) / (mx - mn) formed in fp32, a zero range giving 1."""
    n = T + 1
    cols, ix = indexes[n]
    rng = np.random.default_rng(9)
    per = [special_boosts()["mixed"], [], special_boosts()["gauss"], special_boosts()["const everywhere"]]
    prog = assemble_boost(per)
    rows = rng.standard_normal((4, n)).astype(np.float32)
    rows[3] = np.float32(0.375)                                  # a zero range: every entry reads 1
    mn, mx = rows.min(axis=1), rows.max(axis=1)
    want = boost_rows_np(rows, n, cols, prog, mn=mn, mx=mx)
    _same(_boost(ix, prog, rows, mn=mn, mx=mx)[:, :n], want, "min-max")
    _same(want[1], rows[1], "a query without terms keeps its raw row")
    _same(want[3], np.full(n, -3.0, np.float32), "zero range")
    mn[0], mx[0] = np.float32(-0.5), np.float32(0.25)            # any mn / mx: the definition does not care whose they are
    _same(_boost(ix, prog, rows, mn=mn, mx=mx)[:, :n], boost_rows_np(rows, n, cols, prog, mn=mn, mx=mx), "foreign min-max")


def test_boost_rows_rejects_bad_arguments(indexes):
    import torch
    from hipporag_amd._lib import HRAG_EINVAL
    from hipporag_amd.boost import boost_rows, compile_boosts
    L, lib = _L()
    n = 257
    cols, ix = indexes[n]
    prog = assemble_boost([special_boosts()["mixed"]] * 2)
    good, keep = _desc(prog)
    rows = torch.zeros((2, n + 1), dtype=torch.float32, device="cuda")
    mm = torch.zeros((2,), dtype=torch.float32, device="cuda")

    def call(handle=ix._handle, r=rows.data_ptr(), ld=n + 1, batch=2, mn=None, mx=None, desc=good, edit=None):
        if edit:
            desc = L.BoostProgramDesc.from_buffer_copy(good)
            for k, v in edit.items():
                setattr(desc, k, v)
        return lib.hrag_boost_rows(handle, r, ld, batch, mn, mx, C.byref(desc) if desc is not None else None, 0, _stream())
    assert call() == 0 and call(ld=n) == 0 and call(mn=mm.data_ptr(), mx=mm.data_ptr()) == 0
    assert call(edit=dict(n_terms=0, t_ptr=None, t_op=None)) == 0 and call(edit=dict(n_clauses=0, c_col=None, set_nnz=0)) == 0
    bad = {"a NULL handle": dict(handle=None), "NULL rows": dict(r=None), "a NULL program": dict(desc=None),
           "batch 0": dict(batch=0), "batch 65536": dict(batch=65536), "ld below n": dict(ld=n - 1),
           "misaligned rows": dict(r=rows.data_ptr() + 2), "mn without mx": dict(mn=mm.data_ptr()),
           "mx without mn": dict(mx=mm.data_ptr()), "negative n_terms": dict(edit=dict(n_terms=-1)),
           "negative n_clauses": dict(edit=dict(n_clauses=-1)), "negative set_nnz": dict(edit=dict(set_nnz=-1)),
           "terms missing": dict(edit=dict(t_num=None)), "t_ptr missing": dict(edit=dict(t_ptr=None)),
           "clauses missing": dict(edit=dict(c_lo=None)), "set values missing": dict(edit=dict(set_vals=None))}
    for what, kw in bad.items():
        assert call(**kw) == HRAG_EINVAL, what
        assert lib.hrag_last_error()
    torch.cuda.synchronize()
    # the Python side
    pr = compile_boosts(ix, [{"field": "c3", "add": 1.0}])
    with pytest.raises(ValueError, match="rows"):
        boost_rows(ix, rows.double(), pr)
    with pytest.raises(ValueError, match="rows"):
        boost_rows(ix, rows[:, :n - 1], pr)
    with pytest.raises(ValueError, match="both or neither"):
        boost_rows(ix, rows, pr, mn=mm)
    with pytest.raises(ValueError, match="holds 3 queries, the call 2"):
        boost_rows(ix, rows, compile_boosts(ix, [[], [], []]))
    with pytest.raises(ValueError, match="another index"):
        boost_rows(indexes[256][1], torch.zeros((2, 256), dtype=torch.float32, device="cuda"), pr)
    rows.zero_()
    assert boost_rows(ix, rows, pr) is rows
    _same(_np(rows)[:, :n], boost_rows_np(np.zeros((2, n), np.float32), n, cols, pr.arrays(), True), "the binding")


# ---------------------------------------------------------------------------------- the engine calls
BOOSTS = [
    [{"if": {"tag": ["t3", "t7", "t9"]}, "mul": 1.5},
     {"decay": {"field": "year", "origin": 2023, "scale": 5, "offset": 1, "decay": 0.5, "kind": "exp"}, "mul": 1.0, "missing": 0.25},
     {"field": "score", "modifier": "sqrt", "add": 1e-4, "missing": 0.0}],
    [{"if": {"year": {"$lt": 2010}}, "mul": 0.5}, {"field": "score", "add": 2e-5}],
    None,
    [{"decay": {"field": "score", "origin": 0.0, "scale": 0.7, "kind": "gauss"}, "mul": 2.0},
     {"if": {"$not": {"tag": {"$exists": True}}}, "add": -1e-3}],
    [{"if": {"rare": 1}, "add": 10.0}],
    [{"decay": {"field": "year", "origin": 2000, "scale": 10, "kind": "linear"}, "mul": 1.0},
     {"if": {"$any": {"tag": "t1", "year": 2020}}, "mul": 0.0}],
    [],
]


@pytest.fixture(scope="module")
def case(gpu_device):
    """The smallest case tests/test_gpu_payload.py uses: the small-batch, fp16 and e4m3 states at B = 3, 9, 65."""
    from hipporag_amd.engine import HippoRAGEngine, LexicalIndex
    from hipporag_amd.payload import PayloadIndex, encode_columns
    from tests.group_helpers import random_groups
    from tests.lex_helpers import make_index
    kg, pass_bits, fact_bits, _ = make_case(3000, 24000, 64, seed=4141)
    n_p = kg.n_passages
    rng = np.random.default_rng(5)
    eng = HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                         max_batch=130, max_topk=min(200, n_p))
    groups = random_groups(np.random.default_rng(2), n_p, "shuffled")
    eng.set_passage_groups(groups)
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
    yield gpu_device, kg, pass_bits, fact_bits, eng, ix, host, groups
    eng.close()
    ix.close()
    lex.close()


def _bf16(bits_, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits_).view(np.int16)).to(dev).view(torch.bfloat16)


def _gram_fn(pass_dev, n, dim, dev):
    import torch
    L, lib = _L()

    def gram(ids):
        ids = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(dev)
        r, c = ids.shape
        out = torch.zeros((r, c, c), dtype=torch.float32, device=dev)
        if r:
            L.check(lib.hrag_gram_rows(pass_dev.data_ptr(), n, dim, 0, 0, ids.data_ptr(), r, c, out.data_ptr(), c, _stream()))
        return _np(out)
    return gram


FIELDS = ("doc_idx", "doc_score", "group_idx", "hit_idx", "hit_score", "mmr_value")


def _check(out, want, what, rows=None):
    for name in FIELDS:
        g, w = _np(getattr(out, name)), want[name]
        assert (g is None) == (w is None), (what, name)
        if w is not None:
            _same(g if rows is None else g[rows], w, f"{what}: {name}")


def _same_output(a, b, what):
    import torch
    for name in FIELDS + ("flags", "residual", "iters_used"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                               y.view(torch.int32) if y.dtype == torch.float32 else y), (what, name)


@pytest.mark.parametrize("b,want_state", [(3, 4), (9, 2), (65, 8)])
def test_retrieve_with_a_boost_is_the_restatement_over_the_boosted_rows(case, b, want_state):
    """Every output of retrieve(boost=) and its relatives is expected_outputs(boost_rows_np(R), ...), R the last_doc_scores of
    the same call without the boost; flags / residual / iters_used are that call's."""
    import torch
    from hipporag_amd.boost import compile_boosts
    from hipporag_amd.payload import compile_filters
    from tests.lex_helpers import make_queries
    from tests.payload_helpers import payload_filter_np
    dev, kg, pass_bits, fact_bits, eng, ix, host, groups = case
    n, k = kg.n_passages, 20
    cols = cols_for_restatement(host)
    gram = _gram_fn(_bf16(pass_bits, dev).contiguous(), n, 64, dev)
    per = [BOOSTS[i % len(BOOSTS)] for i in range(b)]
    prog = compile_boosts(ix, per)
    assert not prog.broadcast and prog.batch == b
    boosted = lambda R, pr=prog: boost_rows_np(R[:, :n], n, cols, pr.arrays(), pr.broadcast)
    qf = _bf16(synth.make_queries_np(fact_bits, b, seed=500 + b)[0], dev)
    qp = _bf16(synth.make_queries_np(pass_bits, b, seed=501 + b)[0], dev)
    idx, sc = eng.score_facts(qf, k=5)
    cnt = torch.full((b,), 5, dtype=torch.int32, device=dev)
    cnt[::4] = 0                                              # DPR fallback rows
    kept = (idx, sc, cnt)
    pf = compile_filters(ix, {"year": {"$gte": 2005}})
    allowed = np.broadcast_to(payload_filter_np(n, cols, pf.arrays(), 1), (b, n))
    lex_q = make_queries(np.random.default_rng(b), b)
    lex_q = (lex_q[0], lex_q[1], np.where(np.isfinite(lex_q[2]), lex_q[2], 1.0).astype(np.float32))
    ctx = dict(n_passages=n, groups=groups, allowed=None, gram=gram, max_topk=eng.max_topk)
    mmr_rows = np.array(sorted({0, 1, b - 1}))
    variants = [("plain", {}, {}, None), ("payload filter", dict(doc_filter=pf), {}, allowed),
                ("grouped with hits", dict(group_agg="max", group_hits=2), {}, None),
                ("sum groups under the filter", dict(group_agg="sum", group_hits=3, doc_filter=pf), {}, allowed),
                ("mmr", dict(mmr_lambda=0.5, mmr_candidates=40), {}, None),
                ("lexical", {}, dict(lexical=lex_q, lexical_weight=0.3), None)]
    for what, kw, skw, alw in variants:
        plain = eng.retrieve(qp, *kept, k=1, **skw)
        if what == "plain":
            assert eng.stats()["last_ppr_state"] == want_state
        R = _np(eng.last_doc_scores(b))
        out = eng.retrieve(qp, *kept, k=k, boost=prog, **kw, **skw)
        after = _np(eng.last_doc_scores(b))
        RB = boosted(R)
        _same(after[:, :n], RB, f"{what}: the rows on the handle are the boosted rows")
        spec = oh.CallSpec(entry="retrieve", k=k, group_agg=kw.get("group_agg"), group_hits=kw.get("group_hits"),
                           mmr_lambda=kw.get("mmr_lambda"), mmr_candidates=kw.get("mmr_candidates"))
        rows = mmr_rows if "mmr_lambda" in kw else None
        _check(out, oh.expected_outputs(RB, spec, dict(ctx, allowed=alw), rows=rows), (b, what), rows)
        for name in ("flags", "residual", "iters_used"):
            assert torch.equal(getattr(out, name).view(torch.int32), getattr(plain, name).view(torch.int32)), (what, name)
    _same(boosted(R)[[q for q in range(b) if not per[q]]], R[[q for q in range(b) if not per[q]], :n], "queries without terms")
    # one list for the batch; the grammar itself as the argument; retrieve_scored
    one = compile_boosts(ix, BOOSTS[0])
    assert one.broadcast
    eng.retrieve(qp, *kept, k=1)
    R = _np(eng.last_doc_scores(b))
    spec = oh.CallSpec(entry="retrieve", k=k)
    _check(eng.retrieve(qp, *kept, k=k, boost=BOOSTS[0]), oh.expected_outputs(boosted(R, one), spec, ctx), (b, "broadcast"))
    dense = eng.sim_scores("passages", qp)
    eng.retrieve_scored(dense, *kept, k=1)
    R = _np(eng.last_doc_scores(b))
    _check(eng.retrieve_scored(dense, *kept, k=k, boost=prog), oh.expected_outputs(boosted(R), spec, ctx), (b, "scored"))
    # a fusion after a boosted retrieve fuses boosted rows; last_fused(boost=) boosts the fused rows
    if b == 9:
        mp = [0, 4, 9]
        fspec = oh.CallSpec(entry="last_fused", k=k, fuse="sum", member_ptr=mp)
        eng.retrieve(qp, *kept, k=1)
        R = _np(eng.last_doc_scores(b))
        eng.retrieve(qp, *kept, k=k, boost=prog)
        _check(eng.last_fused(mp, fuse="sum", k=k), oh.expected_outputs(boosted(R), fspec, ctx), "fusion of boosted rows")
        for fuse in ("sum", "rrf"):
            fspec = oh.CallSpec(entry="last_fused", k=k, fuse=fuse, member_ptr=mp, group_agg="max", group_hits=2)
            want_f = oh.expected_outputs(R, fspec, ctx)            # (its "fused" rows: what the boost then reads)
            two = compile_boosts(ix, [BOOSTS[0], BOOSTS[3]])
            FB = boost_rows_np(want_f["fused"], n, cols, two.arrays())
            eng.retrieve(qp, *kept, k=1)
            out = eng.last_fused(mp, fuse=fuse, k=k, group_agg="max", group_hits=2, boost=two)
            _same(_np(eng.last_doc_scores(2))[:, :n], FB, f"{fuse}: the boosted fused rows")
            _check(out, oh.expected_outputs(FB, oh.CallSpec(entry="retrieve", k=k, group_agg="max", group_hits=2), ctx),
                   f"last_fused(boost=) {fuse}")
    # the convergence contract: every run boosts its own rows by its own program rows
    plain = eng.retrieve_converged(qp, *kept, k=k, ppr_tol=1.5e-6, ppr_max_iters=60, want_all_scores=True)
    pend = eng.retrieve_converged_start(qp, *kept, k=k, ppr_tol=1.5e-6, ppr_max_iters=60, want_all_scores=True, boost=prog)
    out = pend.finish()
    RB = boosted(_np(plain.all_scores))
    _same(_np(out.all_scores)[:, :n], RB, "contract: all_scores are the boosted rows")
    _check(out, oh.expected_outputs(RB, spec, ctx), (b, "contract"))
    assert torch.equal(out.flags, plain.flags) and torch.equal(out.iters_used, plain.iters_used)
    # a workspace shares the root's payload index
    if b == 9:
        ws = eng.workspace()
        try:
            eng.retrieve(qp, *kept, k=1)
            R = _np(eng.last_doc_scores(b))
            _check(ws.retrieve(qp, *kept, k=k, boost=prog), oh.expected_outputs(boosted(R), spec, ctx), "workspace")
            _same(_np(ws.last_doc_scores(b))[:, :n], boosted(R), "workspace rows")
            _same(_np(eng.last_doc_scores(b))[:, :n], R[:, :n], "the root's rows are its own")
        finally:
            ws.close()
    # dense_retrieve(boost=): numpy min-max + boost + rank_rows, under the filter too
    raw = _np(dense)[:, :n]
    mn, mx = raw.min(axis=1), raw.max(axis=1)
    DB = boost_rows_np(raw, n, cols, prog.arrays(), mn=mn, mx=mx)
    for flt, alw in ((None, None), (pf, allowed)):
        gi, gs = eng.dense_retrieve(qp, k=k, boost=prog, doc_filter=flt)
        wi, wsc = oh.rank_rows(DB, k, alw)
        _same(_np(gi), wi, "dense ids")
        _same(_np(gs), wsc, "dense scores")
    # Engine.boost_rows on any rows, and last_boosted twice boosts twice
    mine = torch.from_numpy(raw.copy()).to(dev)
    assert eng.boost_rows(mine, prog) is mine
    _same(_np(mine), boost_rows_np(raw, n, cols, prog.arrays()), "Engine.boost_rows")
    eng.retrieve(qp, *kept, k=1)
    R = _np(eng.last_doc_scores(b))
    eng.last_boosted(one, b, k=k)
    out = eng.last_boosted(one, b, k=k)
    _check(out, oh.expected_outputs(boosted(boosted(R, one), one), spec, ctx), "twice")


@pytest.mark.parametrize("b,want_state", [(9, 2), (65, 8)])
def test_the_contract_repeats_boost_each_row_by_its_own_program(gpu_device, b, want_state):
    """retrieve_converged(boost= one program per query) when finish() repeats SOME rows: the ring of
    tests/test_gpu_fp8_adversarial.py mixes slowly and the shortest sweep count its state runs on (12 on the fp16 state, 20
    on the e4m3 one; plus the 9 the device adds) does not reach ppr_tol, so PPR rows are flagged and repeated on the fp32 state, while the DPR-fallback rows (every fourth, row 0 among them)
    converge at once and are not.  The repeat runs rows [1, 2, 3, 5, ...] of the batch and must boost them by the
    programs of exactly those queries (BoostProgram.select) under exactly their filter rows: each query adds its own
    constant to its own set of passages, so a row boosted by a neighbour's program differs in every entry.  Every row of
    all_scores is boost_rows_np of the unboosted contract's row, and the ranked outputs are the restatement over them."""
    import torch
    from hipporag_amd._lib import FLAG_NOT_CONVERGED
    from hipporag_amd.boost import compile_boosts
    from hipporag_amd.engine import HippoRAGEngine
    from hipporag_amd.payload import PayloadIndex, encode_columns
    from tests.group_helpers import random_groups
    from tests.payload_helpers import columns_of, random_metadata
    from tests.test_gpu_fp8_adversarial import CASES, _index
    make, damping, _ = CASES["ring"]
    n_v, src, dst, w, pv, pinned = make()
    csr, pass_bits, fact_bits, index = _index(n_v, src, dst, w, pv, 64, seed=11, pinned_facts=pinned)
    n, k, tol, iters = len(pv), 20, 1.5e-6, (12 if b <= 64 else 20)
    rng = np.random.default_rng(31 + b)
    host = encode_columns(columns_of(random_metadata(rng, n), ["year", "user", "score", "flag", "mixed"]), n)
    cols = cols_for_restatement(host)
    groups = random_groups(rng, n, "shuffled")
    per = [[{"if": {"year": {"$gte": 2018 + q % 6}}, "add": 1.0 + q}, {"mul": 1.0 + q / 64.0}] for q in range(b)]
    allowed = rng.random((b, n)) < 0.5
    qf = _bf16(synth.make_queries_np(fact_bits, b, seed=5)[0], gpu_device)
    qp = _bf16(synth.make_queries_np(pass_bits, b, seed=6)[0], gpu_device)
    ix = PayloadIndex(host)
    try:
        with HippoRAGEngine(csr, index.passage_vertex, pass_bits, fact_bits, index.subj_vertex, index.obj_vertex,
                            index.num_chunks, max_batch=b, max_topk=n) as eng:
            eng.set_payload_index(ix)
            eng.set_passage_groups(groups)
            prog = compile_boosts(ix, per)
            assert not prog.broadcast and prog.batch == b
            gram = _gram_fn(_bf16(pass_bits, gpu_device).contiguous(), n, 64, gpu_device)
            idx, sc = eng.score_facts(qf, k=5)
            cnt = torch.full((b,), 5, dtype=torch.int32, device=gpu_device)
            cnt[::4] = 0                                          # DPR fallback rows
            kw = dict(damping=damping, ppr_iters=iters, ppr_tol=tol, ppr_max_iters=400, want_all_scores=True)
            first = eng.retrieve(qp, idx, sc, cnt, damping=damping, ppr_iters=iters, ppr_tol=tol, ppr_max_iters=400, k=1)
            assert eng.stats()["last_ppr_state"] == want_state
            late = (_np(first.flags) & FLAG_NOT_CONVERGED) != 0   # what finish() will repeat: some rows, not all
            assert late.any() and not late.all() and not late[::4].any(), late
            assert not np.array_equal(np.flatnonzero(late), np.arange(late.sum()))     # (the repeat's rows are not 0 .. r - 1)
            flt = torch.from_numpy(allowed).to(gpu_device)
            for what, okw, alw in (("plain", {}, None),
                                   ("grouped, hits, a filter per query", dict(group_agg="sum", group_hits=2, doc_filter=flt), allowed),
                                   ("mmr", dict(mmr_lambda=0.5, mmr_candidates=40), None)):
                plain = eng.retrieve_converged(qp, idx, sc, cnt, k=k, **kw, **okw)
                pend = eng.retrieve_converged_start(qp, idx, sc, cnt, k=k, boost=prog, **kw, **okw)
                out = pend.finish()
                torch.cuda.synchronize()
                used = _np(out.iters_used)
                assert pend.repeated and len(np.unique(used)) > 1, (what, used)       # repeats happened, on a strict subset
                assert (used[late] > used[~late].max()).all() and not (_np(out.flags) & FLAG_NOT_CONVERGED).any(), (what, used)
                assert torch.equal(out.flags, plain.flags) and torch.equal(out.iters_used, plain.iters_used), what
                assert torch.equal(out.residual.view(torch.int32), plain.residual.view(torch.int32)), what
                R = _np(plain.all_scores)[:, :n]
                RB = boost_rows_np(R, n, cols, prog.arrays())
                got = _np(out.all_scores)[:, :n]
                for q in range(b):                                # row by row: its own program, nobody else's
                    _same(got[q], RB[q], f"{what}: all_scores row {q} ({'repeated' if late[q] else 'first run'})")
                    other = boost_rows_np(R[q:q + 1], n, cols, compile_boosts(host, [per[(q + 1) % b]]).arrays())[0]
                    assert not np.array_equal(other.view(np.uint32), RB[q].view(np.uint32)), q
                spec = oh.CallSpec(entry="retrieve_converged", k=k, group_agg=okw.get("group_agg"), group_hits=okw.get("group_hits"),
                                   mmr_lambda=okw.get("mmr_lambda"), mmr_candidates=okw.get("mmr_candidates"))
                rows = np.array(sorted({0, 1, 2, b - 1})) if "mmr_lambda" in okw else None
                ctx = dict(n_passages=n, groups=groups, allowed=alw, gram=gram, max_topk=n)
                _check(out, oh.expected_outputs(RB, spec, ctx, rows=rows), (b, what), rows)
    finally:
        ix.close()


def test_a_boost_without_terms_is_the_plain_call_and_errors_name_the_argument(case):
    import torch
    from hipporag_amd.boost import compile_boosts
    from hipporag_amd.engine import CapturedPipeline
    from hipporag_amd.payload import PayloadIndex
    dev, kg, pass_bits, fact_bits, eng, ix, host, groups = case
    b, k = 9, 20
    qf = _bf16(synth.make_queries_np(fact_bits, b, seed=77)[0], dev)
    qp = _bf16(synth.make_queries_np(pass_bits, b, seed=78)[0], dev)
    idx, sc = eng.score_facts(qf, k=5)
    cnt = torch.full((b,), 5, dtype=torch.int32, device=dev)
    cnt[::4] = 0
    for none in ([], [None] * b, [[] for _ in range(b)], compile_boosts(ix, [])):
        for kw in ({}, dict(group_agg="max", group_hits=2), dict(mmr_lambda=0.3, mmr_candidates=30)):
            want = eng.retrieve(qp, idx, sc, cnt, k=k, **kw)
            R = eng.last_doc_scores(b)
            _same_output(eng.retrieve(qp, idx, sc, cnt, k=k, boost=none, **kw), want, ("no terms", kw))
            assert torch.equal(eng.last_doc_scores(b).view(torch.int32), R.view(torch.int32))      # -0.0 and NaN bits included
        for x, y in zip(eng.dense_retrieve(qp, k=k, boost=none), eng.dense_retrieve(qp, k=k)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    some = [{"field": "score", "add": 1.0}]
    for name, kw in (("group_agg", dict(group_agg="max", group_hits=2)), ("group_hits", dict(group_hits=2)),
                     ("mmr_lambda", dict(mmr_lambda=0.5, mmr_candidates=30)), ("mmr_candidates", dict(mmr_candidates=30)),
                     ("lexical", dict(lexical=(np.zeros(b + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))))):
        with pytest.raises(ValueError, match=f"dense_retrieve\\(boost=\\) does not serve {name}"):
            eng.dense_retrieve(qp, k=k, boost=some, **kw)
    with pytest.raises(ValueError, match="filter_scope"):
        eng.dense_retrieve(qp, k=k, boost=some, doc_filter=torch.ones(kg.n_passages, dtype=torch.bool), filter_scope="seeds")
    with pytest.raises(ValueError, match="boost: the BoostProgram holds 4 queries, the call 9"):
        eng.retrieve(qp, idx, sc, cnt, k=k, boost=compile_boosts(ix, [some] * 4))
    with pytest.raises(ValueError, match="unknown field 'nope'"):
        eng.retrieve(qp, idx, sc, cnt, k=k, boost=[{"field": "nope", "add": 1.0}])
    other = PayloadIndex.from_columns({"year": [1, 2, 3]}, 3)
    try:
        with pytest.raises(ValueError, match="another index"):
            eng.retrieve(qp, idx, sc, cnt, k=k, boost=compile_boosts(other, [{"field": "year", "add": 1.0}]))
    finally:
        other.close()
    with pytest.raises(NotImplementedError, match="boost"):
        CapturedPipeline(eng, 1, boost=some)
    with pytest.raises(NotImplementedError, match="boost"):
        eng.shard_finish(None, None, None, k, boost=some)
    L, lib = _L()
    d, keep = _desc(compile_boosts(ix, some).arrays())
    o = torch.zeros((b, k), dtype=torch.int32, device=dev)
    s = torch.zeros((b, k), dtype=torch.float32, device=dev)
    args = lambda batch=b, kk=k, pay=ix._handle: (eng._handle, pay, batch, C.byref(d), 1, kk, None, 0, -1, o.data_ptr(),
                                                   s.data_ptr(), None, None, None, _stream())
    eng.retrieve(qp[:4], idx[:4], sc[:4], cnt[:4], k=k)
    from hipporag_amd._lib import HRAG_EINVAL
    assert lib.hrag_last_boosted(*args(batch=5)) == HRAG_EINVAL and b"exceeds the 4 queries" in lib.hrag_last_error()
    assert lib.hrag_last_boosted(*args(batch=4, kk=0)) == HRAG_EINVAL
    assert lib.hrag_last_boosted(*args(batch=4, pay=None)) == HRAG_EINVAL
    assert lib.hrag_last_boosted(*args(batch=4)) == 0
    eng.dense_retrieve(qp, k=k)                                  # (an ungrouped dense call leaves the rows as they were)
    eng.set_payload_index(None)
    try:
        with pytest.raises(ValueError, match="boost needs a payload index on this engine \\(set_payload_index\\)"):
            eng.retrieve(qp, idx, sc, cnt, k=k, boost=some)
        with pytest.raises(ValueError, match="set_payload_index"):
            eng.dense_retrieve(qp, k=k, boost=some)
        with pytest.raises(ValueError, match="set_payload_index"):
            eng.boost_rows(torch.zeros((1, kg.n_passages), device=dev), some)
    finally:
        eng.set_payload_index(ix)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------- the mirror
META = [("s1", {"user": "alice", "year": 2020}), ("s2", {"user": "bob", "year": 2021}), ("s1", {"user": "alice", "year": 2021}),
        (None, {"year": 2022}), ("s3", {"user": "carol"})]        # the metadata of tests/test_gpu_payload.py's mirror


def _mirror(payload_index, **cfg):
    from hipporag_amd.retriever import Chunk, HippoRAG, RetrievalConfig
    from tests.golden.make_golden import DOCS, TRIPLES, MockEmbeddingModel
    chunks = [Chunk(d, source_id=META[i % 5][0], metadata=dict(META[i % 5][1], page=i)) for i, d in enumerate(DOCS)]
    rag = HippoRAG(RetrievalConfig(max_batch=4, retrieval_top_k=len(DOCS) + 3, embedding_precision="bf16",
                                   payload_index=payload_index, **cfg), embedding_model=MockEmbeddingModel())
    rag.index_from_openie(chunks, TRIPLES)
    return rag


def test_the_mirror_boosts_by_the_chunk_metadata(gpu_device):
    from hipporag_amd.boost import compile_boosts
    from tests.golden.make_golden import QUERIES
    on, off = _mirror(True), _mirror(False)
    n = len(on.passage_node_keys)
    full = on.retrieve(QUERIES, num_to_retrieve=n)
    assert all("boosted" not in d for r in full for d in r.doc_metadata)
    text_src = {on.passage_texts[i]: on.chunk_metadata[key].get("source_id") for i, key in enumerate(on.passage_node_keys)}
    # mul 0 on one source: its passages (score 0) go behind every other one, which keep their order and their scores
    got = on.retrieve(QUERIES, num_to_retrieve=n, boost=[{"if": {"source_id": "s1"}, "mul": 0}])
    n_s1 = sum(1 for s in text_src.values() if s == "s1")
    assert n_s1 >= 2
    for g, w in zip(got, full):
        assert all(d["boosted"] is True for d in g.doc_metadata)
        assert {text_src[d] for d in g.docs[-n_s1:]} == {"s1"} and (np.asarray(g.doc_scores[-n_s1:]) == 0).all()
        assert g.docs[:-n_s1] == [d for d in w.docs if text_src[d] != "s1"]
        assert (np.asarray(w.doc_scores) > 0).all()              # (what "behind all others" rests on)
    # a recency decay reorders otherwise tied chunks as the restatement says: every score is zeroed, then the decay of its
    # page is added, so the decay alone breaks the tie
    from hipporag_amd.payload import encode_columns
    recency = [{"mul": 0.0}, {"decay": {"field": "page", "origin": 0, "scale": 3, "kind": "exp"}, "add": 1.0}]
    got = on.retrieve(QUERIES[:2], num_to_retrieve=n, boost=recency)
    cols = cols_for_restatement(encode_columns(on.payload_columns(), n))
    want = boost_rows_np(np.ones((1, n), np.float32), n, cols, compile_boosts(on.payload_index, recency).arrays(), True)[0]
    order = oh.rank_rows(want[None], n)[0][0]
    assert len(set(want.tolist())) == n
    for g in got:
        assert g.docs == [on.passage_texts[i] for i in order]
        _same(np.asarray(g.doc_scores, np.float32), want[order], "the mirror's scores")
    # per-query lists, the config default, retrieve_dpr, rag_qa's path, and the refusals
    per = [[{"if": {"source_id": "s1"}, "mul": 0}] if i % 2 else None for i in range(len(QUERIES))]
    got = on.retrieve(QUERIES, num_to_retrieve=n, boost=per)
    for i, (g, w) in enumerate(zip(got, full)):
        assert g.docs == (w.docs if not i % 2 else [d for d in w.docs if text_src[d] != "s1"] + g.docs[-n_s1:])
    cfg = _mirror(True, boost=[{"if": {"source_id": "s1"}, "mul": 0}])
    for g, w in zip(cfg.retrieve(QUERIES, num_to_retrieve=n), on.retrieve(QUERIES, num_to_retrieve=n,
                                                                         boost=[{"if": {"source_id": "s1"}, "mul": 0}])):
        assert g.docs == w.docs
    dpr = on.retrieve_dpr(QUERIES, num_to_retrieve=n, boost=[{"if": {"source_id": "s1"}, "add": -10.0}])
    for g, w in zip(dpr, on.retrieve_dpr(QUERIES, num_to_retrieve=n)):
        assert g.docs[:-n_s1] == [d for d in w.docs if text_src[d] != "s1"] and all(d["boosted"] for d in g.doc_metadata)
    with pytest.raises(ValueError, match="payload_index"):
        off.retrieve(QUERIES, boost=[{"mul": 2.0}])
    with pytest.raises(ValueError, match="payload_index"):
        off.retrieve_dpr(QUERIES, boost=[{"mul": 2.0}])
    with pytest.raises(ValueError, match="boost"):
        on.retrieve_fused([[QUERIES[0], QUERIES[1]]], boost=[{"mul": 2.0}])
    with pytest.raises(ValueError, match="retrieve_dpr does not serve boost with group_by"):
        on.retrieve_dpr(QUERIES, boost=[{"mul": 2.0}], group_by="source_id", group_agg="max")
