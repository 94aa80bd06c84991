"""Payload filters, host side (hipporag_amd/payload.py, the bindings, the mirror's argument plumbing): nothing here touches
a device.  The grammar is held to the numpy restatement of tests/payload_helpers.py and, for equality dicts, to the mirror's
host path HippoRAG._filter_words."""

import math
import os
import re

import numpy as np
import pytest

from hipporag_amd._lib import (PAY_F64, PAY_I64, PAY_IN, PAY_MAX_CLAUSES, PAY_MAX_COLS, PAY_MUST, PAY_MUST_NOT, PAY_PRESENT,
                               PAY_RANGE, PAY_SHOULD, PAY_TILE)
from hipporag_amd.payload import I64_MAX, I64_MIN, PayloadFilter, compile_filters, encode_columns, f64_bits
from tests.payload_helpers import (assemble, cols_for_restatement, make_columns, payload_filter_np, payload_words_np,
                                   popcount_rows_np, random_metadata, special_programs)

NEW = ("hrag_payload_create", "hrag_payload_destroy", "hrag_payload_filter", "hrag_bitset_count_rows")


def test_symbols_are_declared_bound_and_exported():
    from hipporag_amd import _lib
    hdr = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "hrag.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and re.search(r"hrag_status " + name + r"\(", hdr) and getattr(lib, name) is not None
    for name, value in (("TILE", PAY_TILE), ("MAX_CLAUSES", PAY_MAX_CLAUSES), ("MAX_COLS", PAY_MAX_COLS), ("I64", PAY_I64),
                        ("F64", PAY_F64), ("MUST", PAY_MUST), ("MUST_NOT", PAY_MUST_NOT), ("SHOULD", PAY_SHOULD),
                        ("RANGE", PAY_RANGE), ("IN", PAY_IN), ("PRESENT", PAY_PRESENT)):
        assert int(re.search(rf"#define HRAG_PAY_{name} (\d+)", hdr).group(1)) == value, name
    assert (PAY_TILE, PAY_MAX_CLAUSES, PAY_MAX_COLS) == (2048, 64, 256)
    assert _lib.HRAG_VERSION == 8 and lib.hrag_version() == 8


# ---------------------------------------------------------------------------------- columns
def test_from_columns_type_inference_and_rejections():
    pc = encode_columns({"i": [1, None, True, -(2 ** 63)], "f": [1.5, None, float("nan"), float("inf")],
                         "mix": [1, 2.5, None, 2 ** 53], "s": ["b", "a", None, "b"], "none": [None] * 4,
                         "np_i": np.arange(4, dtype=np.int32), "np_f": np.array([0.5, np.nan, 1, 2], np.float32)}, 4)
    assert pc.columns == {"i": "i64", "f": "f64", "mix": "f64", "s": "keyword", "none": "i64", "np_i": "i64", "np_f": "f64"}
    assert pc.types == [PAY_I64, PAY_F64, PAY_F64, PAY_I64, PAY_I64, PAY_I64, PAY_F64]
    assert pc.values[0].tolist() == [1, 0, 1, I64_MIN] and pc.present[0].tolist() == [0b1101]
    assert pc.values[2].view(np.float64).tolist() == [1.0, 2.5, 0.0, float(2 ** 53)]
    assert pc.vocab == {"s": {"a": 0, "b": 1}} and pc.values[3].tolist() == [1, 0, 0, 1] and pc.present[3].tolist() == [0b1011]
    assert pc.present[4].tolist() == [0] and pc.present[5] is None and pc.present[6] is None
    assert np.isnan(pc.values[6].view(np.float64)[1]) and all(v.dtype == np.int64 for v in pc.values)
    for col, msg in (([1, "a"], "mixes str"), (["a", 2.5], "mixes str"), ([[1], None], "type list"), ([{}, 1], "type dict"),
                     ([1.5, 2 ** 53 + 1], "beyond 2\\^53"), ([2 ** 63, 1], "outside int64"), ([1, 2, 3], "3 values for 2"),
                     ([b"x", None], "type bytes")):
        with pytest.raises(ValueError, match=f"column 'bad'.*{msg}"):
            encode_columns({"bad": col}, 2)
    with pytest.raises(ValueError, match="n_passages"):
        encode_columns({}, 0)
    with pytest.raises(ValueError, match="PAY_MAX_COLS"):
        encode_columns({f"c{i}": [1] for i in range(PAY_MAX_COLS + 1)}, 1)
    assert encode_columns({}, 3).names == []


# ---------------------------------------------------------------------------------- the grammar
@pytest.fixture(scope="module")
def index():
    return encode_columns({"year": [2020, 2021, None, 2022], "user": ["alice", "bob", "alice", None],
                           "x": [1.5, 2, None, -0.0], "flag": [True, False, None, True]}, 4)


def _clauses(index, f):
    pf = compile_filters(index, f)
    assert isinstance(pf, PayloadFilter) and pf.broadcast == isinstance(f, dict)
    out = []
    for j in range(pf.n_clauses):
        s = pf.set_vals[pf.c_set_ptr[j]:pf.c_set_ptr[j + 1]].tolist()
        out.append((int(pf.c_col[j]), int(pf.c_op[j]) & 0xFF, int(pf.c_op[j]) >> 8, int(pf.c_lo[j]), int(pf.c_hi[j]), s))
    return out, pf


def test_every_form_of_the_grammar_compiles_to_the_expected_clauses(index):
    M, MN, S, R, I, P = PAY_MUST, PAY_MUST_NOT, PAY_SHOULD, PAY_RANGE, PAY_IN, PAY_PRESENT
    assert _clauses(index, {"year": 2021})[0] == [(0, M, I, 0, 0, [2021])]
    for alts in ([2022, 2020], (2020, 2022), {2020, 2022}, frozenset([2020, 2022, 2020])):
        assert _clauses(index, {"year": alts})[0] == [(0, M, I, 0, 0, [2020, 2022])]                 # sorted, unique
    assert _clauses(index, {"year": {"$gte": 2021}})[0] == [(0, M, R, 2021, I64_MAX, [])]
    assert _clauses(index, {"year": {"$gt": 2020, "$lt": 2022}})[0] == [(0, M, R, 2021, 2021, [])]   # ONE range
    assert _clauses(index, {"year": {"$exists": True}})[0] == [(0, M, P, 0, 0, [])]
    assert _clauses(index, {"year": {"$exists": False}})[0] == [(0, MN, P, 0, 0, [])]
    assert _clauses(index, {"$not": {"user": "bob", "year": {"$lte": 2020}}})[0] == [(1, MN, I, 0, 0, [1]),
                                                                                    (0, MN, R, I64_MIN, 2020, [])]
    assert _clauses(index, {"$not": {"year": {"$exists": False}}})[0] == [(0, M, P, 0, 0, [])]
    assert _clauses(index, {"$any": {"user": ["alice", "bob"], "flag": True}})[0] == [(1, S, I, 0, 0, [0, 1]), (3, S, I, 0, 0, [1])]
    got, pf = _clauses(index, {"user": "alice", "year": {"$gte": 2020, "$exists": True}, "$not": {"flag": False}})
    assert got == [(1, M, I, 0, 0, [0]), (0, M, P, 0, 0, []), (0, M, R, 2020, I64_MAX, []), (3, MN, I, 0, 0, [0])]
    assert pf.batch == 1 and pf.f_ptr.tolist() == [0, 4] and pf.c_set_ptr.tolist() == [0, 1, 1, 1, 2]
    assert [a.dtype for a in pf.arrays()] == [np.int32, np.int32, np.int32, np.int64, np.int64, np.int32, np.int64]
    # a list: one program per query, None and {} without clauses
    pf = compile_filters(index, [{"year": 2020}, None, {}, {"user": "bob", "flag": [True, False]}])
    assert not pf.broadcast and pf.batch == 4 and pf.f_ptr.tolist() == [0, 1, 1, 1, 3] and pf.set_vals.tolist() == [2020, 1, 0, 1]
    assert compile_filters(index, {}).n_clauses == 0


def test_bound_conversion(index):
    def rng(cond, field="year"):
        (c,), _ = _clauses(index, {field: cond})
        return c[3], c[4]
    assert rng({"$gt": 3.5}) == (4, I64_MAX) and rng({"$lte": 3.5}) == (I64_MIN, 3)
    assert rng({"$gte": 3.5}) == (4, I64_MAX) and rng({"$lt": 3.5}) == (I64_MIN, 3)
    assert rng({"$gt": 3}) == (4, I64_MAX) and rng({"$gte": 3}) == (3, I64_MAX) and rng({"$lt": 3}) == (I64_MIN, 2)
    assert rng({"$gt": -3.5}) == (-3, I64_MAX) and rng({"$lt": -3.5}) == (I64_MIN, -4) and rng({"$gte": True}) == (1, I64_MAX)
    # saturation at the int64 limits; what no int64 satisfies is a clause that hits nothing (lo > hi)
    assert rng({"$gt": -2 ** 70}) == (I64_MIN, I64_MAX) and rng({"$lte": 2 ** 70}) == (I64_MIN, I64_MAX)
    assert rng({"$gte": -1e30, "$lte": 1e30}) == (I64_MIN, I64_MAX) and rng({"$lt": float("inf")}) == (I64_MIN, I64_MAX)
    assert rng({"$gte": I64_MAX}) == (I64_MAX, I64_MAX) and rng({"$lte": I64_MIN}) == (I64_MIN, I64_MIN)
    for cond in ({"$gt": I64_MAX}, {"$gte": 2 ** 70}, {"$lt": I64_MIN}, {"$gt": float("inf")}, {"$lte": -float("inf")},
                 {"$gt": 5, "$lt": 6}, {"$gte": 7, "$lte": 6}):
        lo, hi = rng(cond)
        assert lo > hi, cond
    # F64: nextafter; the bounds are the doubles' bit patterns
    f = lambda cond: tuple(np.array(rng(cond, "x"), np.int64).view(np.float64).tolist())
    assert f({"$gt": 1.5}) == (math.nextafter(1.5, math.inf), math.inf) and f({"$gte": 1.5}) == (1.5, math.inf)
    assert f({"$lt": 1.5}) == (-math.inf, math.nextafter(1.5, -math.inf)) and f({"$lte": 2}) == (-math.inf, 2.0)
    assert f({"$gt": 0.0}) == (5e-324, math.inf) and f({"$gt": -0.0}) == (5e-324, math.inf) and f({"$lt": 0.0})[1] == -5e-324
    lo, hi = rng({"$gte": -0.0, "$lte": 0.0}, "x")
    assert (lo, hi) == (f64_bits(-0.0), f64_bits(0.0)) and lo == I64_MIN                 # the sign bit travels
    assert f({"$gt": 2 ** 53 + 1}) == (float(2 ** 53 + 2), math.inf) and f({"$gte": 2 ** 53 + 1})[0] == float(2 ** 53 + 2)
    assert f({"$lte": 2 ** 53 + 1})[1] == float(2 ** 53) and f({"$gte": -math.inf, "$lte": math.inf}) == (-math.inf, math.inf)
    assert f({"$gt": 10 ** 400}) == (math.inf, math.inf) and f({"$gt": math.inf})[0] > f({"$gt": math.inf})[1]   # inf > 10^400
    assert f({"$gte": math.inf}) == (math.inf, math.inf)


def test_value_handling_keeps_pythons_equality(index):
    def s(field, v):
        (c,), _ = _clauses(index, {field: v})
        return c[5]
    assert s("user", "alice") == [0] and s("user", "zed") == [] and s("user", ["zed", "bob", 3, None, 2.5]) == [1]
    assert s("user", ("a", "b")) == []                    # a tuple is a list of alternatives, none of them known
    assert s("year", True) == [1] and s("year", 2020.0) == [2020] and s("year", 2020.5) == [] and s("year", "2020") == []
    assert s("year", [float("nan"), float("inf"), 2 ** 63, None, 2021]) == [2021]
    assert s("flag", 1) == [1] and s("flag", 1.0) == [1] and s("flag", [True, 0]) == [0, 1] and s("flag", False) == [0]
    fs = lambda v: np.array(s("x", v), np.int64).view(np.float64).tolist()
    assert fs(2) == [2.0] and fs(True) == [1.0] and fs(float("nan")) == [] and fs("1.5") == [] and fs(2 ** 53 + 1) == []
    assert fs([1.5, 1.5, -math.inf]) == [-math.inf, 1.5] and len(fs([0.0, -0.0])) == 1
    assert s("year", {"a": 1}) == [] and s("year", {}) == []         # a plain dict value: nothing a column holds equals it
    # a value the column cannot hold hits nothing -- and therefore everything under $not
    pc = index
    cols = cols_for_restatement(pc)
    for f, want in (({"user": "zed"}, [0, 0, 0, 0]), ({"$not": {"user": "zed"}}, [1, 1, 1, 1]),
                    ({"$not": {"year": 2020.5}}, [1, 1, 1, 1]), ({"x": 0}, [0, 0, 0, 1]), ({"x": [0.0, 2]}, [0, 1, 0, 1]),
                    ({"$not": {"user": "bob"}}, [1, 0, 1, 1]), ({"user": {"$exists": False}}, [0, 0, 0, 1]),
                    ({"$any": {"year": 2020, "user": "bob"}}, [1, 1, 0, 0]), ({"x": {"$gte": 0}}, [1, 1, 0, 1]),
                    ({"x": {"$gt": 0}}, [1, 1, 0, 0]), ({"year": {"$gt": 2020.5, "$lt": 2022}}, [0, 1, 0, 0])):
        got = payload_filter_np(4, cols, compile_filters(pc, f).arrays(), 1)[0]
        assert got.tolist() == [bool(v) for v in want], f


def test_compile_errors_name_the_key(index):
    for f, exc, msg in (({"x": {"$gt": float("nan")}}, ValueError, "'x'.*NaN"), ({"user": {"$gte": "a"}}, ValueError, "'user'.*keyword"),
                        ({"user": {"$gt": 1}}, ValueError, "'user'.*keyword column"), ({"colour": "red"}, ValueError, "unknown field 'colour'"),
                        ({"$not": {"colour": 1}}, ValueError, "unknown field 'colour'"), ({"$or": {"year": 1}}, ValueError, "unknown operator '\\$or'"),
                        ({"year": {"$ne": 1}}, ValueError, "'year'.*unknown operator '\\$ne'"), ({"year": {"$gt": "1"}}, ValueError, "'year'.*number"),
                        ({"$not": {"$any": {"year": 1}}}, ValueError, "'\\$any' inside \\$not"), ({"$any": [1]}, ValueError, "\\$any takes a dict"),
                        ({"year": {"$exists": 1}}, ValueError, "'year'.*\\$exists takes a bool"),
                        ({"$any": {"year": {"$exists": False}}}, ValueError, "'year'.*\\$any"),
                        ({"year": {"$gt": 1, "gt": 2}}, ValueError, "'year'.*unknown operator 'gt'")):
        with pytest.raises(exc, match=msg):
            compile_filters(index, f)
    with pytest.raises(TypeError, match="filters"):
        compile_filters(index, "year=1")
    with pytest.raises(TypeError, match=r"doc_filter\[1\]"):
        compile_filters(index, [None, 3])
    with pytest.raises(ValueError, match="empty list"):
        compile_filters(index, [])
    wide = encode_columns({f"c{i}": [i] for i in range(PAY_MAX_CLAUSES + 1)}, 1)
    compile_filters(wide, {f"c{i}": i for i in range(PAY_MAX_CLAUSES)})                  # exactly the cap
    with pytest.raises(ValueError, match=r"doc_filter\[1\]: 65 clauses.*PAY_MAX_CLAUSES"):
        compile_filters(wide, [None, {f"c{i}": i for i in range(PAY_MAX_CLAUSES + 1)}])


# ---------------------------------------------------------------------------------- the restatement itself
def test_the_restatement_follows_the_headers_rules():
    rng = np.random.default_rng(1)
    n = 100
    cols = make_columns(rng, n)
    sp = special_programs()
    names = list(sp)
    got = payload_filter_np(n, cols, assemble(list(sp.values())), len(sp))
    row = lambda name: got[names.index(name)]
    a, pa = cols[0][1], cols[0][2]
    f, pf = cols[1][1].view(np.float64), cols[1][2]
    assert row("empty").all() and not row("empty set").any() and row("empty set, must_not").all()
    np.testing.assert_array_equal(row("must"), pa & (a >= -2) & (a <= 3))
    np.testing.assert_array_equal(row("must_not"), ~row("must"))
    np.testing.assert_array_equal(row("must_not of a missing value"), ~pa)
    np.testing.assert_array_equal(row("64 clauses"), pa & (cols[2][1] < 500))
    np.testing.assert_array_equal(row("65 clauses"), pa)
    np.testing.assert_array_equal(row("1000 values"), cols[2][1] % 2 == 0)
    assert not row("lo > hi").any() and not row("lo > hi, f64").any() and row("nan bound").all()
    np.testing.assert_array_equal(row("full range"), pa)
    np.testing.assert_array_equal(row("full range, f64"), pf & ~np.isnan(f))
    np.testing.assert_array_equal(row("zeros"), pf & (f == 0))
    assert row("zeros").sum() > (pf & (f == 0) & ~np.signbit(f)).sum() > 0, "-0.0 matches 0.0"
    np.testing.assert_array_equal(row("negative zero bounds"), row("zeros"))
    np.testing.assert_array_equal(row("nan in no set"), pf & (np.isinf(f) | (f == 5e-324)))
    assert not row("column out of range").any() and row("negative column, must_not").all()
    assert row("unknown kind").sum() == 0 and not row("unknown role").any() and not row("high op bits").any()
    np.testing.assert_array_equal(row("extremes"), pa & (np.abs(a.astype(np.float64)) > 10))
    # the cap, the clamps, the base
    assert payload_filter_np(n, cols, assemble([sp["65 clauses"]]), 1, cap=65).sum() == 0
    prog = list(assemble([sp["must"], sp["must_not"]]))
    prog[0] = np.array([-4, 1, 0], np.int32)                         # clamped: [0, 1) and the empty [1, 1)
    got2 = payload_filter_np(n, cols, prog, 2)
    np.testing.assert_array_equal(got2[0], row("must"))
    assert got2[1].all()
    base = rng.random((2, n)) < 0.5
    np.testing.assert_array_equal(payload_filter_np(n, cols, prog, 2, base[0]), got2 & base[0])
    np.testing.assert_array_equal(payload_filter_np(n, cols, prog, 2, base), got2 & base)
    w = payload_words_np(n, cols, prog, 2, base)
    assert w.dtype == np.uint32 and w.shape == (2, 4) and (w[:, 3] >> 4 == 0).all()
    np.testing.assert_array_equal(popcount_rows_np(w, n), (got2 & base).sum(1))
    assert popcount_rows_np(np.full((1, 5), 0xFFFFFFFF, np.uint32), 100).tolist() == [100]


# ---------------------------------------------------------------------------------- against the mirror's host path
class _Embedder:
    def __init__(self, dim=16):
        self.dim = dim

    def batch_encode(self, texts, instruction=None, norm=True):
        texts = [texts] if isinstance(texts, str) else list(texts)
        out = np.stack([np.random.default_rng(abs(hash(t)) % 2 ** 32).standard_normal(self.dim) for t in texts])
        return (out / np.linalg.norm(out, axis=1, keepdims=True)).astype(np.float32)


def _mirror(meta, **cfg):
    from hipporag_amd.retriever import Chunk, HippoRAG, RetrievalConfig
    rag = HippoRAG(RetrievalConfig(max_batch=4, **cfg), embedding_model=_Embedder())
    chunks = [Chunk(f"Passage number {i} says something.", source_id=m.get("source_id"),
                    metadata={k: v for k, v in m.items() if k != "source_id"}) for i, m in enumerate(meta)]
    rag.index_from_openie(chunks, [[(f"Entity{i}", "says", f"thing{i % 7}")] for i in range(len(meta))])
    return rag


def test_equality_dicts_compile_to_what_the_host_path_matches():
    from hipporag_amd.retriever import unpack_mask
    rng = np.random.default_rng(8)
    meta = random_metadata(rng, 150)
    for i, m in enumerate(meta):
        if i % 3:
            m["source_id"] = f"s{i % 5}"
    rag = _mirror(meta)
    n = len(rag.passage_node_keys)
    assert n == 150
    cols = rag.payload_columns()
    assert set(cols) == {"year", "user", "score", "flag", "mixed", "source_id"}
    pc = encode_columns(cols, n)
    assert pc.columns["mixed"] == "f64" and pc.columns["source_id"] == "keyword" and pc.columns["flag"] == "i64"
    rcols = cols_for_restatement(pc)
    values = {"year": [2019, 2021, 2021.0, 2030, True, "2019", 2019.5], "user": ["alice", "dave", "zed", 1, None],
              "score": [0.0, 1.5, 2, 3, True, 99.0, "1.5"], "flag": [True, False, 1, 0, 1.0, 2, "True"],
              "mixed": [1, 1.0, True, 2.5, 3, 3.0, 2], "source_id": ["s0", "s4", "s9", 0]}
    filters = [{k: v} for k, vs in values.items() for v in vs]
    filters += [{k: vs[:3]} for k, vs in values.items()] + [{k: tuple(vs)} for k, vs in values.items()]
    filters += [{"year": 2021, "user": ["alice", "bob"]}, {"flag": True, "score": [0.5, 1.0, 1.5], "source_id": "s1"}, {},
                {"mixed": {1, 3}, "year": [2018, 2019, 2020]}]
    for f in filters:
        want = unpack_mask(rag._filter_words(f), n)
        got = payload_filter_np(n, rcols, compile_filters(pc, f).arrays(), 1)[0]
        np.testing.assert_array_equal(got, want, err_msg=repr(f))
    per = compile_filters(pc, filters)
    np.testing.assert_array_equal(payload_filter_np(n, rcols, per.arrays(), len(filters)),
                                  unpack_mask(np.stack([rag._filter_words(f) for f in filters]), n))


def test_the_mirror_without_the_option_is_unchanged_and_refuses_the_operators():
    from hipporag_amd.retriever import RetrievalConfig, unpack_mask
    assert RetrievalConfig().payload_index is False
    meta = [{"user": "alice", "year": 2020}, {"user": "bob", "year": 2021}, {"year": 2022, "nested": {"$x": 1}}, {"user": "carol"}]
    rag = _mirror(meta)
    n = len(rag.passage_node_keys)
    pos = [rag.passage_texts.index(f"Passage number {i} says something.") for i in range(4)]
    assert rag.payload_index is None

    def allowed(f):
        return sorted(pos.index(p) for p in np.flatnonzero(unpack_mask(rag._doc_filter_words(f, 1), n)))
    assert allowed({"user": "alice"}) == [0] and allowed({"year": [2021, 2022]}) == [1, 2] and allowed({"colour": "red"}) == []
    assert allowed({"user": {"name": "alice"}}) == [] and allowed({}) == [0, 1, 2, 3]       # a plain dict value: equality
    for f in ({"year": {"$gte": 2021}}, {"$not": {"user": "bob"}}, {"$any": {"user": "bob"}}, {"user": {"$exists": False}},
              {"user": "alice", "$nor": 1}, {"nested": {"$x": 1}}):
        with pytest.raises(ValueError, match="payload_index"):
            rag._doc_filter_words(f, 1)
        with pytest.raises(ValueError, match="payload_index"):
            rag._doc_filter_words([None if False else {}, f], 2)
    # the columns the option would build: the key with a dict value is left to the host path
    assert set(rag.payload_columns()) == {"user", "year"}
