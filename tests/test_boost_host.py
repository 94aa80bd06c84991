"""Boosted retrieval without a device (include/hrag.h, "boosted retrieval"): the numpy restatement held to a naive loop over
every element, exp_dec held to libm, the boost grammar and its errors, the refusals of the engine, the multi-GPU retrievers
and the mirror, and the new symbols in the header, the binding and the built library."""

import math
import os
import re
import types

import numpy as np
import pytest

from hipporag_amd._lib import (BOOST_ADD, BOOST_CONST, BOOST_DECAY, BOOST_EXP, BOOST_FIELD, BOOST_GAUSS, BOOST_HAS_MISSING,
                               BOOST_LINEAR, BOOST_MAX_TERMS, BOOST_MUL, BOOST_NONE, BOOST_SQRT, PAY_MAX_CLAUSES)
from hipporag_amd.boost import BoostProgram, check_program, compile_boosts, decay_constant
from hipporag_amd.payload import encode_columns
from tests.boost_helpers import (assemble_boost, boost_columns, boost_rows_naive, boost_rows_np, exp_dec_np, exp_dec_scalar,
                                 make_boosts, random_terms, special_boosts)
from tests.payload_helpers import cols_for_restatement

NEW = ("hrag_boost_rows", "hrag_last_boosted")


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_symbols_are_declared_bound_and_exported():
    from hipporag_amd import _lib
    hdr = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "hrag.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and re.search(r"hrag_status " + name + r"\(", hdr) and getattr(lib, name) is not None
    for name, value in (("MAX_TERMS", BOOST_MAX_TERMS), ("CONST", BOOST_CONST), ("FIELD", BOOST_FIELD), ("DECAY", BOOST_DECAY),
                        ("MUL", BOOST_MUL), ("ADD", BOOST_ADD), ("NONE", BOOST_NONE), ("SQRT", BOOST_SQRT),
                        ("LINEAR", BOOST_LINEAR), ("EXP", BOOST_EXP), ("GAUSS", BOOST_GAUSS)):
        assert int(re.search(rf"#define HRAG_BOOST_{name} (\d+)", hdr).group(1)) == value, name
    assert re.search(r"#define HRAG_BOOST_HAS_MISSING \(1 << 24\)", hdr) and BOOST_HAS_MISSING == 1 << 24
    assert BOOST_MAX_TERMS == 32 and PAY_MAX_CLAUSES == 64
    # the struct of the binding has the header's fields, in its order
    body = re.search(r"typedef struct hrag_boost_program \{(.*?)\} hrag_boost_program;", hdr, re.S).group(1)
    fields = [f.strip().lstrip("*") for decl in body.split(";") if decl.strip()
              for f in decl.strip().split(None, 2 if decl.strip().startswith("const") else 1)[-1].split(",")]
    assert fields == [n for n, _ in _lib.BoostProgramDesc._fields_]
    assert _lib.HRAG_VERSION == 8 and lib.hrag_version() == 8            # additive: the version does not move


def test_exp_dec_is_within_four_ulp_of_libm_and_exact_at_its_ends():
    rng = np.random.default_rng(1)
    x = np.concatenate([-rng.random(200000) * 708.0, -np.exp(rng.uniform(-40, 6.5, 100000)),
                        [-708.0, -707.9999999999999, -1e-300, -5e-324, -0.5 * math.log(2), -math.log(2), -1.5 * math.log(2)]])
    x = x[x >= -708.0]
    got = exp_dec_np(x)
    ref = np.asarray([math.exp(v) for v in x])
    ulp = np.abs(got - ref) / np.spacing(ref)
    print(f"exp_dec_np against math.exp over {len(x)} points of [-708, 0]: max {ulp.max():.3f} ulp")
    assert ulp.max() <= 4.0                      # twice the 2.0 ulp measured against one libm, as margin for another
    assert (got >= 0).all() and (got <= 1).all()
    assert exp_dec_np(0.0) == 1.0 and exp_dec_np(-0.0) == 1.0 and exp_dec_np(3.0) == 1.0
    assert exp_dec_np(-708.0000000000001) == 0.0 and exp_dec_np(-1e300) == 0.0 and exp_dec_np(-np.inf) == 0.0
    assert math.copysign(1.0, float(exp_dec_np(-709.0))) == 1.0
    assert np.isnan(exp_dec_np(np.nan)) and math.isnan(exp_dec_scalar(math.nan))
    assert exp_dec_np(-708.0) > 0 and exp_dec_np(-708.0) >= np.finfo(np.float64).tiny      # the result is never denormal
    some = x[:: max(1, len(x) // 5000)]
    assert all(exp_dec_scalar(float(v)) == float(w) for v, w in zip(some, exp_dec_np(some)))
    assert np.array_equal(exp_dec_np(x.reshape(-1, 1)).ravel(), got)


@pytest.mark.parametrize("n", [1, 33, 300])
def test_the_vectorised_restatement_is_the_naive_loop_bit_for_bit(n):
    """Random programs and every special one, per query and broadcast, with and without the min-max form, over rows with
    NaN payloads, infinities, both zeros and denormals."""
    rng = np.random.default_rng(n)
    cols = boost_columns(rng, n)
    specials = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-39, 3.4e38], np.float32)
    for per in (make_boosts(rng, 65)[:len(special_boosts())], [random_terms(rng) for _ in range(12)], make_boosts(rng, 1)):
        b = len(per)
        prog = assemble_boost(per)
        rows = rng.standard_normal((b, n + 2)).astype(np.float32)
        sp = rng.random(rows.shape) < 0.2
        rows[sp] = specials[rng.integers(0, len(specials), int(sp.sum()))]
        rows.view(np.uint32)[0, 0] = 0x7FA00001
        a, c = boost_rows_np(rows, n, cols, prog), boost_rows_naive(rows, n, cols, prog)
        assert np.array_equal(_bits(a), _bits(c))
        assert np.array_equal(_bits(a[:, n:]), _bits(rows[:, n:]))                       # the columns beyond n
        for q, terms in enumerate(per):
            if not terms:
                assert np.array_equal(_bits(a[q]), _bits(rows[q]))                       # no terms: not touched
        fin = np.where(np.isfinite(rows[:, :n]), rows[:, :n], 0).astype(np.float32)
        mn, mx = fin.min(axis=1), fin.max(axis=1)
        mx[0] = mn[0]                                                                    # a zero range
        assert np.array_equal(_bits(boost_rows_np(rows, n, cols, prog, mn=mn, mx=mx)),
                              _bits(boost_rows_naive(rows, n, cols, prog, mn=mn, mx=mx)))
        one = assemble_boost([per[-1]])
        assert np.array_equal(_bits(boost_rows_np(rows, n, cols, one, True)), _bits(boost_rows_naive(rows, n, cols, one, True)))


def test_the_restatement_says_what_the_definition_says():
    n = 5
    host = encode_columns({"year": [2000, 2010, None, 2020, 2023], "cites": [0, 4, 9, None, 2.25], "src": ["a", "b", "a", None, "c"]}, n)
    cols = cols_for_restatement(host)
    rows = np.array([[1.0, 2.0, -0.0, 4.0, np.nan]], np.float32)
    run = lambda items, **kw: boost_rows_np(rows, n, cols, compile_boosts(host, items).arrays(), True, **kw)[0]
    np.testing.assert_array_equal(run([{"if": {"src": ["a", "c"]}, "mul": 1.5}])[:4], np.float32([1.5, 2.0, -0.0 * 1.5 + 0.0, 4.0]))
    assert np.signbit(rows[0, 2]) and not np.signbit(run([{"if": {"src": "zzz"}, "mul": 9}])[2])      # rewritten: -0 + 0 = +0
    assert _bits(run([{"if": {"src": "zzz"}, "mul": 9}]))[4] == 0x7FC00000
    np.testing.assert_array_equal(run([{"field": "cites", "modifier": "sqrt", "add": 0.5}])[:4], np.float32([1.0, 3.0, 1.5, 4.0]))
    np.testing.assert_array_equal(run([{"field": "cites", "add": 1.0, "missing": -4.0}])[:4], np.float32([1.0, 6.0, 9.0, 0.0]))
    lin = run([{"decay": {"field": "year", "origin": 2020, "scale": 10, "offset": 3, "decay": 0.5, "kind": "linear"}, "mul": 1.0}])
    # c = 20; d = 17, 7, missing, 0, 0 (inside the offset)
    np.testing.assert_array_equal(lin[:4], np.float32([1.0 * (3.0 / 20.0), 2.0 * (13.0 / 20.0), 0.0, 4.0]))
    for kind, f in (("exp", lambda d: 0.5 ** (d / 10.0)), ("gauss", lambda d: 0.5 ** ((d / 10.0) ** 2))):
        got = run([{"decay": {"field": "year", "origin": 2020, "scale": 10, "kind": kind}, "mul": 1.0, "missing": 0.0}])
        np.testing.assert_allclose(got[:4], np.float32([f(20.0), 2 * f(10.0), 0.0, 4.0]), rtol=1e-6)
        assert got[3] == 4.0                                                             # at the origin the decay is exactly 1
    assert decay_constant("linear", 10.0, 0.5) == 20.0 and decay_constant("exp", 10.0, 0.5) == math.log(0.5) / 10.0
    assert decay_constant("gauss", 3.0, 0.25) == math.log(0.25) / 9.0
    two = run([{"mul": 2.0}, {"add": 1.0}, {"mul": 3.0}])                                # s * (2 * 3) + 1: list order within M and A
    np.testing.assert_array_equal(two[:4], np.float32([7.0, 13.0, 1.0, 25.0]))
    np.testing.assert_array_equal(run([{"mul": 2.0}], mn=np.float32([1.0]), mx=np.float32([4.0]))[:4],
                                  np.float32([0.0, 2.0 / 3.0 * 1.0, 2 * np.float32(-1.0) / np.float32(3.0), 2.0]).astype(np.float32))


def test_the_grammar_compiles_and_every_error_names_its_item():
    n = 4
    host = encode_columns({"year": [2000, 2010, None, 2020], "score": [0.5, None, 1.5, 2.0], "src": ["a", "b", "a", None]}, n)
    pr = compile_boosts(host, [{"if": {"src": "a", "year": {"$gte": 2005}}, "mul": 1.5},
                               {"field": "score", "modifier": "sqrt", "add": 0.25, "missing": 1},
                               {"decay": {"field": "year", "origin": 2020, "scale": 5}, "mul": 1.0, "if": {"$not": {"src": "b"}}}])
    assert pr.broadcast and pr.batch == 1 and pr.n_terms == 3 and pr.n_clauses == 3
    assert pr.t_ptr.tolist() == [0, 3] and pr.t_cl_ptr.tolist() == [0, 2, 2, 3]
    assert pr.t_op.tolist() == [BOOST_CONST | BOOST_MUL << 8, BOOST_FIELD | BOOST_ADD << 8 | BOOST_SQRT << 16 | BOOST_HAS_MISSING,
                                BOOST_DECAY | BOOST_MUL << 8 | BOOST_LINEAR << 16]
    assert pr.t_col.tolist() == [0, 1, 0] and pr.t_num.shape == (3, 5) and pr.t_num.dtype == np.float64
    assert pr.t_num[1].tolist() == [0.25, 0.0, 0.0, 0.0, 1.0] and pr.t_num[2].tolist() == [1.0, 2020.0, 0.0, 10.0, 0.0]
    assert [a.dtype for a in pr.arrays()] == [np.int32] * 3 + [np.float64] + [np.int32] * 3 + [np.int64] * 2 + [np.int32, np.int64]
    per = compile_boosts(host, [[{"mul": 2}], None, [], [{"add": 1}, {"field": "year", "add": 1e-3}]], batch=4)
    assert not per.broadcast and per.batch == 4 and per.t_ptr.tolist() == [0, 1, 1, 1, 3]
    sel = per.select([3, 0, 3])
    assert isinstance(sel, BoostProgram) and sel.batch == 3 and sel.t_ptr.tolist() == [0, 2, 3, 5]
    assert sel.t_num[:, 0].tolist() == [1.0, 1e-3, 2.0, 1.0, 1e-3] and pr.select([0, 0]) is pr
    assert per.select(range(1, 3)).n_terms == 0 and compile_boosts(host, []).n_terms == 0
    rows = np.arange(16, dtype=np.float32).reshape(4, 4)
    cols = cols_for_restatement(host)
    assert np.array_equal(boost_rows_np(rows, n, cols, per.arrays())[[3, 0, 3]], boost_rows_np(rows[[3, 0, 3]], n, cols, sel.arrays()))
    assert check_program(host, per, 4) is per and check_program(host, [{"mul": 2}], 9).broadcast
    bad = {
        "a non-finite weight": ([{"mul": math.inf}], r"boost\[0\]: mul"),
        "a NaN weight": ([{"add": math.nan}], r"boost\[0\]: add"),
        "a bool weight": ([{"mul": True}], r"boost\[0\]: mul"),
        "a str weight": ([{"mul": "2"}], r"boost\[0\]: mul"),
        "a non-finite missing": ([{"field": "score", "add": 1, "missing": -math.inf}], r"boost\[0\]: missing"),
        "a non-finite origin": ([{"mul": 1}, {"decay": {"field": "year", "origin": math.nan, "scale": 1}, "mul": 1}], r"boost\[1\]: decay: origin"),
        "scale 0": ([{"decay": {"field": "year", "origin": 0, "scale": 0}, "mul": 1}], r"boost\[0\]: decay: scale"),
        "a negative scale": ([{"decay": {"field": "year", "origin": 0, "scale": -2.0}, "mul": 1}], r"boost\[0\]: decay: scale"),
        "an infinite scale": ([{"decay": {"field": "year", "origin": 0, "scale": math.inf}, "mul": 1}], r"boost\[0\]: decay: scale"),
        "decay 0": ([{"decay": {"field": "year", "origin": 0, "scale": 1, "decay": 0}, "mul": 1}], r"boost\[0\]: decay: decay"),
        "decay 1": ([{"decay": {"field": "year", "origin": 0, "scale": 1, "decay": 1.0}, "mul": 1}], r"boost\[0\]: decay: decay"),
        "a negative offset": ([{"decay": {"field": "year", "origin": 0, "scale": 1, "offset": -1}, "mul": 1}], r"boost\[0\]: decay: offset"),
        "a scale that underflows c": ([{"decay": {"field": "year", "origin": 0, "scale": 1e-200, "kind": "gauss"}, "mul": 1}], r"boost\[0\]: decay: scale"),
        "an unknown key": ([{"mul": 1, "boost": 2}], r"boost\[0\]: unknown key 'boost'"),
        "an unknown decay key": ([{"decay": {"field": "year", "origin": 0, "scale": 1, "sigma": 2}, "mul": 1}], r"boost\[0\]: decay: unknown key 'sigma'"),
        "an unknown kind": ([{"decay": {"field": "year", "origin": 0, "scale": 1, "kind": "log"}, "mul": 1}], r"boost\[0\]: decay: kind"),
        "an unknown modifier": ([{"field": "score", "modifier": "log1p", "mul": 1}], r"boost\[0\]: modifier"),
        "a modifier on a constant": ([{"modifier": "sqrt", "mul": 1}], r"boost\[0\]: unknown key 'modifier'"),
        "missing on a constant": ([{"missing": 1, "mul": 1}], r"boost\[0\]: unknown key 'missing'"),
        "a modifier on a decay": ([{"decay": {"field": "year", "origin": 0, "scale": 1}, "modifier": "sqrt", "mul": 1}], r"boost\[0\]: unknown key 'modifier'"),
        "no origin": ([{"decay": {"field": "year", "scale": 1}, "mul": 1}], r"boost\[0\]: decay: 'origin'"),
        "both modes": ([{"mul": 1, "add": 1}], r"boost\[0\]: exactly one"),
        "no mode": ([{"if": {"src": "a"}}], r"boost\[0\]: exactly one"),
        "field and decay": ([{"field": "score", "decay": {"field": "year", "origin": 0, "scale": 1}, "mul": 1}], r"boost\[0\]: \"field\" and \"decay\""),
        "a keyword field": ([{"field": "src", "add": 1}], r"boost\[0\]: field 'src' is a keyword column"),
        "a keyword decay field": ([{"decay": {"field": "src", "origin": 0, "scale": 1}, "mul": 1}], r"boost\[0\]: decay: field 'src' is a keyword"),
        "an unknown field": ([{"field": "nope", "add": 1}], r"boost\[0\]: unknown field 'nope'"),
        "an unknown condition field": ([{"if": {"nope": 1}, "mul": 2}], r"boost\[0\]: if: unknown field 'nope'"),
        "a bad condition": ([{"if": {"year": {"$near": 1}}, "mul": 2}], r"boost\[0\]: if: 'year': unknown operator"),
        "33 terms": ([{"mul": 1.0}] * 33, r"boost: 33 terms, at most BOOST_MAX_TERMS=32"),
    }
    for what, (items, pattern) in bad.items():
        with pytest.raises(ValueError, match=pattern):
            compile_boosts(host, items)
        with pytest.raises(ValueError, match=pattern.replace(r"boost\[", r"boost\[2\]\[").replace("boost:", r"boost\[2\]:")):
            compile_boosts(host, [None, [], items])                                  # per query: the message names the query too
    compile_boosts(host, [{"if": {"year": 2000, "src": "a"}, "mul": 1.0}] * 32)       # 32 terms, 64 clauses: both caps exactly
    with pytest.raises(ValueError, match=r"boost: 66 condition clauses over its terms, at most PAY_MAX_CLAUSES=64"):
        compile_boosts(host, [{"if": {"year": 2000, "src": "a", "score": 1.5}, "mul": 1.0}] * 22)
    with pytest.raises(ValueError, match=r"boost\[1\]\[0\]: a dict expected"):
        compile_boosts(host, [[], [3]])
    with pytest.raises(TypeError, match="list"):
        compile_boosts(host, {"mul": 1})
    with pytest.raises(TypeError, match=r"boost\[1\]: a list of items"):
        compile_boosts(host, [[{"mul": 1}], {"mul": 1}])
    with pytest.raises(ValueError, match="2 per-query lists for a batch of 3"):
        compile_boosts(host, [[], None], batch=3)
    with pytest.raises(ValueError, match="holds 4 queries, the call 3"):
        check_program(host, per, 3)
    with pytest.raises(ValueError, match="another index"):
        check_program(encode_columns({"year": [1, 2, 3, 4]}, 4), per, 4)
    with pytest.raises(ValueError, match="select"):
        per.select([4])


def test_what_does_not_serve_a_boost_refuses_it_by_name():
    from hipporag_amd.dist import HybridRetriever, NativeShardedRetriever, ShardedRetriever
    from hipporag_amd.engine import CapturedPipeline, HippoRAGEngine, refuse_boost
    from hipporag_amd.retriever import HippoRAG, RetrievalConfig
    some = [{"mul": 2.0}]
    refuse_boost("X", {"boost": None, "group_agg": "max"})
    with pytest.raises(NotImplementedError, match="X does not serve boost"):
        refuse_boost("X", {"boost": some})
    for cls in (ShardedRetriever, NativeShardedRetriever):
        with pytest.raises(NotImplementedError, match=f"{cls.__name__} does not serve boost"):
            cls.retrieve(object(), None, None, None, None, boost=some)
    with pytest.raises(NotImplementedError, match="HybridRetriever does not serve boost"):
        HybridRetriever.retrieve(object(), None, None, None, None, boost=some)
    with pytest.raises(NotImplementedError, match="CapturedPipeline does not serve boost"):
        CapturedPipeline(None, 1, boost=some)
    with pytest.raises(NotImplementedError, match="shard_finish does not serve boost"):
        HippoRAGEngine.shard_finish(object(), None, None, None, 5, boost=some)
    shard = types.SimpleNamespace(n_rows=10, num_vertices=20, passage_rows=5, n_passages=5)
    with pytest.raises(NotImplementedError, match="boost on a row-shard engine"):
        HippoRAGEngine._boost_program(shard, some, 1)
    bare = types.SimpleNamespace(_parent=None)
    with pytest.raises(ValueError, match=r"boost needs a payload index on this engine \(set_payload_index\)"):
        HippoRAGEngine._payload_ix(bare, "boost")
    for name, kw in (("group_agg", dict(group_agg="max")), ("group_hits", dict(group_hits=2)), ("mmr_lambda", dict(mmr_lambda=0.5)),
                     ("mmr_candidates", dict(mmr_candidates=5)), ("lexical", dict(lexical=(1, 2, 3)))):
        with pytest.raises(ValueError, match=rf"dense_retrieve\(boost=\) does not serve {name}"):
            HippoRAGEngine.dense_retrieve(object(), None, boost=some, **kw)
    with pytest.raises(ValueError, match=r'dense_retrieve\(boost=\) does not serve filter_scope="seeds"'):
        HippoRAGEngine.dense_retrieve(object(), None, boost=some, filter_scope="seeds")
    # the mirror: the argument and the config default need the payload index; retrieve_fused names boost
    assert RetrievalConfig().boost is None
    rag = HippoRAG(RetrievalConfig())
    assert rag._boost(None, 3) is None
    with pytest.raises(ValueError, match="boost needs RetrievalConfig.payload_index=True"):
        rag._boost(some, 3)
    with pytest.raises(ValueError, match="payload_index"):
        HippoRAG(RetrievalConfig(boost=some))._boost(None, 3, "retrieve_dpr")
    with pytest.raises(ValueError, match="retrieve_fused does not serve boost"):
        rag.retrieve_fused([["a", "b"]], boost=some)
    with pytest.raises(ValueError, match="retrieve_fused does not serve boost"):
        HippoRAG(RetrievalConfig(boost=some)).retrieve_fused([["a", "b"]])
    host = encode_columns({"year": [1, 2, 3]}, 3)
    rag.payload_index = host                                                  # (a PayloadColumns stands in for the index)
    pr = rag._boost([{"field": "year", "add": 1.0}], 7)
    assert isinstance(pr, BoostProgram) and pr.broadcast and rag._boost(pr, 2) is pr
    with pytest.raises(ValueError, match="2 per-query lists for a batch of 3"):
        rag._boost([[], None], 3)
    rag.payload_index = None
    sols = [types.SimpleNamespace(doc_metadata=[{}, {"a": 1}]), types.SimpleNamespace(doc_metadata=None)]
    HippoRAG._boost_metadata(sols, None)
    assert sols[0].doc_metadata == [{}, {"a": 1}]
    HippoRAG._boost_metadata(sols, pr)
    assert sols[0].doc_metadata == [{"boosted": True}, {"a": 1, "boosted": True}]
