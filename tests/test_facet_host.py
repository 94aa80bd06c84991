"""Facets without a device (include/hrag.h, "facets"): the numpy restatement held to a naive loop over every passage, the
grammar of compile_facet and its errors, labels and the order of .top(), the mirror's refusal, and the new symbols in the
header, the binding and the built library."""

import math
import os
import re

import numpy as np
import pytest

from hipporag_amd._lib import FACET_CODES, FACET_EDGES, FACET_MAX_BINS, FACET_WINDOW
from hipporag_amd.facet import FacetCounts, FacetSpec, compile_facet, top_of
from hipporag_amd.payload import encode_columns, f64_bits
from tests.facet_helpers import (LDS_EDGES, WINDOW, codes, edges_f64, edges_i64, facet_bins_naive, facet_bins_np, facet_columns,
                                 facet_counts_np, facet_ids_np, random_spec, special_specs)
from tests.payload_helpers import I64_MAX, I64_MIN, bits

NEW = ("hrag_payload_facet", "hrag_payload_facet_ids", "hrag_payload_facet_ws_bytes")


def test_symbols_are_declared_bound_and_exported():
    from hipporag_amd import _lib
    hdr = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "hrag.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and re.search(r"hrag_status " + name + r"\(", hdr) and getattr(lib, name) is not None
    for name, value in (("CODES", FACET_CODES), ("EDGES", FACET_EDGES), ("WINDOW", FACET_WINDOW)):
        assert int(re.search(rf"#define HRAG_FACET_{name} (\d+)", hdr).group(1)) == value, name
    assert re.search(r"#define HRAG_FACET_MAX_BINS \(1 << 20\)", hdr) and FACET_MAX_BINS == 1 << 20 and FACET_WINDOW == 4096
    # the struct of the binding has the header's fields, in its order
    body = re.search(r"typedef struct hrag_facet_spec \{(.*?)\} hrag_facet_spec;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [decl.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip()]
    assert fields == [n for n, _ in _lib.FacetSpecDesc._fields_]
    assert _lib.HRAG_VERSION == 8 and lib.hrag_version() == 8            # additive: the version does not move
    # the sizes the tests pick their cases by are the kernels'
    internal = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "facet_bin.h")).read()
    assert int(re.search(r"constexpr int kFacetLdsEdges = (\d+);", internal).group(1)) == LDS_EDGES and WINDOW == FACET_WINDOW


@pytest.mark.parametrize("n", [1, 33, 300])
def test_the_vectorised_restatement_is_the_naive_loop(n):
    """Every special spec and random ones, over the columns with the int64 extremes, NaN, both infinities and both zeros."""
    rng = np.random.default_rng(n)
    cols = facet_columns(rng, n)
    specs = list(special_specs().items()) + [(f"random {i}", random_spec(rng)) for i in range(30)]
    for name, spec in specs:
        got, want = facet_bins_np(n, cols, spec), facet_bins_naive(n, cols, spec)
        np.testing.assert_array_equal(got, want, err_msg=name)
        assert got.min() >= 0 and got.max() <= spec.n_bins + 1
        allowed = rng.random((3, n)) < 0.6
        counts = facet_counts_np(n, cols, spec, allowed)
        assert counts.shape == (3, spec.n_bins + 2) and counts.dtype == np.int32
        np.testing.assert_array_equal(counts.sum(1), allowed.sum(1), err_msg=name)       # a row sums to the allowed passages
        for b in range(3):
            for v in np.unique(want):
                assert counts[b, v] == int((allowed[b] & (want == v)).sum()), (name, b, v)
        ids = rng.integers(-2, n + 2, (2, 2 * n + 3))
        by_id = facet_ids_np(n, cols, spec, ids)
        for b in range(2):
            ref = np.zeros(spec.n_bins + 2, np.int64)
            for i in ids[b]:
                if 0 <= i < n:
                    ref[want[i]] += 1
            np.testing.assert_array_equal(by_id[b], ref, err_msg=name)


def test_the_restatement_says_what_the_definition_says():
    n = 8
    vals = np.array([I64_MIN, I64_MAX, -1, 0, 1, 2, 3, 0], np.int64)
    pres = np.array([1, 1, 1, 1, 1, 1, 1, 0], bool)
    f = bits([np.nan, -np.inf, -0.0, 0.0, 5e-324, 1.5, np.inf, 0.0])
    cols = [(0, vals, pres), (1, f, pres)]
    assert facet_bins_np(n, cols, codes(0, 0, 3)).tolist() == [3, 3, 3, 0, 1, 2, 3, 4]
    assert facet_bins_np(n, cols, codes(0, I64_MAX, 4)).tolist() == [4, 0, 4, 4, 4, 4, 4, 5]       # MIN - MAX wraps to 1: other
    assert facet_bins_np(n, cols, codes(0, I64_MIN, 2)).tolist() == [0, 2, 2, 2, 2, 2, 2, 3]
    assert facet_bins_np(n, cols, edges_i64(0, [0, 2, 2])).tolist() == [0, 3, 0, 1, 1, 3, 3, 5]     # [2, 2) is empty
    assert facet_bins_np(n, cols, edges_i64(0, [])).tolist() == [0] * 7 + [2]
    assert facet_bins_np(n, cols, edges_f64(1, [0.0])).tolist() == [2, 0, 1, 1, 1, 1, 1, 3]         # NaN: other; -0.0 == 0.0
    assert facet_bins_np(n, cols, edges_f64(1, [-np.inf, np.inf])).tolist() == [3, 1, 1, 1, 1, 1, 2, 4]
    assert facet_bins_np(n, cols, edges_f64(1, [])).tolist() == [1, 0, 0, 0, 0, 0, 0, 2]
    c = facet_counts_np(n, cols, codes(0, 0, 3), np.ones(n, bool))
    assert c.tolist() == [[1, 1, 1, 4, 1]]
    assert facet_ids_np(n, cols, codes(0, 0, 3), [[3, 3, -1, 8, 7, 4]]).tolist() == [[2, 1, 0, 0, 1]]


def test_the_grammar_compiles_and_every_error_names_its_field():
    n = 5
    host = encode_columns({"year": [2000, 2010, None, 2020, 2023], "score": [0.5, None, 1.5, 2.0, -1.0],
                           "src": ["b", "a", "c", None, "a"]}, n)
    s = compile_facet(host, "src")
    assert isinstance(s, FacetSpec) and (s.kind, s.lo, s.n_bins, s.column, s.edges) == (FACET_CODES, 0, 3, 2, None)
    assert s.labels == ["a", "b", "c"] and not s.f64 and s.n_edges == 0
    y = compile_facet(host, "year", lo=2000, n_values=24)
    assert (y.kind, y.lo, y.n_bins) == (FACET_CODES, 2000, 24) and list(y.labels) == list(range(2000, 2024))
    assert compile_facet(host, "year", lo=I64_MAX, n_values=2).lo == I64_MAX
    e = compile_facet(host, "year", edges=[2005, 2015.0, True + 2019, 2020])
    assert (e.kind, e.n_bins, e.n_edges) == (FACET_EDGES, 5, 4) and e.edges.tolist() == [2005, 2015, 2020, 2020]
    assert e.labels == [(None, 2005), (2005, 2015), (2015, 2020), (2020, 2020), (2020, None)]
    f = compile_facet(host, "score", edges=[-math.inf, -0.0, 1, 1.5, math.inf])
    assert f.f64 and f.edges.tolist() == [f64_bits(v) for v in (-math.inf, -0.0, 1.0, 1.5, math.inf)]
    assert f.labels[0] == (None, -math.inf) and f.labels[-1] == (math.inf, None) and f.n_bins == 6
    none = compile_facet(host, "score", edges=[])
    assert none.n_bins == 1 and none.labels == [(None, None)] and none.n_edges == 0
    # the compiled specs are the restatement's: same bins through either route
    from tests.payload_helpers import cols_for_restatement
    cols = cols_for_restatement(host)
    assert facet_bins_np(n, cols, edges_i64(0, e.edges)).tolist() == [0, 1, 6, 4, 4]
    assert facet_bins_np(n, cols, codes(2, 0, 3)).tolist() == [1, 0, 2, 4, 0]
    bad = {
        "an unknown field": (dict(field="nope"), r"unknown field 'nope'"),
        "an unhashable field": (dict(field=["src"]), r"unknown field \['src'\]"),
        "edges on a keyword column": (dict(field="src", edges=[1]), r"facet 'src': a keyword column takes no edges"),
        "lo on a keyword column": (dict(field="src", lo=0, n_values=2), r"facet 'src': a keyword column"),
        "lo on an F64 column": (dict(field="score", lo=0, n_values=4), r"facet 'score': lo / n_values on an F64 column"),
        "a NaN edge": (dict(field="score", edges=[0.0, math.nan]), r"facet 'score': a NaN edge"),
        "a NaN edge on an I64 column": (dict(field="year", edges=[math.nan]), r"facet 'year': a NaN edge"),
        "descending edges": (dict(field="score", edges=[1.0, 0.5]), r"facet 'score': descending edges"),
        "descending integer edges": (dict(field="year", edges=[2001, 2000]), r"facet 'year': descending edges"),
        "a fraction on an I64 column": (dict(field="year", edges=[2000.5]), r"facet 'year': the edge 2000.5 is not an integer"),
        "an infinity on an I64 column": (dict(field="year", edges=[math.inf]), r"facet 'year': the edge inf is not an integer"),
        "an integer beyond int64": (dict(field="year", edges=[1 << 63]), r"facet 'year': the edge .* is outside int64"),
        "an integer that is no double": (dict(field="score", edges=[(1 << 53) + 1]), r"facet 'score': the edge .* is not exactly a double"),
        "a str edge": (dict(field="year", edges=["2000"]), r"facet 'year': an edge of type str"),
        "a str edge on an F64 column": (dict(field="score", edges=["x"]), r"facet 'score': an edge of type str"),
        "too many edges": (dict(field="year", edges=range(FACET_MAX_BINS)), rf"facet 'year': {FACET_MAX_BINS + 1} bins, at most FACET_MAX_BINS"),
        "too many values": (dict(field="year", lo=0, n_values=FACET_MAX_BINS + 1), r"facet 'year': .* bins, outside \[1, FACET_MAX_BINS"),
        "no values": (dict(field="year", lo=0, n_values=0), r"facet 'year': 0 bins"),
        "neither form": (dict(field="year"), r"facet 'year': a number column needs edges"),
        "neither form, F64": (dict(field="score"), r"facet 'score': a number column needs edges"),
        "lo alone": (dict(field="year", lo=3), r"facet 'year': lo and n_values are both needed"),
        "a float lo": (dict(field="year", lo=3.0, n_values=2), r"facet 'year': lo and n_values are both needed"),
        "lo beyond int64": (dict(field="year", lo=1 << 63, n_values=2), r"facet 'year': lo=.* is outside int64"),
        "both forms": (dict(field="year", edges=[1], lo=0, n_values=2), r"facet 'year': edges or lo / n_values, not both"),
    }
    for what, (kw, pattern) in bad.items():
        kw = dict(kw)
        with pytest.raises(ValueError, match=pattern):
            compile_facet(host, kw.pop("field"), **kw)
    assert compile_facet(host, "year", edges=range(FACET_MAX_BINS - 1)).n_bins == FACET_MAX_BINS       # the cap exactly
    assert compile_facet(host, "year", lo=-5, n_values=FACET_MAX_BINS).n_bins == FACET_MAX_BINS


def test_top_orders_by_count_then_bin_and_drops_zeros():
    counts = np.array([[3, 0, 5, 3, 5, 1], [0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1]], np.int32)
    labels = list("abcdef")
    top = top_of(counts, labels, 10)
    assert top[0] == [("c", 5), ("e", 5), ("a", 3), ("d", 3), ("f", 1)]                 # ties by bin ascending; the zero dropped
    assert top[1] == [] and top[2] == [(c, 1) for c in labels]
    assert top_of(counts, labels, 2) == [[("c", 5), ("e", 5)], [], [("a", 1), ("b", 1)]]
    assert top_of(counts, labels, 0) == [[], [], []]
    assert top_of(counts[:, :3], range(10, 13), 1)[0] == [(12, 5)]                     # integer labels: a range serves
    # FacetCounts views a raw [B, n_bins + 2] row: counts, other, missing
    host = encode_columns({"src": ["a", "b", None]}, 3)

    class Raw:                       # (the slices FacetCounts takes; a device tensor in the real call)
        def __init__(self, a):
            self.a = a

        def __getitem__(self, key):
            return Raw(self.a[key])

        def cpu(self):
            return self

        def numpy(self):
            return self.a
    fc = FacetCounts(Raw(np.array([[2, 1, 0, 4], [0, 3, 7, 0]], np.int32)), compile_facet(host, "src"))
    assert fc.counts.a.tolist() == [[2, 1], [0, 3]] and fc.other.a.tolist() == [0, 7] and fc.missing.a.tolist() == [4, 0]
    assert fc.labels == ["a", "b"] and fc.top() == [[("a", 2), ("b", 1)], [("b", 3)]] and fc.top(1)[0] == [("a", 2)]


def test_the_mirror_refuses_facets_without_the_payload_index():
    from hipporag_amd.retriever import HippoRAG, RetrievalConfig
    rag = HippoRAG(RetrievalConfig())
    with pytest.raises(ValueError, match="facets needs RetrievalConfig.payload_index=True"):
        rag.facets("source_id")
    with pytest.raises(ValueError, match="payload_index=True"):
        rag.facets(["source_id", "year"], doc_filter={"year": 2020}, limit=3, edges=[2000])


def test_the_engine_names_re_export_the_facet_module():
    from hipporag_amd import engine, facet
    assert engine.compile_facet is facet.compile_facet and engine.FacetSpec is FacetSpec and engine.FacetCounts is FacetCounts
    import types
    bare = types.SimpleNamespace(_parent=None)
    bare._payload_ix = types.MethodType(engine.HippoRAGEngine._payload_ix, bare)
    with pytest.raises(ValueError, match=r"facet needs a payload index on this engine \(set_payload_index\)"):
        engine.HippoRAGEngine.facet(bare, "source")
    assert WINDOW == FACET_WINDOW
