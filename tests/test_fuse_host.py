"""Fused retrieval without a GPU (include/hrag.h "fused retrieval"): the new symbols are declared, bound and exported; the
numpy restatement of tests/fuse_helpers.py passes hand-worked cases; the package's host form is the restatement; the
validators of the engine wrapper and of the mirror reject what the header rejects, before the device is touched."""

import os
import re

import numpy as np
import pytest

from hipporag_amd import _lib
from hipporag_amd.retriever import HippoRAG, RetrievalConfig, fuse_rows_host
from tests.fuse_helpers import fuse_max_np, fuse_np, fuse_sum_np, member_lists_np, partitions, rank_np, rrf_np
from tests.group_helpers import canonical, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hrag_fuse_rows", "hrag_rrf_rows", "hrag_fuse_workspace_bytes", "hrag_last_fused")


def _rows(rng, b, n):
    x = (rng.integers(-40, 40, (b, n)).astype(np.float32) / 8 * rng.random((b, n)).astype(np.float32)).astype(np.float32)
    for i in range(b):
        at = rng.integers(0, n, 6)
        x[i, at[0]], x[i, at[1]], x[i, at[2]], x[i, at[3]] = np.nan, np.inf, -np.inf, -0.0
        x[i, at[4]] = x[i, at[5]]
    return x


def test_symbols_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "hrag.h")).read()
    declared = set(re.findall(r"\b(hrag_[a-z_0-9]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    assert lib.hrag_version() == _lib.HRAG_VERSION == 8
    for name, value in (("HRAG_FUSE_SUM", 0), ("HRAG_FUSE_MAX", 1), ("HRAG_FUSE_RRF", 2)):
        assert re.search(rf"#define {name} {value}\b", header)
    from hipporag_amd.engine import FUSE_MODES
    assert FUSE_MODES == {"sum": 0, "max": 1, "rrf": 2}
    # the workspace size is host arithmetic: member_ptr and weights always, the member lists and filter rows for RRF
    small = lib.hrag_fuse_workspace_bytes(256, 100000, 0, 0, 0)
    assert small >= 257 * 4 + 256 * 4 and small == lib.hrag_fuse_workspace_bytes(256, 100000, 1, 0, 1)
    rrf = lib.hrag_fuse_workspace_bytes(256, 100000, 2, 200, 0)
    assert rrf >= small + 2 * 256 * 200 * 4
    assert lib.hrag_fuse_workspace_bytes(256, 100000, 2, 200, 1) >= rrf + 256 * 3125 * 4
    for bad in ((0, 100, 0, 0, 0), (4, 0, 0, 0, 0), (4, 100, 3, 0, 0), (4, 100, -1, 0, 0), (4, 100, 2, 0, 0)):
        assert lib.hrag_fuse_workspace_bytes(*bad) < 0, bad


def test_restatement_all_singletons_sum_is_the_input_canonical():
    x = _rows(np.random.default_rng(1), 5, 40)
    got = fuse_sum_np(x, np.arange(6), np.ones(5, np.float32))
    assert same_bits(got, canonical(x))
    assert not np.signbit(got[~np.isnan(got)][got[~np.isnan(got)] == 0]).any()          # -0 became +0
    assert (got.view(np.uint32)[np.isnan(got)] == 0x7fc00000).all()
    assert same_bits(fuse_sum_np(x, np.arange(6)), got)                                  # NULL weights are all 1
    assert same_bits(fuse_max_np(x, np.arange(6)), canonical(x))


def test_restatement_max_row_with_nan_is_nan_and_minus_zero_is_plus_zero():
    x = np.array([[1.0, -np.inf, -0.0, 2.0], [np.nan, -np.inf, -0.0, np.inf], [3.0, -1.0, -0.0, -5.0]], np.float32)
    x[1, 0] = np.frombuffer(np.uint32(0xffc12345).tobytes(), np.float32)[0]               # a negative NaN with a payload
    got = fuse_max_np(x, [0, 3])
    assert got.view(np.uint32).tolist() == [[0x7fc00000, np.float32(-1).view(np.uint32), 0, np.float32(np.inf).view(np.uint32)]]
    two = fuse_max_np(x, [0, 1, 3])
    assert two[0].tolist() == [1.0, -np.inf, 0.0, 2.0] and not np.signbit(two[0, 2])
    assert np.isnan(two[1, 0]) and two[1, 1:].tolist() == [-1.0, 0.0, np.inf]


def test_restatement_rrf_two_lists_sharing_one_passage_by_hand():
    lists = np.array([[4, 2, -1], [2, 7, 0]], np.int32)                 # passage 2: rank 2 of member 0, rank 1 of member 1
    got = rrf_np(lists, [0, 2], 8, None, 60)
    f = np.float32
    want = np.zeros(8, np.float32)
    want[4] = f(1 / 61)
    want[2] = f(f(1 / 62) + f(1 / 61))                                 # member order: 0.0f + t_0, then + t_1
    want[7] = f(1 / 62)
    want[0] = f(1 / 63)
    assert got.shape == (1, 8) and got[0].view(np.uint32).tolist() == want.view(np.uint32).tolist()
    w = np.array([0.5, 3.0], np.float32)
    got = rrf_np(lists, [0, 2], 8, w, 0)
    assert got[0, 2] == f(f(0.5 / 2) + f(3.0 / 1)) and got[0, 4] == f(0.5) and got[0, 0] == f(1.0) and got[0, 1] == 0
    apart = rrf_np(lists, [0, 1, 2], 8, None, 60)                       # as two questions nothing is shared
    assert apart[0, 2] == f(1 / 62) and apart[1, 2] == f(1 / 61) and apart[0, 7] == 0
    # the member lists are the project's ranking under the question's filter: ties -> larger index, NaN first
    s = np.array([[0.5, np.nan, 0.5, 0.25], [0.1, 0.2, 0.3, 0.4]], np.float32)
    assert member_lists_np(s, [0, 2], 3).tolist() == [[1, 2, 0], [3, 2, 1]]
    assert member_lists_np(s, [0, 2], 3, np.array([True, False, True, False])).tolist() == [[2, 0, -1], [2, 0, -1]]


def test_restatement_fp64_sum_differs_from_an_fp32_sum():
    big, one = np.float32(2 ** 24), np.float32(1)
    x = np.array([[big], [one], [one], [-big]], np.float32)
    assert fuse_sum_np(x, [0, 4])[0, 0] == 2.0                          # exact in fp64
    acc = np.float32(0)
    for v in x[:, 0]:
        acc = np.float32(acc + v)
    assert acc == 0.0                                                   # the fp32 chain loses both ones
    w = np.array([1, 0.5, 0.5, 1], np.float32)
    assert fuse_sum_np(x, [0, 4], w)[0, 0] == 1.0
    assert fuse_sum_np(x, [0, 2, 4])[:, 0].tolist() == [2.0 ** 24, 1 - 2.0 ** 24]  # 2^24 + 1 rounds once, to even; 1 - 2^24 is exact


def test_the_packages_host_form_is_the_restatement():
    rng = np.random.default_rng(5)
    b, n = 9, 61
    x = _rows(rng, b, n)
    w = (rng.random(b) * 4).astype(np.float32)
    w[2] = 0
    for name, mp in partitions(rng, b).items():
        nq = len(mp) - 1
        allowed = rng.random((nq, n)) < 0.6
        allowed[0] = False
        assert same_bits(fuse_rows_host(x, mp, "sum", w), fuse_np(x, mp, "sum", w)), name
        assert same_bits(fuse_rows_host(x, mp, "sum"), fuse_np(x, mp, "sum")), name
        assert same_bits(fuse_rows_host(x, mp, "max"), fuse_np(x, mp, "max")), name
        for a in (None, allowed, allowed[-1]):
            for c, d in ((0, 1), (60, 7), (60, n)):
                got = fuse_rows_host(x, mp, "rrf", w, c, d, a)
                assert same_bits(got, fuse_np(x, mp, "rrf", w, c, d, a)), (name, c, d)
    idx, sc = rank_np(fuse_np(x, [0, 4, 9], "sum"), 5, np.arange(n) % 2 == 0)
    assert (idx % 2 == 0).all() and idx.shape == (2, 5) and np.isnan(sc[:, 0]).all()


def test_check_fuse():
    from hipporag_amd.engine import check_fuse
    mode, mp, w, c, d = check_fuse("sum", [0, 2, 5], 5, [1, 0, 2.5, 3, 0.25])
    assert mode == 0 and mp.dtype == np.int32 and mp.tolist() == [0, 2, 5] and w.dtype == np.float32 and (c, d) == (0, 0)
    assert check_fuse("max", np.array([0, 5]), 5)[:1] == (1,) and check_fuse("max", [0, 5], 5)[2] is None
    assert check_fuse("rrf", [0, 1, 5], 5, None, 0, 7, 7)[3:] == (0, 7)
    assert check_fuse("rrf", [0, 1, 5], 5, None, 60, np.int64(1), 200)[3:] == (60, 1)
    for bad_ptr in ([0, 2, 2, 5], [0, 3, 2, 5], [1, 5], [0, 4], [0, 6], [5], [], [0.0, 5.0], [[0, 5]]):
        with pytest.raises(ValueError, match="member_ptr"):
            check_fuse("sum", bad_ptr, 5)
    with pytest.raises(ValueError, match="no weights"):
        check_fuse("max", [0, 5], 5, np.ones(5))
    for bad_w in ([1, 1, 1, 1, -1e-9], [1, 1, np.nan, 1, 1], [np.inf, 1, 1, 1, 1], [1, 1, 1, 1], np.ones((5, 1))):
        with pytest.raises(ValueError, match="weight"):
            check_fuse("sum", [0, 5], 5, bad_w)
    for depth in (0, -1, 8, None, 2.5, True):
        with pytest.raises(ValueError, match="rrf_depth"):
            check_fuse("rrf", [0, 5], 5, None, 60, depth, 7)
    for c in (-1, 1.5, None, True):
        with pytest.raises(ValueError, match="rrf_c"):
            check_fuse("rrf", [0, 5], 5, None, c, 3, 7)
    for name in ("mean", None, 2):
        with pytest.raises(ValueError, match="fuse"):
            check_fuse(name, [0, 5], 5)


def test_last_fused_validates_before_the_device_is_touched():
    from hipporag_amd import engine
    eng = object.__new__(engine.HippoRAGEngine)
    eng.max_topk, eng.n_passages = 50, 1000
    for kw in (dict(member_ptr=[0, 2, 2]), dict(member_ptr=[0, 3], weights=[1, 1, 1], fuse="max"),
               dict(member_ptr=[0, 3], weights=[1, -1, 1], fuse="sum"), dict(member_ptr=[0, 3], rrf_depth=51),
               dict(member_ptr=[0, 3], rrf_depth=0), dict(member_ptr=[0, 3], fuse="mean"),
               dict(member_ptr=[0, 3], group_agg="median"), dict(member_ptr=[0, 3], group_hits=3)):
        with pytest.raises(ValueError):
            eng.last_fused(**kw)


def test_retrieve_fused_validates_before_the_device_is_touched():
    rag = object.__new__(HippoRAG)
    rag.global_config = RetrievalConfig()
    for bad in (["a", "b"], [["a"], []], [["a"], "b"], [["a", 3]], "ab"):
        with pytest.raises(ValueError, match="questions"):
            rag.retrieve_fused(bad)
    qs = [["a", "b"], ["c"]]
    with pytest.raises(ValueError, match="no weights"):
        rag.retrieve_fused(qs, weights=[[1, 1], [1]], fuse="max")
    for w in ([[1, -1], [1]], [[1, np.nan], [1]], [[np.inf, 1], [1]], [1, 1, -2], [[1], [1]], [1, 1]):
        with pytest.raises(ValueError, match="weight"):
            rag.retrieve_fused(qs, weights=w, fuse="sum")
    for d in (0, -3):
        with pytest.raises(ValueError, match="rrf_depth"):
            rag.retrieve_fused(qs, rrf_depth=d)
    with pytest.raises(ValueError, match="rrf_c"):
        rag.retrieve_fused(qs, rrf_c=-1)
    with pytest.raises(ValueError, match="fuse"):
        rag.retrieve_fused(qs, fuse="median")
    assert rag.retrieve_fused([]) == []


def test_the_sharded_hybrid_and_captured_classes_refuse():
    from hipporag_amd import dist, engine
    for cls in (dist.ShardedRetriever, dist.NativeShardedRetriever):
        with pytest.raises(NotImplementedError, match="fuse"):
            cls.retrieve(object.__new__(cls), None, None, None, None, fuse="rrf")
    with pytest.raises(NotImplementedError, match="fuse"):
        dist.HybridRetriever.retrieve(object.__new__(dist.HybridRetriever), None, None, None, None, fuse="sum")
    with pytest.raises(NotImplementedError, match="fuse"):
        engine.CapturedPipeline(None, 1, fuse="max")
    # the mirror on an engine object that has no last_fused (the multi-GPU retrievers)
    rag = object.__new__(HippoRAG)
    rag.global_config = RetrievalConfig()
    rag.ready_to_retrieve = True
    rag.engine = object.__new__(dist.ShardedRetriever)
    with pytest.raises(NotImplementedError, match="fuse"):
        rag.retrieve_fused([["a", "b"]])
