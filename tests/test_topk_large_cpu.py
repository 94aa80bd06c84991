"""The large-k ranking's host-side contract without a GPU: the C ABI exports and declares hrag_topk_rows_ws /
hrag_topk_rows_workspace_bytes, the workspace arithmetic is what include/hrag.h documents, and the mirror ranks on the
device whenever the engine was built for the number of documents asked for."""

import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_declared():
    from hipporag_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "hrag.h")).read()
    for name in ("hrag_topk_rows_ws", "hrag_topk_rows_workspace_bytes"):
        assert name in _lib.SIGNATURES
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        getattr(lib, name)


def test_workspace_bytes_arithmetic():
    from hipporag_amd import _lib
    lib = _lib.load()
    f = lib.hrag_topk_rows_workspace_bytes
    tile = 16384
    assert f(256, 125000, 2048) == 0              # today's kernel: no workspace
    assert f(256, 125000, 4096) == 0              # <= 16384 keys per row: sorted in LDS
    assert f(256, 125000, tile) == 0
    assert f(7, 4099, 50000) == 0                 # k beyond n: min(k, n) decides
    for b, n, k in ((256, 125000, 16385), (256, 125000, 125000), (1, 875000, 875000), (7, 125000, 125007),
                    (3, 40000, 20000)):
        kk = min(k, n)
        L = -(-kk // tile) * tile
        assert f(b, n, k) == 2 * b * L * 8 + (-(-(b * 8) // 256) * 256), (b, n, k)
    assert f(2, 40000, 20000) > f(1, 40000, 20000) > 0
    assert f(0, 40000, 20000) == 0


class _RankingEngine:
    """An engine stand-in with the one-call form of phase B: ranks fixed score rows with the library's rule (numpy) for
    the k it is asked for, records the calls, and refuses the host ranking's seam."""

    def __init__(self, scores, max_topk, max_batch=4):
        self.scores, self.max_topk, self.max_batch = scores, max_topk, max_batch
        self.calls = []

    def retrieve_converged(self, q, kept_idx, kept_score, kept_count, *, k, want_all_scores=False, **kw):
        import torch
        self.calls.append((k, want_all_scores))
        rows = self.scores[: q.shape[0]]
        idx = np.argsort(rows, axis=1, kind="stable")[:, ::-1][:, :k].astype(np.int32)

        class Out:
            pass
        o = Out()
        o.doc_idx = torch.from_numpy(idx)
        o.doc_score = torch.from_numpy(np.take_along_axis(rows, idx.astype(np.int64), axis=1))
        o.flags = torch.zeros(q.shape[0], dtype=torch.int32)
        if want_all_scores:
            o.all_scores = torch.from_numpy(rows.copy())
        return o

    def last_doc_scores(self, batch):
        raise AssertionError("the host ranking path was taken")


def _run_mirror_body(eng, n_passages, num_to_retrieve, n_queries=6):
    import torch
    from hipporag_amd.retriever import iter_batched_retrieve
    queries = [f"q{i}" for i in range(n_queries)]
    out = []
    for lo, rows in iter_batched_retrieve(eng, queries, lambda qs, kind: torch.zeros((len(qs), 8)), [], None,
                                          linking_top_k=5, damping=0.5, passage_node_weight=0.05, ppr_iters=20,
                                          num_to_retrieve=num_to_retrieve, n_passages=n_passages):
        out.extend(rows)
    return out


def test_mirror_body_ranks_on_the_device_up_to_max_topk():
    """retriever.iter_batched_retrieve (the body of the mirror's retrieve and of reference_adapter.attach): with an engine
    built for 5000 documents, asking for 4000 or 5000 puts k on the device call and never asks for every score; only a
    call beyond max_topk takes the host ranking (want_all_scores)."""
    rng = np.random.default_rng(0)
    n_p = 8000
    scores = rng.random((4, n_p), dtype=np.float32)
    scores[:, ::7] = scores[:, :1]                    # ties: the larger index first
    want = np.argsort(scores, axis=1, kind="stable")[:, ::-1]
    for ask in (4000, 5000):
        eng = _RankingEngine(scores, max_topk=5000)
        rows = _run_mirror_body(eng, n_p, ask)
        assert eng.calls == [(ask, False), (ask, False)]
        for i, (d_idx, d_sc, _) in enumerate(rows):
            np.testing.assert_array_equal(d_idx, want[i % 4][:ask])
    eng = _RankingEngine(scores, max_topk=5000)
    rows = _run_mirror_body(eng, n_p, 6000)
    assert eng.calls == [(5000, True), (5000, True)]
    for i, (d_idx, d_sc, _) in enumerate(rows):
        np.testing.assert_array_equal(d_idx, want[i % 4][:6000])


def test_mirror_and_adapter_size_the_engine_without_a_2048_clamp():
    """The engine sizing of the mirror and of the adapter: min(retrieval_top_k, passages)."""
    for mod in ("retriever", "reference_adapter"):
        text = open(os.path.join(ROOT, "hipporag_amd", mod + ".py")).read()
        assert "min(2048" not in text, mod
