"""The mirror's batch pipeline (retriever.iter_batched_retrieve: per-batch slicing of the per-query arguments, the clamps,
the host forms beyond max_topk, the A(0) A(1) B(0) A(2) B(1) ... order with its pinned staging copies and the repeated read
path) held to the composed-options restatement, batch by batch: tests/pipeline_helpers.py::expected_batch over the anchor
rows of a DIRECT retrieve_converged(k=1, want_all_scores=True) on each batch's own rows.  Ids exactly, floats bit for bit,
the -1 / 0 padding included; every call also runs through the serial form of the loop (tools/soak_mirror.py::SerialEngine)
and must give identical bits.

The index is the option matrix's (tests/test_gpu_option_matrix.py::CASE: 375 passages, max_topk 200, groups, fact sources,
lexical and payload indexes), one engine per PPR state family with a small max_batch -- 4 (the small-batch kernels), 16
(the fp16 state), 65 (the e4m3 slabs) -- and N = 2 b + 3 queries: three batches, the last one ragged.  The driver is
tools/soak_mirror.py::PipelineCase (its check() is what the soak runs on random option sets)."""

import dataclasses
import itertools
import time

import numpy as np
import pytest

from tests import option_helpers as oh
from tests import pipeline_helpers as ph
from tests.group_helpers import same_bits
from tests.test_gpu_option_matrix import CASE, _tool

pytestmark = pytest.mark.gpu
STATES = {4: 4, 16: 2, 65: 8}              # max_batch -> hrag_stats.last_ppr_state of a full batch
K_F, TOL, MAX_ITERS, NARROW, ITERS = 5, 1.5e-6, 60, 12, 20


def _np(t):
    return None if t is None else t.cpu().numpy()


_rigs = {}


@pytest.fixture(scope="module")
def rigs(gpu_device):
    def rig(b, top=CASE["max_topk"]):
        """tools/soak_mirror.py::PipelineCase of max_batch b over the matrix's index: N = 2 b + 3 queries, strict"""
        if (b, top) not in _rigs:
            _rigs[b, top] = r = _tool("soak_mirror").PipelineCase(dict(CASE, b=b, max_topk=top), gpu_device)
            assert r.c.max_topk == top < r.n and r.n_q == 2 * b + 3 and r.strict
            assert r.ppr_state_of_a_full_batch() == STATES[b]
        return _rigs[b, top]
    yield rig
    for r in _rigs.values():
        r.close()
    _rigs.clear()


def _subsets(boost):
    subsets = [on for r in range(len(ph.TOGGLES) + 1) for on in itertools.combinations(ph.TOGGLES, r)]
    assert len(subsets) == 128
    return [on for on in subsets if ("boost" in on) == boost]


@pytest.mark.parametrize("boost", [False, True], ids=["plain", "boost"])
@pytest.mark.parametrize("b", sorted(STATES))
def test_every_servable_subset_through_three_batches_is_the_restatement(rigs, b, boost):
    """Every servable subset of {filter, seeds, group_agg, group_hits, mmr, lexical, boost} (option_helpers.servable) through
    the pipeline, the option values rotating with the subset's number, the filter as one row or as [N, W] words."""
    rig = rigs(b)
    t0, bad, served = time.time(), [], 0
    for i, on in enumerate(_subsets(boost)):
        spec = ph.pipeline_spec(on, i, rig.n_q, ph.want_of(10, rig.n, rig.c.groups if "group_agg" in on else None))
        if oh.servable(spec, dict(max_topk=rig.c.max_topk, fact_sources=True)) is not None:
            continue
        served += 1
        bad += [(on, w, spec.to_json()) for w in rig.check(spec, 10, keep_all=bool(i % 2), seed=i)]
    print(f"b={b} boost={boost}: {served} calls in {time.time() - t0:.2f} s")
    assert not bad, bad[:5]
    assert served == 30


def test_the_refusals_of_this_layer_are_raised_by_name_before_anything_is_enqueued(rigs):
    rig = rigs(4)
    base = oh.CallSpec(entry="retrieve_converged", k=10)
    before = rig.eng.stats()

    class NoSources:
        def __getattr__(self, name):
            if name == "has_fact_sources":
                return False
            return getattr(rig.eng, name)

    cases = [(rig.eng, dataclasses.replace(base, mmr_lambda=0.5, mmr_candidates=rig.c.max_topk + 1), ValueError, "mmr_candidates"),
             (rig.eng, dataclasses.replace(base, k=rig.c.max_topk + 1, mmr_lambda=0.5), ValueError, "mmr_candidates"),
             (rig.eng, dataclasses.replace(base, filter_kind="half", filter_scope="seeds", lexical_weight=0.3),
              NotImplementedError, "filter_scope"),
             (NoSources(), dataclasses.replace(base, filter_kind="half", filter_scope="seeds"), ValueError, "set_fact_sources")]
    for eng, spec, exc, name in cases:
        allowed = ph.call_allowed(spec, rig.n, rig.n_q, rig.c.payload_allowed)
        with pytest.raises(exc, match=name):
            rig.run(eng, rig.kw(spec, spec.k, allowed, False))
    kw = rig.kw(dataclasses.replace(base, group_agg="max"), 10, None, False)
    kw["group_of"] = None
    with pytest.raises(ValueError, match="group_of"):
        rig.run(rig.eng, kw)
    after = rig.eng.stats()
    assert all(after[k] == before[k] for k in ("calls_retrieve", "calls_score_facts", "queries"))


def _beyond_calls(n_q, want_p, want_g):
    """(name, CallSpec): plain, filtered (a "few" filter leaves fewer than want), boosted (programs 2 and 6: NaN entries, exact
    ties at the two zeros), grouped with and without hits, max and sum"""
    S = lambda k, **kw: oh.CallSpec(entry="retrieve_converged", k=k, filter_form="words", **kw)
    ids = [(2, 6, 3, 9, 0)[r % 5] for r in range(n_q)]
    pay = [r % 7 for r in range(n_q)]
    return [("plain", S(want_p)),
            ("a filter per query", S(want_p, filter_kind="half", filter_per_query=True, filter_seed=11)),
            ("few allowed", S(want_p, filter_kind="few", filter_per_query=True, filter_seed=12)),
            ("boosted per query", S(want_p, boost_kind="per_query", boost_ids=ids, boost_form="program")),
            ("boosted, ties at zero, a filter", S(want_p, boost_kind="one", boost_ids=[6], boost_form="program", filter_kind="payload",
                                                 filter_per_query=True, payload_ids=pay, filter_seed=13)),
            ("seeds", S(want_p, filter_kind="half", filter_per_query=True, filter_seed=14, filter_scope="seeds")),
            ("groups by max", S(want_g, group_agg="max")),
            ("groups by sum, hits", S(want_g, group_agg="sum", group_hits=2)),
            ("groups by max, hits, a filter, a boost", S(want_g, group_agg="max", group_hits=3, filter_kind="payload", payload_ids=pay,
                                                        filter_per_query=True, boost_kind="per_query", boost_ids=ids,
                                                        boost_form="program")),
            ("groups by sum, few allowed, NaN rows", S(want_g, group_agg="sum", group_hits=1, filter_kind="few", filter_seed=15,
                                                      boost_kind="one", boost_ids=[2], boost_form="program")),
            ("groups by max, lexical", S(want_g, group_agg="max", lexical_weight=0.5))]


@pytest.mark.parametrize("num", ["max_topk+1", "n", "n+5"])
@pytest.mark.parametrize("b,top", [(4, 200), (16, 200), (4, 20)])
def test_more_documents_than_the_engine_ranks_are_ranked_on_the_host_as_the_device_would(rigs, b, top, num):
    """num_to_retrieve > max_topk: the host forms (rank_allowed, group_rank_rows, group_hits_rows, the bare argsort) over the
    score rows of every passage agree with the restatement -- which is the device's rule -- on ties, NaN, the two zeros and
    the -1 / 0 padding.  The index has fewer groups than max_topk = 200, where a grouped call is clamped to the groups and
    stays on the device; the engine of max_topk = 20 takes the grouped calls through the host forms as well."""
    rig = rigs(b, top)
    num = {"max_topk+1": rig.c.max_topk + 1, "n": rig.n, "n+5": rig.n + 5}[num]
    want_p, want_g = ph.want_of(num, rig.n), ph.want_of(num, rig.n, rig.c.groups)
    assert want_p > rig.c.max_topk
    t0, bad = time.time(), []
    assert (want_g > rig.c.max_topk) == (top == 20)
    for i, (name, spec) in enumerate(_beyond_calls(rig.n_q, want_p, want_g)):
        bad += [(name, w) for w in rig.check(spec, num, keep_all=bool(i % 2), seed=100 + i)]
    print(f"b={b} num={num}: {time.time() - t0:.2f} s")
    assert not bad, bad[:5]


def test_the_boosted_rows_beyond_max_topk_hold_ties_at_zero_and_nan(rigs):
    """What the test above rests on: programs 2 and 6 of BOOST_PROGRAMS put NaN entries and exact ties at zero over most of a
    row into the rows the host forms rank (the two zeros in one row: tests/test_pipeline_options_host.py, on rows of its own)."""
    rig = rigs(4)
    spec = oh.CallSpec(entry="retrieve_converged", k=rig.n, boost_kind="per_query", boost_form="program",
                       boost_ids=[(2, 6, 3, 9, 0)[r % 5] for r in range(rig.n_q)])
    R, _, _ = rig.anchor(spec, None, 0, 4)
    rows = ph.expected_batch(R, spec, rig.ctx, None, 0, 4, rig.c.columns)["rows"]
    assert np.isnan(rows[0]).any() and not np.isnan(rows[0]).all() and not np.isnan(rows[1]).any()
    assert (rows[1] == 0).sum() > rig.n // 3 and (R[1] == 0).sum() < 10


@pytest.mark.parametrize("b,want_state", [(9, 2)])
def test_a_batch_whose_rows_were_repeated_is_read_from_the_tensors(gpu_device, b, want_state):
    """The ring of tests/test_gpu_boost.py's directed test through a three-batch pipeline: the PPR rows of every batch are
    flagged and repeated by finish() on the fp32 state, the DPR-fallback rows are not, so every batch is read through the
    repeated path (out.*.cpu()) after the next batch was enqueued on the same handle.  A filter and a boost per query,
    ppr_tol > 0.  Every batch is the same retrieve_converged call made directly, bit for bit, and the restatement over the
    unboosted direct call's rows."""
    import torch
    from hipporag_amd import synth
    from hipporag_amd._lib import FLAG_NOT_CONVERGED
    from hipporag_amd.boost import compile_boosts
    from hipporag_amd.engine import HippoRAGEngine, pack_mask
    from hipporag_amd.payload import PayloadIndex, encode_columns
    from hipporag_amd.retriever import iter_batched_retrieve
    from tests.group_helpers import random_groups
    from tests.payload_helpers import columns_of, random_metadata
    from tests.test_gpu_fp8_adversarial import CASES, _index
    make, damping, _ = CASES["ring"]
    n_v, src, dst, w, pv, pinned = make()
    csr, pass_bits, fact_bits, index = _index(n_v, src, dst, w, pv, 64, seed=11, pinned_facts=pinned)
    n, k, n_q = len(pv), 20, 2 * b + 3
    rng = np.random.default_rng(77)
    host = encode_columns(columns_of(random_metadata(rng, n), ["year", "user", "score", "flag", "mixed"]), n)
    groups = random_groups(rng, n, "shuffled")
    per = [[{"if": {"year": {"$gte": 2018 + q % 6}}, "add": 1.0 + q}, {"mul": 1.0 + q / 64.0}] for q in range(n_q)]
    allowed = rng.random((n_q, n)) < 0.5
    assert ph.offsets_differ(allowed, b) and ph.offsets_differ(per, b)
    bf16 = lambda bits: torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(gpu_device).view(torch.bfloat16)
    qf, qp = bf16(synth.make_queries_np(fact_bits, n_q, seed=5)[0]), bf16(synth.make_queries_np(pass_bits, n_q, seed=6)[0])
    queries, facts, flt = [f"q{i}" for i in range(n_q)], range(fact_bits.shape[0]), ph.fact_filter(K_F)
    q_tensor = lambda qs, kind: (qf if kind == "triple" else qp)[torch.tensor([ph.query_number(q) for q in qs], device=gpu_device)]
    ix = PayloadIndex(host)
    try:
        with HippoRAGEngine(csr, index.passage_vertex, pass_bits, fact_bits, index.subj_vertex, index.obj_vertex,
                            index.num_chunks, max_batch=b, max_topk=n) as eng:
            eng.set_payload_index(ix)
            eng.set_passage_groups(groups)
            words = pack_mask(allowed)
            spec = oh.CallSpec(entry="retrieve_converged", k=k, group_agg="sum", group_hits=2, filter_kind="half",
                               filter_per_query=True, boost_kind="per_query")
            kw = dict(linking_top_k=K_F, damping=damping, passage_node_weight=0.05, ppr_iters=ITERS, ppr_tol=TOL,
                      ppr_max_iters=400, ppr_base_iters_narrow=NARROW, num_to_retrieve=k, n_passages=n, doc_filter=words,
                      group_agg="sum", group_of=groups, group_hits=2, keep_all_scores=True, boost=compile_boosts(ix, per, n_q))
            got = list(iter_batched_retrieve(eng, queries, q_tensor, facts, flt, **kw))
            cuts = ph.batch_cuts(n_q, b)
            assert [lo for lo, _ in got] == [lo for lo, _ in cuts] and len(cuts) == 3
            ctx = dict(n_passages=n, groups=groups, max_topk=n)
            for (lo, hi), (_, rows) in zip(cuts, got):
                ids = torch.arange(lo, hi, device=gpu_device)
                idx, sc = eng.score_facts(qf[ids], k=K_F)
                k_idx, k_sc, k_cnt, seeds = ph.kept_facts(_np(idx), _np(sc), queries[lo:hi], facts, flt, K_F)
                assert (k_cnt == 0).any() and (k_cnt > 0).any() and [r[2] for r in rows] == seeds
                kept = tuple(map(torch.from_numpy, (k_idx, k_sc, k_cnt)))
                ckw = dict(link_top_k=K_F, damping=damping, passage_node_weight=0.05, ppr_tol=TOL, ppr_max_iters=400,
                           ppr_iters=ph.base_iters(ITERS, TOL, NARROW, hi - lo, damping), want_all_scores=True)
                first = eng.retrieve(qp[ids], *kept, link_top_k=K_F, damping=damping, passage_node_weight=0.05, k=1,
                                     ppr_iters=ckw["ppr_iters"], ppr_tol=TOL, ppr_max_iters=400)
                late = (_np(first.flags) & FLAG_NOT_CONVERGED) != 0
                assert late.any() and not late.all() and not late[k_cnt == 0].any(), (lo, late)     # some rows repeat, not all
                if hi - lo == b:
                    assert eng.stats()["last_ppr_state"] == want_state
                assert rows.repeated is True
                rows_w = torch.from_numpy(np.ascontiguousarray(words[lo:hi]).view(np.int32))
                direct = eng.retrieve_converged(qp[ids], *kept, k=k, doc_filter=rows_w, group_agg="sum", group_hits=2,
                                                boost=compile_boosts(ix, per[lo:hi], hi - lo), **ckw)
                plain = eng.retrieve_converged(qp[ids], *kept, k=1, **ckw)
                for name in ph.FIELDS[:5]:
                    g, d = getattr(rows, name), _np(getattr(direct, name))
                    assert same_bits(g, d) if d.dtype == np.float32 else np.array_equal(g, d), (lo, name)
                assert same_bits(_np(rows.all_scores), _np(direct.all_scores)), lo
                # (per-query lists that are not BOOST_PROGRAMS: the batch's own lists, compiled here)
                want = oh.expected_outputs(_np(plain.all_scores), dataclasses.replace(spec, boost_kind="per_query"),
                                           dict(ctx, allowed=allowed[lo:hi], boost=_own_boost(host, per[lo:hi])))
                for name in ph.FIELDS[:5]:
                    g, w_ = getattr(rows, name), want[name]
                    assert same_bits(g, w_) if w_.dtype == np.float32 else np.array_equal(g, w_), (lo, name)
                assert same_bits(_np(rows.all_scores)[:, :n], want["rows"]), lo
    finally:
        ix.close()


def _own_boost(host_columns, lists):
    from hipporag_amd.boost import compile_boosts
    from tests.payload_helpers import cols_for_restatement
    prog = compile_boosts(host_columns, list(lists), len(lists))
    return dict(cols=cols_for_restatement(host_columns), prog=prog.arrays(), broadcast=prog.broadcast, n_terms=prog.n_terms)


# ------------------------------------------------------------------------------------------ the string level
FDICTS = [{"user": "alice"}, {"year": [2019, 2020, 2021]}, {"user": ["bob", "carol"], "year": 2022},
          {"source_id": ["s1", "s2", "s3", "s4", "s5", "s6", "s7"]}, {"user": "dave"}]
MIRROR_BOOSTS = (0, 1, 3, 4, 5, 6, 7, 9, 8)          # BOOST_PROGRAMS without the NaN one (metadata dicts are compared by ==)
N_STRINGS = 15                           # four batches of max_batch 4, the last one ragged with a seeded row


def _mirror(dev, payload_index, top):
    """The matrix's index behind a HippoRAG of max_batch 4 with chunk metadata, ~60 sources and texts over a small
    vocabulary; query strings "q<i> <words>" whose embeddings a table holds."""
    from hipporag_amd import synth
    from hipporag_amd.graph import bf16_bits_to_float
    from hipporag_amd.retriever import HippoRAG, RetrievalConfig
    from tests.helpers import make_case
    from tests.payload_helpers import random_metadata
    table_model = _tool("soak_mirror").Table
    kg, pass_bits, fact_bits, _ = make_case(CASE["v"], CASE["e"], CASE["dim"], seed=CASE["seed"], passage_frac=CASE["pfrac"])
    n, rng = kg.n_passages, np.random.default_rng(2718)
    meta = random_metadata(rng, n)
    src = rng.integers(0, 60, n)
    vocab = [f"w{t}" for t in range(30)]
    texts = [f"passage {i} " + " ".join(rng.choice(vocab, 6)) for i in range(n)]
    queries = [f"q{i} " + " ".join(rng.choice(vocab, 1 + i % 3, replace=False)) for i in range(N_STRINGS)]
    qf = bf16_bits_to_float(synth.make_queries_np(fact_bits, N_STRINGS, seed=31)[0])
    qp = bf16_bits_to_float(synth.make_queries_np(pass_bits, N_STRINGS, seed=32)[0])
    rag = HippoRAG.from_arrays(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                               passage_texts=texts, embedding_model=table_model({"f": dict(zip(queries, qf)), "p": dict(zip(queries, qp))}),
                               rerank_filter=ph.fact_filter(K_F),
                               global_config=RetrievalConfig(embedding_precision="bf16", max_batch=4, retrieval_top_k=top,
                                                             payload_index=payload_index))
    rag.chunk_metadata = {key: dict(meta[i], source_id=f"s{src[i]}") for i, key in enumerate(rag.passage_node_keys)}
    rag.prepare_retrieval_objects()
    assert rag.engine.max_batch == 4 and rag.engine.max_topk == top
    return rag, queries, pass_bits


def _allowed_of(rag, filters):
    """metadata dict filters by their definition: keys AND, the values of a key OR, equality"""
    rows = [rag.chunk_metadata[k] for k in rag.passage_node_keys]
    return np.array([[all(key in m and m[key] in (v if isinstance(v, list) else [v]) for key, v in f.items()) for m in rows]
                     for f in filters], bool)


class _Level:
    """The pipeline-level reference of a mirror: anchors through its engine, the restatement, the mapping to strings."""

    def __init__(self, rag, queries, pass_bits, dev):
        import torch
        from hipporag_amd.payload import encode_columns
        from tests.test_gpu_boost import _gram_fn
        self.rag, self.queries, self.dev, self.n = rag, queries, dev, len(rag.passage_node_keys)
        self.table = rag.group_table("source_id")
        bits = torch.from_numpy(np.ascontiguousarray(pass_bits).view(np.int16)).to(dev).view(torch.bfloat16).contiguous()
        self.ctx = dict(n_passages=self.n, groups=self.table[0], gram=_gram_fn(bits, self.n, CASE["dim"], dev),
                        max_topk=rag.engine.max_topk)
        self.columns = encode_columns(rag.payload_columns(), self.n)
        rag.get_query_embeddings(queries)

    def kept(self, ids):
        import torch
        qs = [self.queries[i] for i in ids]
        idx, sc = self.rag.engine.score_facts(self.rag._q_tensor(qs, "triple"), k=K_F)
        k_idx, k_sc, k_cnt, seeds = ph.kept_facts(_np(idx), _np(sc), qs, self.rag.facts, ph.fact_filter(K_F), K_F)
        return tuple(map(torch.from_numpy, (k_idx, k_sc, k_cnt))), seeds

    def anchor(self, ids, lexical_weight=None):
        """(R, kept fact lists) of the queries `ids` as one direct k = 1 call"""
        cfg, qs = self.rag.global_config, [self.queries[i] for i in ids]
        kept, seeds = self.kept(ids)
        kw = {} if lexical_weight is None else dict(lexical=self.rag.lexical_model.encode_queries(qs), lexical_weight=lexical_weight)
        a = self.rag.engine.retrieve_converged(self.rag._q_tensor(qs, "passage"), *kept, k=1, want_all_scores=True,
                                               link_top_k=cfg.linking_top_k, damping=cfg.damping,
                                               passage_node_weight=cfg.passage_node_weight, ppr_tol=cfg.ppr_tol,
                                               ppr_max_iters=cfg.ppr_max_iters,
                                               ppr_iters=ph.base_iters(20, cfg.ppr_tol, cfg.ppr_base_iters_narrow, len(ids), cfg.damping),
                                               **kw)
        return _np(a.all_scores), seeds

    def solutions(self, out, num, extra=None):
        """[(docs, doc_scores, metadata)] per row of expected_outputs' arrays, as _group_solutions builds them"""
        texts, keys, (_, values, sizes) = self.rag.passage_texts, self.rag.passage_node_keys, self.table
        res = []
        for i in range(len(out["doc_idx"])):
            gi = out["group_idx"][i][:num]
            keep = np.flatnonzero(gi >= 0)
            ids = out["doc_idx"][i][:num][keep]
            md = []
            for at, j in enumerate(keep):
                d = dict(self.rag.chunk_metadata[keys[ids[at]]], group=values[gi[j]], group_size=int(sizes[gi[j]]))
                d["group_hits"] = [{"doc": texts[p], "score": float(v), "position": int(p)}
                                   for p, v in zip(out["hit_idx"][i][j], out["hit_score"][i][j]) if p >= 0]
                if out["mmr_value"] is not None:
                    d["mmr_value"] = float(out["mmr_value"][i][at])
                d.update(extra or {})
                md.append(d)
            res.append(([texts[p] for p in ids], out["doc_score"][i][:len(ids)], md))
        return res

    def compare(self, sols, want, seeds=None, what=""):
        assert len(sols) == len(want), what
        for i, (s, (docs, sc, md)) in enumerate(zip(sols, want)):
            assert s.docs == docs, (what, i)
            assert same_bits(np.asarray(s.doc_scores, np.float32), sc) and np.asarray(s.doc_scores).dtype == np.float32, (what, i)
            assert s.doc_metadata == md, (what, i, [k for a, b_ in zip(s.doc_metadata, md) for k in b_ if a.get(k) != b_[k]][:3])
            if seeds is not None:
                assert s.graph_seeds == seeds[i], (what, i)


@pytest.mark.parametrize("payload_index", [True, False], ids=["payload", "host-filters"])
def test_retrieve_and_retrieve_dpr_with_several_options_are_the_reference_mapped_to_strings(gpu_device, payload_index):
    """HippoRAG.retrieve over four device batches (the last ragged) with per-query metadata-dict filters, group_by="source_id"
    with group_hits, mmr_lambda, lexical_weight and -- with the payload index -- a per-query boost in ONE call; retrieve_dpr
    with the filters, the groups, the hits and MMR.  docs, doc_scores and the metadata keys (group, group_size, group_hits,
    mmr_value, lexical_weight, boosted) are the pipeline-level reference mapped through passage_texts."""
    rag, queries, pass_bits = _mirror(gpu_device, payload_index, 200)
    try:
        lv = _Level(rag, queries, pass_bits, gpu_device)
        num, n_q, b = 10, N_STRINGS, 4
        filters = [FDICTS[r % len(FDICTS)] for r in range(n_q)]
        boosts = [oh.BOOST_PROGRAMS[MIRROR_BOOSTS[(2 * r) % len(MIRROR_BOOSTS)]] for r in range(n_q)]
        allowed = _allowed_of(rag, filters)
        assert ph.offsets_differ(allowed, b) and ph.offsets_differ(filters, b) and ph.offsets_differ(boosts, b)
        assert allowed.any(axis=1).all()
        got = rag.retrieve(queries, num_to_retrieve=num, doc_filter=filters, group_by="source_id", group_hits=2, mmr_lambda=0.5,
                           lexical_weight=0.3, boost=boosts if payload_index else None)
        enc = [rag.lexical_model.encode_queries([q]) for q in queries]
        assert ph.offsets_differ([e[1].tolist() + e[2].tolist() for e in enc], b)
        want_k = ph.want_of(num, lv.n, lv.table[0])
        spec = oh.CallSpec(entry="retrieve_converged", k=want_k, filter_kind="half", group_agg="max", group_hits=2, mmr_lambda=0.5,
                           mmr_candidates=ph.pool_of(min(200, oh.MMR_MAX_CANDIDATES), want_k, lv.n, lv.table[0]),
                           lexical_weight=0.3, boost_kind="per_query" if payload_index else None)
        dspec = dataclasses.replace(spec, entry="dense_retrieve", lexical_weight=None, boost_kind=None)
        dpr = rag.retrieve_dpr(queries, num_to_retrieve=num, doc_filter=filters, group_by="source_id", group_hits=2, mmr_lambda=0.5)
        extra = dict(lexical_weight=0.3, **({"boosted": True} if payload_index else {}))
        cuts = ph.batch_cuts(n_q, b)
        assert len(cuts) >= 3
        for lo, hi in cuts:
            R, seeds = lv.anchor(range(lo, hi), 0.3)
            assert any(not s for s in seeds) and any(seeds)
            ctx = dict(lv.ctx, allowed=allowed[lo:hi], boost=_own_boost(lv.columns, boosts[lo:hi]) if payload_index else None)
            lv.compare(got[lo:hi], lv.solutions(oh.expected_outputs(R, spec, ctx), num, extra), seeds, ("retrieve", lo))
            assert [s.question for s in got[lo:hi]] == queries[lo:hi]
            rag.engine.dense_retrieve(rag._q_tensor(queries[lo:hi], "passage"), k=1, group_agg="max")
            D = _np(rag.engine.last_doc_scores(hi - lo))
            lv.compare(dpr[lo:hi], lv.solutions(oh.expected_outputs(D, dspec, dict(lv.ctx, allowed=allowed[lo:hi])), num),
                       None, ("retrieve_dpr", lo))
    finally:
        rag.engine.close()


@pytest.mark.parametrize("form,top,num,fuse", [("device", 200, 10, "rrf"), ("host", 20, 30, "sum")])
def test_retrieve_fused_over_three_chunks_is_the_fusion_of_each_chunk(gpu_device, form, top, num, fuse):
    """retrieve_fused with per-question filters, groups and hits over questions that fill several device chunks: every
    chunk is fuse_np + expected_outputs over the member rows of a direct call -- on the device form (last_fused) and on the
    host form (more groups wanted than the engine ranks: fuse_rows_host + group_rank_rows)."""
    rag, queries, pass_bits = _mirror(gpu_device, True, top)
    try:
        lv = _Level(rag, queries, pass_bits, gpu_device)
        sizes = [2, 1, 3, 2, 1, 2, 2, 2]
        start = np.concatenate([[0], np.cumsum(sizes)])
        assert start[-1] == N_STRINGS
        questions = [queries[start[j]: start[j + 1]] for j in range(len(sizes))]
        filters = [FDICTS[j % len(FDICTS)] for j in range(len(sizes))]
        allowed = _allowed_of(rag, filters)
        assert ph.offsets_differ(allowed, 1)
        got = rag.retrieve_fused(questions, fuse=fuse, num_to_retrieve=num, doc_filter=filters, group_by="source_id", group_hits=2)
        want_k = ph.want_of(num, lv.n, lv.table[0])
        assert (want_k > top) == (form == "host")
        chunks, lo = [], 0
        while lo < len(sizes):              # whole questions, as many as fit into max_batch sub-queries
            hi = lo + 1
            while hi < len(sizes) and start[hi + 1] - start[lo] <= 4:
                hi += 1
            chunks.append((lo, hi))
            lo = hi
        assert len(chunks) >= 3
        for lo, hi in chunks:
            R, seeds = lv.anchor(range(start[lo], start[hi]))
            mp = (start[lo: hi + 1] - start[lo]).tolist()
            spec = oh.CallSpec(entry="last_fused", k=want_k, fuse=fuse, member_ptr=mp, filter_kind="half", group_agg="max",
                               group_hits=2)
            out = oh.expected_outputs(R, spec, dict(lv.ctx, allowed=allowed[lo:hi]))
            q_seeds = [[f for i in range(mp[j], mp[j + 1]) for f in seeds[i]] for j in range(hi - lo)]
            lv.compare(got[lo:hi], lv.solutions(out, num), q_seeds, (form, lo))
            assert [s.question for s in got[lo:hi]] == [q[0] for q in questions[lo:hi]]
    finally:
        rag.engine.close()
