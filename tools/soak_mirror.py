#!/usr/bin/env python
"""Randomised soak of the mirror's batch pipeline (GPU): `HippoRAG.retrieve()` / `retrieve_dpr()` on random indices with
random max_batch, query counts (ragged last batches), num_to_retrieve (also beyond the engine's max_topk) and a
recognition-memory filter that keeps random subsets, drops everything or raises -- against the SAME calls made one batch at
a time through an engine proxy without the two-halves interface (retriever.iter_batched_retrieve then runs its serial form).
Everything must agree bit for bit: the pipeline only reorders when things are enqueued and waited for.

Every case also drives retriever.iter_batched_retrieve itself with a random option set (tests/option_helpers.py: random_spec --
doc filter as one row or per query, filter_scope="seeds", group_agg, group_hits, mmr_*, lexical, boost -- over a random
number of queries, num_to_retrieve also beyond max_topk) on an index of tools/soak_options.py, and holds every batch to the
reference of tests/test_gpu_pipeline_options.py: tests/pipeline_helpers.py::expected_batch over the rows of a direct
retrieve_converged(k=1) on the batch's own rows (PipelineCase.check), the serial form included.

    python tools/soak_mirror.py [--seconds 100] [--seed 1] [--cases N] [--out FILE] [--replay '<json>']

Prints one `ok` / `FAIL` line per case with its JSON (a FAIL line of an option case replays with --replay) and `SOAK OK` /
`SOAK FAILED (n)`.  A call that meets a HIP / HSA fault ends the soak: nothing more is enqueued on that device."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from hipporag_amd import synth  # noqa: E402
from hipporag_amd.graph import bf16_bits_to_float  # noqa: E402
from hipporag_amd.retriever import HippoRAG, RetrievalConfig, batched_retrieve  # noqa: E402
from tests import option_helpers as oh  # noqa: E402
from tests import pipeline_helpers as ph  # noqa: E402
from tests.group_helpers import same_bits  # noqa: E402
from tests.helpers import make_case  # noqa: E402

K_F, TOL, MAX_ITERS, NARROW, ITERS = 5, 1.5e-6, 60, 12, 20       # the pipeline's scoring arguments in PipelineCase


def _np(t):
    return None if t is None else t.cpu().numpy()


def _soak_options():
    """tools/soak_options.py as a module (its Case builds the index pieces)"""
    name = "soak_options"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
        sys.modules[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[name])
    return sys.modules[name]


class Table:
    def __init__(self, t):
        self.t = t

    def batch_encode(self, texts, instruction=None, norm=True):
        return np.stack([self.t["f" if instruction and "fact" in instruction else "p"][x] for x in texts])


class SerialEngine:
    """The engine without retrieve_converged_start: iter_batched_retrieve falls back to one call at a time."""

    def __init__(self, eng):
        object.__setattr__(self, "_eng", eng)

    def __getattr__(self, name):
        if name == "retrieve_converged_start":
            raise AttributeError(name)
        return getattr(self._eng, name)


class PipelineCase:
    """One engine of max_batch b = case["b"] over the index of a soak_options case (groups, fact sources, lexical and
    payload indexes) and the inputs of n_q queries "q0" .. "q<n_q - 1>" (default 2 b + 3: three batches, the last one
    ragged); check() holds one call of iter_batched_retrieve to tests/pipeline_helpers.py::expected_batch per batch and to
    the serial form of the loop.  strict: the conditions tests/test_gpu_pipeline_options.py rests on are asserted -- every
    per-query value of row r differs from row r - b, every batch holds a DPR-fallback row and a seeded row."""

    def __init__(self, case, dev, n_q=None, strict=True):
        from tests.lex_helpers import make_queries
        self.c = c = _soak_options().Case(case, dev)
        self.b, self.dev, self.eng, self.n, self.strict = case["b"], dev, c.eng, c.n, strict
        b = self.b
        self.serial = SerialEngine(c.eng)
        self.n_q = n_q = 2 * b + 3 if n_q is None else n_q
        self.queries = [f"q{i}" for i in range(n_q)]
        bf16 = lambda bits: torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)
        self.qf = bf16(synth.make_queries_np(c.fact_bits, n_q, seed=case["seed"] + 15)[0])
        self.qp = bf16(synth.make_queries_np(c.pass_bits, n_q, seed=case["seed"] + 16)[0])
        q = make_queries(np.random.default_rng(case["seed"] + 17), n_q)
        self.lex_q = (q[0], q[1], np.where(np.isfinite(q[2]), q[2], 1.0).astype(np.float32))
        self.facts = range(c.fact_bits.shape[0])              # any sequence of length n_facts
        self.flt = ph.fact_filter(K_F)
        self.ctx = dict(n_passages=c.n, groups=c.groups, gram=c.gram, max_topk=c.max_topk)
        self._anchors, self._flags = {}, {}
        # the per-query values move between the batches: a wrong offset cannot hide
        assert not strict or ph.offsets_differ([ph.csr_rows(self.lex_q, [r])[1].tolist() + ph.csr_rows(self.lex_q, [r])[2].tolist()
                                                for r in range(n_q)], b)

    def ppr_state_of_a_full_batch(self) -> int:
        """hrag_stats.last_ppr_state behind a plain retrieve of the first max_batch queries"""
        idx, sc = self.eng.score_facts(self.qf[:self.b], k=K_F)
        self.eng.retrieve(self.qp[:self.b], idx, sc, (idx >= 0).sum(dim=1).to(torch.int32), k=1)
        return self.eng.stats()["last_ppr_state"]

    def close(self):
        self.c.close()

    def q_tensor(self, qs, kind):
        ids = torch.tensor([ph.query_number(q) for q in qs], device=self.dev)
        return (self.qf if kind == "triple" else self.qp)[ids]

    def lexical_encode(self, qs):
        return ph.csr_rows(self.lex_q, [ph.query_number(q) for q in qs])

    def words(self, spec, allowed):
        from hipporag_amd.engine import pack_mask
        return None if allowed is None else pack_mask(allowed if spec.filter_per_query else allowed[0])

    def kw(self, spec, num, allowed, keep_all):
        """the keyword arguments of iter_batched_retrieve for the call `spec` over all the queries"""
        from hipporag_amd.boost import compile_boosts
        kw = dict(linking_top_k=K_F, damping=0.5, passage_node_weight=0.05, ppr_iters=ITERS, num_to_retrieve=num,
                  n_passages=self.n, ppr_tol=TOL, ppr_max_iters=MAX_ITERS, ppr_base_iters_narrow=NARROW,
                  keep_all_scores=keep_all)
        if allowed is not None:
            kw.update(doc_filter=self.words(spec, allowed), filter_scope=spec.filter_scope)
        if spec.group_agg is not None:
            kw.update(group_agg=spec.group_agg, group_of=self.c.groups, group_hits=spec.group_hits)
        if spec.mmr_lambda is not None:
            kw.update(mmr_lambda=spec.mmr_lambda, mmr_candidates=spec.mmr_candidates)
        if spec.lexical_weight is not None:
            kw.update(lexical_encode=self.lexical_encode, lexical_weight=spec.lexical_weight)
        if spec.boost_kind is not None:
            kw["boost"] = compile_boosts(self.c.pay, oh.boost_arg(spec, self.n_q), self.n_q)
        return kw

    def run(self, eng, kw):
        from hipporag_amd.retriever import iter_batched_retrieve
        return list(iter_batched_retrieve(eng, self.queries, self.q_tensor, self.facts, self.flt, **kw))

    def anchor(self, spec, words, lo, hi):
        """(R_j numpy [hi - lo, n], kept counts, kept fact lists): the direct k = 1 call of batch [lo, hi) under the
        batch's scoring configuration alone"""
        rows_w = None
        if spec.filter_scope == "seeds":
            rows_w = torch.from_numpy(np.ascontiguousarray(words if words.ndim == 1 else words[lo:hi]).view(np.int32))
        key = (lo, spec.lexical_weight, None if rows_w is None else rows_w.numpy().tobytes())
        if key not in self._anchors:
            qs = self.queries[lo:hi]
            ids = torch.arange(lo, hi, device=self.dev)
            idx, sc = self.eng.score_facts(self.qf[ids], k=K_F, **({} if rows_w is None else {"scope_filter": rows_w}))
            k_idx, k_sc, k_cnt, seeds = ph.kept_facts(_np(idx), _np(sc), qs, self.facts, self.flt, K_F)
            lex = ph.csr_rows(self.lex_q, range(lo, hi))
            kw = ph.anchor_kw(spec, rows_w, lex, ph.base_iters(ITERS, TOL, NARROW, hi - lo, 0.5), TOL, MAX_ITERS)
            a = self.eng.retrieve_converged(self.qp[ids], torch.from_numpy(k_idx), torch.from_numpy(k_sc), torch.from_numpy(k_cnt),
                                            link_top_k=K_F, damping=0.5, passage_node_weight=0.05, **kw)
            self._anchors[key] = (_np(a.all_scores), k_cnt, seeds)
            self._flags[key] = _np(a.flags)
        self.last_flags = self._flags[key]
        return self._anchors[key]

    def expected_assert(self, spec, words):
        """None, or the start of the message of the reference's assert the pipeline must raise (HippoRAG.py:1541, :1644):
        the first row, batch by batch, whose anchor carries flag 4 or 2 -- under filter_scope="seeds" a handful of allowed
        facts puts the weakest one, normalised to 0, among the kept ones, as the reference would on that sub-corpus."""
        for lo, hi in ph.batch_cuts(self.n_q, self.b):
            self.anchor(spec, words, lo, hi)
            for f in self.last_flags:
                if f & 4:
                    return "count_nonzero(all_phrase_weights) != len(linking_score_map)"
                if f & 2:
                    return "No phrases found in the graph for the given facts"
        return None

    # -------------------------------------------------------------------------------------- the check of one call
    def check(self, spec, num, keep_all, seed):
        """-> list of failures of the call `spec` (k = want) with num_to_retrieve = num: the pipelined form against the
        restatement per batch, and the serial form against the pipelined one"""
        allowed = ph.call_allowed(spec, self.n, self.n_q, self.c.payload_allowed)
        words = self.words(spec, allowed)
        if self.strict and spec.filter_per_query:
            assert ph.offsets_differ(allowed, self.b) and (spec.filter_kind != "payload" or ph.offsets_differ(spec.payload_ids, self.b))
        if self.strict and spec.boost_kind == "per_query":
            assert ph.offsets_differ([oh.BOOST_PROGRAMS[j] for j in spec.boost_ids], self.b)
        kw = self.kw(spec, num, allowed, keep_all)
        refusal = self.expected_assert(spec, words)
        if refusal is not None:             # both forms raise the reference's assert, and nothing else
            assert not self.strict, refusal
            bad = []
            for name, eng in (("pipelined", self.eng), ("serial", self.serial)):
                try:
                    self.run(eng, kw)
                    bad.append(f"{name}: served, AssertionError({refusal!r}) expected")
                except AssertionError as exc:
                    if not str(exc).startswith(refusal):
                        bad.append(f"{name}: AssertionError({str(exc)[:80]!r}), {refusal!r} expected")
            return bad
        got, ser = self.run(self.eng, kw), self.run(self.serial, kw)
        cuts = ph.batch_cuts(self.n_q, self.b)
        bad = []
        if [lo for lo, _ in got] != [lo for lo, _ in cuts] or [lo for lo, _ in ser] != [lo for lo, _ in cuts]:
            return [f"batches {[lo for lo, _ in got]} / {[lo for lo, _ in ser]}, {cuts} expected"]
        rng = np.random.default_rng([self.b, seed])
        for (lo, hi), (_, rows), (_, srows) in zip(cuts, got, ser):
            R, k_cnt, seeds = self.anchor(spec, words, lo, hi)
            fallback = np.flatnonzero(k_cnt == 0)
            if self.strict:
                assert len(fallback) and (k_cnt > 0).any(), (lo, k_cnt)      # a DPR-fallback row and a seeded row in every batch
            if [r[2] for r in rows] != seeds or [r[2] for r in srows] != seeds or len(rows) != hi - lo:
                bad.append(f"batch {lo}: the kept facts differ")
            sel_all, sel_hits = ph.batch_loop_rows(spec, hi - lo, fallback, rng)
            want = ph.expected_batch(R, spec, self.ctx, allowed, lo, hi, self.c.columns, rows=sel_all, hit_rows=sel_hits)
            for name in ph.FIELDS:
                g, s, w = getattr(rows, name), getattr(srows, name), want[name]
                if (g is None) != (w is None) or (s is None) != (w is None):
                    bad.append(f"batch {lo}: {name}: {'missing' if w is not None else 'unexpected'}")
                    continue
                if w is None:
                    continue
                same = (lambda x, y: same_bits(x, y)) if w.dtype == np.float32 else (lambda x, y: x.shape == y.shape and np.array_equal(x, y))
                if g.dtype != w.dtype or not same(g, s):
                    bad.append(f"batch {lo}: {name}: the pipelined form differs from the serial one")
                sel = sel_hits if name.startswith("hit_") else sel_all
                if not same(g[sel], w):
                    r = int(np.flatnonzero((g[sel] != w).reshape(len(sel), -1).any(axis=1))[0]) if g[sel].shape == w.shape else -1
                    bad.append(f"batch {lo}: {name} differs from the restatement (first at row {int(sel[r]) if r >= 0 else '?'})")
            for i in range(hi - lo):        # the per-query tuples are the rows of the arrays
                if not (np.array_equal(rows[i][0], rows.doc_idx[i]) and same_bits(rows[i][1], rows.doc_score[i])):
                    bad.append(f"batch {lo}: tuple {i} is not row {i}")
                    break
            if keep_all:
                live = allowed[lo:hi].any(axis=1) if spec.filter_scope == "seeds" else np.ones(hi - lo, bool)
                full = R if want["rows"] is None else want["rows"]
                if not isinstance(rows.repeated, bool) or srows.repeated is not True:
                    bad.append(f"batch {lo}: repeated is {rows.repeated!r} / {srows.repeated!r}")
                if not same_bits(_np(rows.all_scores)[live][:, :self.n], full[live][:, :self.n]):
                    bad.append(f"batch {lo}: all_scores is not the rows the batch ranks")
                if not same_bits(_np(rows.all_scores)[live], _np(srows.all_scores)[live]):
                    bad.append(f"batch {lo}: all_scores: the pipelined form differs from the serial one")
            elif rows.all_scores is not None:
                bad.append(f"batch {lo}: all_scores without keep_all_scores")
        return bad


def random_pipeline_call(rng, pc):
    """(CallSpec with k = want, num_to_retrieve, keep_all_scores): random_spec's draw as a call of the pipeline"""
    top, n = pc.c.max_topk, pc.n
    s = oh.random_spec(rng, dict(batch=max(pc.n_q, 1), n_passages=n, max_topk=top, fact_sources=True))
    s.entry, s.workspace, s.filter_form, s.lexical_empty = "retrieve_converged", False, "words", False
    s.fuse = s.member_ptr = s.weights = s.rrf_depth = None
    num = s.k
    if s.mmr_lambda is None and rng.random() < 0.4:
        num = int(rng.choice([top + 1, n, n + 5]))
    s.k = ph.want_of(num, n, pc.c.groups if s.group_agg is not None else None)
    if s.group_hits is not None and s.k > 20:
        s.group_hits = min(s.group_hits, 8)
    return s, num, bool(rng.random() < 0.5)


def option_case(rng, dev, replay=None):
    """One random index x one random call through the pipeline -> the record (ok, why)"""
    if replay is None:
        v = int(rng.choice([600, 1500, 4000]))
        b = int(rng.choice([1, 3, 4, 8, 9, 16, 64, 65, 70]))
        case = dict(v=v, e=int(v * rng.choice([3, 6, 10])), dim=int(rng.choice([32, 64])), pfrac=float(rng.choice([0.125, 0.3])),
                    b=b, max_topk=[10, 200, "n"][int(rng.integers(0, 3))], groups=str(rng.choice(oh.GROUP_KINDS)),
                    seed=int(rng.integers(1, 1 << 30)))
        rec = dict(kind="options", case=case, n_q=int(rng.integers(1, 3 * b + 4)), call_seed=int(rng.integers(1, 1 << 30)))
    else:
        rec = {k: replay[k] for k in ("kind", "case", "n_q", "call_seed")}
    pc = PipelineCase(rec["case"], dev, n_q=rec["n_q"], strict=False)
    fault = False
    try:
        spec, num, keep_all = random_pipeline_call(np.random.default_rng(rec["call_seed"]), pc)
        rec.update(spec=json.loads(spec.to_json()), num=num, keep_all=keep_all)
        why = pc.check(spec, num, keep_all, rec["call_seed"])
    except Exception as exc:  # noqa: BLE001
        why = [f"{type(exc).__name__}: {str(exc)[:300]}"]
        fault = _soak_options().is_gpu_fault(exc)
    finally:
        if not fault:
            pc.close()
    rec.update(ok=not why, **({"why": why[:5]} if why else {}))
    return rec, fault


def mirror_case(rng):
    """One random index through HippoRAG.retrieve / retrieve_dpr against the serial form -> the record"""
    v = int(rng.choice([800, 3000, 9000]))
    e = int(v * rng.choice([4, 10]))
    seed = int(rng.integers(1, 1 << 30))
    max_batch = int(rng.choice([1, 3, 8, 17, 64, 100, 256]))
    nq = int(rng.integers(1, 4 * max_batch + 3))
    top_k = int(rng.choice([5, 40, 200]))
    prec = str(rng.choice(["bf16", "f32"]))
    mode = int(rng.integers(0, 3))                       # filter: identity / random subsets + empties / raises sometimes
    par = dict(v=v, e=e, seed=seed, max_batch=max_batch, nq=nq, top_k=top_k, prec=prec, filter=mode)
    kg, pass_bits, fact_bits, _ = make_case(v, e, 64, seed=seed)
    qf, _ = synth.make_queries_np(fact_bits, nq, seed=seed + 3)
    qp, _ = synth.make_queries_np(pass_bits, nq, seed=seed + 4)
    queries = [f"question {i}" for i in range(nq)]
    table = {"f": dict(zip(queries, bf16_bits_to_float(qf))), "p": dict(zip(queries, bf16_bits_to_float(qp)))}

    def make_filter():
        frng = {}

        def flt(query, items, indices, len_after_rerank=None):
            r = frng.setdefault(query, np.random.default_rng(abs(hash(query)) % (1 << 31) + seed % 1000))
            if mode == 0:
                return list(indices), list(items), {}
            u = r.random()
            if mode == 2 and u < 0.1:
                raise RuntimeError("filter failed")       # the reference swallows it into the DPR fallback (:1705-1707)
            if u < 0.25:
                return [], [], {}
            keep = [j for j in range(len(indices)) if r.random() < 0.6]
            return [indices[j] for j in keep], [items[j] for j in keep], {}
        return flt

    pass_arg, fact_arg = pass_bits, fact_bits
    if prec == "f32":                                    # fp32 rows (not bf16-representable): the HRAG_F32_SPLIT engine
        def jitter(bits, sd):
            x = bf16_bits_to_float(bits)
            y = x + np.random.default_rng(sd).standard_normal(x.shape).astype(np.float32) * np.float32(2e-3)
            return (y / np.linalg.norm(y, axis=1, keepdims=True)).astype(np.float32)
        pass_arg, fact_arg = jitter(pass_bits, seed + 11), jitter(fact_bits, seed + 12)
    try:
        cfg = RetrievalConfig(embedding_precision=prec, max_batch=max_batch, retrieval_top_k=top_k)
        rag = HippoRAG.from_arrays(kg.csr, kg.passage_vertex, pass_arg, fact_arg, kg.subj_vertex, kg.obj_vertex,
                                   kg.num_chunks, global_config=cfg, embedding_model=Table(table), rerank_filter=make_filter())
        want_n = int(rng.choice([3, top_k, min(kg.n_passages, top_k + 37)]))
        got = rag.retrieve(queries, num_to_retrieve=want_n)
        dpr = rag.retrieve_dpr(queries, num_to_retrieve=want_n)
        # the same through the serial form of the loop, fresh filter state (same per-query random decisions)
        rag.rerank_filter = make_filter()
        rows = batched_retrieve(SerialEngine(rag.engine), queries, rag._q_tensor, rag.facts, rag.rerank_filter,
                                linking_top_k=cfg.linking_top_k, damping=cfg.damping, passage_node_weight=cfg.passage_node_weight,
                                ppr_iters=rag._ppr_iters(), ppr_tol=cfg.ppr_tol, ppr_max_iters=cfg.ppr_max_iters,
                                ppr_base_iters_narrow=cfg.ppr_base_iters_narrow,
                                num_to_retrieve=want_n, n_passages=len(rag.passage_node_keys))
        ok = len(got) == nq == len(rows) == len(dpr)
        why = "" if ok else "lengths"
        for i in range(nq):
            if not ok:
                break
            r = rag._build_retrieval_result(queries[i], rows[i][0], rows[i][1], want_n, rows[i][2])
            if got[i].question != queries[i] or got[i].docs != r.docs or not np.array_equal(got[i].doc_scores, r.scores) \
                    or got[i].graph_seeds != r.graph_seeds:
                ok, why = False, f"query {i} differs from the serial form"
            if len(got[i].docs) != min(want_n, kg.n_passages) or len(dpr[i].docs) != min(want_n, kg.n_passages):
                ok, why = False, f"query {i}: {len(got[i].docs)} / {len(dpr[i].docs)} documents for {want_n}"
            if np.any(np.diff(got[i].doc_scores) > 0) or np.any(np.diff(dpr[i].doc_scores) > 0):
                ok, why = False, f"query {i}: scores not sorted"
        rag.engine.close()
    except Exception as exc:  # noqa: BLE001
        ok, why = False, f"{type(exc).__name__}: {str(exc)[:300]}"
    par.update(kind="mirror", ok=ok)
    if not ok:
        par["why"] = why
    return par


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=100.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--cases", type=int, default=0, help="stop after N cases (0: only the time bound)")
    ap.add_argument("--out", default="", help="write every case's record to this JSON file (default: none is written)")
    ap.add_argument("--replay", action="append", default=[], help="an option case as printed (JSON): run exactly that one; repeatable")
    args = ap.parse_args(argv)
    rng = np.random.default_rng(args.seed)
    dev = torch.device("cuda", 0)
    t_end = time.time() + args.seconds
    records, bad = [], 0

    def note(rec):
        nonlocal bad
        records.append(rec)
        bad += 0 if rec["ok"] else 1
        print("ok  " if rec["ok"] else "FAIL", json.dumps(rec), flush=True)

    fault = False
    if args.replay:
        for text in args.replay:
            rec, fault = option_case(None, dev, replay=json.loads(text))
            note(rec)
            if fault:
                break
    else:
        while time.time() < t_end and not (args.cases and len(records) >= args.cases):
            rec, fault = option_case(rng, dev)
            note(rec)
            if fault:
                break
            if args.cases and len(records) >= args.cases:
                break
            rec = mirror_case(rng)
            note(rec)
            if not rec["ok"] and _soak_options().is_gpu_fault(Exception(rec.get("why", ""))):
                fault = True
                break
    if fault:
        print("the device faulted: the soak stops here", flush=True)
    n_opt = sum(1 for r in records if r["kind"] == "options")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"cases": records, "option_cases": n_opt, "failed": bad}, f, indent=0)
    print(f"{len(records)} cases, {n_opt} with options;", "SOAK OK" if bad == 0 else f"SOAK FAILED ({bad})")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
