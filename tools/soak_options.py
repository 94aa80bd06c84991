#!/usr/bin/env python
"""Randomised soak of COMPOSED retrieve options (GPU): random small indexes x batch sizes x random servable calls of
retrieve / retrieve_scored / dense_retrieve / retrieve_converged / last_fused with the doc filter (bool, packed words,
PayloadFilter; one row or per query), filter_scope="seeds", group_agg, group_hits, fusion, mmr_*, lexical and boost drawn
together (tests/option_helpers.py: random_spec, plan), every output held to ONE numpy restatement of the whole call,
option_helpers.expected_outputs, which composes the per-feature restatements over the score rows R the call leaves on the
handle (last_doc_scores).  Per call: ids exactly, floats bit for bit, the -1 / 0 padding included; flags / residual /
iters_used bit-identical to the plain call of the same scoring configuration (None behind last_fused); last_doc_scores
after the call bit-identical to R (to the fused rows after a fusion): no option may change scoring.

boost= (one term list or one per query, as the grammar or as compile_boosts' program) is the one option that rewrites the
rows: a boosted call is held to expected_outputs over boost_rows_np of the UNBOOSTED call's R (of the fused rows behind
last_fused; of the min-max of the raw rows on dense_retrieve), last_doc_scores after it bit-identical to those boosted rows
on every row, flags / residual / iters_used still the plain call's, and behind a workspace call the root handle's rows
bit-identical to what they were.

The rankings (plain, filtered, grouped), the fused rows and R itself are checked on every row.  The Python-loop
restatements check at most 8 rows per call -- the hit arrays always, every field of an MMR call: row 0, the last row, every
DPR-fallback row among the first 16, the rest drawn from the case's seed -- the selection is part of the replayable case.
A call that meets a HIP / HSA fault ends the soak: nothing more is enqueued on that device.

An ungrouped dense_retrieve leaves no rows on the handle: its R is read behind the grouped call of the same scoring
configuration (the min-max of the blended rows under lexical), and its ids are held to the ranking of the RAW rows
(hrag_sim_scores / the blend), which is what that call ranks -- two raw scores an ulp apart can share one normalised score
(in the "seeds" scope the rows are normalised over the allowed passages before the ranking: there the ids follow R).

This tool does NOT re-check R against the oracle: that is tools/soak_random.py's job and stays there.  A lexical call's R
is held to retrieve_scored over the numpy blend (lex_helpers.blend_np of sim_scores and lex_scores_np; behind
retrieve_converged the rows that needed no repeat, against retrieve_scored with the contract's sweep budget), and
lexical_scores(want_minmax=True) to lex_scores_np / row_minmax_np bit for bit.

    python tools/soak_options.py [--seconds 150] [--seed 1] [--cases N] [--batches 1,8] [--out FILE] [--replay '<json>']

Prints one `ok` / `FAIL` line per call with its JSON (a FAIL line replays with --replay) and `SOAK OK` / `SOAK FAILED (n)`."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from hipporag_amd import _lib, synth  # noqa: E402
from hipporag_amd.boost import compile_boosts  # noqa: E402
from hipporag_amd.engine import HippoRAGEngine, LexicalIndex, pack_mask  # noqa: E402
from hipporag_amd.payload import PayloadIndex, compile_filters, encode_columns  # noqa: E402
from tests import option_helpers as oh  # noqa: E402
from tests.group_helpers import random_groups, same_bits  # noqa: E402
from tests.helpers import make_case  # noqa: E402
from tests.lex_helpers import blend_np, lex_scores_np, make_index, make_queries, minmax_np, row_minmax_np  # noqa: E402
from tests.payload_helpers import columns_of, random_metadata  # noqa: E402

CALLS_PER_CASE = 6
FIELDS = ("doc_idx", "doc_score", "group_idx", "hit_idx", "hit_score", "mmr_value")


def _bf16(bits, dev):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _bits_equal(a, b):
    """torch tensors (or None) bit for bit"""
    if a is None or b is None:
        return a is None and b is None
    v = (lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t)
    return a.shape == b.shape and bool(torch.equal(v(a), v(b)))


def random_sources(n_f, n_p, rng, unsourced=0.1):
    """fact -> source passages as tests/test_gpu_payload.py::_random_sources builds them (0 .. 3 sources, a tenth of the
    facts without one), without the per-fact loop."""
    cnt = np.where(rng.random(n_f) < unsourced, 0, rng.integers(1, 4, n_f))
    row_ptr = np.zeros(n_f + 1, np.int64)
    row_ptr[1:] = np.cumsum(cnt)
    return row_ptr, rng.integers(0, n_p, int(row_ptr[-1])).astype(np.int32)


class Case:
    """One index, one engine (+ one workspace) with groups, fact sources, a lexical and a payload index, and the inputs of
    a batch; check_call / check_refusal hold one CallSpec to option_helpers."""

    def __init__(self, case, dev):
        self.case, self.dev = case, dev
        lim = oh.case_limits(case)
        kg, pass_bits, fact_bits, _ = make_case(case["v"], case["e"], case["dim"], seed=case["seed"], passage_frac=case["pfrac"])
        self.n = n = kg.n_passages
        assert n == lim["n_passages"]
        self.max_topk, self.dim = lim["max_topk"], case["dim"]
        rng = np.random.default_rng(case["seed"] ^ 0xC0FFEE)
        self.groups = random_groups(rng, n, case["groups"])
        self.eng = HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                                  max_batch=case["b"], max_topk=self.max_topk)
        self.eng.set_passage_groups(self.groups)
        self.eng.set_fact_sources(*random_sources(kg.n_facts, n, rng))
        self.lex_host = make_index(rng, n)
        self.lex = LexicalIndex.from_postings(n, *self.lex_host)
        self.eng.set_lexical_index(self.lex)
        self.columns = encode_columns(columns_of(random_metadata(rng, n), ["year", "user", "score", "flag", "mixed"]), n)
        self.pay = PayloadIndex(self.columns)
        self.eng.set_payload_index(self.pay)
        self.payload_allowed = oh.payload_allowed_fn(self.columns)
        self.ws = self.eng.workspace()
        self.pass_dev = _bf16(pass_bits, dev).contiguous()
        self.fact_bits, self.pass_bits = fact_bits, pass_bits
        self.set_batch(case["b"])

    def close(self):
        self.eng.close()
        self.lex.close()
        self.pay.close()

    def set_batch(self, b):
        """The inputs of a batch of b <= max_batch queries: about a quarter of the rows are DPR fallbacks."""
        seed, dev = self.case["seed"], self.dev
        rng = np.random.default_rng([seed, b])        # a function of (case, b): not of the batches set before
        self.b = b
        self.qf = _bf16(synth.make_queries_np(self.fact_bits, b, seed=seed + 5)[0], dev)
        self.qp = _bf16(synth.make_queries_np(self.pass_bits, b, seed=seed + 6)[0], dev)
        self.idx, self.sc = self.eng.score_facts(self.qf, k=5)
        keep = rng.random(b) >= 0.25
        if b >= 4:
            keep[int(rng.integers(0, b))] = False
        self.keep = torch.from_numpy(keep).to(dev)
        self.cnt = torch.where(self.keep, (self.idx >= 0).sum(dim=1), 0).to(torch.int32)
        self.fallback = np.flatnonzero(~keep)
        q = make_queries(rng, b)
        self.lex_q = (q[0], q[1], np.where(np.isfinite(q[2]), q[2], 1.0).astype(np.float32))       # NaN rows: not this tool's
        self.lex_none = (np.zeros(b + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
        self.dense_dev = self.eng.sim_scores("passages", self.qp)
        self.dense = _np(self.dense_dev)
        self._lex_rows, self._anchors, self._plain = {}, {}, None

    # -------------------------------------------------------------------------------------- pieces of a call
    def gram(self, ids):
        """hrag_gram_rows over candidate ids [r, c] -> fp32 [r, c, c] (tests/test_gpu_mmr.py holds the kernel to fp64)"""
        ids = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(self.dev)
        r, c = ids.shape
        out = torch.zeros((r, c, c), dtype=torch.float32, device=self.dev)
        if r:
            _lib.check(_lib.load().hrag_gram_rows(self.pass_dev.data_ptr(), self.n, self.dim, 0, 0, ids.data_ptr(), r, c,
                                                  out.data_ptr(), c, torch.cuda.current_stream().cuda_stream))
        return _np(out)

    def lex_queries(self, spec):
        return self.lex_none if spec.lexical_empty else self.lex_q

    def lex_rows(self, spec):
        """the numpy lexical rows of the spec's queries, and the device's held to them (once per case and query set)"""
        key = spec.lexical_empty
        if key not in self._lex_rows:
            q = self.lex_queries(spec)
            rows = lex_scores_np(self.n, *self.lex_host, *q)
            got, mn, mx = self.eng.lexical_scores(*q, want_minmax=True)
            wmn, wmx = row_minmax_np(rows)
            ok = same_bits(_np(got), rows) and same_bits(_np(mn), wmn) and same_bits(_np(mx), wmx)
            self._lex_rows[key] = (rows, ok)
        return self._lex_rows[key]

    def filter_arg(self, spec, allowed, per_row=None):
        """the doc filter in the spec's form (per_row: the rows to hand over instead, as a bool tensor)"""
        if allowed is None:
            return None
        if per_row is not None:
            return torch.from_numpy(np.array(allowed[per_row], dtype=bool)).to(self.dev)
        a = allowed if spec.filter_per_query else allowed[0]
        if spec.filter_form == "bool":
            return torch.from_numpy(np.array(a, dtype=bool)).to(self.dev)
        if spec.filter_form == "words":
            return torch.from_numpy(pack_mask(a).view(np.int32)).to(self.dev)
        ids = spec.payload_ids[:allowed.shape[0]]
        return compile_filters(self.pay, [oh.PAYLOAD_FILTERS[i] for i in ids] if spec.filter_per_query
                               else oh.PAYLOAD_FILTERS[ids[0]])

    def scoring(self, spec, allowed, h, raw=False):
        """(kept facts, keyword arguments) of the spec's scoring configuration: the scope with its filter (the kept facts
        then come from score_facts(scope_filter=)) and the lexical blend.  raw: nothing is prepared (a refused call)."""
        kw, kept = {}, (self.idx, self.sc, self.cnt)
        if spec.filter_scope == "seeds":
            kw["filter_scope"] = "seeds"
            if allowed is not None:
                qmap = None
                if spec.entry == "last_fused":          # each member row is scored under its question's filter row
                    mp = np.asarray(spec.member_ptr)
                    qmap = np.repeat(np.arange(len(mp) - 1), np.diff(mp))
                kw["doc_filter"] = self.filter_arg(spec, allowed, qmap)
                if not raw:
                    idx, sc = h.score_facts(self.qf, k=5, scope_filter=kw["doc_filter"])
                    kept = (idx, sc, torch.where(self.keep, (idx >= 0).sum(dim=1), 0).to(torch.int32))
        if spec.lexical_weight is not None:
            kw.update(lexical=self.lex_queries(spec), lexical_weight=spec.lexical_weight)
        return kept, kw

    def anchor(self, spec, h, kept, kw):
        """(R numpy [B, n], the plain output or None, failures, raw): the k = 1 call of the spec's scoring configuration.
        raw: the rows an ungrouped dense_retrieve ranks (hrag_sim_scores, or the blended rows); None on the other entries."""
        key = (spec.entry, spec.workspace, spec.lexical_weight, spec.lexical_empty,
               None if spec.filter_scope != "seeds" else (spec.filter_kind, spec.filter_form, spec.filter_per_query,
                                                          spec.filter_seed, tuple(spec.payload_ids or ()),
                                                          tuple(spec.member_ptr or ()), spec.k if spec.filter_kind == "few" else 0))
        if key in self._anchors and spec.entry != "last_fused":
            return self._anchors[key]
        bad, a, raw = [], None, None
        if spec.entry == "retrieve_converged":
            a = h.retrieve_converged(self.qp, *kept, k=1, ppr_tol=1.5e-6, ppr_max_iters=60, want_all_scores=True, **kw)
            R = _np(a.all_scores)
        elif spec.entry == "retrieve_scored":
            a = h.retrieve_scored(self.dense_dev, *kept, k=1, **kw)
            R = _np(h.last_doc_scores(self.b))
        elif spec.entry == "dense_retrieve":
            if spec.lexical_weight is not None:         # no rows are left on the handle: the min-max of the blended rows
                rows, ok = self.lex_rows(spec)
                raw = bl = blend_np(self.dense, rows, spec.lexical_weight)
                R = np.stack([minmax_np(r, *[v[0] for v in row_minmax_np(r[None])]) for r in bl])
                if not ok:
                    bad.append("lexical_scores differs from lex_scores_np / row_minmax_np")
            else:
                h.dense_retrieve(self.qp, k=1, group_agg="max", **kw)
                R, raw = _np(h.last_doc_scores(self.b)), self.dense
        else:
            a = h.retrieve(self.qp, *kept, k=1, **kw)
            R = _np(h.last_doc_scores(self.b))
        if spec.lexical_weight is not None and spec.entry == "retrieve_converged" and key not in self._anchors:
            # the contract's first run is retrieve_scored over the blended rows with the same sweep budget: the rows that
            # needed no repeat (flags and iters_used as that call's) are held to it over blend_np's rows
            rows, ok = self.lex_rows(spec)
            if not ok:
                bad.append("lexical_scores differs from lex_scores_np / row_minmax_np")
            blended = torch.from_numpy(blend_np(self.dense, rows, spec.lexical_weight)).to(self.dev)
            a2 = h.retrieve_scored(blended, *kept, k=1, ppr_tol=1.5e-6, ppr_max_iters=60,
                                   **{n_: v for n_, v in kw.items() if n_ not in ("lexical", "lexical_weight")})
            R2 = _np(h.last_doc_scores(self.b))
            same = _np((a2.flags == a.flags) & (a2.iters_used == a.iters_used)).astype(bool)
            if not same.any():
                bad.append("retrieve_converged(lexical=): every row was repeated, none can be held to retrieve_scored")
            elif not same_bits(R2[same], R[same]):
                bad.append("R of retrieve_converged(lexical=) differs from retrieve_scored over blend_np's rows")
        if spec.lexical_weight is not None and spec.entry in ("retrieve", "retrieve_scored", "last_fused") \
                and key not in self._anchors:
            rows, ok = self.lex_rows(spec)
            if not ok:
                bad.append("lexical_scores differs from lex_scores_np / row_minmax_np")
            blended = torch.from_numpy(blend_np(self.dense, rows, spec.lexical_weight)).to(self.dev)
            h.retrieve_scored(blended, *kept, k=1)
            R2 = _np(h.last_doc_scores(self.b))
            if not same_bits(R2, R):
                bad.append("R of the lexical call differs from retrieve_scored over blend_np's rows")
            if spec.entry == "last_fused":              # the member rows again: the check above replaced them
                a = h.retrieve(self.qp, *kept, k=1, **kw)
        self._anchors[key] = (R, a, bad, raw)
        return self._anchors[key]

    @staticmethod
    def boost_kind(spec):
        """None, "one" or "per_query" (a spec that carries no boost fields is a call without a boost)"""
        return getattr(spec, "boost_kind", None)

    def boost_arg(self, spec):
        """boost= in the spec's form: the grammar itself, or its BoostProgram"""
        arg = oh.boost_arg(spec, spec.rows(self.b))
        return compile_boosts(self.pay, arg) if spec.boost_form == "program" else arg

    def invoke(self, spec, h, flt, kept, skw):
        """make the call -> (fields dict of torch tensors, flags triple or None, the rows the handle holds afterwards)"""
        kw = dict(k=spec.k, group_agg=spec.group_agg, group_hits=spec.group_hits, mmr_lambda=spec.mmr_lambda,
                  mmr_candidates=spec.mmr_candidates)
        if flt is not None:
            kw["doc_filter"] = flt
        if self.boost_kind(spec) is not None:
            kw["boost"] = self.boost_arg(spec)
        if spec.entry == "last_fused":
            out = h.last_fused(spec.member_ptr, weights=spec.weights, fuse=spec.fuse, rrf_c=spec.rrf_c, rrf_depth=spec.rrf_depth,
                               **kw)
            return out, h.last_doc_scores(len(spec.member_ptr) - 1)
        kw.update(skw)                                   # (the scope's filter is the call's filter)
        if spec.entry == "dense_retrieve":
            t = h.dense_retrieve(self.qp, **kw)
            d = dict.fromkeys(FIELDS + ("flags", "residual", "iters_used"))
            if spec.mmr_lambda is not None:
                d["mmr_value"], t = t[-1], t[:-1]
            if spec.group_agg is None:
                d["doc_idx"], d["doc_score"] = t
            else:
                d["group_idx"], d["doc_score"], d["doc_idx"] = t[:3]
                if spec.group_hits is not None:
                    d["hit_idx"], d["hit_score"] = t[3:]
            out = argparse.Namespace(**d)
            return out, (h.last_doc_scores(self.b) if spec.group_agg is not None else None)
        if spec.entry == "retrieve_converged":
            out = h.retrieve_converged(self.qp, *kept, ppr_tol=1.5e-6, ppr_max_iters=60, want_all_scores=True, **kw)
            return out, out.all_scores
        if spec.entry == "retrieve_scored":
            out = h.retrieve_scored(self.dense_dev, *kept, **kw)
        else:
            out = h.retrieve(self.qp, *kept, **kw)
        return out, h.last_doc_scores(self.b)

    # -------------------------------------------------------------------------------------- the two checks
    def check_call(self, spec, row_rng):
        """-> list of failures (empty: the call is the restatement)"""
        h = self.ws if spec.workspace else self.eng
        rows = spec.rows(self.b)
        allowed = oh.make_allowed(spec, self.n, rows, self.payload_allowed)
        kept, skw = self.scoring(spec, allowed, h)
        flt = self.filter_arg(spec, allowed)
        R, a, bad, raw = self.anchor(spec, h, kept, skw)
        bad = list(bad)
        boosted = self.boost_kind(spec) is not None
        root = None
        if boosted and spec.workspace:                  # the root handle holds rows of its own: the workspace's boost must
            self.eng.retrieve(self.qp, self.idx, self.sc, self.cnt, k=1)       # leave them as they are
            root = self.eng.last_doc_scores(self.b)
        out, after = self.invoke(spec, h, flt, kept, skw)
        if root is not None and not _bits_equal(self.eng.last_doc_scores(self.b), root):
            bad.append("a boosted workspace call changed the root handle's rows")
        torch.cuda.synchronize()
        fb = [] if spec.entry == "last_fused" else self.fallback
        sel_all, sel_hits = oh.loop_rows(spec, rows, fb, row_rng)
        want = oh.expected_outputs(R, spec, dict(n_passages=self.n, groups=self.groups, allowed=allowed, gram=self.gram,
                                                 max_topk=self.max_topk, rank_rows=raw,
                                                 boost=oh.boost_ctx(spec, self.columns, rows) if boosted else None),
                                   rows=sel_all, hit_rows=sel_hits)
        for name in FIELDS:
            g, w = _np(getattr(out, name)), want[name]
            sel = sel_hits if name.startswith("hit_") else sel_all
            if (g is None) != (w is None):
                bad.append(f"{name}: {'missing' if g is None else 'unexpected'}")
            elif w is not None:
                g = g[sel]
                same = same_bits(g, w) if w.dtype == np.float32 else (g.shape == w.shape and np.array_equal(g, w))
                if not same:
                    r = int(np.flatnonzero((g != w).reshape(len(sel), -1).any(axis=1))[0]) if g.shape == w.shape else -1
                    bad.append(f"{name} differs (first at row {int(sel[r]) if r >= 0 else '?'} of {len(sel)} checked)")
        for name in ("flags", "residual", "iters_used"):
            g = getattr(out, name)
            w = None if a is None or spec.entry == "last_fused" else getattr(a, name)
            if not _bits_equal(g, w):
                bad.append(f"{name} differs from the plain call's")
        if boosted and after is not None:             # the handle holds the boosted rows (boosted fused rows; all_scores)
            live = np.ones(rows, bool)
            if spec.filter_scope == "seeds" and spec.entry != "last_fused":    # (an empty allowed set leaves a row without meaning)
                live = allowed.any(axis=1)
            if not same_bits(_np(after)[live][:, :self.n], want["rows"][live]):
                bad.append("last_doc_scores after the boosted call is not the boosted rows")
        elif after is not None:
            if spec.entry == "last_fused":
                if not same_bits(_np(after)[:, :self.n], want["fused"]):
                    bad.append("last_doc_scores after the fusion is not the fused rows")
            else:
                live = np.ones(self.b, bool)
                if spec.filter_scope == "seeds":        # (an empty allowed set leaves a row without meaning)
                    live = allowed.any(axis=1)
                if not same_bits(_np(after)[live][:, :self.n], R[live][:, :self.n]):
                    bad.append("last_doc_scores after the call differs from R: an option changed scoring")
        return bad

    def plain(self):
        o = self.eng.retrieve(self.qp, self.idx, self.sc, self.cnt, k=10)
        return [o.doc_idx, o.doc_score, o.flags, o.residual, o.iters_used]

    def check_refusal(self, spec, err):
        """The call must raise err = (type, argument name) and leave a following plain call bit-identical."""
        h = self.ws if spec.workspace else self.eng
        if self._plain is None:
            self._plain = self.plain()
        allowed = oh.make_allowed(spec, self.n, spec.rows(self.b), self.payload_allowed)
        bad = []
        try:
            kept, skw = self.scoring(spec, allowed, h, raw=True)
            if spec.entry == "last_fused":
                h.retrieve(self.qp, *kept, k=1, **skw)
            self.invoke(spec, h, self.filter_arg(spec, allowed), kept, skw)
            bad.append(f"served, {err[0].__name__} naming {err[1]} expected")
        except Exception as exc:  # noqa: BLE001
            if not isinstance(exc, err[0]) or isinstance(exc, NotImplementedError) != (err[0] is NotImplementedError) \
                    or err[1] not in str(exc):
                bad.append(f"{type(exc).__name__}: {exc} -- {err[0].__name__} naming {err[1]} expected")
        if not all(_bits_equal(x, y) for x, y in zip(self.plain(), self._plain)):
            bad.append("the plain call after the refusal differs from the one before")
        return bad


class GpuFault(Exception):
    """A call met a HIP / HSA fault: the soak ends there (args[0]: the case's failed calls so far)."""


def is_gpu_fault(exc) -> bool:
    text = str(exc).lower()
    return any(w in text for w in ("hip error", "hsa_status", "illegal memory access", "device-side assert", "hardware exception",
                                   "unspecified launch failure", "hiperror"))


def run_case(case, specs, dev, only=None, out_lines=None):
    """-> number of failed calls; one line per call.  GpuFault after a call that met a device fault."""
    failed, fault = 0, False
    try:
        c = Case(case, dev)
    except Exception as exc:  # noqa: BLE001
        print("FAIL", json.dumps(dict(case=case, error=f"{type(exc).__name__}: {exc}")), flush=True)
        if is_gpu_fault(exc):
            raise GpuFault(1)
        return 1
    try:
        for i, spec in enumerate(specs):
            if only is not None and i != only:
                continue
            rec = dict(case=case, call=i, spec=json.loads(spec.to_json()), boost_kind=Case.boost_kind(spec))
            fault = False
            try:
                why = c.check_call(spec, np.random.default_rng([case["seed"], i]))
            except Exception as exc:  # noqa: BLE001
                why = [f"{type(exc).__name__}: {exc}"]
                fault = is_gpu_fault(exc)
            if why:
                failed += 1
                rec["why"] = why
            print("FAIL" if why else "ok  ", json.dumps(rec), flush=True)
            if out_lines is not None:
                out_lines.append(rec)
            if fault:           # nothing more is enqueued on a device that faulted: no further call, no close, no new engine
                raise GpuFault(failed)
    finally:
        if not fault:
            c.close()
    return failed


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=150.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--cases", type=int, default=0, help="the first N cases of the seeded plan (0: only the time bound)")
    ap.add_argument("--batches", default="", help="b1,b2,...: run only the plan's cases of these batch sizes")
    ap.add_argument("--calls", type=int, default=CALLS_PER_CASE, help="calls per case")
    ap.add_argument("--out", default="", help="write every call's record to this JSON file (default: none is written)")
    ap.add_argument("--replay", action="append", default=[], help="a call as printed (JSON): run exactly that one; repeatable")
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    t_end = time.time() + args.seconds
    only_b = {int(x) for x in args.batches.split(",") if x}
    lines, bad, n_cases = [], 0, 0
    try:
        if args.replay:
            for text in args.replay:
                rec = json.loads(text)
                spec = oh.CallSpec.from_dict(rec["spec"])
                n_cases += 1
                bad += run_case(rec["case"], [None] * rec["call"] + [spec], dev, only=rec["call"], out_lines=lines)
        else:
            for i, (case, specs) in enumerate(oh.iter_plan(args.seed, args.calls)):
                if (args.cases and i >= args.cases) or time.time() >= t_end:
                    break
                if only_b and case["b"] not in only_b:
                    continue
                n_cases += 1
                bad += run_case(case, specs, dev, out_lines=lines)
    except GpuFault as stop:
        bad += stop.args[0]
        print("the device faulted: the soak stops here", flush=True)
    n_boosted = sum(1 for r in lines if r.get("boost_kind"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"calls": lines, "cases": n_cases, "failed": bad, "boosted": n_boosted,
                       "boosted_entries": sorted({r["spec"]["entry"] for r in lines if r.get("boost_kind")}),
                       "boosted_batches": sorted({r["case"]["b"] for r in lines if r.get("boost_kind")})}, f, indent=0)
    print(f"{n_cases} cases, {len(lines)} calls, {n_boosted} boosted;", "SOAK OK" if bad == 0 else f"SOAK FAILED ({bad})")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
