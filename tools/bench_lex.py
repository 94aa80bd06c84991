"""Cost of lexical retrieval on one MI355X at configs[2] size (1M-node / 10M-edge KG, dim 768, n_passages as bench.py
builds it, batch 256, k = 200) over a synthetic Zipf vocabulary:
  1. the full HippoRAGEngine.retrieve(lexical=, lexical_weight=0.3) call against the plain retrieve on the same engine in
     the same process, in ALTERNATING runs (medians), and the pieces the lexical call adds, each alone: hrag_sim_scores,
     hrag_row_minmax, hrag_lex_scores (with and without its row min / max), hrag_lex_blend_rows;
  2. hrag_lex_scores alone against its traffic floor: B * n_passages * 4 bytes written plus the posting segments read
     (8 bytes per posting of every listed term), at the 8 TB/s DESIGN.md uses.
HIP-event medians.  Prints one JSON line and writes it to --out.

    python tools/bench_lex.py --out lex.json [--small] [--reps 20]
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_filter import _time  # noqa: E402
from tools.bench_mmr import _alternating  # noqa: E402

PEAK_BPS = 8e12


def zipf_corpus(rng, n_passages, n_terms, terms_per_passage, s=1.1):
    """Passage-major CSR of a Zipf vocabulary: every passage draws terms_per_passage term ids with P(t) ~ 1 / (t + 1)^s and
    keeps the distinct ones; BM25-like weights in (0.2, 2.2)."""
    p = 1.0 / np.arange(1, n_terms + 1) ** s
    cdf = np.cumsum(p / p.sum())
    draws = np.searchsorted(cdf, rng.random((n_passages, terms_per_passage))).astype(np.int64)
    draws = np.minimum(draws, n_terms - 1)
    draws.sort(axis=1)
    keep = np.ones_like(draws, bool)
    keep[:, 1:] = draws[:, 1:] != draws[:, :-1]
    row_ptr = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64)
    term = draws[keep].astype(np.int32)
    weight = (0.2 + 2.0 * rng.random(term.shape[0])).astype(np.float32)
    return row_ptr, term, weight, cdf


def zipf_queries(rng, cdf, batch, terms_per_query):
    t = np.minimum(np.searchsorted(cdf, rng.random((batch, terms_per_query))), len(cdf) - 1)
    q_ptr = (np.arange(batch + 1) * terms_per_query).astype(np.int32)
    return q_ptr, t.reshape(-1).astype(np.int32), np.ones(batch * terms_per_query, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tiny sizes (a rehearsal of the script, not a measurement)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--terms", type=int, default=50000)
    ap.add_argument("--terms-per-passage", type=int, default=80)
    ap.add_argument("--terms-per-query", type=int, default=12)
    args = ap.parse_args()
    import torch
    from hipporag_amd import _lib, synth
    from hipporag_amd.engine import HippoRAGEngine, LexicalIndex, row_minmax
    from hipporag_amd.lexical import invert_postings
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    name, V, E, D, B = ("small", 40000, 400000, 128, 64) if args.small else ("configs[2]", 1_000_000, 10_000_000, 768, 256)
    k, alpha = 200, 0.3
    kg = synth.make_kg(V, E, 1237)
    pass_bits = synth.make_embeddings_np(kg.n_passages, D, 1238)
    fact_bits = synth.make_embeddings_np(kg.n_facts, D, 1239)
    n_p = kg.n_passages
    rng = np.random.default_rng(1240)
    row_ptr, term, weight, cdf = zipf_corpus(rng, n_p, args.terms, args.terms_per_passage)
    term_ptr, post_doc, post_w = invert_postings(n_p, args.terms, row_ptr, term, weight)
    q = zipf_queries(rng, cdf, B, args.terms_per_query)
    seg = int(np.diff(term_ptr)[q[1]].sum())                      # postings of every listed term, over the whole batch
    res = dict(tool="bench_lex", config=name, V=V, E=E, D=D, batch=B, n_passages=n_p, k=k, lexical_weight=alpha, reps=args.reps,
               n_terms=args.terms, postings=int(post_doc.shape[0]), terms_per_query=args.terms_per_query,
               postings_read_per_batch=seg, peak_TBps=PEAK_BPS / 1e12)
    stream = torch.cuda.current_stream().cuda_stream
    to_q = lambda bits: torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)  # noqa: E731
    with LexicalIndex.from_postings(n_p, term_ptr, post_doc, post_w) as ix, \
            HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                           max_batch=B, max_topk=k) as eng:
        eng.set_lexical_index(ix)
        qf = to_q(synth.make_queries_np(fact_bits, B, seed=1)[0])
        qp = to_q(synth.make_queries_np(pass_bits, B, seed=2)[0])
        idx, sc = eng.score_facts(qf, k=5)
        cnt = torch.full((B,), 5, dtype=torch.int32, device=dev)

        def retrieve(**kw):
            return eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=k, want_residual=False, **kw)

        res["retrieve_ms"], res["retrieve_lexical_ms"] = _alternating(
            retrieve, lambda: retrieve(lexical=q, lexical_weight=alpha), args.reps)
        res["lexical_extra_ms"] = round(res["retrieve_lexical_ms"] - res["retrieve_ms"], 4)
        # the pieces, each alone
        d_q = [torch.from_numpy(a).to(dev) for a in q]
        rows = torch.empty((B, n_p), dtype=torch.float32, device=dev)
        mn_l, mx_l = (torch.empty((B,), dtype=torch.float32, device=dev) for _ in range(2))

        def lex(mn, mx):
            _lib.check(lib.hrag_lex_scores(ix._handle, d_q[0].data_ptr(), d_q[1].data_ptr(), d_q[2].data_ptr(), d_q[1].shape[0],
                                           B, rows.data_ptr(), n_p, mn, mx, stream))

        res["lex_scores_ms"] = _time(lambda: lex(None, None), args.reps)
        res["lex_scores_minmax_ms"] = _time(lambda: lex(mn_l.data_ptr(), mx_l.data_ptr()), args.reps)
        floor_ms = (B * n_p * 4 + seg * 8) / PEAK_BPS * 1e3
        res["lex_scores_floor_ms"] = round(floor_ms, 5)
        res["lex_scores_over_floor"] = round(res["lex_scores_ms"] / floor_ms, 2)
        res["sim_scores_ms"] = _time(lambda: eng.sim_scores("passages", qp), args.reps)
        dense = eng.sim_scores("passages", qp)
        res["row_minmax_ms"] = _time(lambda: row_minmax(dense), args.reps)
        mn_d, mx_d = row_minmax(dense)
        out = torch.empty_like(dense)
        res["blend_ms"] = _time(lambda: _lib.check(lib.hrag_lex_blend_rows(
            dense.data_ptr(), n_p, rows.data_ptr(), n_p, B, n_p, mn_d.data_ptr(), mx_d.data_ptr(), mn_l.data_ptr(),
            mx_l.data_ptr(), alpha, out.data_ptr(), n_p, stream)), args.reps)
        res["blend_floor_ms"] = round(3 * B * n_p * 4 / PEAK_BPS * 1e3, 5)
        res["retrieve_scored_ms"] = _time(lambda: eng.retrieve_scored(out, idx, sc, cnt, ppr_iters=20, k=k), args.reps)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
