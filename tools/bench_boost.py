"""Cost of boosted retrieval on one MI355X at configs[2] size (1M-node / 10M-edge KG, dim 768, n_passages as bench.py builds
it, batch 256, k = 200) with a three-term program -- a keyword condition `mul`, an exp decay over an integer timestamp, a
`sqrt` field `add` -- over three synthetic columns:
  (a) HippoRAGEngine.retrieve and (b) retrieve(boost=), in ALTERNATING runs: the added time per call;
  (c) hrag_boost_rows alone over [B, n_passages] rows against its traffic floor -- the rows read once and written once at the
      8 TB/s DESIGN.md uses (the columns, 8 bytes per passage and term, are shared by the batch and come from L2 / MALL) --
      and against the project's own yardstick for the same row traffic, hrag_lex_blend_rows, measured in the same run;
      then with one term at a time, which says whether the fp64 arithmetic, the IN-set search or the column reads set it;
  (d) the ranking alone (hrag_last_boosted with a program without terms): what the discarded first ranking of (b) costs;
  (e) the host alternative: last_doc_scores read back to the host (the numpy arithmetic not even counted).
HIP-event medians.  Prints one JSON line and writes it to --out.

    python tools/bench_boost.py --out profiles/boost_cfg2_bench_boost.json [--small] [--reps 20]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_filter import _time  # noqa: E402
from tools.bench_mmr import _alternating  # noqa: E402

PEAK_BPS = 8e12
N_KW = 1000
NOW = 1_700_000_000                      # the newest timestamp (seconds); the passages spread over the five years before it
DAY = 86400


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tiny sizes (a rehearsal of the script, not a measurement)")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from hipporag_amd import _lib, synth
    from hipporag_amd.boost import compile_boosts
    from hipporag_amd.engine import HippoRAGEngine, _stream, row_minmax
    from hipporag_amd.payload import PayloadIndex
    dev = torch.device("cuda", 0)
    name, V, E, D, B = ("small", 40000, 400000, 128, 64) if args.small else ("configs[2]", 1_000_000, 10_000_000, 768, 256)
    k = 200
    kg = synth.make_kg(V, E, 1237)
    pass_bits = synth.make_embeddings_np(kg.n_passages, D, 1238)
    fact_bits = synth.make_embeddings_np(kg.n_facts, D, 1239)
    n_p = kg.n_passages
    rng = np.random.default_rng(1243)
    ts = (NOW - rng.integers(0, 5 * 365 * DAY, n_p)).astype(np.int64)
    kw = [f"k{v}" for v in rng.integers(0, N_KW, n_p)]
    cites = rng.integers(0, 400, n_p).astype(np.float64)
    terms = {"keyword mul": {"if": {"source": [f"k{v}" for v in rng.choice(N_KW, 300, replace=False)]}, "mul": 1.5},
             "exp decay": {"decay": {"field": "ts", "origin": NOW, "scale": 90 * DAY, "offset": 7 * DAY, "kind": "exp"}, "mul": 1.0},
             "sqrt add": {"field": "cites", "modifier": "sqrt", "add": 1e-5}}
    res = dict(tool="bench_boost", config=name, V=V, E=E, D=D, batch=B, n_passages=n_p, k=k, reps=args.reps,
               peak_TBps=PEAK_BPS / 1e12, terms=list(terms))
    to_q = lambda bits: torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)  # noqa: E731
    t0 = time.perf_counter()
    ix = PayloadIndex.from_columns({"ts": ts, "source": kw, "cites": cites}, n_p)
    res["index_build_s"] = round(time.perf_counter() - t0, 3)
    with ix, HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                            max_batch=B, max_topk=k) as eng:
        eng.set_payload_index(ix)
        qf = to_q(synth.make_queries_np(fact_bits, B, seed=1)[0])
        qp = to_q(synth.make_queries_np(pass_bits, B, seed=2)[0])
        idx, sc = eng.score_facts(qf, k=5)
        cnt = torch.full((B,), 5, dtype=torch.int32, device=dev)
        t0 = time.perf_counter()
        prog = compile_boosts(ix, list(terms.values()))
        res["compile_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        none = compile_boosts(ix, [])

        def retrieve(boost=None):
            return eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=k, want_residual=False, boost=boost)

        plain, boosted = retrieve(), retrieve(prog)
        res["top1_moved"] = round(float((plain.doc_idx[:, 0] != boosted.doc_idx[:, 0]).float().mean().item()), 3)
        # (a) and (b)
        a_ms, b_ms = _alternating(retrieve, lambda: retrieve(prog), args.reps)
        res["retrieve_plain_ms"], res["retrieve_boost_ms"], res["boost_extra_ms"] = a_ms, b_ms, round(b_ms - a_ms, 4)
        # (c) the kernel alone; the rows are rewritten in place every run, so they are refilled now and then to stay finite
        rows = eng.last_doc_scores(B).clone()
        work = rows.clone()

        def kernel(p):
            work.copy_(rows)
            return _time(lambda: eng.boost_rows(work, p), args.reps)
        res["copy_rows_ms"] = _time(lambda: work.copy_(rows), args.reps)
        res["boost_rows_ms"] = kernel(prog)
        floor_ms = 2 * B * n_p * 4 / PEAK_BPS * 1e3
        res["boost_rows_floor_ms"] = round(floor_ms, 6)
        res["boost_rows_over_floor"] = round(res["boost_rows_ms"] / floor_ms, 1)
        for label, item in terms.items():
            res[f"boost_rows_{label.replace(' ', '_')}_ms"] = kernel(compile_boosts(ix, [item]))
        res["boost_rows_const_ms"] = kernel(compile_boosts(ix, [{"mul": 1.5}]))          # the row traffic and nothing else
        mn, mx = row_minmax(rows, n_p)
        lib = _lib.load()
        res["lex_blend_rows_ms"] = _time(lambda: _lib.check(lib.hrag_lex_blend_rows(
            work.data_ptr(), work.stride(0), rows.data_ptr(), rows.stride(0), B, n_p, mn.data_ptr(), mx.data_ptr(), mn.data_ptr(),
            mx.data_ptr(), 0.5, work.data_ptr(), work.stride(0), _stream())), args.reps)
        res["boost_rows_over_lex_blend"] = round(res["boost_rows_ms"] / res["lex_blend_rows_ms"], 2)
        # (d) the ranking alone: what the discarded first ranking costs
        retrieve()
        res["ranking_alone_ms"] = _time(lambda: eng.last_boosted(none, B, k=k), args.reps)
        # (e) the host alternative's read-back
        res["host_readback_ms"] = _time(lambda: eng.last_doc_scores(B).cpu(), max(3, args.reps // 4))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
