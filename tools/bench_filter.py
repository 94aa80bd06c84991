"""Cost of the doc filter on one MI355X: hrag_retrieve against hrag_retrieve_filtered at configs[2] (1M-node / 10M-edge
KG, 1M x 768 bf16) with k = 200, batch 256, 64 and 1, at selectivities 1, 0.5, 0.01 and 1e-4, with one filter row per
query and with one broadcast row; and the ranking alone (hrag_topk_rows_ws against hrag_topk_rows_masked on the engine's
own [B, passages] score rows).  HIP-event medians.  Prints one JSON line and writes it
to --out.  The ranking kernels' own times come from a separate run under rocprofv3 --kernel-trace --stats.

    python tools/bench_filter.py --out filter.json [--small] [--reps 20]
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SELECTIVITY = (1.0, 0.5, 0.01, 1e-4)


def _time(fn, reps, warm=3):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return round(float(np.median(ts)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tiny sizes (a rehearsal of the script, not a measurement)")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from hipporag_amd import _lib, synth
    from hipporag_amd.engine import HippoRAGEngine, pack_mask
    V, E, D = (40000, 400000, 128) if args.small else (1_000_000, 10_000_000, 768)
    kg = synth.make_kg(V, E, 1237)
    pass_bits = synth.make_embeddings_np(kg.n_passages, D, 1238)
    fact_bits = synth.make_embeddings_np(kg.n_facts, D, 1239)
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    n_p, k = kg.n_passages, 200

    def bf16(bits):
        return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)

    res = dict(tool="bench_filter", config="configs[2]" if not args.small else "small", V=V, E=E, D=D, n_passages=n_p,
               k=k, reps=args.reps, retrieve_ms={}, ranking_ms={})
    with HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                        max_batch=256, max_topk=k) as eng:
        for B in (256, 64, 1):
            qf = bf16(synth.make_queries_np(fact_bits, B, seed=1)[0])
            qp = bf16(synth.make_queries_np(pass_bits, B, seed=2)[0])
            idx, sc = eng.score_facts(qf, k=5)
            cnt = torch.full((B,), 5, dtype=torch.int32, device=dev)
            rng = np.random.default_rng(B)
            row = res["retrieve_ms"][f"B{B}"] = {}
            row["unfiltered"] = _time(lambda: eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=k, want_residual=False),
                                      args.reps)
            masks = {}
            for p in SELECTIVITY:
                m = rng.random((B, n_p)) < p
                for form, rows in (("per_query", m), ("broadcast", m[:1])):
                    w = torch.from_numpy(pack_mask(rows).view(np.int32)).to(dev)
                    w = w if form == "per_query" else w[0].contiguous()
                    masks[(p, form)] = w
                    row[f"filtered_{form}_{p:g}"] = _time(
                        lambda: eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=k, want_residual=False, doc_filter=w),
                        args.reps)
            # the ranking alone, on this batch's own score rows (one workgroup per row on both sides: no workspace)
            scores = eng.last_doc_scores(B)
            oi = torch.empty((B, k), dtype=torch.int32, device=dev)
            ov = torch.empty((B, k), dtype=torch.float32, device=dev)
            stream = torch.cuda.current_stream().cuda_stream
            rk = res["ranking_ms"][f"B{B}"] = {}
            rk["unfiltered"] = _time(lambda: _lib.check(lib.hrag_topk_rows_ws(
                scores.data_ptr(), B, n_p, n_p, k, 0, 0, oi.data_ptr(), ov.data_ptr(), None, None, None, 0, stream)),
                args.reps)
            for (p, form), w in masks.items():
                ld = w.shape[1] if w.dim() == 2 else 0
                rk[f"filtered_{form}_{p:g}"] = _time(lambda: _lib.check(lib.hrag_topk_rows_masked(
                    scores.data_ptr(), B, n_p, n_p, k, 0, 0, w.data_ptr(), ld, 0, oi.data_ptr(), ov.data_ptr(), None,
                    None, None, 0, stream)), args.reps)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
