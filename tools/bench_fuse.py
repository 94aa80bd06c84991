"""Cost of fused retrieval on one MI355X: phase B (retrieve, k = 200) against the same call at k = 1 followed by the fusion
(last_fused, k = 200) at configs[1] (100k-node KG, batch 64) and configs[2] (1M-node / 10M-edge KG, batch 256) sizes, for
Q = B (all singletons), B / 4 and 1 questions in each mode ("sum" weighted, "max", "rrf" at c = 60, depth 200); and the
column kernel alone (hrag_fuse_rows in place on a copy of the call's score rows) and the RRF scatter alone (hrag_rrf_rows
on the ranked lists of those rows) against the traffic floor of the column kernel, (B + Q) * N_p * 4 bytes at 8 TB/s.
HIP-event medians.  Prints one JSON line and writes it to --out.

    python tools/bench_fuse.py --out fuse.json [--small] [--reps 20] [--only "configs[2]"]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tiny sizes (a rehearsal of the script, not a measurement)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=None, help="measure this configuration only, e.g. configs[2]")
    args = ap.parse_args()
    import torch
    from hipporag_amd import _lib, synth
    from hipporag_amd.engine import HippoRAGEngine, topk_rows
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    k, depth, c = 200, 200, 60
    configs = [("small", 40000, 400000, 128, 64)] if args.small else [("configs[1]", 100_000, 1_000_000, 768, 64),
                                                                      ("configs[2]", 1_000_000, 10_000_000, 768, 256)]
    if args.only:
        configs = [cfg for cfg in configs if cfg[0] == args.only]
    res = dict(tool="bench_fuse", k=k, rrf_depth=depth, rrf_c=c, reps=args.reps, configs={})

    def bf16(bits):
        return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)

    for name, V, E, D, B in configs:
        kg = synth.make_kg(V, E, 1237)
        pass_bits = synth.make_embeddings_np(kg.n_passages, D, 1238)
        fact_bits = synth.make_embeddings_np(kg.n_facts, D, 1239)
        n_p = kg.n_passages
        row = res["configs"][name] = dict(V=V, E=E, D=D, batch=B, n_passages=n_p, retrieve_ms={}, retrieve_fused_ms={},
                                          kernel_ms={}, kernel_floor_ms={}, kernel_over_floor={})
        with HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                            max_batch=B, max_topk=k) as eng:
            qf = bf16(synth.make_queries_np(fact_bits, B, seed=1)[0])
            qp = bf16(synth.make_queries_np(pass_bits, B, seed=2)[0])
            idx, sc = eng.score_facts(qf, k=5)
            cnt = torch.full((B,), 5, dtype=torch.int32, device=dev)
            w = (np.random.default_rng(3).random(B) * 4).astype(np.float32)

            def retrieve(kk):
                return eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=kk, want_residual=False)

            row["retrieve_ms"]["k200"] = _time(lambda: retrieve(k), args.reps)
            row["retrieve_ms"]["k1"] = _time(lambda: retrieve(1), args.reps)
            retrieve(1)
            scores = eng.last_doc_scores(B)
            lists = topk_rows(scores, depth)[0]
            stream = torch.cuda.current_stream().cuda_stream
            w_d = torch.from_numpy(w).to(dev)
            for Q in sorted({B, max(1, B // 4), 1}, reverse=True):
                mp = (np.arange(Q + 1, dtype=np.int64) * B // Q).astype(np.int32)
                mp_d = torch.from_numpy(mp).to(dev)
                floor = (B + Q) * n_p * 4 / 8e12 * 1e3
                row["kernel_floor_ms"][f"Q{Q}"] = round(floor, 5)
                for mode, weights in (("sum", w), ("max", None), ("rrf", w)):
                    def fused():
                        retrieve(1)
                        return eng.last_fused(mp, weights=weights, fuse=mode, rrf_c=c, rrf_depth=depth, k=k)

                    row["retrieve_fused_ms"][f"Q{Q}_{mode}"] = _time(fused, args.reps)
                    if mode == "rrf":
                        out = torch.empty((Q, n_p), dtype=torch.float32, device=dev)
                        ms = _time(lambda: _lib.check(lib.hrag_rrf_rows(lists.data_ptr(), B, depth, mp_d.data_ptr(), Q,
                                                                        w_d.data_ptr(), c, out.data_ptr(), n_p, n_p, stream)),
                                   args.reps)
                    else:
                        work = scores.clone()        # in place: later repetitions fuse fused rows -- the same traffic
                        ms = _time(lambda: _lib.check(lib.hrag_fuse_rows(
                            work.data_ptr(), B, n_p, n_p, mp_d.data_ptr(), Q, w_d.data_ptr() if weights is not None else None,
                            0 if mode == "sum" else 1, stream)), args.reps)
                        row["kernel_over_floor"][f"Q{Q}_{mode}"] = round(ms / floor, 2)
                    row["kernel_ms"][f"Q{Q}_{mode}"] = ms
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
