"""Cost of diversified retrieval (MMR) on one MI355X: phase B (retrieve, k picks) with and without mmr_lambda over c = 200
ranked candidates, in ALTERNATING runs, at configs[2] (1M-node / 10M-edge KG, dim 768) and configs[3] (the same graph, dim
4096) size, batch 256, k in {5, 20, 200}, for a bf16 and a split (fp32-faithful) engine; and each kernel alone:
  - gram_gather_kernel (hrag_gram_rows) against its traffic floor B * c * kdim * 2 + B * c^2 * 4 bytes at the achievable
    bandwidth measured here (a device-to-device copy of 1 GiB), and its MFMA rate (2 * B * tiles * 64 * 64 * kdim flop,
    tiles = the 64 x 64 tiles of the upper triangle);
  - mmr_select_kernel (hrag_mmr_rows) per selection step.
HIP-event medians.  Prints one JSON line and writes it to --out.

    python tools/bench_mmr.py --out mmr.json [--small] [--reps 20] [--only "configs[2]"] [--kinds bf16,split]
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


def _alternating(fa, fb, reps):
    """medians (ms) of two calls measured in alternating runs: drift of the clocks hits both alike"""
    import torch
    ta, tb = [], []
    for f in (fa, fb):
        f()
    torch.cuda.synchronize()
    for _ in range(reps):
        for f, acc in ((fa, ta), (fb, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            acc.append(e0.elapsed_time(e1))
    return round(float(np.median(ta)), 4), round(float(np.median(tb)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tiny sizes (a rehearsal of the script, not a measurement)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=None, help="measure this configuration only, e.g. configs[2]")
    ap.add_argument("--kinds", default="bf16,split")
    args = ap.parse_args()
    import torch
    from hipporag_amd import _lib, synth
    from hipporag_amd.graph import bf16_bits_to_float
    from hipporag_amd.engine import HippoRAGEngine
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    c, lam = 200, 0.5
    configs = [("small", 40000, 400000, 128, 64)] if args.small else [("configs[2]", 1_000_000, 10_000_000, 768, 256),
                                                                      ("configs[3]", 1_000_000, 10_000_000, 4096, 256)]
    if args.only:
        configs = [cfg for cfg in configs if cfg[0] == args.only]
    res = dict(tool="bench_mmr", candidates=c, mmr_lambda=lam, reps=args.reps, configs={})

    big = torch.empty((1 << 28,), dtype=torch.float32, device=dev)
    dst = torch.empty_like(big)
    copy_ms = _time(lambda: dst.copy_(big), args.reps)
    bw = 2 * big.numel() * 4 / (copy_ms * 1e-3)               # read + write
    res["achievable_bandwidth_TBps"] = round(bw / 1e12, 3)
    del big, dst
    stream = torch.cuda.current_stream().cuda_stream

    for name, V, E, D, B in configs:
        kg = synth.make_kg(V, E, 1237)
        pass_bits = synth.make_embeddings_np(kg.n_passages, D, 1238)
        fact_bits = synth.make_embeddings_np(kg.n_facts, D, 1239)
        n_p = kg.n_passages
        for kind in args.kinds.split(","):
            row = res["configs"][f"{name}/{kind}"] = dict(V=V, E=E, D=D, batch=B, n_passages=n_p)
            if kind == "split":
                pas, fac = bf16_bits_to_float(pass_bits).astype(np.float32), bf16_bits_to_float(fact_bits).astype(np.float32)
                to_q = lambda bits: torch.from_numpy(bf16_bits_to_float(bits).astype(np.float32)).to(dev)      # noqa: E731
            else:
                pas, fac = pass_bits, fact_bits
                to_q = lambda bits: torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)  # noqa: E731
            with HippoRAGEngine(kg.csr, kg.passage_vertex, pas, fac, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                                max_batch=B, max_topk=c) as eng:
                qf = to_q(synth.make_queries_np(fact_bits, B, seed=1)[0])
                qp = to_q(synth.make_queries_np(pass_bits, B, seed=2)[0])
                idx, sc = eng.score_facts(qf, k=5)
                cnt = torch.full((B,), 5, dtype=torch.int32, device=dev)

                def retrieve(kk, **kw):
                    return eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=kk, want_residual=False, **kw)

                row["retrieve_ms"], row["retrieve_mmr_ms"] = {}, {}
                for k in (5, 20, 200):
                    a, b = _alternating(lambda: retrieve(k), lambda: retrieve(k, mmr_lambda=lam, mmr_candidates=c), args.reps)
                    row["retrieve_ms"][f"k{k}"], row["retrieve_mmr_ms"][f"k{k}"] = a, b
                row["retrieve_c_ms"] = _time(lambda: retrieve(c), args.reps)        # the plain call at the candidate depth
                plain = retrieve(c)
                # each kernel alone, over the engine's own passage rows (a device copy in the engine's layout)
                kdim = 3 * D if kind == "split" else D
                if kind == "split":
                    emb = torch.empty((n_p, kdim), dtype=torch.float16, device=dev)
                    src = torch.from_numpy(pas).to(dev)
                    _lib.check(lib.hrag_split_f32(src.data_ptr(), n_p, D, 0, 0, emb.data_ptr(), stream))
                    del src
                    dt = 1
                else:
                    emb, dt = to_q(pass_bits).contiguous(), 0
                ld = c + (-c) % 4
                g = torch.empty((B, c, ld), dtype=torch.float32, device=dev)
                ids, scs = plain.doc_idx.contiguous(), plain.doc_score.contiguous()
                gram_ms = _time(lambda: _lib.check(lib.hrag_gram_rows(emb.data_ptr(), n_p, kdim, dt, 1 if kind == "split" else 0,
                                                                      ids.data_ptr(), B, c, g.data_ptr(), ld, stream)), args.reps)
                floor_ms = (B * c * kdim * 2 + B * c * c * 4) / bw * 1e3
                nt = -(-c // 64)
                flop = 2.0 * B * (nt * (nt + 1) // 2) * 64 * 64 * kdim
                row["gram_ms"], row["gram_floor_ms"] = gram_ms, round(floor_ms, 5)
                row["gram_over_floor"] = round(gram_ms / floor_ms, 2)
                row["gram_mfma_tflops"] = round(flop / (gram_ms * 1e-3) / 1e12, 2)
                row["select_ms"], row["select_us_per_step"] = {}, {}
                for k in (5, 20, 200):
                    o = [torch.empty((B, k), dtype=torch.int32, device=dev) for _ in range(2)] + \
                        [torch.empty((B, k), dtype=torch.float32, device=dev) for _ in range(2)]
                    ms = _time(lambda: _lib.check(lib.hrag_mmr_rows(scs.data_ptr(), ids.data_ptr(), g.data_ptr(), ld, B, c, k, lam,
                                                                    1, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                                                    o[3].data_ptr(), stream)), args.reps)
                    row["select_ms"][f"k{k}"] = ms
                    row["select_us_per_step"][f"k{k}"] = round(ms * 1e3 / k, 3)
                del emb, g
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
