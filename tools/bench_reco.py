"""Cost of recommend by example on one MI355X at configs[2] size (1M-node / 10M-edge KG, dim 768, bf16, n_passages as
bench.py builds it), for B in {256, 1}, 1 / 8 / 32 examples per query (the last one a negative when there are several) and
both row strategies:
  (a) hrag_reco_scores (the fused product-and-reduce) against the three-step path it replaces on the same inputs --
      gather the E example rows, hrag_sim_gemm into an [E, Np] fp32 matrix, hrag_reco_rows -- in ALTERNATING runs, HIP-event
      medians after warm-up; the two results are compared bit for bit;
  (b) the peak device memory either path allocates on top of its inputs and its [B, Np] output;
  (c) floors of the fused kernel: traffic -- the passage table once, the example rows, the result -- over the 6.29 TB/s a
      streaming copy measures on this part (8 TB/s spec beside it), and the MFMA work -- 2 Np kdim flops per live column of
      a 16-column block -- over the 2.5 PFLOP/s dense bf16 peak;
  (d) HippoRAGEngine.recommend(k=200) end to end, and retrieve(feedback=) against the plain retrieve, alternating.
Prints one JSON line and writes it to --out.

    python tools/bench_reco.py --out profiles/reco_cfg2_bench_reco.json [--small] [--reps 20]
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

STREAM_BPS, SPEC_BPS, MFMA_FLOPS = 6.29e12, 8e12, 2.5e15
MODES = {"best_score": 0, "sum_scores": 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tiny sizes (a rehearsal of the script, not a measurement)")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from hipporag_amd import _lib, synth
    from hipporag_amd.engine import Examples, HippoRAGEngine, _stream
    dev = torch.device("cuda", 0)
    name, V, E, D, batches = (("small", 40000, 400000, 128, (16, 1)) if args.small
                              else ("configs[2]", 1_000_000, 10_000_000, 768, (256, 1)))
    k = 200
    kg = synth.make_kg(V, E, 1237)
    pass_bits = synth.make_embeddings_np(kg.n_passages, D, 1238)
    fact_bits = synth.make_embeddings_np(kg.n_facts, D, 1239)
    n_p = kg.n_passages
    ld = n_p + (-n_p) % 4
    res = dict(tool="bench_reco", config=name, V=V, E=E, D=D, n_passages=n_p, k=k, reps=args.reps, stream_TBps=STREAM_BPS / 1e12,
               spec_TBps=SPEC_BPS / 1e12, mfma_peak_PFLOPs=MFMA_FLOPS / 1e15, cases=[], calls=[])
    to_q = lambda bits: torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)  # noqa: E731
    lib = _lib.load()
    pass_dev = to_q(pass_bits).contiguous()
    rng = np.random.default_rng(1246)
    with HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                        max_batch=max(batches), max_topk=k) as eng:
        for B in batches:
            qf = to_q(synth.make_queries_np(fact_bits, B, seed=1)[0])
            qp = to_q(synth.make_queries_np(pass_bits, B, seed=2)[0])
            idx, sc = eng.score_facts(qf, k=5)
            cnt = torch.full((B,), 5, dtype=torch.int32, device=dev)
            for per in (1, 8, 32):
                pos = [rng.choice(n_p, per - (1 if per > 1 else 0), replace=False).tolist() for _ in range(B)]
                neg = [rng.choice(n_p, 1 if per > 1 else 0, replace=False).tolist() for _ in range(B)]
                ex = Examples.from_lists(pos, neg)
                n_ex = ex.n_examples
                ws = torch.empty((int(lib.hrag_reco_workspace_bytes(B)),), dtype=torch.uint8, device=dev)
                sel = ex.ex_idx.long()
                for mode, code in MODES.items():
                    case = dict(batch=B, examples_per_query=per, strategy=mode, examples=n_ex)
                    out_f = torch.empty((B, ld), dtype=torch.float32, device=dev)
                    out_t = torch.empty((B, ld), dtype=torch.float32, device=dev)

                    def fused():
                        _lib.check(lib.hrag_reco_scores(eng._handle, ex.ex_ptr.ctypes.data, ex.ex_ptr_dev.data_ptr(),
                                                        ex.ex_idx.data_ptr(), ex.ex_sign.data_ptr(), B, code, out_f.data_ptr(), ld,
                                                        ws.data_ptr(), ws.numel(), _stream()))

                    def three_step():
                        rows = pass_dev[sel]                                          # the gathered copy [E, D]
                        if n_ex < 3:                                                  # (one or two queries take the GEMV)
                            rows = torch.cat([rows, rows.new_zeros((3 - n_ex, D))])
                        # (allocated inside the timed region: after the warm-up runs the caching allocator hands the same
                        # block back without a device call, so the time is the three launches')
                        mat = torch.empty((rows.shape[0], ld), dtype=torch.float32, device=dev)
                        _lib.check(lib.hrag_sim_gemm(pass_dev.data_ptr(), n_p, D, rows.data_ptr(), rows.shape[0], mat.data_ptr(),
                                                     ld, 0, 0, _stream()))
                        _lib.check(lib.hrag_reco_rows(mat.data_ptr(), ld, ex.ex_ptr_dev.data_ptr(), ex.ex_sign.data_ptr(), B, n_p,
                                                      code, out_t.data_ptr(), ld, _stream()))

                    for fn, key in ((fused, "fused_peak_extra_MB"), (three_step, "three_step_peak_extra_MB")):
                        torch.cuda.synchronize()
                        torch.cuda.empty_cache()
                        torch.cuda.reset_peak_memory_stats()
                        base = torch.cuda.memory_allocated()
                        fn()
                        torch.cuda.synchronize()
                        case[key] = round((torch.cuda.max_memory_allocated() - base) / 1e6, 3)
                    case["fused_peak_extra_MB"] = round(case["fused_peak_extra_MB"] + ws.numel() / 1e6, 3)   # its column table
                    case["fused_ms"], case["three_step_ms"] = _alternating(fused, three_step, args.reps)
                    case["fused_over_three_step"] = round(case["fused_ms"] / case["three_step_ms"], 3)
                    case["bit_identical"] = bool(torch.equal(out_f[:, :n_p].view(torch.int32), out_t[:, :n_p].view(torch.int32)))
                    blocks = B * (2 if per > 16 else 1)
                    nbytes = n_p * D * 2 + n_ex * D * 2 + B * n_p * 4
                    flops = 2.0 * n_p * D * blocks * 16
                    case.update(traffic_GB=round(nbytes / 1e9, 4), traffic_floor_ms=round(nbytes / STREAM_BPS * 1e3, 5),
                                traffic_floor_spec_ms=round(nbytes / SPEC_BPS * 1e3, 5), mfma_GFLOP=round(flops / 1e9, 2),
                                mfma_floor_ms=round(flops / MFMA_FLOPS * 1e3, 5))
                    case["fused_over_floor"] = round(case["fused_ms"] / max(case["traffic_floor_ms"], case["mfma_floor_ms"]), 2)
                    res["cases"].append(case)
                call = dict(batch=B, examples_per_query=per)
                for mode in (*MODES, "average_vector"):
                    call[f"recommend_{mode}_ms"] = _time(lambda: eng.recommend(ex, k=k, strategy=mode), args.reps)

                def retrieve(**kw):
                    return eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=k, want_residual=False, **kw)

                call["retrieve_plain_ms"], call["retrieve_feedback_ms"] = _alternating(
                    retrieve, lambda: retrieve(feedback=ex, feedback_weight=0.3), args.reps)
                call["feedback_extra_ms"] = round(call["retrieve_feedback_ms"] - call["retrieve_plain_ms"], 4)
                res["calls"].append(call)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
