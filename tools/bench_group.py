"""Cost of grouped retrieval on one MI355X: phase B (retrieve) ungrouped against group_agg = "max" / "sum" at configs[1]
(100k-node KG, batch 64) and configs[2] (1M-node / 10M-edge KG, batch 256) sizes, k = 200, with G = N_p / 8 groups of
consecutive passages, the same groups shuffled, and one skewed table (a power law with one group of N_p / 3 passages);
and the reduce kernel alone (hrag_group_rows on the call's own score rows) against its traffic floor B * N_p * 4 bytes at
8 TB/s.  The hits leg (--hits 3,8): the same grouped calls with group_hits = m (the follow-up hrag_last_group_hits
included), and the selection kernel alone (hrag_group_hits_rows on the call's score rows and ranked group ids) against its
traffic floor: B * k * (mean members of the ranked groups) * 8 bytes of member and score reads plus the B * k * m * 8
bytes it writes, at 8 TB/s.  HIP-event medians.  Prints one JSON line and writes it to --out.

    python tools/bench_group.py --out group.json [--small] [--reps 20] [--hits 3,8] [--only "configs[2]"]
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


def tables(n_p, rng):
    contiguous = (np.arange(n_p) // 8).astype(np.int32)
    sizes, left = [n_p // 3], n_p - n_p // 3
    while left > 0:
        sz = int(min(left, max(1, rng.pareto(1.0) * 3)))
        sizes.append(sz)
        left -= sz
    skewed = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    return {"contiguous_np8": contiguous, "shuffled_np8": contiguous[rng.permutation(n_p)], "skewed": skewed}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tiny sizes (a rehearsal of the script, not a measurement)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--hits", default="3,8", help="group_hits values of the hits leg, comma separated ('' skips the leg)")
    ap.add_argument("--only", default=None, help="measure this configuration only, e.g. configs[2]")
    args = ap.parse_args()
    import torch
    from hipporag_amd import _lib, synth
    from hipporag_amd.engine import HippoRAGEngine, group_table_csr
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    k = 200
    configs = [("small", 40000, 400000, 128, 64)] if args.small else [("configs[1]", 100_000, 1_000_000, 768, 64),
                                                                      ("configs[2]", 1_000_000, 10_000_000, 768, 256)]
    if args.only:
        configs = [c for c in configs if c[0] == args.only]
    hits = [int(m) for m in args.hits.split(",") if m]
    res = dict(tool="bench_group", k=k, reps=args.reps, hits=hits, configs={})

    def bf16(bits):
        return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)

    for name, V, E, D, B in configs:
        kg = synth.make_kg(V, E, 1237)
        pass_bits = synth.make_embeddings_np(kg.n_passages, D, 1238)
        fact_bits = synth.make_embeddings_np(kg.n_facts, D, 1239)
        n_p = kg.n_passages
        row = res["configs"][name] = dict(V=V, E=E, D=D, batch=B, n_passages=n_p, retrieve_ms={}, reduce_ms={},
                                          reduce_floor_ms=round(B * n_p * 4 / 8e12 * 1e3, 5))
        with HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                            max_batch=B, max_topk=k) as eng:
            qf = bf16(synth.make_queries_np(fact_bits, B, seed=1)[0])
            qp = bf16(synth.make_queries_np(pass_bits, B, seed=2)[0])
            idx, sc = eng.score_facts(qf, k=5)
            cnt = torch.full((B,), 5, dtype=torch.int32, device=dev)

            def run(agg=None, m=None):
                return eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=k, want_residual=False, group_agg=agg, group_hits=m)

            row["retrieve_ms"]["ungrouped"] = _time(run, args.reps)
            stream = torch.cuda.current_stream().cuda_stream
            for tname, g in tables(n_p, np.random.default_rng(7)).items():
                eng.set_passage_groups(g)
                n_groups = int(g.max()) + 1
                row.setdefault("n_groups", {})[tname] = n_groups
                for agg in ("max", "sum"):
                    row["retrieve_ms"][f"{tname}_{agg}"] = _time(lambda: run(agg), args.reps)
                scores = eng.last_doc_scores(B)
                ptr, members = group_table_csr(g, n_groups)
                ptr_d, mem_d = torch.from_numpy(ptr).to(dev), torch.from_numpy(members).to(dev)
                gs = torch.empty((B, n_groups), dtype=torch.float32, device=dev)
                gb = torch.empty((B, n_groups), dtype=torch.int32, device=dev)
                for agg, code in (("max", 0), ("sum", 1)):
                    row["reduce_ms"][f"{tname}_{agg}"] = _time(lambda: _lib.check(lib.hrag_group_rows(
                        scores.data_ptr(), B, n_p, n_p, ptr_d.data_ptr(), mem_d.data_ptr(), n_groups, code, None, 0, 0,
                        gs.data_ptr(), gb.data_ptr(), n_groups, stream)), args.reps)
                for m in hits:
                    for agg in ("max", "sum"):
                        row.setdefault("retrieve_hits_ms", {})[f"{tname}_{agg}_m{m}"] = _time(lambda: run(agg, m), args.reps)
                    gi = run("max").group_idx                 # the ranked groups the kernel alone is timed on
                    ids = gi.cpu().numpy()
                    mean_members = float(np.bincount(g, minlength=n_groups)[ids[ids >= 0]].mean())
                    hi = torch.empty((B, k, m), dtype=torch.int32, device=dev)
                    hs = torch.empty((B, k, m), dtype=torch.float32, device=dev)
                    row.setdefault("hits_ms", {})[f"{tname}_m{m}"] = _time(lambda: _lib.check(lib.hrag_group_hits_rows(
                        scores.data_ptr(), B, n_p, n_p, ptr_d.data_ptr(), mem_d.data_ptr(), n_groups, gi.data_ptr(), k, m,
                        None, 0, 0, hi.data_ptr(), hs.data_ptr(), stream)), args.reps)
                    row.setdefault("hits_mean_members", {})[tname] = round(mean_members, 2)
                    row.setdefault("hits_floor_ms", {})[f"{tname}_m{m}"] = round(
                        (B * k * mean_members * 8 + B * k * m * 8) / 8e12 * 1e3, 5)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
