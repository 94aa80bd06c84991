"""Large-k ranking (K4', hrag_topk_rows_ws) on one MI355X: the kernel on [256 x 125 000] score rows next to torch's
sort / topk on the same GPU (yardsticks only: torch's tie order differs and the library never calls it), hrag_retrieve
at configs[2] with k = 200, 5000 and every passage next to the host ranking it replaces, and retrieve_knn(k=4096) on
875 000 keys.  Prints one JSON object and writes it to --out.

    python tools/bench_topk_large.py --out topk_large.json [--small]
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


def _time(fn, reps, warm=2):
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
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "reps": reps}


def bench_kernel(res, b, n, reps):
    import torch
    from hipporag_amd import _lib
    lib = _lib.load()
    x = torch.rand((b, n), device="cuda")
    out = {}
    for k in (2048, 4096, 16384, n):
        idx = torch.empty((b, k), dtype=torch.int32, device="cuda")
        val = torch.empty((b, k), dtype=torch.float32, device="cuda")
        need = int(lib.hrag_topk_rows_workspace_bytes(b, n, k))
        ws = torch.empty((max(need, 1),), dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream

        def run():
            _lib.check(lib.hrag_topk_rows_ws(x.data_ptr(), b, n, n, k, 0, 0, idx.data_ptr(), val.data_ptr(), None, None,
                                             ws.data_ptr() if need else None, need, stream))
        out[f"hrag_topk_rows_ws_k{k}"] = dict(_time(run, reps), workspace_bytes=need)
        out[f"torch_topk_sorted_k{k}"] = _time(lambda: torch.topk(x, k, dim=1, sorted=True), reps)
    out["torch_sort_full"] = _time(lambda: torch.sort(x, dim=1, descending=True), reps)
    res["kernel"] = dict(batch=b, n=n, **out)


def bench_retrieve(res, V, E, D, B, seed, reps):
    import torch
    from hipporag_amd import synth
    from hipporag_amd.engine import HippoRAGEngine
    t0 = time.time()
    kg = synth.make_kg(V, E, seed)
    pass_bits = synth.make_embeddings_np(kg.n_passages, D, seed + 1)
    fact_bits = synth.make_embeddings_np(kg.n_facts, D, seed + 2)
    build_s = time.time() - t0
    dev = torch.device("cuda", 0)

    def bf16(bits):
        return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)

    qf = bf16(synth.make_queries_np(fact_bits, B, seed=1)[0])
    qp = bf16(synth.make_queries_np(pass_bits, B, seed=2)[0])
    n_p = kg.n_passages
    out = dict(V=V, E=E, D=D, batch=B, n_passages=n_p, build_s=build_s)
    with HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                        max_batch=B, max_topk=n_p) as eng:
        out["workspace_bytes"] = eng.stats()["workspace_bytes"]
        idx, sc = eng.score_facts(qf, k=5)
        cnt = torch.full((B,), 5, dtype=torch.int32, device=dev)
        for k in (200, 2048, 5000, n_p):
            out[f"retrieve_k{k}"] = _time(lambda: eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=k), reps)
        # the host path the mirror took beyond 2048 until now: k = 2048 on the device + every score over PCIe + one
        # stable argsort per query on the host
        for k in (5000, n_p):
            ts = []
            for _ in range(max(2, reps // 4)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=2048)
                full = eng.last_doc_scores(B).cpu().numpy()
                d_idx = np.stack([np.argsort(r, kind="stable")[::-1][:k] for r in full])
                np.take_along_axis(full, d_idx, axis=1)
                ts.append((time.perf_counter() - t0) * 1e3)
            out[f"host_path_k{k}"] = {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "reps": len(ts)}
            t0 = time.perf_counter()
            o = eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=k)
            o.doc_idx.cpu().numpy(), o.doc_score.cpu().numpy()
            out[f"device_path_k{k}_with_copy_ms"] = (time.perf_counter() - t0) * 1e3
    res["retrieve"] = out


def bench_knn(res, nk, nq, dim, k):
    import torch
    from hipporag_amd.knn import retrieve_knn
    rng = np.random.default_rng(875)
    keys = rng.standard_normal((nk, dim), dtype=np.float32)
    q = keys[rng.integers(0, nk, nq)] + np.float32(0.3) * rng.standard_normal((nq, dim), dtype=np.float32)
    retrieve_knn(None, None, q[:8], keys, k=k, return_arrays=True)     # warm-up
    out = dict(n_keys=nk, queries=nq, dim=dim)
    for kk in (2047, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        retrieve_knn(None, None, q, keys, k=kk, return_arrays=True)
        out[f"retrieve_knn_k{kk}_s"] = time.perf_counter() - t0
    res["knn"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tiny sizes (a rehearsal of the script, not a measurement)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="kernel,retrieve,knn")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_topk_large needs the GPU"
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0)}
    parts = args.only.split(",")
    if "kernel" in parts:
        bench_kernel(res, 16 if args.small else 256, 20000 if args.small else 125000, args.reps)
    if "retrieve" in parts:
        if args.small:
            bench_retrieve(res, 40000, 400000, 128, 64, 1237, 3)
        else:
            bench_retrieve(res, 1_000_000, 10_000_000, 768, 256, 1237, args.reps)
    if "knn" in parts:
        bench_knn(res, 20000 if args.small else 875000, 64 if args.small else 1000, 768, 4096)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
