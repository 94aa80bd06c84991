"""Cost of payload filters on one MI355X at configs[2] size (1M-node / 10M-edge KG, dim 768, n_passages as bench.py builds
it, batch 256, k = 200) over four synthetic columns -- an integer year, a keyword with 1 000 values, a float, a keyword
missing on 30 % of the passages -- and per-query programs of three clauses, roughly 10 % selective:
  (a) HippoRAGEngine.retrieve with ready device words and (b) retrieve(doc_filter=PayloadFilter), in ALTERNATING runs, for
      the rich programs (ranges, $exists) and for an equality-only set of the same shape;
  (c) hrag_payload_filter alone against its traffic floor: B * W * 4 bytes written plus the touched columns (values and
      presence words) read once, at the 8 TB/s DESIGN.md uses -- the per-query re-reads of the columns come from L2 / MALL;
  (d) the host path's way of serving the equality-only set: HippoRAG._doc_filter_words on a cold and on a warm
      _filter_cache, plus the upload of its [B, W] words;
  (e) hrag_bitset_count_rows over the [B, W] words.
HIP-event medians for device work, host clocks around a synchronise for (d).  Prints one JSON line and writes it to --out.

    python tools/bench_payload.py --out payload.json [--small] [--reps 20]
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
N_KW, N_YEARS, OPT = 1000, 24, ["a", "b", "c", "d", "e"]


def make_columns(rng, n):
    year = (2000 + rng.integers(0, N_YEARS, n)).astype(np.int64)
    kw = rng.integers(0, N_KW, n)
    score = rng.random(n)
    opt = rng.integers(0, len(OPT), n)
    has_opt = rng.random(n) >= 0.3
    return year, kw, score, opt, has_opt


def rich_filters(rng, batch):
    """year in a 12-year window (0.5) AND kw in 300 of 1 000 values (0.3) AND score < 0.7 or opt present (0.7)"""
    out = []
    for i in range(batch):
        y0 = 2000 + int(rng.integers(0, N_YEARS - 11))
        f = {"year": {"$gte": y0, "$lt": y0 + 12}, "kw": [f"k{v}" for v in rng.choice(N_KW, 300, replace=False)]}
        if i % 2:
            f["opt"] = {"$exists": True}
        else:
            f["score"] = {"$lt": 0.7}
        out.append(f)
    return out


def equality_filters(rng, batch):
    """the same shape with equality only: 12 years, 300 keyword values, every value of opt (= present)"""
    return [{"year": [2000 + int(v) for v in rng.choice(N_YEARS, 12, replace=False)],
             "kw": [f"k{v}" for v in rng.choice(N_KW, 300, replace=False)], "opt": list(OPT)} for _ in range(batch)]


def _host_ms(fn, reps):
    import torch
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tiny sizes (a rehearsal of the script, not a measurement)")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from hipporag_amd import synth
    from hipporag_amd.engine import HippoRAGEngine
    from hipporag_amd.payload import PayloadIndex, compile_filters, count_rows
    from hipporag_amd.retriever import HippoRAG, RetrievalConfig
    dev = torch.device("cuda", 0)
    name, V, E, D, B = ("small", 40000, 400000, 128, 64) if args.small else ("configs[2]", 1_000_000, 10_000_000, 768, 256)
    k = 200
    kg = synth.make_kg(V, E, 1237)
    pass_bits = synth.make_embeddings_np(kg.n_passages, D, 1238)
    fact_bits = synth.make_embeddings_np(kg.n_facts, D, 1239)
    n_p = kg.n_passages
    W = (n_p + 31) // 32
    rng = np.random.default_rng(1241)
    year, kw, score, opt, has_opt = make_columns(rng, n_p)
    kw_s = [f"k{v}" for v in kw]
    opt_s = [OPT[v] if h else None for v, h in zip(opt, has_opt)]
    res = dict(tool="bench_payload", config=name, V=V, E=E, D=D, batch=B, n_passages=n_p, words=W, k=k, reps=args.reps,
               peak_TBps=PEAK_BPS / 1e12)
    to_q = lambda bits: torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)  # noqa: E731
    t0 = time.perf_counter()
    ix = PayloadIndex.from_columns({"year": year, "kw": kw_s, "score": score, "opt": opt_s}, n_p)
    res["index_build_s"] = round(time.perf_counter() - t0, 3)
    with ix, HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                            max_batch=B, max_topk=k) as eng:
        eng.set_payload_index(ix)
        qf = to_q(synth.make_queries_np(fact_bits, B, seed=1)[0])
        qp = to_q(synth.make_queries_np(pass_bits, B, seed=2)[0])
        idx, sc = eng.score_facts(qf, k=5)
        cnt = torch.full((B,), 5, dtype=torch.int32, device=dev)

        def retrieve(f):
            return eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=k, want_residual=False, doc_filter=f)

        sets = {"rich": rich_filters(rng, B), "equality": equality_filters(rng, B)}
        for label, filters in sets.items():
            t0 = time.perf_counter()
            pf = compile_filters(ix, filters)
            res[f"{label}_compile_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            words = ix.evaluate(pf).clone()
            res[f"{label}_selectivity"] = round(float(count_rows(words, n_p).float().mean().item()) / n_p, 4)
            res[f"{label}_clauses"], res[f"{label}_set_values"] = pf.n_clauses, int(pf.set_vals.shape[0])
            same = retrieve(pf)
            want = retrieve(words)
            assert torch.equal(same.doc_idx, want.doc_idx) and torch.equal(same.doc_score, want.doc_score)
            # (a) and (b)
            a_ms, b_ms = _alternating(lambda: retrieve(words), lambda: retrieve(pf), args.reps)
            res[f"{label}_retrieve_words_ms"], res[f"{label}_retrieve_payload_ms"] = a_ms, b_ms
            res[f"{label}_payload_extra_ms"] = round(b_ms - a_ms, 4)
            # (c) the kernel alone, the clause arrays already on the device
            out = torch.empty((B, W), dtype=torch.int32, device=dev)
            res[f"{label}_payload_filter_ms"] = _time(lambda: ix.evaluate(pf, out=out), args.reps)
            touched = sorted(set(pf.c_col.tolist()))
            col_bytes = sum(8 * n_p + (4 * W if ix.names[c] == "opt" else 0) for c in touched)
            floor_ms = (B * W * 4 + col_bytes) / PEAK_BPS * 1e3
            res[f"{label}_payload_filter_floor_ms"] = round(floor_ms, 6)
            res[f"{label}_payload_filter_over_floor"] = round(res[f"{label}_payload_filter_ms"] / floor_ms, 1)
            # (e)
            res[f"{label}_count_rows_ms"] = _time(lambda: count_rows(words, n_p), args.reps)
        # (d) the host path over the same metadata: cold cache (one pass over the passages per new (key, value)), warm
        # cache (ORs and ANDs of W-word arrays per query), and the upload of [B, W] words
        rag = HippoRAG(RetrievalConfig())
        rag.passage_node_keys = [f"p{i}" for i in range(n_p)]
        rag.chunk_metadata = {key: dict({"year": int(y), "kw": s}, **({"opt": o} if o is not None else {}))
                              for key, y, s, o in zip(rag.passage_node_keys, year, kw_s, opt_s)}
        eq = sets["equality"]
        t0 = time.perf_counter()
        host_words = rag._doc_filter_words(eq, B)
        res["host_cold_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["host_cache_entries"] = len(rag._filter_cache)
        dev_words = ix.evaluate(compile_filters(ix, eq))
        tail = np.uint32((1 << (n_p % 32)) - 1) if n_p % 32 else np.uint32(0xFFFFFFFF)
        host_cmp = host_words.copy()
        host_cmp[:, -1] &= tail
        assert np.array_equal(dev_words.cpu().numpy().view(np.uint32), host_cmp), "the two paths disagree"
        res["host_warm_ms"] = _host_ms(lambda: rag._doc_filter_words(eq, B), 3)
        res["host_upload_ms"] = _host_ms(lambda: torch.from_numpy(host_words.view(np.int32)).to(dev), 5)
        res["host_warm_plus_upload_ms"] = round(res["host_warm_ms"] + res["host_upload_ms"], 3)
        res["payload_extra_below_host_warm"] = bool(res["equality_payload_extra_ms"] < res["host_warm_ms"])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
