"""Cost of the scoped doc filter on one MI355X: phase A + phase B (score_facts + retrieve) at configs[2] (1M-node /
10M-edge KG, 1M x 768 bf16), batch 256, k = 200 -- unfiltered; the "ranking" scope (post-filter); the "seeds" scope with
one broadcast filter row at selectivity 1, 0.1 and 1e-3; the "seeds" scope with one filter row per query (0.1).
HIP-event medians.  Prints one JSON line and writes it to --out.

The synthetic KG records no fact -> passage table, so this tool takes a fact's source passages to be the passages
adjacent to its subject or object vertex in the graph (what the OpenIE step of a real index would have recorded).

    python tools/bench_scope.py --out scope.json [--small] [--reps 20]
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


def adjacent_sources(kg):
    """Fact f's sources: the passages adjacent to subj_vertex[f] or obj_vertex[f] -> (row_ptr int64, pos int32)."""
    rp = kg.csr.row_ptr.astype(np.int64)
    col = kg.csr.col_idx
    pos_of = np.full(kg.num_vertices, -1, np.int64)
    pos_of[kg.passage_vertex] = np.arange(kg.n_passages)
    fid, pp = [], []
    for v in (kg.subj_vertex, kg.obj_vertex):
        f = np.flatnonzero(v >= 0)
        starts, lens = rp[v[f]], rp[v[f] + 1] - rp[v[f]]
        offs = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)
        p = pos_of[col[np.repeat(starts, lens) + offs]]
        keep = p >= 0
        fid.append(np.repeat(f, lens)[keep])
        pp.append(p[keep])
    fid, pp = np.concatenate(fid), np.concatenate(pp)
    pair = np.unique(fid * kg.n_passages + pp)
    fid, pp = pair // kg.n_passages, pair % kg.n_passages
    row_ptr = np.zeros(kg.n_facts + 1, np.int64)
    row_ptr[1:] = np.cumsum(np.bincount(fid, minlength=kg.n_facts))
    return row_ptr, pp.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tiny sizes (a rehearsal of the script, not a measurement)")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from hipporag_amd import synth
    from hipporag_amd.engine import HippoRAGEngine, pack_mask
    V, E, D = (40000, 400000, 128) if args.small else (1_000_000, 10_000_000, 768)
    kg = synth.make_kg(V, E, 1237)
    pass_bits = synth.make_embeddings_np(kg.n_passages, D, 1238)
    fact_bits = synth.make_embeddings_np(kg.n_facts, D, 1239)
    row_ptr, pos = adjacent_sources(kg)
    dev = torch.device("cuda", 0)
    n_p, k, B = kg.n_passages, 200, 256

    def bf16(bits):
        return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)

    res = dict(tool="bench_scope", config="configs[2]" if not args.small else "small", V=V, E=E, D=D, n_passages=n_p,
               n_facts=kg.n_facts, fact_sources=int(len(pos)), sources="passages adjacent to the subject or object",
               batch=B, k=k, reps=args.reps, phase_ab_ms={}, no_allowed_fact_rows={})
    with HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                        max_batch=B, max_topk=k) as eng:
        eng.set_fact_sources(row_ptr, pos)
        qf = bf16(synth.make_queries_np(fact_bits, B, seed=1)[0])
        qp = bf16(synth.make_queries_np(pass_bits, B, seed=2)[0])
        rng = np.random.default_rng(5)

        def run(doc_filter=None, scope="ranking"):
            kw = {} if doc_filter is None else {"doc_filter": doc_filter, "filter_scope": scope}
            if scope == "seeds":
                idx, sc = eng.score_facts(qf, k=5, scope_filter=doc_filter)
            else:
                idx, sc = eng.score_facts(qf, k=5)
            cnt = (idx >= 0).sum(dim=1).to(torch.int32)
            return eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=k, want_residual=False, **kw)

        ms = res["phase_ab_ms"]
        ms["unfiltered"] = _time(run, args.reps)
        one = torch.from_numpy(pack_mask(rng.random(n_p) < 0.1).view(np.int32)).to(dev)
        ms["ranking_broadcast_0.1"] = _time(lambda: run(one, "ranking"), args.reps)
        for p in (1.0, 0.1, 1e-3):
            w = torch.from_numpy(pack_mask(rng.random(n_p) < p).view(np.int32)).to(dev)
            ms[f"seeds_broadcast_{p:g}"] = _time(lambda: run(w, "seeds"), args.reps)
            res["no_allowed_fact_rows"][f"broadcast_{p:g}"] = int((run(w, "seeds").flags.cpu().numpy() & 1).sum())
        per = torch.from_numpy(pack_mask(rng.random((B, n_p)) < 0.1).view(np.int32)).to(dev)
        ms["seeds_per_query_0.1"] = _time(lambda: run(per, "seeds"), args.reps)
        ms["ranking_per_query_0.1"] = _time(lambda: run(per, "ranking"), args.reps)
        # phase A alone: the unscoped (fused) path and the scoped (fact bitset + two-step) path
        ms["phase_a_unscoped"] = _time(lambda: eng.score_facts(qf, k=5), args.reps)
        ms["phase_a_seeds_broadcast_0.1"] = _time(lambda: eng.score_facts(qf, k=5, scope_filter=one), args.reps)
        ms["phase_a_seeds_per_query_0.1"] = _time(lambda: eng.score_facts(qf, k=5, scope_filter=per), args.reps)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
