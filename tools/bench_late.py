"""Cost of late-interaction reranking on one MI355X at configs[2] size (1M-node / 10M-edge KG, dim 768, n_passages as
bench.py builds it) with a token index of 60 .. 300 tokens per passage, dim 128, bf16, and 32 tokens per query, for
B in {256, 1} and c in {200, 1024}:
  (a) call cost: HippoRAGEngine.retrieve(k=200) and retrieve(k=200, late=, late_candidates=c) in ALTERNATING runs -- the
      added time per call (the late call also ranks c instead of 200 entries first);
  (b) kernel times: hrag_late_scores and hrag_late_rank_rows alone over the candidates that call ranked, HIP-event medians
      after warm-up;
  (c) traffic floor of the scores kernel: the bytes of the gathered token rows (every candidate's rows once) plus the query
      tokens, over the 6.29 TB/s a streaming copy measures on this part (8 TB/s spec is reported beside it), and the ratio
      of the kernel's time to that floor;
  (d) the torch comparison on the same GPU, what a caller does today: a padded gather of the candidates' token rows,
      einsum, amax over the (masked) passage tokens, sum over the query tokens, topk, then the read-back of the ids --
      in slices of queries, the padded gather of a whole batch being tens of gigabytes.
Prints one JSON line and writes it to --out.

    python tools/bench_late.py --out profiles/late_cfg2_bench_late.json [--small] [--reps 20]
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

STREAM_BPS, SPEC_BPS = 6.29e12, 8e12
TOK_DIM, Q_TOKENS, LEN_LO, LEN_HI = 128, 32, 60, 300


def torch_maxsim(tok_emb, tok_ptr_dev, q_tok, cand, k, slice_q):
    """The caller's side computation: (ids on the host, scores) of the k best candidates by MaxSim, in torch."""
    import torch
    b, c = cand.shape
    lmax = LEN_HI
    j = torch.arange(lmax, device=cand.device)
    out_i, out_s = [], []
    for lo in range(0, b, slice_q):
        cd = cand[lo:lo + slice_q].long()
        start, length = tok_ptr_dev[cd], tok_ptr_dev[cd + 1] - tok_ptr_dev[cd]
        live = j[None, None, :] < length[..., None]                              # [s, c, lmax]
        pos = torch.where(live, start[..., None] + j, torch.zeros_like(start[..., None]))
        rows = tok_emb[pos]                                                      # the padded gather [s, c, lmax, dim]
        s = torch.einsum("qid,qcjd->qcij", q_tok[lo:lo + slice_q], rows).float()
        s = s.masked_fill(~live[:, :, None, :], float("-inf"))
        sc = s.amax(dim=3).sum(dim=2)                                            # [s, c]
        top = sc.topk(k, dim=1)
        out_i.append(torch.gather(cand[lo:lo + slice_q], 1, top.indices))
        out_s.append(top.values)
    return torch.cat(out_i).cpu(), torch.cat(out_s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tiny sizes (a rehearsal of the script, not a measurement)")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from hipporag_amd import _lib, synth
    from hipporag_amd.engine import HippoRAGEngine, LateQueries, TokenIndex, _stream
    dev = torch.device("cuda", 0)
    name, V, E, D, batches, cs = (("small", 40000, 400000, 128, (16, 1), (50, 200)) if args.small
                                  else ("configs[2]", 1_000_000, 10_000_000, 768, (256, 1), (200, 1024)))
    k = min(200, cs[0])
    kg = synth.make_kg(V, E, 1237)
    pass_bits = synth.make_embeddings_np(kg.n_passages, D, 1238)
    fact_bits = synth.make_embeddings_np(kg.n_facts, D, 1239)
    n_p = kg.n_passages
    rng = np.random.default_rng(1244)
    lens = rng.integers(LEN_LO, LEN_HI + 1, n_p)
    tok_ptr = np.zeros(n_p + 1, np.int64)
    tok_ptr[1:] = np.cumsum(lens)
    n_tok = int(tok_ptr[-1])
    g = torch.Generator(device=dev)
    g.manual_seed(1245)
    tok_emb = torch.empty((n_tok, TOK_DIM), dtype=torch.bfloat16, device=dev)
    for lo in range(0, n_tok, 1 << 20):                                          # unit-norm Gaussian tokens, in slices
        x = torch.randn((min(1 << 20, n_tok - lo), TOK_DIM), generator=g, device=dev)
        tok_emb[lo:lo + x.shape[0]] = (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16)
    res = dict(tool="bench_late", config=name, V=V, E=E, D=D, n_passages=n_p, k=k, reps=args.reps, tok_dim=TOK_DIM,
               query_tokens=Q_TOKENS, passage_tokens=[LEN_LO, LEN_HI], n_tokens=n_tok, token_index_GB=round(n_tok * TOK_DIM * 2 / 1e9, 3),
               stream_TBps=STREAM_BPS / 1e12, spec_TBps=SPEC_BPS / 1e12, cases=[])
    to_q = lambda bits: torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)  # noqa: E731
    lib = _lib.load()
    tok_ptr_dev = torch.from_numpy(tok_ptr).to(dev)
    t0 = time.perf_counter()
    tix = TokenIndex.from_csr(tok_ptr, tok_emb, "bf16")
    res["index_build_s"] = round(time.perf_counter() - t0, 3)
    with tix, HippoRAGEngine(kg.csr, kg.passage_vertex, pass_bits, fact_bits, kg.subj_vertex, kg.obj_vertex, kg.num_chunks,
                             max_batch=max(batches), max_topk=max(cs)) as eng:
        eng.set_token_index(tix)
        for B in batches:
            qf = to_q(synth.make_queries_np(fact_bits, B, seed=1)[0])
            qp = to_q(synth.make_queries_np(pass_bits, B, seed=2)[0])
            idx, sc = eng.score_facts(qf, k=5)
            cnt = torch.full((B,), 5, dtype=torch.int32, device=dev)
            qt = torch.randn((B * Q_TOKENS, TOK_DIM), generator=g, device=dev)
            qt = (qt / qt.norm(dim=1, keepdim=True)).to(torch.bfloat16)
            lq = LateQueries(np.arange(B + 1) * Q_TOKENS, qt, "bf16")
            q3 = qt.view(B, Q_TOKENS, TOK_DIM)

            def retrieve(**kw):
                return eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=k, want_residual=False, **kw)

            for c in cs:
                case = dict(batch=B, c=c)
                plain_ms, late_ms = _alternating(retrieve, lambda: retrieve(late=lq, late_candidates=c), args.reps)
                case.update(retrieve_plain_ms=plain_ms, retrieve_late_ms=late_ms, late_extra_ms=round(late_ms - plain_ms, 4))
                cand = eng.retrieve(qp, idx, sc, cnt, ppr_iters=20, k=c, want_residual=False).doc_idx.contiguous()
                out = torch.empty((B, c), dtype=torch.float32, device=dev)
                sel, oi = (torch.empty((B, k), dtype=torch.int32, device=dev) for _ in range(2))
                os_ = torch.empty((B, k), dtype=torch.float32, device=dev)
                case["late_scores_ms"] = _time(lambda: _lib.check(lib.hrag_late_scores(
                    tix._handle, lq.q_ptr.ctypes.data, lq.q_ptr_dev.data_ptr(), lq.q_tok.data_ptr(), B, cand.data_ptr(), c,
                    out.data_ptr(), c, _stream())), args.reps)
                case["late_rank_rows_ms"] = _time(lambda: _lib.check(lib.hrag_late_rank_rows(
                    out.data_ptr(), c, cand.data_ptr(), n_p, B, c, k, sel.data_ptr(), oi.data_ptr(), os_.data_ptr(), _stream())),
                    args.reps)
                rows = int(lens[cand.clamp_min(0).cpu().numpy()].sum())
                nbytes = rows * TOK_DIM * 2 + B * Q_TOKENS * TOK_DIM * 2
                floor_ms = nbytes / STREAM_BPS * 1e3
                case.update(gathered_token_rows=rows, traffic_GB=round(nbytes / 1e9, 4), floor_ms=round(floor_ms, 5),
                            floor_spec_ms=round(nbytes / SPEC_BPS * 1e3, 5),
                            scores_over_floor=round(case["late_scores_ms"] / floor_ms, 2),
                            mfma_per_call=int(-(-rows // 16) * (TOK_DIM // 32) * (Q_TOKENS // 16)))
                slice_q = max(1, min(B, (1 << 30) // (c * LEN_HI * TOK_DIM * 2)))        # <= 1 GiB of padded rows per slice
                case["torch_slice_queries"] = slice_q
                case["torch_ms"] = _time(lambda: torch_maxsim(tok_emb, tok_ptr_dev, q3, cand, k, slice_q), max(3, args.reps // 4), 1)
                ti, _ = torch_maxsim(tok_emb, tok_ptr_dev, q3, cand, k, slice_q)
                li, _ = eng.late_rerank(cand, lq, k)
                case["torch_top1_agrees"] = round(float((ti[:, 0] == li.cpu()[:, 0]).float().mean().item()), 3)
                res["cases"].append(case)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
