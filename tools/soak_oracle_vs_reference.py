#!/usr/bin/env python
"""Randomised soak of the ORACLE against the real reference package (CPU, authoring container only: needs
/root/reference): random synthetic corpora (documents, OpenIE triples incl. duplicates, shared facts, passages without
triples, near-duplicate entity names -> synonymy edges), random configurations (damping, linking_top_k,
passage_node_weight) and filter behaviours (identity / subsets in the filter's own order / nothing kept) are indexed and
queried by the reference's own code (tests/golden/ref_harness.py: everything real except igraph -> an in-memory multigraph
whose PageRank is oracle/prpack_port.c, the LLM steps and the embedding model), and every stage the reference produced --
fact scores, candidates, reset vectors, run_ppr rankings, retrieve() and retrieve_dpr() results -- is checked against the
oracle with the assertions of tests/test_ref_golden.py.  The committed fixtures are three such cases; this widens the pin.
--record FILE keeps what the reference produced for every case; --replay FILE checks the oracle against such a recording
instead of running the reference (same --cases / --seed: the corpora and configurations come from the same generator), which
is how tests/test_ref_golden.py runs it on tests/golden/ref_soak_oracle_s11.npz.

    python tools/soak_oracle_vs_reference.py [--cases 40] [--seed 1] [--record FILE | --replay FILE]"""
import argparse
import json
import os
import sys
import time
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=40)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "gpurun_out", "soak_oracle_vs_reference.json"))
    ap.add_argument("--record", default=None, help="write the reference's output of every case to this .npz")
    ap.add_argument("--replay", default=None, help="check against the reference outputs recorded in this .npz")
    args = ap.parse_args()
    import ref_harness as rh
    if not args.replay and not rh.reference_available():
        print("the reference sources are not present: nothing to do")
        return 0
    recorded = dict(np.load(args.replay)) if args.replay else {}
    import make_ref_golden as mg
    from tests import test_ref_golden as trg
    import oracle
    from hipporag_amd.retriever import sweeps_for_damping
    from tests.helpers import tie_aware_equal

    fixed_count_err = []

    def ppr_matches_reference_run_ppr(case):
        """tests/test_ref_golden.py::test_oracle_ppr_matches_reference_run_ppr with the sweep count of the case's damping
        (the fixture test hard-codes the 20 sweeps of damping 0.5)."""
        t = trg.load(case)
        index = trg.ref_index(t)
        damping = float(t["damping"])
        for q in range(len(t["qf"])):
            if t["used_dpr"][q]:
                continue
            ids, sc, _ = oracle.run_ppr(index, t["reset"][q], damping)
            np.testing.assert_allclose(sc, t["ppr_scores"][q], rtol=2e-8, atol=1e-13)
            assert tie_aware_equal(ids, t["ppr_ids"][q], t["ppr_scores"][q], rel_gap=1e-7)
            ids_k, sc_k, _ = oracle.run_ppr(index, t["reset"][q], damping, mode="power", iters=sweeps_for_damping(damping))
            by_pos = np.empty(len(sc_k)); by_pos[ids_k] = sc_k
            ref_by_pos = np.empty(len(sc_k)); ref_by_pos[t["ppr_ids"][q]] = t["ppr_scores"][q]
            nz = ref_by_pos > 0
            # what that many sweeps leave: a fixed count is only as accurate as the graph mixes (the reference's PRPACK
            # iterates to 1e-10 whatever the graph) -- recorded, not asserted: it is why the product has ppr_tol
            fixed_count_err.append(float(np.max(np.abs(by_pos[nz] - ref_by_pos[nz]) / ref_by_pos[nz])))

    checks = [trg.test_oracle_similarity_matches_reference, trg.test_oracle_fact_candidates_match_reference,
              trg.test_oracle_reset_vector_matches_reference, ppr_matches_reference_run_ppr,
              trg.test_oracle_end_to_end_matches_reference_retrieve, trg.test_oracle_retrieve_dpr_matches_reference]
    rng = np.random.default_rng(args.seed)
    rows, bad = [], 0
    for n in range(args.cases):
        n_docs, n_ent = int(rng.integers(12, 220)), int(rng.integers(20, 320))
        cfg = dict(damping=float(rng.choice([0.5, 0.5, 0.3, 0.7, 0.85])), linking_top_k=int(rng.choice([5, 5, 2, 8])),
                   passage_node_weight=float(rng.choice([0.05, 0.05, 0.01, 0.5])))
        mode = str(rng.choice(["identity", "mixed"]))
        seed = int(rng.integers(1, 1 << 30))
        par = dict(n_docs=n_docs, n_ent=n_ent, seed=seed, filter=mode, **cfg)
        t0 = time.time()
        try:
            if args.replay:
                out = {k.split("__", 1)[1]: v for k, v in recorded.items() if k.startswith(f"c{n}__")}
                assert out, f"case {n} is not in {args.replay}"
            else:
                docs, triples, queries = mg.synth_corpus(n_docs, n_ent, seed)
                out = mg.run_case(f"soak{n}", docs, triples, queries, mode, save=False, **cfg)
                if args.record:
                    recorded.update({f"c{n}__{k}": np.asarray(v) for k, v in out.items()})
            trg.load = lambda case, _o=out: _o
            failed = []
            for chk in checks:
                try:
                    chk("soak")
                except AssertionError as exc:
                    failed.append(f"{chk.__name__}: {str(exc)[:200]}")
            par.update(ok=not failed, seconds=round(time.time() - t0, 1), V=int(out["num_vertices"]), facts=int(len(out["subj_vertex"])),
                       dpr_fallbacks=int(out["used_dpr"].sum()), fixed_sweep_count_max_rel_err=max(fixed_count_err, default=0.0))
            fixed_count_err.clear()
            if failed:
                par["failed"] = failed
        except Exception as exc:  # noqa: BLE001
            par.update(ok=False, error=f"{type(exc).__name__}: {str(exc)[:300]}", trace=traceback.format_exc()[-600:])
        bad += 0 if par["ok"] else 1
        print("ok  " if par["ok"] else "FAIL", json.dumps(par), flush=True)
        rows.append(par)
    if args.record:
        np.savez_compressed(args.record, **recorded)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump({"cases": rows, "failed": bad}, open(args.out, "w"), indent=0)
    print(f"{len(rows)} cases;", "SOAK OK" if bad == 0 else f"SOAK FAILED ({bad})")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
