"""Cost of facets on one MI355X at configs[2] size (125 000 passages: the 1M-node KG's passage share as bench.py builds it)
for B = 1 and B = 256, over four specs -- a keyword column of 300 values, one of about 15 000 values (the source_id shape:
four windows of HRAG_FACET_WINDOW bins), a 12-edge timestamp facet over an F64 column, and a SKEWED 300-value keyword where
one value holds a third of the passages -- under per-query doc filter words that allow about half of the passages:
  (a) hrag_payload_facet alone (PayloadIndex.facet into a ready output, the per-call workspace allocation included);
  (b) hrag_payload_facet_ids over k = 200 ids per query;
  (c) a traffic floor for (a): the column, its presence words, the B rows of filter words and the B rows of counts, each
      moved once, at the 8 TB/s DESIGN.md uses -- the per-query re-reads of the column come from L2 / MALL;
  (d) the host alternative the project has today: the [B, W] words read back, np.unpackbits and one np.bincount per query;
  (e) the skewed column against the uniform one of the same shape: a ratio above 2 means the ballot step of
      csrc/facet.hip does not take the contention away.
HIP-event medians after a warm-up for device work, host clocks around a synchronise for (d).  Every result is checked
against the host count before it is timed.  Prints one JSON line and writes it to --out.

    python tools/bench_facet.py --out facet.json [--small] [--reps 20]
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
from tools.bench_payload import _host_ms  # noqa: E402

PEAK_BPS = 8e12
K_IDS = 200


def host_counts(words, n, codes, n_bins):
    """What a caller does today: unpack the words that came back, one bincount per query."""
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)
    return np.stack([np.bincount(codes[row], minlength=n_bins) for row in bits])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tiny sizes (a rehearsal of the script, not a measurement)")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from hipporag_amd.engine import pack_mask
    from hipporag_amd.facet import compile_facet, facet_splits
    from hipporag_amd.payload import PayloadColumns, PayloadIndex
    from hipporag_amd._lib import PAY_F64, PAY_I64
    dev = torch.device("cuda", 0)
    name, n_p, batches, n_src = ("small", 20000, (1, 16), 9000) if args.small else ("configs[2]", 125_000, (1, 256), 15000)
    W = (n_p + 31) // 32
    rng = np.random.default_rng(1251)
    kw = rng.integers(0, 300, n_p).astype(np.int64)
    src = rng.integers(0, n_src, n_p).astype(np.int64)
    ts = rng.random(n_p) * 365.0
    skew = rng.integers(0, 300, n_p).astype(np.int64)
    skew[rng.random(n_p) < 1 / 3] = 7
    has_src = rng.random(n_p) >= 0.1
    host = PayloadColumns(n_p)
    for cname, typ, vals, pres, vocab in (("kw", PAY_I64, kw, None, 300), ("source_id", PAY_I64, src, has_src, n_src),
                                          ("ts", PAY_F64, ts, None, None), ("skew", PAY_I64, skew, None, 300)):
        host._add(cname, typ, vals, pres, None if vocab is None else {f"v{i:05d}": i for i in range(vocab)})
    res = dict(tool="bench_facet", config=name, n_passages=n_p, words=W, k_ids=K_IDS, reps=args.reps, peak_TBps=PEAK_BPS / 1e12)
    with PayloadIndex(host) as ix:
        specs = {"kw300": (compile_facet(ix, "kw"), kw, None), "source15k": (compile_facet(ix, "source_id"), src, has_src),
                 "ts12": (compile_facet(ix, "ts", edges=[float(e) for e in np.linspace(28.0, 336.0, 12)]), None, None),
                 "skew300": (compile_facet(ix, "skew"), skew, None)}
        for B in batches:
            allowed = rng.random((B, n_p)) < 0.5
            words_np = pack_mask(allowed)
            words = torch.from_numpy(words_np.view(np.int32)).to(dev)
            ids = torch.from_numpy(rng.integers(0, n_p, (B, K_IDS)).astype(np.int32)).to(dev)
            ids[:, -7:] = -1
            for label, (spec, codes, pres) in specs.items():
                key = f"{label}_b{B}"
                out = torch.empty((B, spec.n_bins + 2), dtype=torch.int32, device=dev)
                got = ix.facet(spec, words, out=out).raw.cpu().numpy()
                if codes is not None:        # the check: the host count of the same words
                    live = allowed if pres is None else allowed & pres
                    want = np.stack([np.bincount(codes[r], minlength=spec.n_bins) for r in live])
                    assert np.array_equal(got[:, :spec.n_bins], want), f"{key}: the device counts differ from the host's"
                else:
                    want = np.stack([np.bincount(np.searchsorted(np.linspace(28.0, 336.0, 12), ts[r], side="right"),
                                                 minlength=spec.n_bins) for r in allowed])
                    assert np.array_equal(got[:, :spec.n_bins], want), f"{key}: the device counts differ from the host's"
                assert np.array_equal(got.sum(1), allowed.sum(1))
                res[f"{key}_n_bins"], res[f"{key}_splits"] = spec.n_bins, facet_splits(ix, spec.n_bins, B)
                res[f"{key}_facet_ms"] = _time(lambda: ix.facet(spec, words, out=out), args.reps)
                res[f"{key}_facet_ids_ms"] = _time(lambda: ix.facet(spec, ids=ids, out=out), args.reps)
                floor = (8 * n_p + (4 * W if pres is not None else 0) + B * W * 4 + B * (spec.n_bins + 2) * 4) / PEAK_BPS * 1e3
                res[f"{key}_floor_ms"] = round(floor, 6)
                res[f"{key}_over_floor"] = round(res[f"{key}_facet_ms"] / floor, 1)
                if codes is not None:
                    res[f"{key}_host_ms"] = _host_ms(lambda: host_counts(words.cpu().numpy(), n_p, codes, spec.n_bins), 3)
            res[f"skew_over_uniform_b{B}"] = round(res[f"skew300_b{B}_facet_ms"] / res[f"kw300_b{B}_facet_ms"], 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
