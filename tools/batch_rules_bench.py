#!/usr/bin/env python3
"""Time a batch with per-field rules (BatchEngine.set_rules) against uniform batches.  One
JSON line, printed and appended to --out (default profiles/batch_rules/batch_rules_bench.jsonl).

On n = 65536 fields of 64 x 64 and of 16 x 16, init_random, step(1024), four variants:

  conway        a uniform B3/S23 batch (the pair-sum kernel);
  generic       a uniform B36/S23 batch (the generic kernel: two scalar masks);
  table_same    a rule table with B36/S23 in every field (the per-lane-rule kernel);
  table_random  a table of seeded random rules.

`generic` is the yardstick of `table_same`: the same rule, the same fields, the same work
apart from the rule network.  `table_over_generic` is the ratio of their median rates, with
both spreads (max - min of the repeats' rates) beside it; no ratio is fixed in advance.
The fields of `table_random` evolve differently, so it is reported as a rate only.  The
variants alternate, --repeats times each after a warm-up, a host clock around work that
ends in a synchronise.

It needs a GPU: creating the first batch fails without one, and so does the tool.

  python tools/batch_rules_bench.py --out profiles/batch_rules/batch_rules_bench.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B36S23 = (0b1001000, 0b1100)
VARIANTS = ["conway", "generic", "table_same", "table_random"]


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=65536, help="fields per batch")
    ap.add_argument("--gens", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=950, help="seed of the random rule table")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_rules",
                                                  "batch_rules_bench.jsonl"))
    a = ap.parse_args()

    import numpy as np

    import __graft_entry__ as entry
    pkg = entry.load_package()
    n, gens = a.n, a.gens
    rng = np.random.default_rng(a.seed)
    rand = rng.integers(0, 512, size=(2, n), dtype=np.uint32)

    def make(variant, h, w):
        rule = pkg.CONWAY if variant == "conway" else B36S23
        b = pkg.BatchEngine(n, h, w, rule=rule, device=0)
        if variant == "table_same":
            b.set_rules(np.full(n, B36S23[0]), np.full(n, B36S23[1]))
        elif variant == "table_random":
            b.set_rules(rand[0], rand[1])
        return b

    def run(b):
        b.init_random(1)
        b.sync()
        return timed_ms(lambda: (b.step(gens), b.sync()))

    rec = {"tool": "batch_rules_bench", "n": n, "gens": gens, "repeats": a.repeats,
           "seed": a.seed, "shapes": {}}
    for h, w in ((64, 64), (16, 16)):
        batches = {v: make(v, h, w) for v in VARIANTS}
        assert [batches[v].per_field_rules for v in VARIANTS] == [False, False, True, True]
        for _ in range(2):  # warm-up: code objects, clocks
            for v in VARIANTS:
                run(batches[v])
        ms = {v: [] for v in VARIANTS}
        for r in range(a.repeats):
            for v in VARIANTS:
                ms[v].append(run(batches[v]))
            print(f"# {h}x{w} repeat {r + 1}: " +
                  " ".join(f"{v}={ms[v][-1]:.2f}ms" for v in VARIANTS), file=sys.stderr, flush=True)
        cells = n * h * w
        out = {"rows_in_regs": batches["conway"].rows_in_regs}
        for v in VARIANTS:
            rates = [cells * gens / (t / 1e3) for t in ms[v]]
            out[v] = {"median_ms": round(statistics.median(ms[v]), 4),
                      "ms": [round(x, 4) for x in ms[v]],
                      "cell_gens_per_s": statistics.median(rates),
                      "spread_cell_gens_per_s": max(rates) - min(rates)}
            batches[v].close()
        out["table_over_generic"] = round(out["table_same"]["cell_gens_per_s"] /
                                          out["generic"]["cell_gens_per_s"], 4)
        rec["shapes"][f"{h}x{w}"] = out
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
