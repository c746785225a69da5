#!/usr/bin/env python3
"""Time BatchEngine.step_until_periodic against BatchEngine.step.  One JSON line, printed
and appended to --out (default profiles/batch_until/batch_until_bench.jsonl).

  overhead  where nothing settles: n = 65536 fields of 64 x 64, B3/S23, init_random;
            step_until_periodic(1024, lag=2, check_every=64) against step(1024) on the
            same batch.  Both medians, the spread (max - min) of step's repeats and the
            ratio; `within_expectation`: the overhead is no larger than the greater of
            that spread and 3 % of step's median.
  gain      where fields settle: n = 65536 fields of 16 x 16 with a dead border, B3/S23,
            init_random; step_until_periodic(16384, lag=6) against step(16384).  Both
            times, launches, found / n and wave_generations / (waves * 16384): the
            share of the generations the kernel still computed, against which the time
            ratio is to be read.

The variants alternate, --repeats times each after a warm-up, every run from the same
init_random fields, a host clock around work that ends in a synchronise
(step_until_periodic is synchronous by itself).  It needs a GPU.

  python tools/batch_until_bench.py --out profiles/batch_until/batch_until_bench.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "ms": [round(x, 4) for x in ms]}


def compare(b, gens, lag, check_every, repeats, warmup):
    """step(gens) and step_until_periodic(gens, lag, check_every) on batch b, alternating."""
    last = {}

    def run_step():
        b.init_random(1)
        b.sync()
        return timed_ms(lambda: (b.step(gens), b.sync()))

    def run_until():
        b.init_random(1)
        b.sync()
        return timed_ms(lambda: last.update(r=b.step_until_periodic(gens, lag, check_every)))

    for _ in range(warmup):
        run_step()
        run_until()
    step_ms, until_ms = [], []
    for _ in range(repeats):
        step_ms.append(run_step())
        until_ms.append(run_until())
    r = last["r"]
    waves = -(-b.n // b.fields_per_wave)
    return {**b.info, "gens": gens, "lag": r.lag, "check_every": r.check_every,
            "step": stats(step_ms), "until": stats(until_ms),
            "step_spread_ms": round(max(step_ms) - min(step_ms), 4),
            "ratio": round(statistics.median(until_ms) / statistics.median(step_ms), 4),
            "launches": r.launches, "found": r.found, "found_fraction": round(r.found / b.n, 4),
            "waves": waves, "wave_generations": r.wave_generations,
            "computed_fraction": round(r.wave_generations / (waves * gens), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=65536, help="fields per batch")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--overhead-gens", type=int, default=1024)
    ap.add_argument("--gain-gens", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_until",
                                                  "batch_until_bench.jsonl"))
    a = ap.parse_args()

    import __graft_entry__ as entry
    pkg = entry.load_package()
    rec = {"tool": "batch_until_bench", "n": a.n, "repeats": a.repeats, "rule": "B3/S23"}
    with pkg.BatchEngine(a.n, 64, 64, rule=pkg.CONWAY, device=0) as b:
        o = compare(b, a.overhead_gens, 2, 64, a.repeats, a.warmup)
    over_ms = o["until"]["median_ms"] - o["step"]["median_ms"]
    allowed_ms = max(o["step_spread_ms"], 0.03 * o["step"]["median_ms"])
    o.update(overhead_ms=round(over_ms, 4), overhead_fraction=round(o["ratio"] - 1, 4),
             allowed_ms=round(allowed_ms, 4), within_expectation=over_ms <= allowed_ms)
    rec["overhead"] = o
    with pkg.BatchEngine(a.n, 16, 16, rule=pkg.CONWAY, device=0) as b:
        rec["gain"] = compare(b, a.gain_gens, 6, 0, a.repeats, a.warmup)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
