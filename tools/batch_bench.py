#!/usr/bin/env python3
"""Time the batch engine (BatchEngine, gol_batch) against its two yardsticks.  One JSON
line, printed and appended to --out (default profiles/batch/batch_bench.jsonl).

  batch       n = 65536 fields of 64 x 64 (2^28 cells, the cell count of a 16384^2
              field), B3/S23, init_random, step(1024); the same at 16 x 16 and at
              64 x 256.  Cell-generations per second.
  yardstick 1 the streaming engine's computing rate: Engine(16384, 16384), B3/S23,
              init_random, step(1024), created with GOL_DEV_ACTIVITY_SKIP=0, in the same
              units.  The variants alternate, --repeats times each after a warm-up, a
              host clock around work that ends in a synchronise.  `meets_target`: the
              64 x 64 batch's median rate is at least the engine's median rate less the
              spread (max - min) of the engine's own repeats.
  yardstick 2 256 Engine(64, 64) handles, created once, stepped 1024 generations one
              after another and then synchronised: time per field against the batch's
              time per field.
  launch      one launch of the 64-row B3/S23 kernel at the default launch cap
              (step(launch_generations) on the 65536 x 64 x 64 batch), in ms.

It needs a GPU: creating the first engine fails without one, and so does the tool.

  python tools/batch_bench.py --out profiles/batch/batch_bench.jsonl
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=65536, help="fields per batch")
    ap.add_argument("--gens", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--field", type=int, default=16384, help="side of the streaming engine's field")
    ap.add_argument("--handles", type=int, default=256, help="Engine(64, 64) handles of yardstick 2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch", "batch_bench.jsonl"))
    a = ap.parse_args()

    import __graft_entry__ as entry
    pkg = entry.load_package()
    gens = a.gens

    # the streaming engine, as the parent commit runs it, without the activity skip
    old = os.environ.get("GOL_DEV_ACTIVITY_SKIP")
    os.environ["GOL_DEV_ACTIVITY_SKIP"] = "0"
    engine = pkg.Engine(a.field, a.field, rule=pkg.CONWAY, device=0)
    if old is None:
        del os.environ["GOL_DEV_ACTIVITY_SKIP"]
    else:
        os.environ["GOL_DEV_ACTIVITY_SKIP"] = old
    shapes = [(64, 64), (16, 16), (64, 256)]
    batches = {s: pkg.BatchEngine(a.n, s[0], s[1], rule=pkg.CONWAY, device=0) for s in shapes}

    def run(obj, seed):
        obj.init_random(seed)
        obj.sync()
        return timed_ms(lambda: (obj.step(gens), obj.sync()))

    for _ in range(2):  # warm-up: code objects, graphs, staging
        run(engine, 1)
        for b in batches.values():
            run(b, 1)
    ms = {"engine": [], **{s: [] for s in shapes}}
    for r in range(a.repeats):
        ms["engine"].append(run(engine, 1))
        for s in shapes:
            ms[s].append(run(batches[s], 1))

    def rate(cells, t_ms):
        return cells * gens / (t_ms / 1e3)

    ecells = a.field * a.field
    erates = [rate(ecells, t) for t in ms["engine"]]
    rec = {"tool": "batch_bench", "n": a.n, "gens": gens, "repeats": a.repeats, "rule": "B3/S23",
           "engine": {"h": a.field, "w": a.field, "tb_depth": engine.tb_depth,
                      "resident": engine.resident is not None, **stats(ms["engine"]),
                      "cell_gens_per_s": statistics.median(erates),
                      "spread_cell_gens_per_s": max(erates) - min(erates)},
           "batch": {}}
    for s in shapes:
        b = batches[s]
        cells = a.n * s[0] * s[1]
        rates = [rate(cells, t) for t in ms[s]]
        rec["batch"][f"{s[0]}x{s[1]}"] = {**b.info, **stats(ms[s]),
                                          "cell_gens_per_s": statistics.median(rates),
                                          "us_per_field": statistics.median(ms[s]) * 1e3 / a.n}
    b64 = rec["batch"]["64x64"]
    target = rec["engine"]["cell_gens_per_s"] - rec["engine"]["spread_cell_gens_per_s"]
    rec["target_cell_gens_per_s"] = target
    rec["ratio_to_engine"] = round(b64["cell_gens_per_s"] / rec["engine"]["cell_gens_per_s"], 4)
    rec["meets_target"] = b64["cell_gens_per_s"] >= target

    # one launch at the default cap
    b = batches[(64, 64)]
    cap = b.launch_generations
    launch = []
    for _ in range(3):
        b.init_random(1)
        b.sync()
        launch.append(timed_ms(lambda: (b.step(cap), b.sync())))
    rec["launch_at_cap"] = {"launch_generations": cap, **stats(launch)}
    engine.close()
    for b in batches.values():
        b.close()

    # yardstick 2: one handle per field
    handles = [pkg.Engine(64, 64, rule=pkg.CONWAY, device=0) for _ in range(a.handles)]

    def step_all():
        for e in handles:
            e.step(gens)
        for e in handles:
            e.sync()

    for i, e in enumerate(handles):
        e.init_random(1 + i)
    step_all()  # warm-up
    per = []
    for _ in range(a.repeats):
        for i, e in enumerate(handles):
            e.init_random(1 + i)
        for e in handles:
            e.sync()
        per.append(timed_ms(step_all))
    for e in handles:
        e.close()
    us_handle = statistics.median(per) * 1e3 / a.handles
    rec["handles"] = {"count": a.handles, "resident": handles[0].resident is not None, **stats(per),
                      "us_per_field": us_handle,
                      "batch_us_per_field": b64["us_per_field"],
                      "ratio": round(us_handle / b64["us_per_field"], 1)}
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
