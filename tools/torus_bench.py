#!/usr/bin/env python3
"""Time a torus engine against the dead-border engine of the same size.

For each size (N for an N x N field, or HxW; B3/S23, p = 0.5) this steps, with the
activity skip off on both sides (GOL_DEV_ACTIVITY_SKIP=0):
  * the dead-border engine, streams=1;
  * a torus engine with the auto round length G;
  * torus engines with each --sweep value as halo_depth (the auto-G sweep);
  * with --control, a dead-border engine of the auto torus's padded size: what the
    inner engine costs without wrap and rounds (its ms per generation are per
    padded field; the ratio is to the h x w dead-border engine like the others).
All engines of a size live at once and the samples alternate between them, so
drift of the shared machine hits every engine alike.  A sample is the host time
around `reps` calls of step(gens) ending in sync(), reps chosen so that a sample
takes about --sample-ms; the figure reported is the median over --samples.

Prints one JSON line per engine: ms per generation, the ratio to the dead-border
engine, the padded-area ratio (h + 2G)(w + 128 Gx) / (h w), and what the ratio
leaves unexplained.  The wrap kernel's own time is not in these figures; take it
from a kernel trace of a run of this tool (torus_wrap_kernel's rows).

  python tools/torus_bench.py --sizes 4096,16384 --out profiles/torus/bench.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ["GOL_DEV_ACTIVITY_SKIP"] = "0"
# every engine plans as if alone on the device (hand-off blocks, the resident
# kernel): they are stepped one at a time, each sample ending in a sync
os.environ["GOL_DEV_SHARED_WAITS"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def sample(e, gens, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        e.step(gens)
    e.sync()
    return (time.perf_counter() - t0) * 1e3 / (gens * reps)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="4096,16384,65536")
    ap.add_argument("--sweep", default="16,32,64,128,256", help="halo_depth values to try")
    ap.add_argument("--gens", type=int, default=1024, help="generations per step() call")
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--sample-ms", type=float, default=250.0)
    ap.add_argument("--control", action="store_true",
                    help="also time a dead-border engine of the padded size")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    pkg = entry.load_package()
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for size in a.sizes.split(","):
        h, w = (int(x) for x in size.split("x")) if "x" in size else (int(size), int(size))
        engines = [("dead_border", pkg.Engine(h, w, rule=pkg.CONWAY, device=0, streams=1))]
        engines.append(("torus_auto", pkg.Engine(h, w, rule=pkg.CONWAY, device=0,
                                                 semantics=pkg.SEM_TORUS)))
        for G in (int(s) for s in a.sweep.split(",") if s):
            if G != engines[1][1].halo_depth:
                engines.append((f"torus_G{G}", pkg.Engine(h, w, rule=pkg.CONWAY, device=0,
                                                          semantics=pkg.SEM_TORUS, halo_depth=G)))
        if a.control:
            g = pkg.torus_geometry(h, w, rule=pkg.CONWAY)
            engines.append(("dead_border_padded", pkg.Engine(g["padded_h"], g["padded_w"],
                                                             rule=pkg.CONWAY, device=0, streams=1)))
        reps = {}
        for name, e in engines:
            e.init_random(1)
            e.step(a.gens)  # warm-up: code objects, the step graph of this length
            e.sync()
            once = sample(e, a.gens, 1)
            reps[name] = max(1, int(a.sample_ms / (once * a.gens)))
        times = {name: [] for name, _ in engines}
        for _ in range(a.samples):
            for name, e in engines:
                times[name].append(sample(e, a.gens, reps[name]))
        base = statistics.median(times["dead_border"])
        for name, e in engines:
            med = statistics.median(times[name])
            rec = {"h": h, "w": w, "engine": name, "gens_per_step": a.gens, "reps": reps[name],
                   "ms_per_gen": round(med, 6), "min": round(min(times[name]), 6),
                   "max": round(max(times[name]), 6),
                   "tcups": round(e.h * e.w / med / 1e9, 2), "tb_depth": e.tb_depth,
                   "resident": e.resident, "rows_per_wave": e.rows_per_wave}
            if name == "dead_border_padded":
                rec.update({"ratio": round(med / base, 4),
                            "area_ratio": round(e.h * e.w / (h * w), 4)})
            elif name != "dead_border":
                G = e.halo_depth
                Gx = (G + 63) // 64
                area = (h + 2 * G) * (w + 128 * Gx) / (h * w)
                rec.update({"G": G, "ratio": round(med / base, 4), "area_ratio": round(area, 4),
                            "beyond_area": round(med / base - area, 4),
                            "rounds_per_step": -(-a.gens // G)})
            emit(rec)
        for _, e in engines:
            e.close()


if __name__ == "__main__":
    main()
