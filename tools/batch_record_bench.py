#!/usr/bin/env python3
"""Time a batch's recorded rollout (BatchEngine.step_record) against plain stepping and
against the loop it replaces.  One JSON line, printed and appended to --out (default
profiles/batch_record/batch_record_bench.jsonl).

On n = 65536 B3/S23 fields of 64 x 64 and of 16 x 16, init_random, for the settings
(G, E) = (1024, 64), (1024, 16) and (128, 1) -- at every = 1 only 128 generations, so that
the frames stay at 4 GB (1 GB) on a shared machine:

  step_G            (a) step(G);
  rec_tensor_E      (b) step_record_tensor(G, E): the frames stay on the device;
  rec_device_E      gol_batch_step_record_device itself into a tensor made before the clock
                    starts: rec_tensor_E without torch's allocation, fill and stream
                    synchronise;
  loop_E            (c) G / E times step(E) + store_tensor(), the tensors kept: what gave
                    the frames before;
  rec_host_E        step_record(G, E): the frames end in a numpy array;
  window_1          step_record_tensor(1024, 1, first, 64): 64 fields out of the n, every
                    generation, against step_1024.

`step_G` is the yardstick of the record calls (the same kernels' pass, the same fields, no
frames) and `loop_E` the alternative they replace.  The ratios are ratios of median times,
with each variant's spread (max - min of the repeats) beside its median; no ratio is fixed
in advance.  store_GBps_E is the frames' bytes over rec_device_E's median, and
store_extra_GBps_E the same bytes over (rec_device_E - step_G): the rate at which the
kernel's stores go out beside its passes.  The variants alternate, --repeats times each
after a warm-up, a host clock around work that ends in a synchronise (the record calls are
synchronous themselves).

It needs a GPU: creating the first batch fails without one, and so does the tool.

  python tools/batch_record_bench.py --out profiles/batch_record/batch_record_bench.jsonl
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (generations, every)
SETTINGS = ((1024, 64), (1024, 16), (128, 1))
WINDOW_GENS, WINDOW_COUNT = 1024, 64


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=65536, help="fields per batch")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="64x64,16x16")
    ap.add_argument("--no-host", action="store_true", help="leave the host form out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_record",
                                                  "batch_record_bench.jsonl"))
    a = ap.parse_args()

    import torch
    import __graft_entry__ as entry
    pkg = entry.load_package()
    n = a.n
    count_w = min(WINDOW_COUNT, n)
    first_w = (n - count_w) // 2 + 1 if n > count_w + 1 else 0

    def loop(b, gens, every):
        kept = []
        for _ in range(gens // every):
            b.step(every)
            kept.append(b.store_tensor())
        return kept

    def prealloc(b, gens, every):
        dev = torch.device("cuda", torch.cuda.current_device())
        t = torch.zeros((gens // every, n, b.h, b.wq), dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        return t

    def record_device(b, t, gens, every):
        r = pkg.BatchRecord(struct_size=ctypes.sizeof(pkg.BatchRecord))
        fs = b.h * b.wq
        st = pkg.lib().gol_batch_step_record_device(b._h, gens, every, 0, n, t.data_ptr(),
                                                    n * fs, fs, b.wq, ctypes.byref(r))
        assert st == pkg.GOL_OK and r.samples == gens // every

    held = {}
    variants = {}
    for g in sorted({g for g, _ in SETTINGS} | {WINDOW_GENS}):
        variants[f"step_{g}"] = lambda b, g=g: (b.step(g), b.sync())
    for g, e in SETTINGS:
        variants[f"rec_tensor_{e}"] = lambda b, g=g, e=e: b.step_record_tensor(g, e)
        variants[f"rec_device_{e}"] = lambda b, g=g, e=e: record_device(b, held["t"], g, e)
        variants[f"loop_{e}"] = lambda b, g=g, e=e: loop(b, g, e)
        if not a.no_host:
            variants[f"rec_host_{e}"] = lambda b, g=g, e=e: b.step_record(g, e)
    variants["window_1"] = lambda b: b.step_record_tensor(WINDOW_GENS, 1, first_w, count_w)
    settings_of = {f"rec_device_{e}": (g, e) for g, e in SETTINGS}

    def run(b, v):
        b.init_random(1)
        b.sync()
        held.pop("t", None)
        if v in settings_of:
            held["t"] = prealloc(b, *settings_of[v])
        return timed_ms(lambda: variants[v](b))

    rec = {"tool": "batch_record_bench", "n": n, "repeats": a.repeats, "rule": "B3/S23",
           "settings": [list(s) for s in SETTINGS], "window": [first_w, count_w, WINDOW_GENS],
           "shapes": {}}
    for shape in a.shapes.split(","):
        h, w = (int(x) for x in shape.split("x"))
        with pkg.BatchEngine(n, h, w, rule=pkg.CONWAY, device=0) as b:
            for v in variants:  # warm-up: code objects, the record buffer, torch's pool
                run(b, v)
            ms = {v: [] for v in variants}
            for r in range(a.repeats):
                for v in variants:
                    ms[v].append(run(b, v))
                print(f"# {h}x{w} repeat {r + 1}: " +
                      " ".join(f"{v}={ms[v][-1]:.2f}ms" for v in variants),
                      file=sys.stderr, flush=True)
            out = {"rows_in_regs": b.rows_in_regs, "frame_bytes": n * b.h * b.wq * 8}
        held.pop("t", None)
        torch.cuda.empty_cache()
        for v in variants:
            out[v] = {"median_ms": round(statistics.median(ms[v]), 4),
                      "spread_ms": round(max(ms[v]) - min(ms[v]), 4),
                      "ms": [round(x, 4) for x in ms[v]]}
        med = lambda v: out[v]["median_ms"]
        for g, e in SETTINGS:
            step = med(f"step_{g}")
            out[f"b_over_a_tensor_{e}"] = round(med(f"rec_tensor_{e}") / step, 4)
            out[f"b_over_a_device_{e}"] = round(med(f"rec_device_{e}") / step, 4)
            out[f"c_over_b_tensor_{e}"] = round(med(f"loop_{e}") / med(f"rec_tensor_{e}"), 4)
            out[f"c_over_b_device_{e}"] = round(med(f"loop_{e}") / med(f"rec_device_{e}"), 4)
            if not a.no_host:
                out[f"b_over_a_host_{e}"] = round(med(f"rec_host_{e}") / step, 4)
                out[f"c_over_b_host_{e}"] = round(med(f"loop_{e}") / med(f"rec_host_{e}"), 4)
            gb = out["frame_bytes"] * (g // e) / 1e9
            out[f"store_GBps_{e}"] = round(gb / (med(f"rec_device_{e}") / 1e3), 2)
            extra = med(f"rec_device_{e}") - step
            out[f"store_extra_GBps_{e}"] = round(gb / (extra / 1e3), 2) if extra > 0 else None
        out["window_over_step"] = round(med("window_1") / med(f"step_{WINDOW_GENS}"), 4)
        for g in {g for g, _ in SETTINGS}:
            out[f"step_{g}_spread_over_median"] = round(
                out[f"step_{g}"]["spread_ms"] / med(f"step_{g}"), 4)
        rec["shapes"][f"{h}x{w}"] = out
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
