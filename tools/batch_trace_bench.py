#!/usr/bin/env python3
"""Time a batch's population trace (BatchEngine.step_trace) against plain stepping and
against the loop it replaces.  One JSON line, printed and appended to --out (default
profiles/batch_trace/batch_trace_bench.jsonl).

On n = 65536 B3/S23 fields of 64 x 64 and of 16 x 16, init_random, 1024 generations:

  step              (a) step(1024);
  trace_host_E      (b) step_trace(1024, E), E in 1, 16, 64: the samples end in a numpy array;
  trace_tensor_E    (b) step_trace_tensor(1024, E): the samples stay on the device;
  loop_E            (c) 1024 / E times step(E) + digest(): what gave the curve before;
  trace_device_64   gol_batch_step_trace_device itself, every 64, into a tensor made before
                    the clock starts: trace_tensor_64 without torch's allocation, fill and
                    stream synchronise, which alloc_64 times alone.

`step` is the yardstick of the trace calls (the same kernels' pass, the same fields, no
samples) and `loop_E` the alternative they replace.  b_over_a and c_over_b are ratios of
median times, with each variant's spread (max - min of the repeats) beside its median; no
ratio is fixed in advance.  The variants alternate, --repeats times each after a warm-up,
a host clock around work that ends in a synchronise (the trace calls and digest() are
synchronous themselves).

It needs a GPU: creating the first batch fails without one, and so does the tool.

  python tools/batch_trace_bench.py --out profiles/batch_trace/batch_trace_bench.jsonl
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

EVERY = (1, 16, 64)


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=65536, help="fields per batch")
    ap.add_argument("--gens", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_trace",
                                                  "batch_trace_bench.jsonl"))
    a = ap.parse_args()

    import __graft_entry__ as entry
    pkg = entry.load_package()
    n, gens = a.n, a.gens

    def loop(b, every):
        for _ in range(gens // every):
            b.step(every)
            b.digest()

    variants = {"step": lambda b: (b.step(gens), b.sync())}
    for e in EVERY:
        variants[f"trace_host_{e}"] = lambda b, e=e: b.step_trace(gens, e)
        variants[f"trace_tensor_{e}"] = lambda b, e=e: b.step_trace_tensor(gens, e)
        variants[f"loop_{e}"] = lambda b, e=e: loop(b, e)
    held = {}
    variants["trace_device_64"] = lambda b: trace_device(b, held["t"])
    variants["alloc_64"] = lambda b: prealloc(b)

    def prealloc(b):
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        t = torch.zeros((gens // 64, n), dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        return t

    def trace_device(b, t):
        r = pkg.BatchTrace(struct_size=ctypes.sizeof(pkg.BatchTrace))
        st = pkg.lib().gol_batch_step_trace_device(b._h, gens, 64, t.data_ptr(), n,
                                                   ctypes.byref(r))
        assert st == pkg.GOL_OK and r.samples == gens // 64

    def run(b, v):
        b.init_random(1)
        b.sync()
        if v == "trace_device_64":
            held["t"] = prealloc(b)
        return timed_ms(lambda: variants[v](b))

    rec = {"tool": "batch_trace_bench", "n": n, "gens": gens, "repeats": a.repeats,
           "rule": "B3/S23", "shapes": {}}
    for h, w in ((64, 64), (16, 16)):
        with pkg.BatchEngine(n, h, w, rule=pkg.CONWAY, device=0) as b:
            for v in variants:  # warm-up: code objects, the trace and staging buffers, clocks
                run(b, v)
            ms = {v: [] for v in variants}
            for r in range(a.repeats):
                for v in variants:
                    ms[v].append(run(b, v))
                print(f"# {h}x{w} repeat {r + 1}: " +
                      " ".join(f"{v}={ms[v][-1]:.2f}ms" for v in variants),
                      file=sys.stderr, flush=True)
            out = {"rows_in_regs": b.rows_in_regs}
        for v in variants:
            out[v] = {"median_ms": round(statistics.median(ms[v]), 4),
                      "spread_ms": round(max(ms[v]) - min(ms[v]), 4),
                      "ms": [round(x, 4) for x in ms[v]]}
        med = lambda v: out[v]["median_ms"]
        out["b_over_a_device_64"] = round(med("trace_device_64") / med("step"), 4)
        out["step_spread_over_median"] = round(out["step"]["spread_ms"] / med("step"), 4)
        for e in EVERY:
            out[f"b_over_a_host_{e}"] = round(med(f"trace_host_{e}") / med("step"), 4)
            out[f"b_over_a_tensor_{e}"] = round(med(f"trace_tensor_{e}") / med("step"), 4)
            out[f"c_over_b_host_{e}"] = round(med(f"loop_{e}") / med(f"trace_host_{e}"), 4)
            out[f"c_over_b_tensor_{e}"] = round(med(f"loop_{e}") / med(f"trace_tensor_{e}"), 4)
        rec["shapes"][f"{h}x{w}"] = out
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
