#!/usr/bin/env python3
"""Time the snapshot slot (snapshot_same / snapshot_diff / step_until_periodic) on a
large field.  One JSON line per case:

  same_equal  snapshot_same() on two equal N x N fields, its worst case: it reads both
              buffers (2 x N * N / 8 bytes) and stores one word.  Yardstick: one
              hipMemcpyAsync device-to-device copy of N * N / 8 bytes in the same
              process, which moves the same bytes (half of them as writes).  The two
              alternate, --repeats times each after a warm-up, host clock around a
              synchronise.  `within_copy`: the comparison's median does not exceed the
              copy's slowest sample.  snapshot_diff() on the same fields and
              snapshot() itself are timed alongside.
  moving      a B3/S23 soup one generation after its snapshot: snapshot_same(), whose
              early exit should make it a small fraction of same_equal, and
              snapshot_diff(), which reads everything.
  until       from a fresh init_random B/S2 field: step_until_periodic(1000, lag 16,
              finish) against step(1000), alternated, wall time each; `advanced` and
              `checks` of the former.
  bench_ab    (with --parent-root, a built checkout of the parent commit) this tree's
              bench.py and the parent's, alternated, --ab-runs each: gol_step is untouched when this
              build's median ms_per_step lies within the parent's own min-max spread
              placed around the parent's median (median -+ spread / 2).

Without --case every case runs in a child process of its own under a time limit, one
after the other, and the first that fails or runs out of time ends the run.

  python tools/snapshot_bench.py --out profiles/r14/snapshot_bench.jsonl
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("same_equal", "moving", "until")


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4)}


class Hip:
    """The few HIP runtime calls the yardstick needs (the runtime libgol.so loaded)."""

    def __init__(self):
        # the copy of the runtime this process already runs on, not a second one
        with open("/proc/self/maps") as f:
            paths = {ln.split()[-1] for ln in f if "libamdhip64.so" in ln}
        if len(paths) != 1:
            raise RuntimeError(f"expected one loaded HIP runtime, found {sorted(paths)}")
        self.rt = ctypes.CDLL(paths.pop(), mode=ctypes.RTLD_GLOBAL)
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        self.rt.hipMalloc.argtypes = [ctypes.POINTER(vp), sz]
        self.rt.hipFree.argtypes = [vp]
        self.rt.hipMemset.argtypes = [vp, ctypes.c_int, sz]
        self.rt.hipMemcpyAsync.argtypes = [vp, vp, sz, ctypes.c_int, vp]
        self.rt.hipDeviceSynchronize.argtypes = []

    def ok(self, st):
        if st != 0:
            raise RuntimeError(f"HIP error {st}")

    def malloc(self, n):
        p = ctypes.c_void_p()
        self.ok(self.rt.hipMalloc(ctypes.byref(p), n))
        self.ok(self.rt.hipMemset(p, 0x5A, n))
        return p

    def copy_d2d(self, dst, src, n):
        self.ok(self.rt.hipMemcpyAsync(dst, src, n, 3, None))  # hipMemcpyDeviceToDevice
        self.ok(self.rt.hipDeviceSynchronize())


def case_same_equal(pkg, n, repeats, streams):
    nbytes = n * ((n + 63) // 64) * 8
    with pkg.Engine(n, n, rule=pkg.CONWAY, device=0, streams=streams) as e:
        hip = Hip()
        src, dst = hip.malloc(nbytes), hip.malloc(nbytes)
        e.init_random(1)
        e.snapshot()
        e.sync()
        for _ in range(3):  # warm-up: code objects, the copy engine's path
            hip.copy_d2d(dst, src, nbytes)
            assert e.snapshot_same() is True and e.snapshot_diff() == 0
        cp, same, diff, snap = [], [], [], []
        for _ in range(repeats):
            cp.append(timed(lambda: hip.copy_d2d(dst, src, nbytes)))
            same.append(timed(e.snapshot_same))
            diff.append(timed(e.snapshot_diff))
            snap.append(timed(lambda: (e.snapshot(), e.sync())))
        hip.ok(hip.rt.hipFree(src))
        hip.ok(hip.rt.hipFree(dst))
        c, s, d = stats(cp), stats(same), stats(diff)
        gb = 2 * nbytes / 1e9
        return {"case": "same_equal", "n": n, "streams": streams, "repeats": repeats,
                "bytes_moved": 2 * nbytes, "copy_d2d": c, "snapshot_same": s,
                "snapshot_diff": d, "snapshot": stats(snap),
                "copy_gb_s": round(gb / (c["median_ms"] / 1e3), 1),
                "same_gb_s": round(gb / (s["median_ms"] / 1e3), 1),
                "diff_gb_s": round(gb / (d["median_ms"] / 1e3), 1),
                "copy_ms": [round(x, 4) for x in cp], "same_ms": [round(x, 4) for x in same],
                "within_copy": s["median_ms"] <= c["max_ms"]}


def case_moving(pkg, n, repeats, streams):
    with pkg.Engine(n, n, rule=pkg.CONWAY, device=0, streams=streams) as e:
        e.init_random(1)
        e.step(32)  # a soup in motion everywhere
        e.snapshot()
        e.step(1)
        e.sync()
        for _ in range(3):
            assert e.snapshot_same() is False
            cells = e.snapshot_diff()
        same, diff = [], []
        for _ in range(repeats):
            same.append(timed(e.snapshot_same))
            diff.append(timed(e.snapshot_diff))
        return {"case": "moving", "n": n, "streams": streams, "repeats": repeats,
                "cells_differing": cells, "snapshot_same": stats(same),
                "snapshot_diff": stats(diff)}


def case_until(pkg, n, repeats, streams):
    reps = max(3, min(repeats, 5))
    with pkg.Engine(n, n, device=0, streams=streams) as e:
        def fresh():
            e.init_random(1)
            e.sync()
        fresh()
        e.step_until_periodic(1000, 16, finish=True)  # warm-up: graphs, the slot
        fresh()
        e.step(1000)
        e.sync()
        until, plain, found = [], [], None
        for _ in range(reps):
            fresh()
            box = []
            until.append(timed(lambda: (box.append(e.step_until_periodic(1000, 16, finish=True)),
                                        e.sync())))
            found = box[0]
            d_until = e.digest()
            fresh()
            plain.append(timed(lambda: (e.step(1000), e.sync())))
            assert e.digest() == d_until  # the field gol_step(1000) leaves
        return {"case": "until", "n": n, "streams": streams, "repeats": reps, "rule": "B/S2",
                "step_until_periodic_1000_lag16_finish": stats(until), "step_1000": stats(plain),
                "advanced": found.advanced, "period": found.period, "checks": found.checks,
                "check_every": found.check_every, "extra_generations": found.extra_generations}


def bench_ab(parent_root, runs, limit):
    """bench.py of the parent's checkout and of this tree, alternated."""
    ms = {"parent": [], "this": []}
    env = dict(os.environ)
    env.pop("GOL_LIB", None)
    for _ in range(runs):
        for name, root in (("parent", os.path.abspath(parent_root)), ("this", ROOT)):
            r = subprocess.run([sys.executable, os.path.join(root, "bench.py")], env=env, cwd=root,
                               capture_output=True, text=True, timeout=limit)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"bench.py ({name}): exit status {r.returncode}; stopping")
            ms[name].append(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"])
    p, t = ms["parent"], ms["this"]
    pm, spread = statistics.median(p), max(p) - min(p)
    return {"case": "bench_ab", "runs": runs, "parent_ms_per_step": p, "this_ms_per_step": t,
            "parent_median": pm, "this_median": statistics.median(t),
            "parent_spread": round(spread, 4),
            "interval": [round(pm - spread / 2, 4), round(pm + spread / 2, 4)],
            "within_parent_spread": abs(statistics.median(t) - pm) <= spread / 2}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--streams", type=int, default=0, help="gol_config.streams (0 = auto)")
    ap.add_argument("--case", choices=CASES, help="run this case in this process")
    ap.add_argument("--limit", type=int, default=240, help="seconds per case / bench.py run")
    ap.add_argument("--parent-root", default=None,
                    help="a built checkout of the parent commit: also bench_ab")
    ap.add_argument("--ab-runs", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if a.case:
        import __graft_entry__ as entry
        pkg = entry.load_package()
        rec = {"same_equal": case_same_equal, "moving": case_moving, "until": case_until}[a.case](
            pkg, a.n, a.repeats, a.streams)
        print(json.dumps(rec), flush=True)
        return 0
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "a") if a.out else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for case in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--n", str(a.n),
               "--repeats", str(a.repeats), "--streams", str(a.streams)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"{case}: no result within {a.limit} s; stopping", file=sys.stderr)
            return 1
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"{case}: exit status {r.returncode}; stopping", file=sys.stderr)
            return 1
        emit(r.stdout.strip().splitlines()[-1])
    if a.parent_root:
        emit(json.dumps(bench_ab(a.parent_root, a.ab_runs, a.limit)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
