#!/usr/bin/env python3
"""Time the region I/O (read_rect / write_rect / density) on a large field.

Three cases on an N x N field (default 65536) after init_random, one JSON line each:

  density  density() over the whole field in 256 x 256 blocks against digest() of
           the same engine, which reads the same words and does more arithmetic per
           word.  Median, min and max over --repeats alternating calls, the implied
           GB/s (N * N / 8 bytes read), and `within_spread`: density's median is not
           above the digest's by more than the digest's own max - min.
  rect     read_rect / write_rect of a 1024 x 1024 rectangle at an unaligned offset
           against store_packed / load_packed of the whole field.
  skip     B/S2 until the field is still, one XOR of a 2 x 2 block into an empty
           spot, step(1000): activity() before and after, to show that the skip
           takes over again once the edit has died down (single stream, classic
           blocks: the plans that skip).

digest, store_packed and load_packed are the library's whole-field calls, so their
times are also what a build without the region I/O gives.

Without --case every case runs in a child process of its own under a time limit,
one after the other, and the first that fails or runs out of time ends the run.

  python tools/rect_bench.py --out profiles/rect/bench.jsonl
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("density", "rect", "skip")


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4)}


def case_density(pkg, n, repeats, streams):
    with pkg.Engine(n, n, rule=pkg.CONWAY, device=0, streams=streams) as e:
        e.init_random(1)
        e.sync()
        for _ in range(3):  # warm-up: code objects, the staging buffer
            e.digest()
            counts = e.density(0, 0, n, n, 256, 256)
        assert int(counts.sum(dtype="uint64")) == e.digest()[0]
        dig, den = [], []
        for _ in range(repeats):
            dig.append(timed(e.digest))
            den.append(timed(lambda: e.density(0, 0, n, n, 256, 256)))
        d, c = stats(dig), stats(den)
        gb = n * n / 8 / 1e9
        return {"case": "density", "n": n, "streams": streams, "block": [256, 256],
                "repeats": repeats, "digest": d, "density": c,
                "digest_gb_s": round(gb / (d["median_ms"] / 1e3), 1),
                "density_gb_s": round(gb / (c["median_ms"] / 1e3), 1),
                "digest_spread_ms": round(d["max_ms"] - d["min_ms"], 4),
                "within_spread": c["median_ms"] - d["median_ms"] <= d["max_ms"] - d["min_ms"]}


def case_rect(pkg, n, repeats, streams):
    import numpy as np
    y, x, side = 12345 % max(1, n - 1024), 4321 % max(1, n - 1024), min(1024, n)
    with pkg.Engine(n, n, rule=pkg.CONWAY, device=0, streams=streams) as e:
        e.init_random(1)
        e.sync()
        win = e.read_rect(y, x, side, side)
        e.write_rect(y, x, win, side, pkg.RECT_XOR)
        e.write_rect(y, x, win, side, pkg.RECT_XOR)
        rd = [timed(lambda: e.read_rect(y, x, side, side)) for _ in range(repeats)]
        wr = [timed(lambda: e.write_rect(y, x, win, side, pkg.RECT_SET)) for _ in range(repeats)]
        whole = []
        st = [timed(lambda: whole.append(e.store_packed())) for _ in range(3)]
        field = whole[-1]
        del whole
        crop = np.zeros_like(win)
        pkg.rect_blit(field[y:y + side], x, crop, 0, side, side)
        assert (crop == win).all()
        ld = [timed(lambda: e.load_packed(field)) for _ in range(3)]
        return {"case": "rect", "n": n, "streams": streams, "rect": [y, x, side, side],
                "rect_bytes": int(win.nbytes), "field_bytes": int(field.nbytes),
                "read_rect": stats(rd), "write_rect": stats(wr), "store_packed": stats(st),
                "load_packed": stats(ld)}


def case_skip(pkg, n, repeats, streams):
    import numpy as np
    with pkg.Engine(n, n, device=0, streams=1, resident=1, handoff=1) as e:
        e.init_random(1)
        e.step(64)  # B/S2 from p = 0.5 is still within a dozen generations
        e.sync()
        e.reset_timing()
        t_still = timed(lambda: (e.step(1000), e.sync()))
        still = e.activity()
        # an empty 4 x 4 spot: the 2 x 2 block in its middle has no other neighbour
        y0, x0 = n // 2, n // 2 + 1
        win = e.read_rect(y0, x0, 64, 64)
        bits = np.unpackbits(win.view(np.uint8).reshape(64, 8), axis=1, bitorder="little")
        spot = next((i, j) for i in range(60) for j in range(60) if not bits[i:i + 4, j:j + 4].any())
        live0 = e.digest()[0]
        e.reset_timing()
        e.write_rect(y0 + spot[0] + 1, x0 + spot[1] + 1, np.array([[3], [3]], dtype=np.uint64), 2,
                     pkg.RECT_XOR)
        assert e.digest()[0] == live0 + 4
        t_edit = timed(lambda: (e.step(1000), e.sync()))
        after = e.activity()
        assert e.digest()[0] == live0  # the block's cells have 3 neighbours each: they die
        return {"case": "skip", "n": n, "tb_depth": e.tb_depth,
                "still_step1000": {"ms": round(t_still, 3), "computed": still[0], "skipped": still[1]},
                "edited_step1000": {"ms": round(t_edit, 3), "computed": after[0],
                                    "skipped": after[1]}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--streams", type=int, default=0, help="gol_config.streams (0 = auto)")
    ap.add_argument("--case", choices=CASES, help="run this case in this process")
    ap.add_argument("--limit", type=int, default=240, help="seconds per case")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if a.case:
        import __graft_entry__ as entry
        pkg = entry.load_package()
        rec = {"density": case_density, "rect": case_rect, "skip": case_skip}[a.case](
            pkg, a.n, a.repeats, a.streams)
        print(json.dumps(rec), flush=True)
        return 0
    out = open(a.out, "a") if a.out else None
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
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
