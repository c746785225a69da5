#!/usr/bin/env python3
"""Per-launch times of the flagship's still steps in a rocprofv3 kernel trace of
`bench.py --gpus 1 --steps N --warmup W` (profiles/r09, r10 trace_launches.json).

A step of 1000 generations at K = 16 is 62 depth-16 launches and a depth-8 remainder;
with the copy pass (life_copy.hip) life_calm_kernel and life_copy_kernel precede
launch 2 and the remainder, and with the probe pass (life_probe.hip)
life_probe_zero_kernel and life_probe_kernel precede launch 1.  Medians over the last `--steps` whole steps of: launch 1
(the still probe), the pass and launch 2 (each, and from the pass's start to the
launch's end),
launch 3 (skips by its lists), launches 4-62 (the one-load exit; duration and pitch),
the remainder likewise, and the step's span.  A short step (DESIGN §4 "Short step")
has three depth-16 launches and life_still_span_kernel in place of the others: its
duration is still_span_us, and launches_per_step counts every kernel of the step.
A fixed step (DESIGN §4 "Fixed step") is life_still_step_kernel alone: a step of one
kernel, whose duration is fixed_step_us and the step's span; fixed_steps counts them
among the steps read.  With pending fixed steps a fixed step may have no
kernel: fixed_launches_in_timed_region counts the kernels behind the last step that was
not fixed, and kernels_per_timed_step divides them by --steps.

    python tools/trace_launches.py TRACE_kernel_trace.csv [--steps 20] [--depth 16]
"""
import argparse
import csv
import json
import re
import statistics


def depth_of(name):
    m = re.search(r"life_tb_kernel(?:<|ILi)(\d+)", name)
    return int(m.group(1)) if m else None


def main():
    p = argparse.ArgumentParser()
    p.add_argument("trace")
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--depth", type=int, default=16)
    a = p.parse_args()
    ev = []
    for r in csv.DictReader(open(a.trace)):
        name = r["Kernel_Name"]
        kind = ("copy" if ("life_copy_kernel" in name or "life_calm_kernel" in name)
                else "probe" if "life_probe_" in name
                else "span" if "life_still_span_kernel" in name
                else "fixed" if "life_still_step_kernel" in name else depth_of(name))
        if kind is not None:
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind))
    ev.sort()
    # a step ends with its remainder launch (a depth below --depth)
    steps, cur = [], []
    for s, e, kind in ev:
        cur.append((s, e, kind))
        if kind == "fixed":  # a step of its own
            steps.append(cur)
            cur = []
            continue
        if kind not in ("copy", "probe", "span") and kind != a.depth:
            steps.append(cur)
            cur = []
    full = [st for st in steps if st[-1][2] == "fixed" or sum(1 for x in st if x[2] == a.depth) >= 4
            or (any(x[2] == "span" for x in st) and sum(1 for x in st if x[2] == a.depth) == 3)][-a.steps:]
    cols = {}

    def add(key, ns):
        cols.setdefault(key, []).append(ns / 1e3)

    for st in full:
        if st[-1][2] == "fixed":
            add("fixed_step_us", st[-1][1] - st[-1][0])
            add("step_span_us", st[-1][1] - st[0][0])
            continue
        deep = [x for x in st if x[2] == a.depth]
        rem = st[-1]
        copies = [x for x in st if x[2] == "copy"]
        add("launch1_us", deep[0][1] - deep[0][0])
        pp = [x for x in st if x[2] == "probe" and x[0] <= deep[0][0]]
        if pp:
            add("probe_pass_us", pp[-1][1] - pp[0][0])
            add("probe_pass_tile_kernel_us", pp[-1][1] - pp[-1][0])
        add("launch1_with_pass_us", deep[0][1] - (pp[0][0] if pp else deep[0][0]))
        add("launch2_us", deep[1][1] - deep[1][0])
        add("launch3_us", deep[2][1] - deep[2][0])
        for x, y in zip(deep[3:], deep[4:]):
            add("launch4_on_us", x[1] - x[0])
            add("launch4_on_pitch_us", y[0] - x[0])
        add("remainder_us", rem[1] - rem[0])
        for x in st:
            if x[2] == "span":
                add("still_span_us", x[1] - x[0])
        p2 = [c for c in copies if deep[0][1] <= c[0] <= deep[1][0]]
        pr = [c for c in copies if deep[-1][1] <= c[0] <= rem[0]]
        if p2:
            add("pass2_us", p2[-1][1] - p2[0][0])
        add("launch2_with_pass_us", deep[1][1] - (p2[0][0] if p2 else deep[1][0]))
        if pr:
            add("pass_remainder_us", pr[-1][1] - pr[0][0])
        add("remainder_with_pass_us", rem[1] - (pr[0][0] if pr else rem[0]))
        add("step_span_us", rem[1] - (pp[0][0] if pp else deep[0][0]))
    out = {"steps": len(full), "fixed_steps": sum(1 for st in full if st[-1][2] == "fixed"),
           "launches_per_step": statistics.median(len(st) for st in full)}
    # Pending fixed steps (DESIGN §4 "Fixed step"): a timed step may have no kernel at
    # all.  The timed region is what follows the last step that was not a fixed one
    # (the warm-up's): its kernels over the --steps steps the caller says it held.
    last_other = max((i for i, st in enumerate(steps) if st[-1][2] != "fixed"), default=-1)
    tail = steps[last_other + 1:]
    out["fixed_launches_in_timed_region"] = len(tail)
    out["kernels_per_timed_step"] = round(sum(len(st) for st in tail) / a.steps, 3)
    out.update({k: round(statistics.median(v), 2) for k, v in cols.items()})
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
