"""CPU suite: pending fixed steps (csrc/still_pending.h, DESIGN §4 "Fixed step"), without
a GPU.  A run of fixed steps folded by still_accumulate and applied once must leave a
simulated activity state word for word as the steps' kernels leave it one by one
(still_pending_sweep.cpp), on the real effects of gol_plan_still_step for every kernel
depth and the lengths 5K .. 9K - 1, on synthetic ones with increments near 2^32, and on
start values within one increment of wrapping.
"""
import os
import subprocess

from conftest import ROOT

DEPTHS = (16, 12, 8, 7, 6, 4, 2, 1)  # life_internal.h kDepthList, the shipped library's
FIELDS = ("launches", "computed", "skipped", "copied", "probed", "pass_probed", "elided",
          "busy0_add", "busy1", "streak0", "streak1", "need", "held", "moved", "twin",
          "twin_ok", "kept_passes", "sure_passes")  # gol.h gol_still_effect, in order


def write_effects(pkg, path):
    n = 0
    with open(path, "w") as f:
        for K in DEPTHS:
            for gens in range(5 * K, 9 * K):
                fx = pkg.plan_still_step(K, gens)
                f.write(" ".join(str(fx[k]) for k in FIELDS) + "\n")
                n += 1
    return n


def test_plumbing(pkg):
    assert "gol_activity_fixed_launches" in pkg.EXPORTS
    L = pkg.lib()
    assert L.gol_activity_fixed_launches.argtypes == L.gol_activity_fixed_steps.argtypes
    assert hasattr(pkg.Engine, "activity_fixed_launches")
    assert L.gol_activity_fixed_launches(None, None) != 0


def test_effect_fields_are_the_structs(pkg):
    assert tuple(k for k, _ in pkg.StillEffect._fields_) == FIELDS


def test_a_run_folded_is_the_steps_one_by_one(pkg, tmp_path):
    """still_pending.h compiles without HIP, and the fold equals the steps applied one
    after the other, wrapping and a failed proof included."""
    effects = tmp_path / "effects.txt"
    n = write_effects(pkg, effects)
    assert n == sum(4 * K for K in DEPTHS)
    exe = tmp_path / "sweep"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror",
                    f"-I{ROOT}/mpi-game-of-life_amd/csrc",
                    os.path.join(ROOT, "tests", "still_pending_sweep.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe), str(effects)], capture_output=True, text=True)
    out = r.stdout.split()
    assert r.returncode == 0 and out[0] == "ok", r.stdout[-2000:] + r.stderr[-2000:]
    assert int(out[1]) == 20000 and int(out[2]) > 20000 and int(out[3]) == n
