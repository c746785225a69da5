"""CPU suite: gol_plan_still_step, what a step on a proven fixed point does to the
activity state (step.cpp still_effect, a fold over the step's schedule of step_plan.h;
DESIGN §4 "Fixed step"), without a GPU; and that schedule against a counter-driven walk
(step_plan_sweep.cpp).

The pins are those of tests/test_gpu_short_step.py::test_still_field, which the engine
with every kernel in place produces on the GPU: per unit, in the order computed,
skipped, copied, probed, elided, pass_probed, with one kept and one sure probe pass
per step.  `skipped` there sums the units' own skips and the launches that every unit
left at the one-load exit (busy[0], once per unit), as gol_activity does.
"""
import os
import subprocess

import pytest

from conftest import ROOT

DEPTHS = (16, 12, 8, 7, 6, 4, 2, 1)  # life_internal.h kDepthList, the shipped library's


def pick_depth(K, left):
    """step_plan.h pick_depth: the largest kernel depth that fits K and what is left."""
    for d in DEPTHS:
        if d <= K and d <= left:
            return d
    return 1


def launches(K, gens):
    """The schedule's depths (step_plan.h StepSchedule): those of the step's launches."""
    out, left = [], gens
    while left > 0:
        d = pick_depth(K, left)
        out.append(d)
        left -= d
    return out


def six(fx):
    return (fx["computed"], fx["skipped"] + fx["busy0_add"], fx["copied"], fx["probed"],
            fx["elided"], fx["pass_probed"])


def test_plumbing(pkg):
    for name in ("gol_plan_still_step", "gol_activity_fixed_steps", "gol_activity_state"):
        assert name in pkg.EXPORTS
    L = pkg.lib()
    assert L.gol_activity_fixed_steps.argtypes == L.gol_activity_short_steps.argtypes
    assert hasattr(pkg.Engine, "activity_fixed_steps") and hasattr(pkg.Engine, "activity_state")
    assert L.gol_activity_fixed_steps(None, None) != 0
    assert L.gol_activity_state(None, None, 0, None) != 0
    assert L.gol_plan_still_step(16, 104, None) != 0


@pytest.mark.parametrize("gens,pin", [(6 * 16 + 8, (3, 4, 2, 1, 2, 1)),
                                      (7 * 16 + 3, (4, 5, 3, 1, 3, 1))])
def test_pins_of_the_short_step_test(pkg, gens, pin):
    fx = pkg.plan_still_step(16, gens)
    assert six(fx) == pin
    assert (fx["kept_passes"], fx["sure_passes"]) == (1, 1)


@pytest.mark.parametrize("K,gens", [(16, 6 * 16 + 8), (16, 7 * 16 + 3), (16, 5 * 16 + 1),
                                    (16, 62 * 16 + 8), (16, 6 * 16), (16, 5 * 16),
                                    (16, 5 * 16 + 15), (8, 6 * 8 + 3), (8, 9 * 8),
                                    (12, 5 * 12 + 11), (12, 7 * 12)])
def test_against_the_launch_loop(pkg, K, gens):
    fx = pkg.plan_still_step(K, gens)
    ls = launches(K, gens)
    nK = gens // K
    rem = [d for d in ls if d != K]
    assert ls[:nK] == [K] * nK and len(rem) == len(ls) - nK
    assert fx["launches"] == len(ls)
    # launches 4 .. nK leave at the one-load exit; launch 3 skips unit by unit
    assert fx["busy0_add"] == nK - 3 and fx["skipped"] == 1
    # launches 1 and 2 and every remainder launch store or copy
    assert fx["computed"] == 2 + len(rem)
    assert fx["copied"] == 1 + len(rem) and fx["elided"] == 1 + len(rem)
    assert fx["probed"] == 1 and fx["pass_probed"] == 1
    # final values: none depends on the step's length but twin
    assert (fx["busy1"], fx["streak0"], fx["streak1"]) == (2, 2, 3)
    assert (fx["need"], fx["held"], fx["moved"], fx["twin_ok"]) == (0, 1, 0, 1)
    assert fx["twin"] == (2 if rem else 1)
    assert (fx["kept_passes"], fx["sure_passes"]) == (1, 1)


def test_the_benchmark_step(pkg):
    """step(1000) at K = 16: 62 depth-K launches and one of depth 8."""
    fx = pkg.plan_still_step(16, 1000)
    assert launches(16, 1000) == [16] * 62 + [8]
    assert fx["launches"] == 63 and fx["busy0_add"] == 59 and fx["twin"] == 2


@pytest.mark.parametrize("K,gens", [(16, 4 * 16 + 8), (16, 16), (16, 3), (8, 39), (0, 100),
                                    (3, 100), (5, 100), (20, 200)])
def test_not_a_short_step(pkg, K, gens):
    """Fewer than 5 depth-K launches, or a depth without a kernel."""
    with pytest.raises(pkg.GolError) as err:
        pkg.plan_still_step(K, gens)
    assert err.value.status == pkg.GOL_EINVAL


def test_a_very_long_step_is_computed_in_closed_form(pkg):
    fx = pkg.plan_still_step(16, 16 * (2 ** 32 + 2) + 5)
    assert fx["busy0_add"] == 2 ** 32 - 1 and fx["launches"] == 2 ** 32 + 2 + 2
    with pytest.raises(pkg.GolError):
        pkg.plan_still_step(16, 16 * (2 ** 32 + 3))


def test_schedule_against_the_counter_walk(tmp_path):
    """step_plan.h compiles without HIP, and for every kernel depth, step length up to
    9K - 1 and combination of switches its records are those of step_plan_sweep.cpp's
    walk."""
    exe = tmp_path / "sweep"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror",
                    f"-I{ROOT}/mpi-game-of-life_amd/csrc",
                    os.path.join(ROOT, "tests", "step_plan_sweep.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    out = r.stdout.split()
    assert r.returncode == 0 and out[0] == "ok" and int(out[1]) > 100000, r.stdout[-2000:]
