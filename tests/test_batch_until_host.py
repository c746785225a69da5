"""CPU suite: the period-detection reference (batch_until_ref.py) on crafted patterns
with the expected values written out, and gol_batch_step_until_periodic's host-only
side: the launch plan and the argument checks, which never touch a GPU."""
import ctypes

import numpy as np
import pytest

import batch_until_ref
import rule_ref

GLIDER = [(0, 1), (1, 2), (2, 0), (2, 1), (2, 2)]


def crafted_8x8():
    """glider, blinker, block, empty: 8 x 8 each."""
    cells = np.zeros((4, 8, 8), dtype=np.uint8)
    for r, c in GLIDER:
        cells[0, r + 1, c + 1] = 1
    cells[1, 3, 2:5] = 1
    cells[2, 3:5, 3:5] = 1
    return cells


def pentadecathlon():
    """A row of ten cells, a phase of the period-15 pentadecathlon, with the room its
    other phases need on 18 x 18."""
    cells = np.zeros((1, 18, 18), dtype=np.uint8)
    cells[0, 9, 4:14] = 1
    return cells


# (cells, torus, max_g, lag, check_every, period, generation)
CRAFTED = [
    (crafted_8x8, True, 200, 64, 64, [32, 2, 1, 1], [64, 64, 64, 64]),
    (crafted_8x8, True, 200, 16, 16, [0, 2, 1, 1], [200, 16, 16, 16]),
    (crafted_8x8, True, 200, 2, 5, [0, 2, 1, 1], [200, 5, 5, 5]),
    (pentadecathlon, False, 200, 30, 0, [15], [64]),
    (pentadecathlon, False, 200, 15, 20, [15], [20]),
    (pentadecathlon, False, 200, 5, 5, [0], [200]),
]
CRAFTED_IDS = ["8x8-lag64", "8x8-lag16", "8x8-lag2-every5", "pd-lag30", "pd-lag15", "pd-lag5"]


@pytest.mark.parametrize("make,torus,max_g,lag,every,period,generation", CRAFTED, ids=CRAFTED_IDS)
def test_reference_on_crafted_patterns(make, torus, max_g, lag, every, period, generation):
    cells = make()
    p, g, final = batch_until_ref.until_ref(cells, max_g, lag, every, rule_ref.CONWAY, torus)
    assert p.dtype == np.uint32 and g.dtype == np.uint64
    assert p.tolist() == period and g.tolist() == generation
    import batch_ref
    assert (final == batch_ref.run(cells, max_g, rule_ref.CONWAY, torus)).all()


def test_reference_counters_written_out():
    ref = batch_until_ref
    period = np.array([1, 2, 1, 0, 3, 3], dtype=np.uint32)
    generation = np.array([64, 128, 64, 1000, 192, 64], dtype=np.uint64)
    # waves of 2 fields: {64, 128} found at 128, {64, unfound}, {192, 64} found at 192
    assert ref.wave_exits(period, generation, 2) == [128, None, 192]
    # lag 6: 128 + (1000 - 128) % 6 = 130, 1000, 192 + (1000 - 192) % 6 = 196
    assert ref.wave_generations(period, generation, 1000, 6, 2) == 130 + 1000 + 196
    assert ref.launches(period, generation, 1000, 6, 64, 2, launch_generations=128) == 8
    found = period.copy()
    found[3] = 1
    generation[3] = 320
    # every wave has left by generation 320: launches of 128 generations -> 3 of the 8
    assert ref.launches(found, generation, 1000, 6, 64, 2, launch_generations=128) == 3
    assert ref.launches(found, generation, 1000, 6, 64, 2) == 1
    assert ref.wave_generations(found[:2], generation[:2], 128, 6, 2) == 128


@pytest.mark.parametrize("lag,every,want", [(1, 0, 64), (64, 0, 64), (65, 0, 128), (30, 0, 64),
                                            (1024, 0, 1024), (1000, 0, 1024), (30, 30, 30),
                                            (30, 100, 100), (7, 65536, 65536)])
def test_plan_resolves_check_every(pkg, lag, every, want):
    assert pkg.batch_until_plan(1000, lag, every)["check_every"] == want
    assert batch_until_ref.resolve(lag, every) == want


DIVISORS = {1: [], 2: [1], 12: [1, 2, 3, 4, 6], 30: [1, 2, 3, 5, 6, 10, 15],
            1024: [1, 2, 4, 8, 16, 32, 64, 128, 256, 512]}


@pytest.mark.parametrize("lag", sorted(DIVISORS) + [840])
def test_plan_lists_proper_divisors(pkg, lag):
    got = pkg.batch_until_plan(5000, lag)["divisors"]
    assert got == [d for d in range(1, lag) if lag % d == 0]
    if lag == 840:
        assert len(got) == 31 and got[-1] == 420
    else:
        assert got == DIVISORS[lag]


# (max_g, lag, every, launch_generations) -> checks, tail, checks_per_launch, launches
PLANS = {
    (1000, 2, 64, 4096): (15, 40, 64, 1),
    (16384, 6, 0, 4096): (256, 0, 64, 4),
    (16385, 6, 0, 4096): (256, 1, 64, 4),
    (16448, 6, 0, 4096): (257, 0, 64, 5),
    (320, 12, 16, 16): (20, 0, 1, 20),
    (320, 12, 16, 5): (20, 0, 1, 20),      # a cap below check_every: one interval per launch
    (320, 12, 16, 40): (20, 0, 2, 10),
    (330, 12, 16, 48): (20, 10, 3, 7),
    (10, 2, 64, 4096): (0, 10, 64, 1),     # max_generations < check_every: the tail alone
    (0, 2, 64, 4096): (0, 0, 64, 0),
    (2 ** 40, 1, 0, 4096): (2 ** 34, 0, 64, 2 ** 28),
}


@pytest.mark.parametrize("case", sorted(PLANS))
def test_plan_counts(pkg, case):
    max_g, lag, every, lg = case
    p = pkg.batch_until_plan(max_g, lag, every, lg)
    assert (p["checks"], p["tail"], p["checks_per_launch"], p["launches"]) == PLANS[case]
    assert p == batch_until_ref.plan(max_g, lag, every, lg)


def einval(pkg, status):
    assert status == pkg.GOL_EINVAL
    msg = pkg.lib().gol_last_error().decode()
    assert msg
    return msg


BAD_ARGS = [(0, 0), (1025, 0), (2 ** 31, 0), (30, 29), (30, 1), (1024, 1023), (2, 65537),
            (1024, 2 ** 31)]


@pytest.mark.parametrize("lag,every", BAD_ARGS)
def test_plan_and_call_reject_bad_lag_and_check_every(pkg, lag, every):
    L = pkg.lib()
    plan = pkg.BatchUntilPlan()
    m1 = einval(pkg, L.gol_batch_until_plan_of(100, lag, every, 4096, ctypes.byref(plan)))
    with pytest.raises(pkg.GolError) as ei:
        pkg.batch_until_plan(100, lag, every)
    assert ei.value.status == pkg.GOL_EINVAL
    # the call itself checks them before it looks at the batch
    out = pkg.BatchUntil(struct_size=ctypes.sizeof(pkg.BatchUntil))
    m2 = einval(pkg, L.gol_batch_step_until_periodic(None, 100, lag, every, None, None,
                                                     ctypes.byref(out)))
    assert m1 == m2


def test_call_rejects_null_batch_null_out_and_struct_size(pkg):
    L = pkg.lib()
    out = pkg.BatchUntil(struct_size=ctypes.sizeof(pkg.BatchUntil))
    assert ctypes.sizeof(pkg.BatchUntil) == 40
    assert "batch" in einval(pkg, L.gol_batch_step_until_periodic(None, 100, 2, 0, None, None,
                                                                  ctypes.byref(out)))
    assert "out" in einval(pkg, L.gol_batch_step_until_periodic(None, 100, 2, 0, None, None, None))
    for size in (0, 39, 41):
        bad = pkg.BatchUntil(struct_size=size)
        assert "struct_size" in einval(pkg, L.gol_batch_step_until_periodic(
            None, 100, 2, 0, None, None, ctypes.byref(bad)))
    assert "out" in einval(pkg, L.gol_batch_until_plan_of(100, 2, 0, 4096, None))
