"""CPU suite: the population-trace reference (batch_trace_ref.py) against the
single-field references, the conditions the GPU cases rest on, and
gol_batch_step_trace's host-only side: the launch plan and the argument checks that never
touch a GPU."""
import ctypes

import numpy as np
import pytest

import batch_ref
import batch_rules_ref
import batch_trace_ref
import rule_ref
import torus_ref
from batch_trace_ref import CASES, CASE_IDS

EVERY = (1, 3, 64, 4096, 4097, 65536)
CAPS = (1, 7, 4096)


def generations_of(every):
    return sorted({0, 1, every - 1, every, every + 1, 5 * every + 2, 4096, 4097, 64 * every,
                   64 * every + every - 1, 2 ** 40 + 5})


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("every", EVERY)
def test_plan_matches_restatement(pkg, every, cap):
    for g in generations_of(every):
        got = pkg.batch_trace_plan(g, every, cap)
        assert got == batch_trace_ref.plan(g, every, cap), (g, every, cap)
        # the plan's launches cover every sample once and run the tail in the last
        spl, samples = got["samples_per_launch"], got["samples"]
        assert samples * every + got["tail"] == g and got["tail"] < every
        assert (got["launches"] == 0) == (g == 0)
        if g > 0:
            assert (got["launches"] - 1) * spl < max(samples, 1) <= got["launches"] * spl


# (generations, every, cap) -> samples, tail, samples_per_launch, launches
PLANS = {
    (1024, 1, 4096): (1024, 0, 4096, 1),
    (1024, 16, 4096): (64, 0, 256, 1),
    (8192, 1, 4096): (8192, 0, 4096, 2),
    (8193, 2, 4096): (4096, 1, 2048, 2),
    (50, 3, 1): (16, 2, 1, 16),      # a cap below `every`: one interval per launch
    (50, 3, 3): (16, 2, 1, 16),
    (50, 3, 7): (16, 2, 2, 8),
    (45, 7, 15): (6, 3, 2, 3),
    (2, 3, 4096): (0, 2, 1365, 1),   # generations < every: the tail alone, one launch
    (0, 3, 4096): (0, 0, 1365, 0),
    (10, 1, 0): (10, 0, 1, 10),
}


@pytest.mark.parametrize("case", sorted(PLANS))
def test_plan_counts_written_out(pkg, case):
    p = pkg.batch_trace_plan(*case)
    assert (p["samples"], p["tail"], p["samples_per_launch"], p["launches"]) == PLANS[case]


def einval(pkg, status):
    assert status == pkg.GOL_EINVAL
    msg = pkg.lib().gol_last_error().decode()
    assert msg
    return msg


@pytest.mark.parametrize("every", [0, 65537, 2 ** 31, 2 ** 32 - 1])
def test_plan_and_call_reject_bad_every(pkg, every):
    L = pkg.lib()
    plan = pkg.BatchTracePlan()
    m1 = einval(pkg, L.gol_batch_trace_plan_of(100, every, 4096, ctypes.byref(plan)))
    assert "every" in m1
    with pytest.raises(pkg.GolError) as ei:
        pkg.batch_trace_plan(100, every)
    assert ei.value.status == pkg.GOL_EINVAL


def test_plan_rejects_null_out(pkg):
    assert "out" in einval(pkg, pkg.lib().gol_batch_trace_plan_of(100, 1, 4096, None))


def test_call_rejects_null_batch_null_out_and_struct_size(pkg):
    """(the checks that need a batch are in test_gpu_batch_trace.py)"""
    L = pkg.lib()
    assert ctypes.sizeof(pkg.BatchTrace) == 24 and ctypes.sizeof(pkg.BatchTracePlan) == 24
    buf = np.zeros(4, dtype=np.uint32)
    for fn in (L.gol_batch_step_trace, L.gol_batch_step_trace_device):
        out = pkg.BatchTrace(struct_size=ctypes.sizeof(pkg.BatchTrace))
        assert "batch" in einval(pkg, fn(None, 10, 1, buf.ctypes.data, 4, ctypes.byref(out)))
        assert "batch" in einval(pkg, fn(None, 10, 1, buf.ctypes.data, 4, None))


@pytest.mark.parametrize("torus", [False, True], ids=["dead", "torus"])
def test_reference_column_is_the_single_field_population(torus):
    n, h, w, gens, every = 5, 9, 13, 14, 3
    cells = batch_ref.random_batch(n, h, w, seed=31, p=.4)
    birth, survive = batch_rules_ref.random_rules(n, seed=5)

    def alone(bits, g, rule):
        if torus:
            return torus_ref.unpack(torus_ref.roll_run(torus_ref.pack(bits), w, g, rule), w)
        return rule_ref.numpy_run(bits, g, rule)

    for rules, rule_of in (((birth, survive), lambda i: (int(birth[i]), int(survive[i]))),
                           (rule_ref.CONWAY, lambda i: rule_ref.CONWAY)):
        live, final = batch_trace_ref.trace_ref(cells, gens, every, rules, torus)
        assert live.dtype == np.uint32 and live.shape == (gens // every, n)
        for i in range(n):
            pops = [int(alone(cells[i], g, rule_of(i)).sum()) for g in range(1, gens + 1)]
            assert live[:, i].tolist() == pops[every - 1::every][:gens // every]
            assert (final[i] == alone(cells[i], gens, rule_of(i))).all()


def test_reference_edge_shapes():
    cells = batch_ref.random_batch(3, 8, 8, seed=1)
    live, final = batch_trace_ref.trace_ref(cells, 2, 3, rule_ref.CONWAY)
    assert live.shape == (0, 3) and (final == batch_ref.run(cells, 2, rule_ref.CONWAY)).all()
    live, final = batch_trace_ref.trace_ref(cells, 0, 1, rule_ref.CONWAY)
    assert live.shape == (0, 3) and (final == cells).all()
    live, final = batch_trace_ref.trace_ref(cells, 2, 1, batch_trace_ref.STILL)
    assert (live == cells.sum(axis=(1, 2))[None, :]).all() and (final == cells).all()


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_case_conditions(i):
    """What the GPU cases rest on, on the reference alone: no field's trace is constant and
    no two fields' traces are equal, so a constant or repeated sample cannot pass."""
    h, w, n, rule, torus, gens, every, p = CASES[i]
    cells, live, final = batch_trace_ref.case(i)
    assert live.shape == (gens // every, n)
    assert min(len(set(live[:, f].tolist())) for f in range(n)) >= 2
    assert len({tuple(live[:, f].tolist()) for f in range(n)}) == n
    assert int(live.max()) <= h * w


def test_cases_cover_the_geometries(pkg):
    geo = [pkg.batch_geometry(n, h, w) for h, w, n, *_ in CASES]
    assert {g["rows_in_regs"] for g in geo} == {8, 16, 32, 64}
    assert {g["lanes_per_field"] for g in geo} >= {1, 2, 4, 64}
    # padding lanes (ceil(w/64) below lanes_per_field) and partly filled last wavefronts
    assert any((c[1] + 63) // 64 < g["lanes_per_field"] for c, g in zip(CASES, geo))
    assert any(c[2] % g["fields_per_wave"] for c, g in zip(CASES, geo))
    assert any(c[5] % c[6] for c in CASES)  # a tail
    assert {c[4] for c in CASES} == {False, True}
    assert {c[3] for c in CASES} == {rule_ref.REF_RULE, rule_ref.CONWAY, batch_trace_ref.B36S23}
    assert max(int(batch_trace_ref.case(i)[1].max()) for i in range(len(CASES))) == 75425


def test_lane_sum_pattern():
    for wq, n in ((1, 3), (3, 5), (33, 3), (64, 3)):
        cells = batch_trace_ref.lane_sum_cells(wq, n)
        per_word = cells.reshape(n, 8, wq, 64).sum(axis=(1, 3))
        want = 1 + (np.arange(wq)[None, :] + 3 * np.arange(n)[:, None]) % 8
        assert (per_word == want).all()
        # neighbouring lanes and neighbouring fields differ
        assert wq == 1 or (per_word[:, 1:] != per_word[:, :-1]).all()
        assert (per_word[1:] != per_word[:-1]).all()
    planes = batch_trace_ref.lane_sum_cells(3, 5).any(axis=(0, 1))
    assert planes[0::2].any() and planes[1::2].any()
