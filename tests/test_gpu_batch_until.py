"""GPU suite: BatchEngine.step_until_periodic (gol_batch_step_until_periodic) -- period,
generation, found, the stored fields, wave_generations and launches of every case,
exactly, against batch_until_ref's plain numpy."""
import collections
import ctypes

import numpy as np
import pytest

import batch_ref
import batch_until_ref
import rule_ref
from test_batch_until_host import CRAFTED, CRAFTED_IDS

pytestmark = pytest.mark.gpu

CONWAY, REF_RULE = rule_ref.CONWAY, rule_ref.REF_RULE


def sem_of(pkg, torus):
    return pkg.SEM_TORUS if torus else pkg.SEM_GLOBAL


def check_result(pkg, b, got, fields, ref, max_g, lag, every, w):
    """One call's results and the batch's fields against the reference's (period,
    generation, final cells)."""
    period, generation, final = ref
    fpw, lg = b.fields_per_wave, b.launch_generations
    assert got.period.dtype == np.uint32 and got.generation.dtype == np.uint64
    assert got.period.tolist() == period.tolist()
    assert got.generation.tolist() == generation.tolist()
    assert got.found == int((period != 0).sum())
    assert (got.lag, got.check_every) == (lag, batch_until_ref.resolve(lag, every))
    bad = np.argwhere((fields != batch_ref.pack(final)).any(axis=(1, 2))).ravel()
    assert bad.size == 0, bad[:8].tolist()
    assert got.wave_generations == batch_until_ref.wave_generations(period, generation, max_g,
                                                                    lag, fpw)
    assert got.launches == batch_until_ref.launches(period, generation, max_g, lag, every, fpw, lg)


def run_case(pkg, cells, rule, torus, max_g, lag, every, ref=None):
    n, h, w = cells.shape
    if ref is None:
        ref = batch_until_ref.until_ref(cells, max_g, lag, every, rule, torus)
    with pkg.BatchEngine(n, h, w, rule=rule, device=0, semantics=sem_of(pkg, torus)) as b:
        b.load_packed(batch_ref.pack(cells))
        got = b.step_until_periodic(max_g, lag, every)
        check_result(pkg, b, got, b.store_packed(), ref, max_g, lag, every, w)
    return got


# (h, w, n, rule, torus, max_g, lag, check_every, p) -> the reference's period histogram
RANDOM_CASES = [
    ((16, 16, 130, CONWAY, False, 192, 2, 64, .5), {0: 6, 1: 90, 2: 34}),
    ((16, 16, 130, CONWAY, True, 192, 4, 64, .5), {0: 26, 1: 69, 2: 35}),
    ((9, 65, 70, CONWAY, False, 203, 6, 8, .4), {0: 3, 1: 33, 2: 26, 3: 2, 6: 6}),
    ((17, 130, 33, CONWAY, True, 320, 12, 16, .08), {0: 6, 1: 3, 2: 24}),
    ((17, 130, 33, CONWAY, False, 320, 12, 16, .12), {0: 5, 2: 22, 6: 6}),
    ((64, 64, 66, CONWAY, False, 512, 2, 0, .08), {0: 10, 1: 3, 2: 53}),
    ((8, 8, 200, CONWAY, True, 256, 32, 32, .35), {0: 12, 1: 176, 2: 7, 32: 5}),
    ((33, 200, 20, CONWAY, True, 300, 30, 0, .06), {0: 9, 1: 1, 2: 10}),
]
_refs = {}


def random_case(case):
    """The case's cells and reference, computed once."""
    if case not in _refs:
        h, w, n, rule, torus, max_g, lag, every, p = case
        cells = batch_ref.random_batch(n, h, w, seed=h * 1000 + w, p=p)
        cells.setflags(write=False)
        _refs[case] = (cells, batch_until_ref.until_ref(cells, max_g, lag, every, rule, torus))
    return _refs[case]


@pytest.mark.parametrize("case,histogram", RANDOM_CASES, ids=[str(i + 1) for i in range(8)])
def test_random_cases_match_reference(pkg, case, histogram):
    h, w, n, rule, torus, max_g, lag, every, p = case
    cells, ref = random_case(case)
    # on the reference alone: the case holds found and unfound fields
    assert (ref[0] != 0).any() and (ref[0] == 0).any()
    assert dict(collections.Counter(ref[0].tolist())) == histogram
    run_case(pkg, cells, rule, torus, max_g, lag, every, ref)


def test_whole_wave_exit(pkg):
    h, w, n, max_g, lag, every = 33, 200, 20, 40, 1, 3
    cells = batch_ref.random_batch(n, h, w, seed=h * 1000 + w, p=.15)
    ref = batch_until_ref.until_ref(cells, max_g, lag, every, REF_RULE, False)
    assert (ref[0] == 1).all() and (ref[1] == 6).all()  # every field found, at generation 6
    got = run_case(pkg, cells, REF_RULE, False, max_g, lag, every, ref)
    assert got.wave_generations == 12 and got.launches == 1 and got.found == n


@pytest.mark.parametrize("torus", [False, True], ids=["dead", "torus"])
def test_64_lanes_per_field(pkg, torus):
    h, w, n = 64, 4096, 2
    cells = np.zeros((n, h, w), dtype=np.uint8)
    cells[0, 10, 63:66] = 1      # a blinker across the seam of words 0 and 1
    cells[0, 40, 4093:4096] = 1  # and one that ends at the last column
    got = run_case(pkg, cells, CONWAY, torus, 10, 2, 4)
    assert got.period.tolist() == [2, 1] and got.generation.tolist() == [4, 4]


@pytest.mark.parametrize("make,torus,max_g,lag,every,period,generation", CRAFTED, ids=CRAFTED_IDS)
def test_crafted_patterns(pkg, make, torus, max_g, lag, every, period, generation):
    got = run_case(pkg, make(), CONWAY, torus, max_g, lag, every)
    assert got.period.tolist() == period and got.generation.tolist() == generation


@pytest.mark.parametrize("cap", [16, 5])
def test_launch_split(pkg, monkeypatch, cap):
    case = RANDOM_CASES[4][0]
    h, w, n, rule, torus, max_g, lag, every, p = case
    cells, ref = random_case(case)
    monkeypatch.delenv("GOL_DEV_BATCH_LAUNCH_GENS", raising=False)
    whole = run_case(pkg, cells, rule, torus, max_g, lag, every, ref)
    assert whole.launches == 1
    monkeypatch.setenv("GOL_DEV_BATCH_LAUNCH_GENS", str(cap))
    with pkg.BatchEngine(n, h, w, rule=rule, device=0, semantics=sem_of(pkg, torus)) as b:
        assert b.launch_generations == cap
    split = run_case(pkg, cells, rule, torus, max_g, lag, every, ref)
    assert split.period.tolist() == whole.period.tolist()
    assert split.generation.tolist() == whole.generation.tolist()
    # an unfound field keeps its wavefront to the end: one interval per launch
    assert split.launches == max_g // every


def test_early_stop(pkg):
    h, w, n, max_g = 16, 16, 130, 2 ** 20
    cells = np.zeros((n, h, w), dtype=np.uint8)
    cells[:, 7:9, 7:9] = 1
    start = batch_ref.pack(cells)
    with pkg.BatchEngine(n, h, w, rule=CONWAY, device=0) as b:
        b.load_packed(start)
        got = b.step_until_periodic(max_g, 1)
        waves = -(-n // b.fields_per_wave)
        assert got.launches == 1 and got.check_every == 64 and got.found == n
        assert (got.generation == 64).all() and (got.period == 1).all()
        assert (b.store_packed() == start).all()
        assert got.wave_generations == waves * 64


def test_composition(pkg):
    h, w, n, lag, every = 9, 65, 70, 6, 8
    cells = batch_ref.random_batch(n, h, w, seed=11, p=.4)
    ref1 = batch_until_ref.until_ref(cells, 100, lag, every, CONWAY, False)
    ref2 = batch_until_ref.until_ref(batch_ref.run(cells, 128, CONWAY), 60, lag, every, CONWAY,
                                     False)
    assert (ref1[0] == 0).any() and (ref2[0] != ref1[0]).any()
    L = pkg.lib()
    with pkg.BatchEngine(n, h, w, rule=CONWAY, device=0) as b:
        b.load_packed(batch_ref.pack(cells))
        first = b.step_until_periodic(100, lag, every)
        check_result(pkg, b, first, b.store_packed(), ref1, 100, lag, every, w)
        b.step(28)
        at128 = b.store_packed()
        assert (at128 == batch_ref.pack(batch_ref.run(cells, 128, CONWAY))).all()
        assert not (at128[:, :, 1] >> np.uint64(1)).any()  # columns >= 65
        # a second call counts from 0 and forgets the first one's results
        second = b.step_until_periodic(60, lag, every)
        check_result(pkg, b, second, b.store_packed(), ref2, 60, lag, every, w)
        # NULL result arrays, and max_generations == 0
        out = pkg.BatchUntil(struct_size=ctypes.sizeof(pkg.BatchUntil))
        assert L.gol_batch_step_until_periodic(b._h, 12, lag, every, None, None,
                                               ctypes.byref(out)) == pkg.GOL_OK
        want = batch_until_ref.until_ref(batch_ref.run(cells, 188, CONWAY), 12, lag, every,
                                         CONWAY, False)
        assert out.found == int((want[0] != 0).sum())
        assert (b.store_packed() == batch_ref.pack(want[2])).all()
        none = b.step_until_periodic(0, lag, every)
        assert not none.period.any() and not none.generation.any()
        assert (none.launches, none.found, none.wave_generations) == (0, 0, 0)
        assert (b.store_packed() == batch_ref.pack(want[2])).all()


@pytest.mark.parametrize("h,w,n", [(8, 8, 130), (17, 130, 33)])
def test_fields_are_isolated(pkg, h, w, n):
    """One glider on a torus in the middle of a wavefront of empty fields, at a lag that
    misses its period: a compare that reads a neighbour's lanes, or a ballot mask off by
    a field, marks the wrong field."""
    mid = pkg.batch_geometry(n, h, w)["fields_per_wave"] // 2
    cells = np.zeros((n, h, w), dtype=np.uint8)
    for r, c in ((0, 1), (1, 2), (2, 0), (2, 1), (2, 2)):
        cells[mid, r + 2, c + w - 4] = 1
    got = run_case(pkg, cells, CONWAY, True, 24, 4, 4)
    want = np.ones(n, dtype=np.uint32)
    want[mid] = 0
    assert got.period.tolist() == want.tolist()
