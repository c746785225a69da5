"""GPU: Engine.step_until_periodic (gol_step_until_periodic).

The expected generation g, period p, extra generations and field come from the CPU
oracle (torus_ref for tori) run by the documented schedule -- checks at c * check_every,
generation g - lag against generation g, then the walk over lag's proper divisors --
never from the engine.  The (g, p) each case names were found with the oracle on the
CPU; expected() recomputes them in the test, so a case that drifts shows as such.
"""
import numpy as np
import pytest

import torus_ref

pytestmark = pytest.mark.gpu

CONWAY = (1 << 3, (1 << 2) | (1 << 3))
REF = (0, 1 << 2)
STREAMING = dict(tb_depth=8, resident=1)
GLIDER = np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]], dtype=np.uint8)


def expected(run, start, lag, every, max_gens):
    """(g, p, field at g, extra generations, checks) by the schedule of gol.h;
    run(field, n) advances a field n generations."""
    g, field, checks = 0, start, 0
    while g + every <= max_gens:
        before = run(field, every - lag)
        field = run(before, lag)
        g += every
        checks += 1
        if not (before == field).all():
            continue
        p, at, cur = lag, 0, field
        for d in (d for d in range(1, lag) if lag % d == 0):
            cur = run(cur, d - at)
            at = d
            if (cur == field).all():
                p = d
                break
        return g, p, field, at, checks
    return max_gens, 0, run(field, max_gens - g), 0, checks


def dead_border(oracle, w, rule):
    return lambda f, n: oracle.bp_run(f, w, n, rule) if n else f


def torus(oracle, w, rule):
    return lambda f, n: torus_ref.torus_run(oracle, f, w, n, rule) if n else f


def check(e, r, want, lag, every):
    g, p, field, extra, checks = want
    assert (r.advanced, r.period) == (g, p), r
    assert (r.lag, r.check_every, r.checks, r.extra_generations) == (lag, every, checks, extra), r
    assert (e.store_packed() == field).all()


# h, w, seed, lag, check_every, max_generations, g, p
CONWAY_CASES = [
    (100, 90, 6, 6, 64, 4096, 576, 6),
    (100, 90, 1, 6, 64, 4096, 576, 2),
    (100, 90, 1, 30, 64, 4096, 640, 2),
    (96, 96, 4, 30, 64, 4096, 576, 6),
]


@pytest.mark.parametrize("kw", [dict(), STREAMING], ids=["default", "streaming"])
@pytest.mark.parametrize("case", CONWAY_CASES, ids=lambda c: "%dx%d-s%d-lag%d" % c[:4])
def test_dead_border(pkg, oracle, case, kw):
    h, w, seed, lag, every, max_gens, g, p = case
    start = oracle.bp_random(h, w, seed)
    want = expected(dead_border(oracle, w, CONWAY), start, lag, every, max_gens)
    assert want[:2] == (g, p)
    with pkg.Engine(h, w, rule=CONWAY, device=0, **kw) as e:
        e.load_packed(start)
        r = e.step_until_periodic(max_gens, lag, every)
        # (the field at g: also the restore after the divisor walk)
        check(e, r, want, lag, every)
        # the slot holds generation g - lag's field, which is generation g's
        assert e.snapshot_same() is True


@pytest.mark.parametrize("kw", [dict(), STREAMING], ids=["default", "streaming"])
def test_no_period_within_the_limit(pkg, oracle, kw):
    h, w, lag, every, max_gens = 100, 90, 6, 64, 500  # (500 = 7 x 64 + 52: a tail step)
    start = oracle.bp_random(h, w, 1)
    want = expected(dead_border(oracle, w, CONWAY), start, lag, every, max_gens)
    assert want[:2] == (500, 0) and want[4] == 7
    with pkg.Engine(h, w, rule=CONWAY, device=0, **kw) as e:
        e.load_packed(start)
        for finish in (False, True):
            r = e.step_until_periodic(max_gens, lag, every, finish=finish)
            check(e, r, want, lag, every)
            e.load_packed(start)


@pytest.mark.parametrize("kw", [dict(), STREAMING], ids=["default", "streaming"])
def test_finish(pkg, oracle, kw):
    h, w, lag, every, max_gens = 100, 90, 6, 64, 4099
    start = oracle.bp_random(h, w, 6)
    with pkg.Engine(h, w, rule=CONWAY, device=0, **kw) as e:
        e.load_packed(start)
        r = e.step_until_periodic(max_gens, lag, every, finish=True)
        assert (r.advanced, r.period) == (576, 6)
        assert (4099 - 576) % 6  # (a residue is run)
        assert (e.store_packed() == oracle.bp_run(start, w, max_gens, CONWAY)).all()


@pytest.mark.parametrize("seed,g", [(1, 4), (2, 4), (3, 8)])
def test_reference_rule(pkg, oracle, seed, g):
    h, w = 100, 90
    start = oracle.bp_random(h, w, seed)
    want = expected(dead_border(oracle, w, REF), start, 1, 4, 200)
    assert want[:2] == (g, 1)
    assert want[2].any() == (seed != 3)  # (seed 3 ends empty)
    with pkg.Engine(h, w, rule=REF, device=0) as e:
        e.load_packed(start)
        check(e, e.step_until_periodic(200, 1, 4), want, 1, 4)
        if seed == 1:  # check_every = 0: the least multiple of 64 >= lag
            e.load_packed(start)
            r = e.step_until_periodic(200, 1)
            assert (r.check_every, r.advanced, r.period, r.checks) == (64, 64, 1, 1)
            assert (e.store_packed() == want[2]).all()


def glider_field(h, w):
    bits = np.zeros((h, w), dtype=np.uint8)
    bits[1:4, 1:4] = GLIDER
    return torus_ref.pack(bits)


@pytest.mark.parametrize("h,w,lag,extra", [(8, 8, 32, 16), (12, 20, 240, 120)])
def test_torus_glider(pkg, h, w, lag, extra):
    start = glider_field(h, w)
    with pkg.Engine(h, w, rule=CONWAY, device=0, semantics=pkg.SEM_TORUS) as e:
        e.load_packed(start)
        r = e.step_until_periodic(10 * lag, lag, lag)
        assert (r.advanced, r.period, r.checks) == (lag, lag, 1), r
        assert r.extra_generations == extra
        back = torus_ref.roll_run(start, w, lag, CONWAY)
        assert (back == start).all()  # (the glider's period on this torus)
        assert (e.store_packed() == back).all()


@pytest.mark.parametrize("kw", [dict(), STREAMING], ids=["torus", "torus_streaming"])
def test_torus_random(pkg, oracle, kw):
    h, w, lag, every = 40, 72, 6, 64
    start = oracle.bp_random(h, w, 2)
    want = expected(torus(oracle, w, CONWAY), start, lag, every, 4096)
    assert want[:2] == (320, 2)
    with pkg.Engine(h, w, rule=CONWAY, device=0, semantics=pkg.SEM_TORUS, **kw) as e:
        e.load_packed(start)
        check(e, e.step_until_periodic(4096, lag, every), want, lag, every)


PULSAR_ROWS = ["0011100011100", "0000000000000", "1000010100001", "1000010100001",
               "1000010100001", "0011100011100", "0000000000000", "0011100011100",
               "1000010100001", "1000010100001", "1000010100001", "0000000000000",
               "0011100011100"]


@pytest.mark.parametrize("lag,extra", [(6, 3), (12, 6)])
def test_composite(pkg, oracle, lag, extra):
    h, w, every = 1500, 500, 16
    b = pkg.rank_rows(h, 2, 1)[0]  # first row of the second stripe
    bits = np.zeros((h, w), dtype=np.uint8)
    bits[b - 1:b + 2, 100] = 1  # a blinker across the stripe boundary
    bits[b - 40:b - 27, 200:213] = np.array([[int(c) for c in r] for r in PULSAR_ROWS], dtype=np.uint8)
    bits[b + 20:b + 22, 300:302] = 1  # a block
    start = torus_ref.pack(bits)
    want = expected(dead_border(oracle, w, CONWAY), start, lag, every, 1000)
    assert want[:2] == (16, 6) and want[3] == extra
    with pkg.Engine(h, w, rule=CONWAY, device=0, streams=2) as e:
        e.load_packed(np.zeros_like(start))
        for y, x, rh, rw in ((b - 1, 100, 3, 1), (b - 40, 200, 13, 13), (b + 20, 300, 2, 2)):
            e.write_rect(y, x, torus_ref.pack(bits[y:y + rh, x:x + rw]), rw, pkg.RECT_OR)
        assert (e.store_packed() == start).all()
        check(e, e.step_until_periodic(1000, lag, every), want, lag, every)


def test_errors(pkg):
    with pkg.Engine(37, 500, device=0) as e:
        e.init_random(1)
        before = e.store_packed()
        for lag, every in ((0, 0), (0, 64), (6, 3), (65537, 0)):
            with pytest.raises(pkg.GolError) as ei:
                e.step_until_periodic(100, lag, every)
            assert ei.value.status == pkg.GOL_EINVAL, (lag, every)
        L = pkg.lib()
        r = pkg.Until(struct_size=4)
        assert L.gol_step_until_periodic(e._h, 100, 6, 0, 0, r) == pkg.GOL_EINVAL
        r = pkg.Until(struct_size=pkg.ctypes.sizeof(pkg.Until))
        assert L.gol_step_until_periodic(e._h, 100, 6, 0, 2, r) == pkg.GOL_EINVAL  # unknown flag
        assert L.gol_step_until_periodic(e._h, 100, 6, 0, 0, None) == pkg.GOL_EINVAL
        assert (e.store_packed() == before).all()  # nothing was stepped
