"""GPU: the snapshot slot -- Engine.snapshot / snapshot_same / snapshot_diff /
snapshot_restore / snapshot_drop (gol_snapshot*) on every engine kind that has one.

Expectations come from numpy on the fields the test loads or edits itself, from the CPU
oracle (bp_random, bp_run) and, for tori, from torus_ref (roll_run, torus_run); never
from the engine.  The shapes are the smallest at which the compare kernel takes another
path: one word, a masked last word, exactly one tile row (8 rows), a partial tile row,
a second word, and 65 words per row (17 x 4160), where a row spans two tile columns.
"""
import numpy as np
import pytest

import torus_ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 63), (8, 64), (9, 65), (37, 500), (17, 4160)]
BIG = (1500, 500)
CONWAY = (1 << 3, (1 << 2) | (1 << 3))

# name -> (constructor keywords, torus)
KINDS = {
    "default": (dict(), False),
    "streaming": (dict(tb_depth=8, resident=1), False),
    "torus": (dict(semantics=2), True),
    "torus_streaming": (dict(semantics=2, tb_depth=8, resident=1), True),
    "streams2": (dict(streams=2), False),
}
SMALL_KINDS = ["default", "streaming", "torus", "torus_streaming"]
CASES = [(k, s) for k in SMALL_KINDS for s in SHAPES] + [("streams2", BIG)]
CASE_IDS = [f"{k}-{h}x{w}" for k, (h, w) in CASES]
STEP_CASES = [(k, (37, 500)) for k in SMALL_KINDS] + [("streams2", BIG)]
STEP_IDS = [f"{k}-{h}x{w}" for k, (h, w) in STEP_CASES]


def make(pkg, kind, h, w, rule=CONWAY):
    return pkg.Engine(h, w, rule=rule, device=0, **KINDS[kind][0])


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words, dtype=np.uint64).view(np.uint8)).sum())


def step_gens(K):
    """At least 4 K generations and no multiple of K: a replayed step graph that ends
    with a remainder launch (as tests/test_gpu_rect.py)."""
    g = 4 * K + 5
    return g if g % K else g + 1


def run(oracle, torus, words, w, gens, rule=CONWAY):
    if torus:
        return torus_ref.torus_run(oracle, words, w, gens, rule)
    return oracle.bp_run(words, w, gens, rule)


ONE = np.ones((1, 1), dtype=np.uint64)


@pytest.mark.parametrize("kind,shape", CASES, ids=CASE_IDS)
def test_one_cell_flips(pkg, oracle, kind, shape):
    h, w = shape
    cells = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    if w > 63:
        cells.append((h // 2, 63))
    if h > 8 and w > 4095:
        cells.append((8, 4095))
    with make(pkg, kind, h, w) as e:
        e.load_packed(oracle.bp_random(h, w, 11))
        e.snapshot()
        assert e.snapshot_same() is True and e.snapshot_diff() == 0
        for y, x in sorted(set(cells)):
            e.write_rect(y, x, ONE, 1, pkg.RECT_XOR)
            assert e.snapshot_same() is False, (y, x)
            assert e.snapshot_diff() == 1, (y, x)
            e.write_rect(y, x, ONE, 1, pkg.RECT_XOR)
            assert e.snapshot_same() is True and e.snapshot_diff() == 0, (y, x)


@pytest.mark.parametrize("kind,shape", CASES, ids=CASE_IDS)
def test_many_flips(pkg, oracle, kind, shape):
    h, w = shape
    rng = np.random.default_rng(h * 10000 + w)
    with make(pkg, kind, h, w) as e:
        e.load_packed(oracle.bp_random(h, w, 12))
        e.snapshot()
        # the whole field, then a window that starts and ends inside words
        for y, x, rh, rw in ((0, 0, h, w), (h // 3, w // 3, h - h // 3, w - w // 3)):
            win = rng.integers(0, 2, (rh, rw), dtype=np.uint8)
            win[-1, -1] = 1  # (a 1 x 1 window too flips a cell)
            e.write_rect(y, x, torus_ref.pack(win), rw, pkg.RECT_XOR)
            assert e.snapshot_diff() == int(win.sum()), (y, x, rh, rw)
            assert e.snapshot_same() is False
            e.write_rect(y, x, torus_ref.pack(win), rw, pkg.RECT_XOR)
        assert e.snapshot_diff() == 0 and e.snapshot_same() is True


@pytest.mark.parametrize("shape", [(9, 65), (37, 500)])
@pytest.mark.parametrize("kind", ["torus", "torus_streaming"])
def test_torus(pkg, oracle, kind, shape):
    h, w = shape
    with make(pkg, kind, h, w) as e:
        gens = 2 * e.halo_depth + 3  # two whole wrap rounds and a part of a third
        start = oracle.bp_random(h, w, 13)
        e.load_packed(start)
        e.snapshot()
        e.step(gens)
        later = torus_ref.roll_run(start, w, gens, CONWAY)
        assert popcount(later ^ start) > 0
        # (the ghost cells differ from the snapshot's by now: they do not count)
        assert e.snapshot_diff() == popcount(later ^ start)
        assert e.snapshot_same() is False
        e.snapshot_restore()
        assert (e.store_packed() == start).all()
        assert e.snapshot_same() is True and e.snapshot_diff() == 0
        e.step(gens)
        assert (e.store_packed() == later).all()


@pytest.mark.parametrize("kind,shape", STEP_CASES, ids=STEP_IDS)
def test_restore_then_step(pkg, oracle, kind, shape):
    """Step n, snapshot, step n, restore, step n: the field of generation 2 n.  The step
    after the restore replays a graph captured before it, ends with a remainder launch,
    and must not inherit activity history or "rows both buffers hold" from the step the
    restore undid."""
    h, w = shape
    torus = KINDS[kind][1]
    with make(pkg, kind, h, w) as e:
        n = step_gens(e.tb_depth)
        assert n >= 4 * e.tb_depth and n % e.tb_depth
        start = oracle.bp_random(h, w, 14)
        at_n = run(oracle, torus, start, w, n)
        at_2n = run(oracle, torus, at_n, w, n)
        if kind == "streams2":  # live cells on both sides of the stripe boundary
            b = pkg.rank_rows(h, 2, 1)[0]
            for f in (at_n, at_2n):
                assert f[b - 1].any() and f[b].any()
        e.load_packed(start)
        e.step(n)
        e.snapshot()
        e.step(n)
        assert (e.store_packed() == at_2n).all()
        assert e.snapshot_diff() == popcount(at_n ^ at_2n) > 0
        e.snapshot_restore()
        assert (e.store_packed() == at_n).all()
        e.step(n)
        assert (e.store_packed() == at_2n).all()
        assert tuple(e.digest()) == tuple(oracle.bp_digest(at_2n, w))


@pytest.mark.parametrize("kind,shape", STEP_CASES, ids=STEP_IDS)
def test_load_after_snapshot(pkg, oracle, kind, shape):
    h, w = shape
    with make(pkg, kind, h, w) as e:
        a, b = oracle.bp_random(h, w, 15), oracle.bp_random(h, w, 16)
        e.load_packed(a)
        e.snapshot()
        e.load_packed(b)
        assert e.snapshot_diff() == popcount(a ^ b) > 0
        e.init_random(15)  # (the engine's own bp_random field)
        assert e.snapshot_diff() == 0 and e.snapshot_same() is True
        # a second snapshot replaces the first
        e.load_packed(b)
        e.snapshot()
        e.load_packed(a)
        e.snapshot_restore()
        assert (e.store_packed() == b).all()


def test_errors(pkg):
    h, w = 37, 500

    def estate(fn):
        with pytest.raises(pkg.GolError) as ei:
            fn()
        assert ei.value.status == pkg.GOL_ESTATE, ei.value
        assert str(ei.value).split(":", 1)[1].strip()  # a message

    for kw in (dict(), dict(semantics=2), dict(streams=2)):
        hh = 1500 if kw.get("streams") else h
        with pkg.Engine(hh, w, device=0, **kw) as e:
            e.init_random(1)
            for fn in (e.snapshot_same, e.snapshot_diff, e.snapshot_restore):
                estate(fn)
            e.snapshot_drop()  # nothing to drop: fine
            e.snapshot()
            assert e.snapshot_same() is True
            e.snapshot_drop()
            for fn in (e.snapshot_same, e.snapshot_diff, e.snapshot_restore):
                estate(fn)
            e.snapshot()  # and the slot comes back
            assert e.snapshot_diff() == 0
            L = pkg.lib()
            assert L.gol_snapshot_same(e._h, None) == pkg.GOL_EINVAL
            assert L.gol_snapshot_diff(e._h, None) == pkg.GOL_EINVAL
    calls = ("snapshot", "snapshot_same", "snapshot_diff", "snapshot_restore", "snapshot_drop")
    with pkg.Engine(h, w, device=0, semantics=pkg.SEM_REF_STRIPES, ref_ranks=3) as r:
        r.init_random(1)
        for name in calls:
            estate(getattr(r, name))
        estate(lambda: r.step_until_periodic(10, 1))
    with pkg.Group(1500, w, 2) as g:
        g.init_random(1)
        for name in calls:
            estate(getattr(g.members[1], name))
        estate(lambda: g.members[0].step_until_periodic(10, 1))


@pytest.mark.parametrize("shape", [(1, 127), (8, 128), (9, 129), (37, 500)])
def test_four_planes(pkg, oracle, shape):
    """The compare of an NP = 4 leaf (leaf_view: both words of the last lane group
    masked): only a library built with the 4-plane kernels (the dev build, through
    GOL_LIB) creates such an engine."""
    h, w = shape
    try:
        e = pkg.Engine(h, w, rule=CONWAY, device=0, word_planes=4, streams=1)
    except pkg.GolError as err:
        assert err.status == pkg.GOL_EINVAL
        pytest.skip("the loaded library has no 4-plane kernels")
    with e:
        assert e.word_planes == 4
        a, b = oracle.bp_random(h, w, 17), oracle.bp_random(h, w, 18)
        e.load_packed(a)
        e.snapshot()
        assert e.snapshot_same() is True and e.snapshot_diff() == 0
        # either word of a lane group, the group's edges, the last column
        for x in sorted({x for x in (0, 63, 64, 127, 128, w - 1) if x < w}):
            for y in sorted({0, h - 1}):
                e.write_rect(y, x, ONE, 1, pkg.RECT_XOR)
                assert e.snapshot_diff() == 1, (y, x)
                assert e.snapshot_same() is False, (y, x)
                e.write_rect(y, x, ONE, 1, pkg.RECT_XOR)
                assert e.snapshot_diff() == 0 and e.snapshot_same() is True, (y, x)
        e.load_packed(b)
        assert e.snapshot_diff() == popcount(a ^ b)
        e.snapshot_restore()
        assert (e.store_packed() == a).all()
