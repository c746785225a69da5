"""GPU: the still probe of a step's first launch (life_stencil.h) against
the CPU oracle, against the same engine with the probe switched off
(GOL_DEV_STILL_PROBE=0 at create) and with the skip switched off
(GOL_DEV_ACTIVITY_SKIP=0), and against a model of which units may probe through.

The first launch of a step has no history.  Each of its units runs one generation
over the rows it streams and, where that generation equals the input on the unit's
output rectangles dilated by K - 1 cells, stores its input rows and ends the launch
quiet.  Such a unit counts as computed and in Engine.activity_probed(), not as
copied.  The model (`may_probe`) restates the condition from the oracle's
generations 0 and 1 and gol_plan_neighbours' rectangles.  The kernel compares on
exactly that domain (the rows it streams less the outermost two, every column of
its storing lanes and the K - 1 nearest columns of the lane on either side), so it
probes through the model's units, no more and no fewer.  The probe is on for every
plan the skip is on for, narrow strips included.

Shapes and engine settings are those of test_gpu_activity.py.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BASE = dict(resident=1, handoff=1, streams=1)
WIDTHS = [64 * 126, 64 * 127, 64 * 141 - 37, 64 * 156]
GLIDER = [(0, 1), (1, 2), (2, 0), (2, 1), (2, 2)]
BLOCK = [(0, 0), (0, 1), (1, 0), (1, 1)]
BLINKER = [(0, 0), (0, 1), (0, 2)]
SEEDS = (1 << 2, 0)
K = 16


def empty(h, w):
    return np.zeros((h, (w + 63) // 64), dtype=np.uint64)


def put(g, r, c, cells):
    for dr, dc in cells:
        g[r + dr, (c + dc) // 64] |= np.uint64(1) << np.uint64((c + dc) % 64)
    return g


def random_field(h, w, p, seed):
    bits = np.random.default_rng(seed).random((h, ((w + 63) // 64) * 64)) < p
    bits[:, w:] = False
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint64).copy()


def make(pkg, monkeypatch, h, w, probe=True, skip=True, **kw):
    cfg = dict(BASE, rows_per_wave=64, tb_depth=K, device=0)
    cfg.update(kw)
    for name in ("GOL_DEV_ACTIVITY_SKIP", "GOL_DEV_COPY_THROUGH", "GOL_DEV_STILL_EXIT",
                 "GOL_DEV_STILL_PROBE"):
        monkeypatch.delenv(name, raising=False)
    if not skip:
        monkeypatch.setenv("GOL_DEV_ACTIVITY_SKIP", "0")
    if not probe:
        monkeypatch.setenv("GOL_DEV_STILL_PROBE", "0")
    return pkg.Engine(h, w, **cfg)


def plan(pkg, h, w, **kw):
    cfg = dict(BASE, rows_per_wave=64, tb_depth=K)
    cfg.update(kw)
    return pkg.plan_neighbours(h, w, **cfg)


def may_probe(oracle, g0, w, rule, depth, pl):
    """The units that may probe through in a launch from g0: generations 0 and 1
    agree on each of the unit's rectangles dilated by depth - 1 cells and clipped to
    the field."""
    rects = pl[0]
    h = g0.shape[0]
    g1 = oracle.bp_run(g0, w, 1, rule)
    diff = np.unpackbits((g0 ^ g1).view(np.uint8), axis=1, bitorder="little")
    d = depth - 1
    ok = set()
    for u in range(rects.shape[0]):
        same = True
        for r0, r1, q0, q1 in rects[u]:
            if r1 > r0 and q1 > q0:
                same = same and not diff[max(0, r0 - d):min(h, r1 + d),
                                         max(0, 64 * q0 - d):min(w, 64 * q1 + d)].any()
        if same:
            ok.add(u)
    return ok


def one_step(e, g0, gens):
    e.load_packed(g0)
    e.reset_timing()
    e.step(gens)
    got = e.store_packed()
    c, k = e.activity()
    return got, (c, k, e.activity_copied(), e.activity_probed())


def blocks_field(h, w):
    """2 x 2 blocks on all four borders, in the corners, in the masked last lane
    group and all over the half strip's pair units."""
    g0 = empty(h, w)
    for r, c in ((0, 0), (0, w - 2), (h - 2, 0), (h - 2, w - 2), (0, 5000), (h - 2, 2500),
                 (400, 0), (150, w - 2), (300, w - 30)):
        put(g0, r, c, BLOCK)
    for r in range(20, h - 2, 31):
        for c in range(64 * 60 + 7, min(w - 2, 64 * 82), 449):
            put(g0, r, c, BLOCK)
    return g0


def still_cases(pkg, oracle):
    for w in WIDTHS:
        g = oracle.bp_run(oracle.bp_random(333, w, 3), w, 2 * K)
        yield f"ref-{w}", 333, w, pkg.REF_RULE, g
    for w in (64 * 141 - 37, 64 * 126 + 1):
        h = 64 * 9 + 13
        yield f"blocks-{w}", h, w, pkg.CONWAY, blocks_field(h, w)


@pytest.mark.parametrize("case", range(6))
def test_still_field(pkg, oracle, monkeypatch, case):
    """A field that is still from the start: the first launch probes every unit
    through, the second copies, the rest skip; with the probe off the same fields
    and the same counters but `probed`."""
    name, h, w, rule, g0 = list(still_cases(pkg, oracle))[case]
    assert (oracle.bp_run(g0, w, 1, rule) == g0).all() and g0.any(), name
    pl = plan(pkg, h, w, rule=rule)
    units = pl[0].shape[0]
    if name == f"blocks-{64 * 141 - 37}":  # the half strip: units with two row blocks
        assert any(r[0][1] > r[0][0] and r[1][1] > r[1][0] for r in pl[0])
    with make(pkg, monkeypatch, h, w, rule=rule) as e:
        got, act = one_step(e, g0, K)
        assert (got == g0).all() and act == (units, 0, 0, units), name
        got, act = one_step(e, g0, 6 * K + 8)
        assert (got == g0).all() and e.digest() == oracle.bp_digest(g0, w)
        assert act == (3 * units, 4 * units, 2 * units, units), name
    with make(pkg, monkeypatch, h, w, probe=False, rule=rule) as e:
        got, act = one_step(e, g0, K)
        assert (got == g0).all() and act == (units, 0, 0, 0), name
        got, act = one_step(e, g0, 6 * K + 8)
        assert (got == g0).all() and act == (3 * units, 4 * units, 2 * units, 0), name


@pytest.mark.parametrize("side", ["below", "above", "right", "left"])
def test_dilation_edge(pkg, oracle, monkeypatch, side):
    """Seeds (B2/S, fronts move one cell per generation), K = 12, a domino whose
    nearest cell is d cells from a tile for d = K - 2 .. K + 1: the tile probes
    through exactly when the model says so, and so does every other unit.  (In the
    vertical cases the domino is also far from every strip boundary.)"""
    h, w, depth = 333, 64 * 141 - 37, 12
    pl = plan(pkg, h, w, rule=SEEDS, tb_depth=depth)
    rects = pl[0]
    units = rects.shape[0]
    single = [u for u in range(units) if rects[u][1][1] <= rects[u][1][0]]
    inner = [u for u in single if rects[u][0][0] >= 64 and rects[u][0][1] <= h - 64]
    vertical = side in ("below", "above")
    if vertical or side == "right":
        tile = next(u for u in inner if rects[u][0][2] == 0)          # strip 0
    else:
        tile = max(inner, key=lambda u: rects[u][0][2])               # the last strip
    r0, r1, q0, q1 = (int(x) for x in rects[tile][0])
    assert q0 > 0 or side != "left"
    assert 64 * q1 < w - 64 or side != "right"
    seen = []
    with make(pkg, monkeypatch, h, w, rule=SEEDS, tb_depth=depth) as e:
        for d in (depth - 2, depth - 1, depth, depth + 1):
            g0 = empty(h, w)
            mid = 64 * ((q0 + q1) // 2) + 10
            if side == "below":
                put(g0, r1 - 1 + d, mid, [(0, 0), (0, 1)])
            elif side == "above":
                put(g0, r0 - d, mid, [(0, 0), (0, 1)])
            elif side == "right":
                put(g0, (r0 + r1) // 2, 64 * q1 - 1 + d, [(0, 0), (1, 0)])
            else:
                put(g0, (r0 + r1) // 2, 64 * q0 - d, [(0, 0), (1, 0)])
            if vertical:  # >= 64 + K columns from every strip boundary
                edges = {64 * int(q) for r in rects for rr in r if rr[1] > rr[0] for q in rr[2:]}
                assert all(abs(mid - x) >= 64 + depth for x in edges)
            ok = may_probe(oracle, g0, w, SEEDS, depth, pl)
            got, (c, k, cp, pr) = one_step(e, g0, depth)
            assert (got == oracle.bp_run(g0, w, depth, SEEDS)).all(), (side, d)
            assert (c, k, cp) == (units, 0, 0) and pr == len(ok), (side, d)
            seen.append((d, tile in ok, pr, len(ok)))
    print(side, seen)
    # the births next to the domino reach the dilated tile up to d = K, not beyond
    assert [t for _, t, _, _ in seen] == [False, False, False, True]


def test_settles_late(pkg, oracle, monkeypatch):
    """Patterns that become still lifes 1 and 2 generations into the first launch
    (test_gpu_activity.test_settles_mid_launch): the units within K - 1 cells of them
    run their stage logic, the others probe through; the skip counts stay."""
    h, w, rule, n = 333, 64 * 127, pkg.CONWAY, 10
    g0 = empty(h, w)
    put(g0, 30, 300, [(0, 0), (0, 1), (1, 0)])
    put(g0, 200, 5000, [(0, 0), (0, 1), (0, 2), (0, 3)])
    pl = plan(pkg, h, w, rule=rule)
    units = pl[0].shape[0]
    ok = may_probe(oracle, g0, w, rule, K, pl)
    assert 0 < len(ok) < units
    with make(pkg, monkeypatch, h, w, rule=rule) as e:
        got, (c, k, cp, pr) = one_step(e, g0, K * n + 8)
        assert (got == oracle.bp_run(g0, w, K * n + 8, rule)).all()
        assert (c, k) == (3 * units, (n - 2) * units)
        assert pr == len(ok)


def test_period_2(pkg, oracle, monkeypatch):
    """A blinker: its unit and every unit within K - 1 cells of it never probe
    through, in any step; every other unit does in every step."""
    h, w, rule = 333, 64 * 141 - 37, pkg.CONWAY
    g0 = put(empty(h, w), 160, 4500, BLINKER)
    pl = plan(pkg, h, w, rule=rule)
    units = pl[0].shape[0]
    g1 = oracle.bp_run(g0, w, 1, rule)
    ok0, ok1 = may_probe(oracle, g0, w, rule, K, pl), may_probe(oracle, g1, w, rule, K, pl)
    assert ok0 == ok1 and 0 < len(ok0) < units
    with make(pkg, monkeypatch, h, w, rule=rule) as e:
        e.load_packed(g0)
        e.reset_timing()
        want = g0
        for i, gens in enumerate((K, 2 * K + 1, 5 * K, 5 * K)):
            e.step(gens)
            want = oracle.bp_run(want, w, gens, rule)
            assert (e.store_packed() == want).all()
            assert e.activity_probed() == (i + 1) * len(ok0)


@pytest.mark.parametrize("w", [64 * 126, 64 * 141 - 37])
def test_wake_up(pkg, oracle, monkeypatch, w):
    """B3/S23 blocks plus gliders that cross a row-block and a strip boundary
    (test_gpu_activity.test_wake_up's field), one step of K n generations for n = 1..6:
    skipped and copied units per launch are those of an engine with the probe off,
    and the first launch probes through the model's units."""
    h, rule = 525, pkg.CONWAY
    g0 = empty(h, w)
    for r in range(20, h - 2, 64):
        for c in (100, 2000, 4500, 6000, w - 40):
            put(g0, r, c, BLOCK)
    put(g0, 40, 4008, GLIDER)
    put(g0, 168, 4968, GLIDER)
    pl = plan(pkg, h, w, rule=rule)
    units = pl[0].shape[0]
    ok = may_probe(oracle, g0, w, rule, K, pl)
    assert 0 < len(ok) < units
    want = g0
    with make(pkg, monkeypatch, h, w, rule=rule) as e, \
            make(pkg, monkeypatch, h, w, probe=False, rule=rule) as off:
        for n in range(1, 7):
            got, (c, k, cp, pr) = one_step(e, g0, K * n)
            ref, (co, ko, cpo, pro) = one_step(off, g0, K * n)
            want = oracle.bp_run(want, w, K, rule)
            assert (got == want).all() and (ref == want).all(), f"after {K * n} generations"
            assert (c, k, cp) == (co, ko, cpo) and pro == 0
            assert pr == len(ok)


def test_step_shapes(pkg, oracle, monkeypatch):
    """A plain step of K, then three steps of 5K (capture and two replays): every
    step's first launch probes every unit through; then a glider is loaded."""
    h, w, rule = 333, 64 * 141 - 37, pkg.CONWAY
    g0 = empty(h, w)
    for r in range(20, h - 2, 64):
        for c in (100, 4500, w - 40):
            put(g0, r, c, BLOCK)
    units = plan(pkg, h, w, rule=rule)[0].shape[0]
    with make(pkg, monkeypatch, h, w, rule=rule) as e:
        got, act = one_step(e, g0, K)
        assert (got == g0).all() and act == (units, 0, 0, units)
        for i in range(3):
            e.step(5 * K)
            assert (e.store_packed() == g0).all()
            assert e.activity_probed() == (i + 2) * units
            assert e.activity() == (units + 2 * units * (i + 1), 3 * units * (i + 1))
        g1 = put(g0.copy(), 150, 4400, GLIDER)
        got, (c, k, cp, pr) = one_step(e, g1, 5 * K)
        assert (got == oracle.bp_run(g1, w, 5 * K, rule)).all()
        assert 0 < pr < units and c + k == 5 * units


OFF_CASES = {
    "handoff": dict(tb_depth=8, rows_per_wave=22, handoff=2, streams=1, resident=1),
    "streams": dict(tb_depth=16, streams=2, resident=1),
    "resident": dict(),
    "timing": dict(BASE, tb_depth=16, rows_per_wave=64),
    "skip_off": dict(BASE, tb_depth=16, rows_per_wave=64),
}


@pytest.mark.parametrize("case", sorted(OFF_CASES))
def test_off_where_the_skip_is_off(pkg, oracle, monkeypatch, case):
    """Hand-off plans, multi-stream engines, the resident kernel, launches timed with
    events and GOL_DEV_ACTIVITY_SKIP=0: no unit probes through; results are unchanged.
    (No narrow-strip plan is excluded: the probe is on wherever the skip is.)"""
    for name in ("GOL_DEV_ACTIVITY_SKIP", "GOL_DEV_COPY_THROUGH", "GOL_DEV_STILL_PROBE"):
        monkeypatch.delenv(name, raising=False)
    if case == "skip_off":
        monkeypatch.setenv("GOL_DEV_ACTIVITY_SKIP", "0")
    h, w = (512, 4096) if case == "resident" else (600, 64 * 127)
    rule = pkg.CONWAY
    g0 = empty(h, w)
    for r in range(20, h - 2, 64):
        put(g0, r, 100, BLOCK)
    put(g0, 200, 3000, GLIDER)
    with pkg.Engine(h, w, rule=rule, device=0, **OFF_CASES[case]) as e:
        if case == "handoff":
            assert e.handoff
        if case == "resident":
            assert e.resident is not None
        e.load_packed(g0)
        e.reset_timing()
        if case == "timing":
            e.set_timing(1)
        e.step(16 * 6 + 7)
        got = e.store_packed()
        assert (got == oracle.bp_run(g0, w, 16 * 6 + 7, rule)).all()
        assert e.activity()[1] == 0 and e.activity_probed() == 0


SWEEP_RULES = {"ref": (0, 1 << 2), "conway": (1 << 3, (1 << 2) | (1 << 3)),
               "highlife": ((1 << 3) | (1 << 6), (1 << 2) | (1 << 3))}


@pytest.mark.parametrize("seed", range(12))
def test_differential_sweep(pkg, oracle, monkeypatch, seed):
    """Seeded sweep of the kind of test_gpu_activity.test_differential_sweep: three
    rules, depths 8, 12 and 16, three steps of mixed lengths; probe on, probe off and
    skip off agree with the oracle after every step."""
    rnd = np.random.default_rng(3000 + seed)
    name = sorted(SWEEP_RULES)[seed % 3]
    rule = SWEEP_RULES[name]
    p = [0.02, 0.05, 0.12, 0.3, 0.5][int(rnd.integers(5))]
    h = int(rnd.integers(130, 700))
    w = int(rnd.choice(WIDTHS + [3000, 64 * 190 + 5])) - int(rnd.integers(0, 64))
    depth = 12 if name == "highlife" else int(rnd.choice([8, 16]))
    rpw = int(rnd.choice([48, 61, 64, 90]))
    chunks = [int(rnd.choice([3 * depth, 5 * depth + 3, 8 * depth, 4 * depth + 1, 2 * depth + 7]))
              for _ in range(3)]
    g0 = random_field(h, w, p, seed)
    cfg = dict(rule=rule, tb_depth=depth, rows_per_wave=rpw)
    with make(pkg, monkeypatch, h, w, **cfg) as on, \
            make(pkg, monkeypatch, h, w, probe=False, **cfg) as noprobe, \
            make(pkg, monkeypatch, h, w, skip=False, **cfg) as off:
        engines = (on, noprobe, off)
        for e in engines:
            e.load_packed(g0)
        want = g0
        for gens in chunks:
            want = oracle.bp_run(want, w, gens, rule)
            for e in engines:
                e.step(gens)
                assert (e.store_packed() == want).all(), (name, p, h, w, depth, rpw, gens)
        assert on.digest() == oracle.bp_digest(want, w)
        assert noprobe.activity_probed() == 0 and off.activity_probed() == 0
        assert off.activity()[1] == 0
        assert sum(on.activity()) == sum(noprobe.activity()) == sum(off.activity())
        assert on.activity() == noprobe.activity()
        assert on.activity_copied() == noprobe.activity_copied()
        # B/S2 is still when the second step starts: its first launch probes through
        assert name != "ref" or on.activity_probed() > 0
        print(name, p, h, w, depth, rpw, chunks, on.activity(), on.activity_probed())
