"""GPU: the copy pass (life_copy.hip, DESIGN §4 "Copy pass") against the CPU oracle
and against the same engine with the pass switched off (GOL_DEV_COPY_PASS=0 at
create), which runs the stencil kernel's own copy loop.

Before a step's second depth-K launch and before every remainder launch of a step
with history, life_copy_kernel stores the rows of every calm unit (neighbour list
all streak >= 1); the launch after it then stores no row for those units and only
writes their streaks and counters.  The pass writes field words alone, so the field
and every counter (activity, activity_copied, activity_probed) must be exactly
those of the engine without it.

Shapes, fields and engine settings are those of test_gpu_copy_through.py: the
smallest with several strips, several row blocks per strip and the half strip.
"""
import numpy as np
import pytest

import torus_ref

pytestmark = pytest.mark.gpu

BASE = dict(resident=1, handoff=1, streams=1)
WIDTHS = [64 * 126, 64 * 127, 64 * 141 - 37, 64 * 156]
GLIDER = [(0, 1), (1, 2), (2, 0), (2, 1), (2, 2)]
BLOCK = [(0, 0), (0, 1), (1, 0), (1, 1)]
BLINKER = [(0, 0), (0, 1), (0, 2)]
K = 16
SWITCHES = ("GOL_DEV_ACTIVITY_SKIP", "GOL_DEV_COPY_THROUGH", "GOL_DEV_STILL_EXIT",
            "GOL_DEV_STILL_PROBE", "GOL_DEV_COPY_PASS")


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


def clear_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def make(pkg, monkeypatch, h, w, copy_pass=True, skip=True, **kw):
    """The switches are read at create, so each engine keeps what it was made with."""
    cfg = dict(BASE, rows_per_wave=64, tb_depth=K, device=0)
    cfg.update(kw)
    clear_switches(monkeypatch)
    if not skip:
        monkeypatch.setenv("GOL_DEV_ACTIVITY_SKIP", "0")
    if not copy_pass:
        monkeypatch.setenv("GOL_DEV_COPY_PASS", "0")
    return pkg.Engine(h, w, **cfg)


def units_of(pkg, h, w, **kw):
    cfg = dict(BASE, rows_per_wave=64, tb_depth=K)
    cfg.update(kw)
    return pkg.plan_neighbours(h, w, **cfg)[0].shape[0]


def counters(e):
    c, k = e.activity()
    return c, k, e.activity_copied(), e.activity_probed()


def one_step(e, g0, gens):
    e.load_packed(g0)
    e.reset_timing()
    e.step(gens)
    return e.store_packed(), counters(e)


def blocks_field(h, w, cols):
    g0 = empty(h, w)
    for r in range(20, h - 2, 64):
        for c in cols:
            put(g0, r, c, BLOCK)
    return g0


@pytest.mark.parametrize("w", WIDTHS)
def test_still_field(pkg, oracle, monkeypatch, w):
    """B/S2, p = 0.5, still by generation 15: the pass copies every unit before launch
    2 and before the remainder; the counters are those of
    test_gpu_copy_through.test_frozen_field."""
    h = 333
    g0 = oracle.bp_random(h, w, 3)
    u = units_of(pkg, h, w)
    want2 = oracle.bp_run(g0, w, 2 * K)
    want = oracle.bp_run(want2, w, 4 * K + 8)
    with make(pkg, monkeypatch, h, w) as e, make(pkg, monkeypatch, h, w, copy_pass=False) as off:
        got, cn = one_step(e, g0, 2 * K)
        ref, co = one_step(off, g0, 2 * K)
        assert (got == want2).all() and (ref == want2).all()
        assert cn[:3] == (2 * u, 0, u) and cn == co
        got, cn = one_step(e, g0, 6 * K + 8)
        ref, co = one_step(off, g0, 6 * K + 8)
        assert (got == want).all() and (ref == want).all()
        assert e.digest() == oracle.bp_digest(want, w) == off.digest()
        assert cn[:3] == (3 * u, 4 * u, 2 * u) and cn == co


@pytest.mark.parametrize("w", [64 * 126, 64 * 141 - 37])
def test_copy_beside_compute(pkg, oracle, monkeypatch, w):
    """The wake-up field of test_gpu_copy_through.test_wake_up: B3/S23 blocks plus two
    gliders.  One step of K n generations from the start for n = 2..6: in launch 2
    the pass copies the calm units while the units around the gliders compute.  The
    cumulative counters of steps n and n - 1 differ by launch n's, so equal counters
    at every n are equal copied and skipped counts per launch."""
    h, rule = 525, pkg.CONWAY
    g0 = blocks_field(h, w, (100, 2000, 4500, 6000, w - 40))
    put(g0, 40, 4008, GLIDER)
    put(g0, 168, 4968, GLIDER)
    u = units_of(pkg, h, w, rule=rule)
    want = oracle.bp_run(g0, w, K, rule)
    copied = []
    with make(pkg, monkeypatch, h, w, rule=rule) as e, \
            make(pkg, monkeypatch, h, w, copy_pass=False, rule=rule) as off:
        for n in range(2, 7):
            want = oracle.bp_run(want, w, K, rule)
            got, cn = one_step(e, g0, K * n)
            ref, co = one_step(off, g0, K * n)
            assert (got == want).all() and (ref == want).all(), f"after {K * n} generations"
            assert cn == co and cn[0] + cn[1] == n * u, f"n = {n}"
            copied.append(cn[2])
    # launch 2 copies some units while others compute
    assert 0 < copied[0] < u and copied == sorted(copied)


@pytest.mark.parametrize("w", [64 * 141 - 37, 64 * 126 + 1])
def test_edges(pkg, oracle, monkeypatch, w):
    """test_gpu_copy_through.test_edges' field: half-strip pair units with two row
    blocks, a height that is no multiple of the block, blocks and blinkers on all four
    borders and in the masked last lane group."""
    h, rule, n = 64 * 9 + 13, pkg.CONWAY, 6
    g0 = empty(h, w)
    for r, c in ((0, 0), (0, w - 2), (h - 2, 0), (h - 2, w - 2), (0, 5000), (h - 2, 2500),
                 (400, 0), (150, w - 2)):
        put(g0, r, c, BLOCK)
    for r, c in ((1, 2000), (h - 2, 6000), (300, 0), (500, w - 3)):
        put(g0, r, c, BLINKER)
    rects = pkg.plan_neighbours(h, w, **dict(BASE, rows_per_wave=64, tb_depth=K, rule=rule))[0]
    if w == 64 * 141 - 37:  # the half strip: units with two row blocks
        assert any(r[0][1] > r[0][0] and r[1][1] > r[1][0] for r in rects)
    want = oracle.bp_run(g0, w, K * n + 7, rule)
    with make(pkg, monkeypatch, h, w, rule=rule) as e, \
            make(pkg, monkeypatch, h, w, copy_pass=False, rule=rule) as off:
        got, cn = one_step(e, g0, K * n + 7)
        ref, co = one_step(off, g0, K * n + 7)
        assert (got == want).all() and (ref == want).all()
        assert cn == co and 0 < cn[2] and 0 < cn[1]
        # launch 2 alone (pair units among the calm ones) and with the remainder
        for gens in (2 * K, 2 * K + 7):
            got, cn = one_step(e, g0, gens)
            ref, co = one_step(off, g0, gens)
            assert (got == oracle.bp_run(g0, w, gens, rule)).all() and (ref == got).all()
            assert cn == co and cn[2] > 0


@pytest.mark.parametrize("glider", [False, True])
def test_remainder_depths(pkg, oracle, monkeypatch, glider):
    """Steps of 3K + r for the shipped remainder depths, each preceded by a pass; r = 3
    is two remainder launches (2 + 1) and two passes."""
    h, w, rule = 333, 64 * 141 - 37, pkg.CONWAY
    g0 = blocks_field(h, w, (100, 4500, w - 40))
    if glider:
        put(g0, 150, 4400, GLIDER)
    u = units_of(pkg, h, w, rule=rule)
    with make(pkg, monkeypatch, h, w, rule=rule) as e, \
            make(pkg, monkeypatch, h, w, copy_pass=False, rule=rule) as off:
        _, c3 = one_step(e, g0, 3 * K)
        for r in (1, 7, 8, 12, 2, 4, 6, 3):
            n = 2 if r == 3 else 1
            got, cn = one_step(e, g0, 3 * K + r)
            ref, co = one_step(off, g0, 3 * K + r)
            want = oracle.bp_run(g0, w, 3 * K + r, rule)
            assert (got == want).all() and (ref == want).all(), f"r = {r}"
            assert cn == co, f"r = {r}"
            assert (cn[0], cn[1]) == (c3[0] + n * u, c3[1]), f"r = {r}"
            per_launch = (cn[2] - c3[2]) // n
            assert per_launch == u if not glider else 0 < per_launch < u, f"r = {r}"


def test_replay(pkg, oracle, monkeypatch):
    """A step of 40 K generations on a still field, captured and then replayed (the
    pass is a node of the step's graph), as test_gpu_copy_through.test_one_load_exit;
    then a glider is loaded and the next step computes around it."""
    h, w, rule = 333, 64 * 141 - 37, pkg.CONWAY
    g0 = blocks_field(h, w, (100, 4500, w - 40))
    u = units_of(pkg, h, w, rule=rule)
    g1 = put(g0.copy(), 150, 4400, GLIDER)
    want1 = oracle.bp_run(g1, w, 40 * K, rule)
    with make(pkg, monkeypatch, h, w, rule=rule) as e, \
            make(pkg, monkeypatch, h, w, copy_pass=False, rule=rule) as off:
        for x in (e, off):
            got, cn = one_step(x, g0, 40 * K)
            assert (got == g0).all()
            assert cn[:3] == (2 * u, 38 * u, u)
            x.step(40 * K)
            assert (x.store_packed() == g0).all()
            assert counters(x)[:3] == (4 * u, 76 * u, 2 * u)
        assert counters(e) == counters(off)
        got, cn = one_step(e, g1, 40 * K)
        ref, co = one_step(off, g1, 40 * K)
        assert (got == want1).all() and (ref == want1).all()
        assert cn == co and cn[0] + cn[1] == 40 * u and 0 < cn[1] < 38 * u


OFF_CASES = {
    "handoff": dict(tb_depth=8, rows_per_wave=22, handoff=2, streams=1, resident=1),
    "streams": dict(tb_depth=16, streams=2, resident=1),
    "resident": dict(),
    "timing": dict(BASE, tb_depth=16, rows_per_wave=64),
    "skip_off": dict(BASE, tb_depth=16, rows_per_wave=64),
}


@pytest.mark.parametrize("case", sorted(OFF_CASES))
def test_off_where_the_skip_is_off(pkg, oracle, monkeypatch, case):
    """The five cases of test_gpu_copy_through.py in which no unit copies: the pass is
    never enqueued either; results are unchanged and copied == 0."""
    clear_switches(monkeypatch)
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
        got, (c, k), cp = e.store_packed(), e.activity(), e.activity_copied()
        assert (got == oracle.bp_run(g0, w, 16 * 6 + 7, rule)).all()
        assert (k, cp) == (0, 0)


SWEEP_RULES = {"ref": (0, 1 << 2), "conway": (1 << 3, (1 << 2) | (1 << 3)),
               "highlife": ((1 << 3) | (1 << 6), (1 << 2) | (1 << 3))}


@pytest.mark.parametrize("seed", range(12))
def test_differential_sweep(pkg, oracle, monkeypatch, seed):
    """The seeded generator of test_gpu_copy_through.test_differential_sweep (three
    rules, depths 8, 12 and 16, rows per wavefront 48, 61, 64 and 90, three steps):
    pass on, pass off and skip off agree with the oracle after every step."""
    rnd = np.random.default_rng(2000 + seed)
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
            make(pkg, monkeypatch, h, w, copy_pass=False, **cfg) as nopass, \
            make(pkg, monkeypatch, h, w, skip=False, **cfg) as off:
        engines = (on, nopass, off)
        for e in engines:
            e.load_packed(g0)
        want = g0
        for gens in chunks:
            want = oracle.bp_run(want, w, gens, rule)
            for e in engines:
                e.step(gens)
                assert (e.store_packed() == want).all(), (name, p, h, w, depth, rpw, gens)
        assert on.digest() == oracle.bp_digest(want, w)
        assert counters(on) == counters(nopass)
        assert off.activity_copied() == 0 and off.activity()[1] == 0
        assert sum(on.activity()) == sum(off.activity())
        # B/S2 is still when the second step starts: the pass copies before its launch 2
        assert name != "ref" or on.activity_copied() > 0
        print(name, p, h, w, depth, rpw, chunks, counters(on))


def test_torus(pkg, oracle, monkeypatch):
    """A GOL_SEM_TORUS engine, 300 x 500, B3/S23 blocks, 300 generations against
    tests/torus_ref.py: the inner streaming engine takes the pass in every round."""
    h, w, rule, gens = 300, 500, (1 << 3, (1 << 2) | (1 << 3)), 300
    g0 = blocks_field(h, w, (10, 250, w - 2))  # (the last block wraps around the edge)
    g0[:, -1] &= np.uint64((1 << (w % 64)) - 1)
    bits = torus_ref.unpack(g0, w)
    bits[20:22, 0] = 1  # ... its other half
    start = torus_ref.pack(bits)
    want = torus_ref.torus_run(oracle, start, w, gens, rule, chunk=64)
    seen = {}
    for copy_pass in (True, False):
        clear_switches(monkeypatch)
        if not copy_pass:
            monkeypatch.setenv("GOL_DEV_COPY_PASS", "0")
        with pkg.Engine(h, w, rule=rule, semantics=pkg.SEM_TORUS, tb_depth=8, resident=1,
                        handoff=1, halo_depth=64) as e:
            e.load_packed(start)
            e.reset_timing()
            e.step(gens)
            assert (e.store_packed() == want).all()
            assert e.digest() == oracle.bp_digest(want, w)
            seen[copy_pass] = counters(e)
    assert seen[True] == seen[False] and seen[True][2] > 0
