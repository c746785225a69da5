"""GPU: copy-through and the one-load exit of the activity skip (life_stencil.h,
DESIGN §4) against the CPU oracle, against the same engine with copy-through
switched off (GOL_DEV_COPY_THROUGH=0 at create) and with the skip switched off
(GOL_DEV_ACTIVITY_SKIP=0), and against a model of which units may copy.

A unit whose neighbour list ended the launch before quiet (every streak >= 1) but
not the two launches before (not every streak >= 2) copies its rows from the input
buffer to the output buffer without stage logic; so does such a unit in the
remainder launch of a step with history, which never skips.  A copied unit counts
as computed (it stored its rows) and in Engine.activity_copied().  The model
(`model`) restates this from the oracle's fields and gol_plan_neighbours, as
test_gpu_activity.py's `expected` does for the skip: calm[n] = units whose list is
all >= 1 before launch n, still[n] = all >= 2.  The kernel's streaks are at most the
model's (it may call a quiet unit "changed", never the reverse), so copied + skipped
units are at most |calm|; where nothing changes within 7 rows below a block they are
the model's sets.

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


def make(pkg, monkeypatch, h, w, through=True, skip=True, **kw):
    cfg = dict(BASE, rows_per_wave=64, tb_depth=K, device=0)
    cfg.update(kw)
    monkeypatch.delenv("GOL_DEV_ACTIVITY_SKIP", raising=False)
    monkeypatch.delenv("GOL_DEV_COPY_THROUGH", raising=False)
    monkeypatch.delenv("GOL_DEV_STILL_EXIT", raising=False)
    if not skip:
        monkeypatch.setenv("GOL_DEV_ACTIVITY_SKIP", "0")
    if not through:
        monkeypatch.setenv("GOL_DEV_COPY_THROUGH", "0")
    return pkg.Engine(h, w, **cfg)


def plan(pkg, h, w, **kw):
    cfg = dict(BASE, rows_per_wave=64, tb_depth=K)
    cfg.update(kw)
    return pkg.plan_neighbours(h, w, **cfg)


def model(oracle, g0, w, rule, depth, launches, pl):
    """Per depth-`depth` launch n of one step from g0: (calm, still), the sets of
    units whose list is all >= 1 / all >= 2 before the launch (both empty at n = 0,
    which carries no history); and the calm set after the last launch, which is
    what a remainder launch copies."""
    rects, offs, ids = pl
    units = rects.shape[0]
    streak = np.zeros(units, dtype=np.int64)
    lists = [ids[offs[u]:offs[u + 1]] for u in range(units)]
    g = g0
    out = []
    for n in range(launches):
        calm = {u for u in range(units) if n >= 1 and (streak[lists[u]] >= 1).all()}
        still = {u for u in range(units) if n >= 1 and (streak[lists[u]] >= 2).all()}
        out.append((calm, still))
        prev = oracle.bp_run(g, w, depth - 1, rule)
        g = oracle.bp_run(prev, w, 1, rule)
        diff = g != prev
        quiet = np.ones(units, dtype=bool)
        for u in range(units):
            for r0, r1, q0, q1 in rects[u]:
                if r1 > r0 and diff[r0:r1, q0:q1].any():
                    quiet[u] = False
        assert all(quiet[u] for u in calm)  # the argument of DESIGN §4
        streak = np.where(quiet, np.minimum(streak + 1, 255), 0)
    last = {u for u in range(units) if launches >= 1 and (streak[lists[u]] >= 1).all()}
    return out, last


def one_step(e, g0, gens):
    e.load_packed(g0)
    e.reset_timing()
    e.step(gens)
    got = e.store_packed()
    c, k = e.activity()
    return got, (c, k, e.activity_copied())


@pytest.mark.parametrize("w", WIDTHS)
def test_frozen_field(pkg, oracle, monkeypatch, w):
    """B/S2, p = 0.5, still by generation 15: launch 2 and the remainder copy every
    unit through; the skip counts are those of test_gpu_activity.test_frozen_field."""
    h = 333
    g0 = oracle.bp_random(h, w, 3)
    units = plan(pkg, h, w)[0].shape[0]
    with make(pkg, monkeypatch, h, w) as e:
        got, (c, k, cp) = one_step(e, g0, 2 * K)
        want2 = oracle.bp_run(g0, w, 2 * K)
        assert (got == want2).all()
        assert (c, k, cp) == (2 * units, 0, units)
        got, (c, k, cp) = one_step(e, g0, 6 * K + 8)
        want = oracle.bp_run(want2, w, 4 * K + 8)
        assert (got == want).all() and e.digest() == oracle.bp_digest(want, w)
        assert (c, k, cp) == (3 * units, 4 * units, 2 * units)
    with make(pkg, monkeypatch, h, w, through=False) as e:
        got, (c, k, cp) = one_step(e, g0, 6 * K + 8)
        assert (got == want).all() and (c, k, cp) == (3 * units, 4 * units, 0)


@pytest.mark.parametrize("w", [64 * 126, 64 * 141 - 37])
def test_wake_up(pkg, oracle, monkeypatch, w):
    """B3/S23 blocks plus gliders that cross a row-block and a strip boundary (the
    scenario of test_gpu_activity.test_wake_up), one step of 16 n generations from the
    start for n = 1..12: per launch, the copied units against the model's set
    calm - still, next to an engine with copy-through off and the oracle."""
    h, rule = 525, pkg.CONWAY
    g0 = empty(h, w)
    for r in range(20, h - 2, 64):
        for c in (100, 2000, 4500, 6000, w - 40):
            put(g0, r, c, BLOCK)
    put(g0, 40, 4008, GLIDER)
    put(g0, 168, 4968, GLIDER)
    pl = plan(pkg, h, w, rule=rule)
    units = pl[0].shape[0]
    sets, _ = model(oracle, g0, w, rule, K, 12, pl)
    copied, skipped = [0], [0]
    want = g0
    with make(pkg, monkeypatch, h, w, rule=rule) as e, \
            make(pkg, monkeypatch, h, w, through=False, rule=rule) as off:
        for n in range(1, 13):
            got, (c, k, cp) = one_step(e, g0, K * n)
            ref, (co, ko, cpo) = one_step(off, g0, K * n)
            want = oracle.bp_run(want, w, K, rule)
            assert (got == want).all() and (ref == want).all(), f"after {K * n} generations"
            assert c + k == n * units and (co, ko, cpo) == (c, k, 0)
            copied.append(cp)
            skipped.append(k)
    cp_n, k_n = np.diff(copied).tolist(), np.diff(skipped).tolist()
    m_copy = [len(calm - still) for calm, still in sets]
    print("copied per launch", cp_n, "model", m_copy, "skipped", k_n)
    for n, (calm, still) in enumerate(sets):
        assert cp_n[n] <= len(calm - still) and cp_n[n] + k_n[n] <= len(calm)
    # nothing lives within 7 rows below a block here: the kernel's sets are the model's
    assert k_n == [len(still) for _, still in sets] and cp_n == m_copy
    assert cp_n[0] == 0 and 0 < cp_n[1] < units
    # a unit that copies beside one that runs its stage logic: a listed unit that
    # is not calm itself
    _, offs, ids = pl
    beside = [(n, u) for n, (calm, still) in enumerate(sets) for u in calm - still
              if any(v not in calm for v in ids[offs[u]:offs[u + 1]])]
    assert beside, "no unit copies next to one that computes in this scenario"


def test_period_2(pkg, oracle, monkeypatch):
    """A blinker: its unit and every unit listing it never copy and never skip."""
    h, w, rule, n = 333, 64 * 141 - 37, pkg.CONWAY, 8
    g0 = put(empty(h, w), 160, 4500, BLINKER)
    pl = plan(pkg, h, w, rule=rule)
    rects, offs, ids = pl
    units = rects.shape[0]
    owner = [u for u in range(units) for r0, r1, q0, q1 in rects[u]
             if r0 <= 160 < r1 and q0 <= 4500 // 64 < q1]
    assert len(owner) == 1
    awake = {u for u in range(units) if owner[0] in ids[offs[u]:offs[u + 1]]}
    assert 1 < len(awake) < units
    sets, last = model(oracle, g0, w, rule, K, n, pl)
    assert all(not (calm & awake) for calm, _ in sets) and not (last & awake)
    with make(pkg, monkeypatch, h, w, rule=rule) as e:
        got, (c, k, cp) = one_step(e, g0, K * n + 8)
        assert (got == oracle.bp_run(g0, w, K * n + 8, rule)).all()
        # everything else: launch 2 and the remainder copy, launches 3..n skip; the
        # awake units run their stage logic in all n + 1 launches
        rest = units - len(awake)
        assert k == (n - 2) * rest and cp == 2 * rest
        assert c - cp == (n + 1) * len(awake) + rest


@pytest.mark.parametrize("w", [64 * 141 - 37, 64 * 126 + 1])
def test_edges(pkg, oracle, monkeypatch, w):
    """Half-strip pair units with two row blocks, a height that is no multiple of the
    block, blocks and blinkers on all four borders and in the masked last lane group
    (the scenario of test_gpu_activity.test_edges)."""
    h, rule, n = 64 * 9 + 13, pkg.CONWAY, 6
    g0 = empty(h, w)
    for r, c in ((0, 0), (0, w - 2), (h - 2, 0), (h - 2, w - 2), (0, 5000), (h - 2, 2500),
                 (400, 0), (150, w - 2)):
        put(g0, r, c, BLOCK)
    for r, c in ((1, 2000), (h - 2, 6000), (300, 0), (500, w - 3)):
        put(g0, r, c, BLINKER)
    pl = plan(pkg, h, w, rule=rule)
    rects = pl[0]
    units = rects.shape[0]
    if w == 64 * 141 - 37:  # the half strip: units with two row blocks
        assert any(r[0][1] > r[0][0] and r[1][1] > r[1][0] for r in rects)
    sets, last = model(oracle, g0, w, rule, K, n, pl)
    want_k = sum(len(still) for _, still in sets)
    want_cp = sum(len(calm - still) for calm, still in sets) + len(last)
    assert 0 < want_k < (n - 2) * units and 0 < len(last) < units
    with make(pkg, monkeypatch, h, w, rule=rule) as e, \
            make(pkg, monkeypatch, h, w, through=False, rule=rule) as off:
        got, (c, k, cp) = one_step(e, g0, K * n + 7)
        ref, (co, ko, cpo) = one_step(off, g0, K * n + 7)
        want = oracle.bp_run(g0, w, K * n + 7, rule)
        assert (got == want).all() and (ref == want).all()
        assert (c, k, cp) == ((n + 1) * units - want_k, want_k, want_cp)
        assert (co, ko, cpo) == (c, k, 0)


@pytest.mark.parametrize("glider", [False, True])
def test_remainder_depths(pkg, oracle, monkeypatch, glider):
    """Steps of 3K + r for the shipped remainder depths: the remainder launch copies
    the model's calm set of the last depth-K launch and computes the rest."""
    h, w, rule = 333, 64 * 141 - 37, pkg.CONWAY
    g0 = empty(h, w)
    for r in range(20, h - 2, 64):
        for c in (100, 4500, w - 40):
            put(g0, r, c, BLOCK)
    if glider:
        put(g0, 150, 4400, GLIDER)
    pl = plan(pkg, h, w, rule=rule)
    units = pl[0].shape[0]
    sets, last = model(oracle, g0, w, rule, K, 3, pl)
    assert len(last) == units if not glider else 0 < len(last) < units
    with make(pkg, monkeypatch, h, w, rule=rule) as e:
        _, (c3, k3, cp3) = one_step(e, g0, 3 * K)
        assert cp3 == sum(len(calm - still) for calm, still in sets)
        # every shipped depth below K; r = 3 is two remainder launches (2 + 1), which
        # both read the streaks of the last depth-K launch
        for r in (1, 7, 8, 12, 2, 4, 6, 3):
            n = 2 if r == 3 else 1
            got, (c, k, cp) = one_step(e, g0, 3 * K + r)
            assert (got == oracle.bp_run(g0, w, 3 * K + r, rule)).all(), f"r = {r}"
            assert (c, k) == (c3 + n * units, k3), f"r = {r}"
            assert cp - cp3 == n * len(last), f"r = {r}"


SWEEP_RULES = {"ref": (0, 1 << 2), "conway": (1 << 3, (1 << 2) | (1 << 3)),
               "highlife": ((1 << 3) | (1 << 6), (1 << 2) | (1 << 3))}


@pytest.mark.parametrize("seed", range(12))
def test_differential_sweep(pkg, oracle, monkeypatch, seed):
    """Seeded sweep of the kind of test_gpu_activity.test_differential_sweep: three
    rules, depths 8, 12 and 16, several steps; copy-through on, copy-through off and
    skip off agree with the oracle after every step."""
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
            make(pkg, monkeypatch, h, w, through=False, **cfg) as nocopy, \
            make(pkg, monkeypatch, h, w, skip=False, **cfg) as off:
        engines = (on, nocopy, off)
        for e in engines:
            e.load_packed(g0)
        want = g0
        for gens in chunks:
            want = oracle.bp_run(want, w, gens, rule)
            for e in engines:
                e.step(gens)
                assert (e.store_packed() == want).all(), (name, p, h, w, depth, rpw, gens)
        assert on.digest() == oracle.bp_digest(want, w)
        assert nocopy.activity_copied() == 0 and off.activity_copied() == 0
        assert off.activity()[1] == 0
        assert sum(on.activity()) == sum(nocopy.activity()) == sum(off.activity())
        # B/S2 is still when the second step starts: its second launch copies
        assert name != "ref" or on.activity_copied() > 0
        print(name, p, h, w, depth, rpw, chunks, on.activity(), on.activity_copied())


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
    events and GOL_DEV_ACTIVITY_SKIP=0: no unit copies; results are unchanged."""
    monkeypatch.delenv("GOL_DEV_ACTIVITY_SKIP", raising=False)
    monkeypatch.delenv("GOL_DEV_COPY_THROUGH", raising=False)
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


def test_one_load_exit(pkg, oracle, monkeypatch):
    """One step of 40 K generations on a field that is still from the start: launches
    1 and 2 store rows, launch 3 skips unit by unit, and launches 4 to 40 find that
    nobody stored a row in the launch before and leave at the first load; all 38
    count as skipped.  Then a glider is loaded: the next step computes around it."""
    h, w, rule = 333, 64 * 141 - 37, pkg.CONWAY
    g0 = empty(h, w)
    for r in range(20, h - 2, 64):
        for c in (100, 4500, w - 40):
            put(g0, r, c, BLOCK)
    units = plan(pkg, h, w, rule=rule)[0].shape[0]
    with make(pkg, monkeypatch, h, w, rule=rule) as e:
        got, (c, k, cp) = one_step(e, g0, 40 * K)
        assert (got == g0).all()
        assert (c, k, cp) == (2 * units, 38 * units, units)
        # the replayed graph: the same again, the counters add up
        e.step(40 * K)
        assert (e.store_packed() == g0).all()
        assert e.activity() == (4 * units, 76 * units) and e.activity_copied() == 2 * units
        g1 = put(g0.copy(), 150, 4400, GLIDER)
        got, (c, k, cp) = one_step(e, g1, 40 * K)
        assert (got == oracle.bp_run(g1, w, 40 * K, rule)).all()
        assert c + k == 40 * units and 0 < k < 38 * units
