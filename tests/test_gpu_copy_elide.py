"""GPU: copy elision in the copy pass (life_copy.hip, DESIGN §4 "Copy pass") against
the CPU oracle, against the same engine with the elision switched off
(GOL_DEV_COPY_ELIDE=0 at create) and against a model of which units it may leave.

The pass before a step's second launch and before its remainder launches moves the
rows of the calm units.  It now leaves a calm unit alone when the buffer it writes
already holds the unit's rows:
  (P) the unit probed through in the step's first launch and the pass goes before
      the second launch, whose output buffer was the first one's input;
  (S) every streak of the unit's neighbour list is >= 2 (a remainder launch);
  (R) the second and later launches of one remainder (3 = 2 + 1): every calm unit.
Such a unit counts in Engine.activity_elided() and nowhere else: the field and the
four other counters must be exactly those of the engine that copies every calm unit.
A wrong elision leaves the rows of two launches ago in the field.

`expected_elided` restates the three cases from the oracle's fields and
gol_plan_neighbours, as test_gpu_copy_through.py's `model` does for the calm sets and
test_gpu_still_probe.py's `may_probe` for the probe.  The kernel's streaks are at most
the model's, so its count is at most the model's, and equal to it where every unit
the model calls quiet stores nothing new in the kernel's wider comparison either (the
still fields, the patterns that settle early in the first launch).

Shapes, fields and engine settings are those of test_gpu_copy_pass.py and
test_gpu_still_probe.py.
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
SEEDS = (1 << 2, 0)
K = 16
SWITCHES = ("GOL_DEV_ACTIVITY_SKIP", "GOL_DEV_COPY_THROUGH", "GOL_DEV_STILL_EXIT",
            "GOL_DEV_STILL_PROBE", "GOL_DEV_COPY_PASS", "GOL_DEV_COPY_ELIDE")
REMAINDERS = {1: 1, 2: 1, 3: 2, 4: 1, 6: 1, 7: 1, 8: 1, 12: 1}  # depth -> launches


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


def make(pkg, monkeypatch, h, w, elide=True, probe=True, skip=True, **kw):
    """The switches are read at create, so each engine keeps what it was made with."""
    cfg = dict(BASE, rows_per_wave=64, tb_depth=K, device=0)
    cfg.update(kw)
    clear_switches(monkeypatch)
    if not skip:
        monkeypatch.setenv("GOL_DEV_ACTIVITY_SKIP", "0")
    if not probe:
        monkeypatch.setenv("GOL_DEV_STILL_PROBE", "0")
    if not elide:
        monkeypatch.setenv("GOL_DEV_COPY_ELIDE", "0")
    return pkg.Engine(h, w, **cfg)


def plan(pkg, h, w, **kw):
    cfg = dict(BASE, rows_per_wave=64, tb_depth=K)
    cfg.update(kw)
    return pkg.plan_neighbours(h, w, **cfg)


def counters(e):
    c, k = e.activity()
    return c, k, e.activity_copied(), e.activity_probed()


def one_step(e, g0, gens):
    e.load_packed(g0)
    e.reset_timing()
    e.step(gens)
    return e.store_packed(), counters(e), e.activity_elided()


def both(on, off, oracle, g0, w, gens, rule, msg=""):
    """One step on the engine with the elision and on the one without: both fields are
    the oracle's, the four existing counters agree, the second elides nothing.
    Returns the first engine's counters and its elided count."""
    want = oracle.bp_run(g0, w, gens, rule)
    got, cn, el = one_step(on, g0, gens)
    ref, co, el_off = one_step(off, g0, gens)
    assert (got == want).all(), f"elide on, {gens} generations {msg}"
    assert (ref == want).all(), f"elide off, {gens} generations {msg}"
    assert cn == co and el_off == 0, f"{gens} generations {msg}"
    return cn, el


def may_probe(oracle, g0, w, rule, depth, pl):
    """test_gpu_still_probe.may_probe: the units whose rectangles, dilated by depth - 1
    cells and clipped to the field, are the same in generations 0 and 1."""
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


def streaks_after(oracle, g0, w, rule, depth, launches, pl):
    """test_gpu_copy_through.model: the units' streaks after each of `launches`
    depth-`depth` launches of one step from g0 (quiet = generations depth - 1 and depth
    of the launch agree on the unit's rectangles)."""
    rects = pl[0]
    units = rects.shape[0]
    streak = np.zeros(units, dtype=np.int64)
    g, out = g0, []
    for _ in range(launches):
        prev = oracle.bp_run(g, w, depth - 1, rule)
        g = oracle.bp_run(prev, w, 1, rule)
        diff = g != prev
        quiet = np.ones(units, dtype=bool)
        for u in range(units):
            for r0, r1, q0, q1 in rects[u]:
                if r1 > r0 and diff[r0:r1, q0:q1].any():
                    quiet[u] = False
        streak = np.where(quiet, np.minimum(streak + 1, 255), 0)
        out.append(streak.copy())
    return out


def listed(pl, streak, least):
    """Units whose whole neighbour list has a streak of at least `least`."""
    _, offs, ids = pl
    return {u for u in range(len(offs) - 1)
            if offs[u + 1] > offs[u] and (streak[ids[offs[u]:offs[u + 1]]] >= least).all()}


def expected_elided(oracle, g0, w, rule, depth, gens, pl, probe=True):
    """(elided, calm and not held) summed over the passes of one step of `gens`
    generations from g0: the pass before launch 2 (P), before the first remainder
    launch (P if it is the step's second launch, else S) and the later launches of the
    remainder (R, every calm unit)."""
    launches, rem = gens // depth, gens % depth
    st = streaks_after(oracle, g0, w, rule, depth, launches, pl)
    probed = may_probe(oracle, g0, w, rule, depth, pl) if probe else set()
    elided = kept = 0
    if launches >= 2:
        calm = listed(pl, st[0], 1)
        elided += len(calm & probed)
        kept += len(calm - probed)
    if rem and launches >= 1:
        last = st[launches - 1]
        calm = listed(pl, last, 1)
        held = (calm & probed) if launches == 1 else listed(pl, last, 2)
        elided += len(held) + (REMAINDERS[rem] - 1) * len(calm)
        kept += len(calm - held)
    return elided, kept


def blocks_field(h, w, cols):
    g0 = empty(h, w)
    for r in range(20, h - 2, 64):
        for c in cols:
            put(g0, r, c, BLOCK)
    return g0


def probe_blocks_field(h, w):
    """test_gpu_still_probe.blocks_field: 2 x 2 blocks on all four borders, in the
    corners, in the masked last lane group and all over the half strip's pair units."""
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
        yield f"blocks-{w}", h, w, pkg.CONWAY, probe_blocks_field(h, w)


@pytest.mark.parametrize("case", range(6))
def test_still_field(pkg, oracle, monkeypatch, case):
    """test_gpu_still_probe.test_still_field's six fields, still from the start: no
    pass in a step of K; (P) before launch 2; (P) before a remainder that comes second;
    (P) then (S); with the probe off (S) alone, from the remainder."""
    name, h, w, rule, g0 = list(still_cases(pkg, oracle))[case]
    assert (oracle.bp_run(g0, w, 1, rule) == g0).all() and g0.any(), name
    pl = plan(pkg, h, w, rule=rule)
    u = pl[0].shape[0]
    with make(pkg, monkeypatch, h, w, rule=rule) as e, \
            make(pkg, monkeypatch, h, w, elide=False, rule=rule) as off:
        cn, el = both(e, off, oracle, g0, w, K, rule, name)
        assert cn == (u, 0, 0, u) and el == 0, name
        cn, el = both(e, off, oracle, g0, w, 6 * K + 8, rule, name)
        assert cn == (3 * u, 4 * u, 2 * u, u) and el == 2 * u, name
        assert e.digest() == oracle.bp_digest(g0, w)
        cn, el = both(e, off, oracle, g0, w, K + 8, rule, name)
        assert cn == (2 * u, 0, u, u) and el == u, name
        cn, el = both(e, off, oracle, g0, w, 2 * K + 8, rule, name)
        assert cn == (3 * u, 0, 2 * u, u) and el == 2 * u, name
        for gens in (K, 6 * K + 8, K + 8, 2 * K + 8):
            assert expected_elided(oracle, g0, w, rule, K, gens, pl)[0] == \
                {K: 0, K + 8: u}.get(gens, 2 * u)
    with make(pkg, monkeypatch, h, w, probe=False, rule=rule) as e, \
            make(pkg, monkeypatch, h, w, probe=False, elide=False, rule=rule) as off:
        cn, el = both(e, off, oracle, g0, w, 6 * K + 8, rule, name)
        assert cn == (3 * u, 4 * u, 2 * u, 0) and el == u, name
        cn, el = both(e, off, oracle, g0, w, K + 8, rule, name)
        assert cn == (2 * u, 0, u, 0) and el == 0, name


def test_calm_not_probed(pkg, oracle, monkeypatch):
    """test_gpu_still_probe.test_settles_late's field: patterns that become still
    lifes 1 and 2 generations into launch 1.  The units within K - 1 cells of them fail
    the probe, are calm at launch 2 and must be copied; the others are elided.  From
    generation 2 on nothing changes, so the kernel's streaks are the model's and the
    counts are exact, launch by launch: the pass of a step of 2K, then that pass and
    the remainder's (S: every unit)."""
    h, w, rule = 333, 64 * 127, pkg.CONWAY
    g0 = empty(h, w)
    put(g0, 30, 300, [(0, 0), (0, 1), (1, 0)])
    put(g0, 200, 5000, [(0, 0), (0, 1), (0, 2), (0, 3)])
    pl = plan(pkg, h, w, rule=rule)
    u = pl[0].shape[0]
    probed = may_probe(oracle, g0, w, rule, K, pl)
    calm1 = listed(pl, streaks_after(oracle, g0, w, rule, K, 1, pl)[0], 1)
    # calm and not probed: without such a unit the test checks nothing
    assert len(calm1 - probed) > 0 and len(calm1 & probed) > 0
    assert calm1 == set(range(u))
    with make(pkg, monkeypatch, h, w, rule=rule) as e, \
            make(pkg, monkeypatch, h, w, elide=False, rule=rule) as off:
        cn, el = both(e, off, oracle, g0, w, 2 * K, rule)
        assert cn == (2 * u, 0, u, len(probed))
        assert el == len(calm1 & probed) == expected_elided(oracle, g0, w, rule, K, 2 * K, pl)[0]
        for n in (2, 3, 10):
            cn, el = both(e, off, oracle, g0, w, K * n + 8, rule)
            assert cn[:2] == (3 * u, (n - 2) * u) and cn[3] == len(probed)
            want, kept = expected_elided(oracle, g0, w, rule, K, K * n + 8, pl)
            assert el == want == len(calm1 & probed) + u and kept == len(calm1 - probed)


def settles_between(oracle, rule, lo, hi):
    """Seeded search through the oracle: a random 6 x 6 box in a 64 x 64 field whose
    first generation t with s(t) == s(t + 1) lies in [lo, hi].  Returns the box's cells
    and t."""
    for seed in range(64):
        box = np.random.default_rng(7000 + seed).random((6, 6)) < 0.5
        cells = [(int(r), int(c)) for r, c in zip(*np.nonzero(box))]
        g = put(empty(64, 64), 29, 29, cells)
        for t in range(hi + 1):
            nxt = oracle.bp_run(g, 64, 1, rule)
            if (nxt == g).all():
                break
            g = nxt
        else:
            continue
        if lo <= t <= hi:
            return cells, t
    raise AssertionError("no pattern found")


def test_calm_not_still_at_remainder(pkg, oracle, monkeypatch):
    """A B3/S23 pattern that goes still between generations K + 2 and 2K - 2, across a
    row-block seam and away from the strip borders: its units compute in launches 1
    and 2, end launch 2 quiet (streak 1) and are calm but not still at the remainder
    of a step of 2K + r.  The remainder's output buffer holds s(K) != s(2K) there, so
    eliding them would show in the field."""
    h, w, rule = 333, 64 * 141 - 37, pkg.CONWAY
    cells, t = settles_between(oracle, rule, K + 2, 2 * K - 2)
    assert K + 2 <= t <= 2 * K - 2
    pl = plan(pkg, h, w, rule=rule)
    rects = pl[0]
    u = rects.shape[0]
    # a unit of the second strip with a row block below it: the seam is its last row
    top = next(x for x in range(u) if rects[x][0][2] > 0 and 64 <= rects[x][0][1] < h - 64
               and rects[x][1][1] <= rects[x][1][0])
    seam, q0, q1 = int(rects[top][0][1]), int(rects[top][0][2]), int(rects[top][0][3])
    col = 64 * ((q0 + q1) // 2)
    assert 64 * q0 + 64 <= col <= 64 * q1 - 64
    g0 = blocks_field(h, w, (100, w - 40))
    put(g0, seam - 3, col, cells)
    # the property: s(K) and s(2K) differ on both sides of the seam's units, s(2K) is still
    sK, s2K = oracle.bp_run(g0, w, K, rule), oracle.bp_run(g0, w, 2 * K, rule)
    assert (sK != s2K).any() and (oracle.bp_run(s2K, w, 1, rule) == s2K).all()
    changed = [x for x in range(u) for r0, r1, a, b in rects[x]
               if r1 > r0 and (sK[r0:r1, a:b] != s2K[r0:r1, a:b]).any()]
    st = streaks_after(oracle, g0, w, rule, K, 2, pl)
    calm2, still2 = listed(pl, st[1], 1), listed(pl, st[1], 2)
    assert changed and all(x in calm2 and x not in still2 for x in changed)
    probed = may_probe(oracle, g0, w, rule, K, pl)
    assert not (set(changed) & probed)
    with make(pkg, monkeypatch, h, w, rule=rule) as e, \
            make(pkg, monkeypatch, h, w, elide=False, rule=rule) as off:
        for r in sorted(REMAINDERS):
            cn, el = both(e, off, oracle, g0, w, 2 * K + r, rule, f"r = {r}")
            want, kept = expected_elided(oracle, g0, w, rule, K, 2 * K + r, pl)
            print(r, cn, el, want, kept)
            assert kept >= len(set(changed)) and 0 < el <= want, f"r = {r}"


@pytest.mark.parametrize("w", [64 * 126, 64 * 141 - 37])
def test_beside_compute(pkg, oracle, monkeypatch, w):
    """The wake-up field (blocks plus gliders crossing a row-block and a strip
    boundary), steps of 2K to 6K and 2K + 7: elided units, copied units and computing
    units side by side."""
    h, rule = 525, pkg.CONWAY
    g0 = blocks_field(h, w, (100, 2000, 4500, 6000, w - 40))
    put(g0, 40, 4008, GLIDER)
    put(g0, 168, 4968, GLIDER)
    pl = plan(pkg, h, w, rule=rule)
    u = pl[0].shape[0]
    with make(pkg, monkeypatch, h, w, rule=rule) as e, \
            make(pkg, monkeypatch, h, w, elide=False, rule=rule) as off:
        for gens in [K * n for n in range(2, 7)] + [2 * K + 7]:
            cn, el = both(e, off, oracle, g0, w, gens, rule)
            want, _ = expected_elided(oracle, g0, w, rule, K, gens, pl)
            print(gens, cn, el, want)
            assert 0 < el <= want and el <= cn[2] < (gens // K) * u, gens


@pytest.mark.parametrize("w", [64 * 141 - 37, 64 * 126 + 1])
def test_edges(pkg, oracle, monkeypatch, w):
    """test_gpu_copy_pass.test_edges' field: half-strip pair units with two row blocks,
    a height that is no multiple of the block, blocks and blinkers on all four borders
    and in the masked last lane group."""
    h, rule, n = 64 * 9 + 13, pkg.CONWAY, 6
    g0 = empty(h, w)
    for r, c in ((0, 0), (0, w - 2), (h - 2, 0), (h - 2, w - 2), (0, 5000), (h - 2, 2500),
                 (400, 0), (150, w - 2)):
        put(g0, r, c, BLOCK)
    for r, c in ((1, 2000), (h - 2, 6000), (300, 0), (500, w - 3)):
        put(g0, r, c, BLINKER)
    pl = plan(pkg, h, w, rule=rule)
    if w == 64 * 141 - 37:  # the half strip: units with two row blocks
        assert any(r[0][1] > r[0][0] and r[1][1] > r[1][0] for r in pl[0])
    with make(pkg, monkeypatch, h, w, rule=rule) as e, \
            make(pkg, monkeypatch, h, w, elide=False, rule=rule) as off:
        for gens in (K * n + 7, 2 * K, 2 * K + 7, K + 3):
            cn, el = both(e, off, oracle, g0, w, gens, rule)
            want, _ = expected_elided(oracle, g0, w, rule, K, gens, pl)
            assert 0 < el <= want and cn[2] > 0, gens


@pytest.mark.parametrize("glider", [False, True])
def test_remainder_3(pkg, oracle, monkeypatch, glider):
    """Steps of 3K + r for the shipped remainder depths; r = 3 is two remainder
    launches (2 + 1): the second takes no tiles at all and elides every calm unit (R)."""
    h, w, rule = 333, 64 * 141 - 37, pkg.CONWAY
    g0 = blocks_field(h, w, (100, 4500, w - 40))
    if glider:
        put(g0, 150, 4400, GLIDER)
    pl = plan(pkg, h, w, rule=rule)
    u = pl[0].shape[0]
    with make(pkg, monkeypatch, h, w, rule=rule) as e, \
            make(pkg, monkeypatch, h, w, elide=False, rule=rule) as off:
        c3, e3 = both(e, off, oracle, g0, w, 3 * K, rule)
        seen = {}
        for r in (1, 7, 8, 12, 2, 4, 6, 3):
            cn, el = both(e, off, oracle, g0, w, 3 * K + r, rule, f"r = {r}")
            assert (cn[0], cn[1]) == (c3[0] + REMAINDERS[r] * u, c3[1]), f"r = {r}"
            seen[r] = (el - e3, (cn[2] - c3[2]) // REMAINDERS[r])
        print(glider, e3, seen)
        # one remainder launch: (S) of the calm units; r = 3: the second launch's pass
        # also elides every calm unit, the ones the first one's pass had to copy too
        calm = seen[2][1]
        assert all(seen[r] == seen[2] for r in (1, 7, 8, 12, 4, 6))
        assert seen[3] == (seen[2][0] + calm, calm)
        if not glider:
            assert e3 == u and seen[2] == (u, u)
        else:
            assert 0 < seen[2][0] <= calm < u
        # K + 3: the first remainder launch is the step's second launch (P), then (R)
        cn, el = both(e, off, oracle, g0, w, K + 3, rule)
        assert 0 < el <= cn[2] and (glider or el == 2 * u)


def test_replay(pkg, oracle, monkeypatch):
    """A step of 40 K + 8 on a still field, captured and replayed twice; a glider is
    loaded and the same graph replayed; the still field again.  A step of exactly K
    (no pass, it consumes no flag) sits between two longer steps.  No probed flag of an
    earlier step survives: every first launch that probes rewrites every unit's."""
    h, w, rule = 333, 64 * 141 - 37, pkg.CONWAY
    g0 = blocks_field(h, w, (100, 4500, w - 40))
    g1 = put(g0.copy(), 150, 4400, GLIDER)
    pl = plan(pkg, h, w, rule=rule)
    u = pl[0].shape[0]
    gens = 40 * K + 8
    with make(pkg, monkeypatch, h, w, rule=rule) as e, \
            make(pkg, monkeypatch, h, w, elide=False, rule=rule) as off:
        cn, el = both(e, off, oracle, g0, w, gens, rule)
        assert cn == (3 * u, 38 * u, 2 * u, u) and el == 2 * u
        for i in range(2):
            for x in (e, off):
                x.step(gens)
                assert (x.store_packed() == g0).all()
            assert counters(e) == counters(off) == (3 * u * (i + 2), 38 * u * (i + 2),
                                                    2 * u * (i + 2), u * (i + 2))
            assert e.activity_elided() == 2 * u * (i + 2) and off.activity_elided() == 0
        cn, el = both(e, off, oracle, g1, w, gens, rule, "glider")
        probed = may_probe(oracle, g1, w, rule, K, pl)
        assert cn[3] == len(probed) < u and 0 < el < 2 * u
        # a step of K on the glider's field (every flag rewritten, none read), then the
        # still field: its own flags count
        cn, el = both(e, off, oracle, g1, w, K, rule, "glider, K")
        assert el == 0 and cn[3] == len(probed)
        cn, el = both(e, off, oracle, g0, w, gens, rule, "still again")
        assert cn == (3 * u, 38 * u, 2 * u, u) and el == 2 * u
        # ... and the other way round: all flags 1, then the glider's field
        cn, el = both(e, off, oracle, g0, w, K, rule)
        assert el == 0 and cn == (u, 0, 0, u)
        cn, el = both(e, off, oracle, g1, w, 2 * K, rule, "glider after still")
        want, _ = expected_elided(oracle, g1, w, rule, K, 2 * K, pl)
        assert cn[3] == len(probed) and 0 < el <= want < u


OFF_CASES = {
    "handoff": dict(tb_depth=8, rows_per_wave=22, handoff=2, streams=1, resident=1),
    "streams": dict(tb_depth=16, streams=2, resident=1),
    "resident": dict(),
    "timing": dict(BASE, tb_depth=16, rows_per_wave=64),
    "skip_off": dict(BASE, tb_depth=16, rows_per_wave=64),
}


@pytest.mark.parametrize("case", sorted(OFF_CASES))
def test_off_where_the_pass_is_off(pkg, oracle, monkeypatch, case):
    """The five cases of test_gpu_copy_pass.test_off_where_the_skip_is_off, in which no
    pass is enqueued: nothing is elided; results are unchanged."""
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
        assert (e.store_packed() == oracle.bp_run(g0, w, 16 * 6 + 7, rule)).all()
        assert e.activity_elided() == 0 and e.activity_copied() == 0


def test_off_with_the_copy_pass(pkg, oracle, monkeypatch):
    """GOL_DEV_COPY_PASS=0: the stencil kernel's own copy loop moves the rows; there is
    no pass to leave any out."""
    h, w, rule = 333, 64 * 127, pkg.CONWAY
    g0 = blocks_field(h, w, (100, 4500, w - 40))
    clear_switches(monkeypatch)
    monkeypatch.setenv("GOL_DEV_COPY_PASS", "0")
    with pkg.Engine(h, w, rule=rule, **dict(BASE, rows_per_wave=64, tb_depth=K, device=0)) as e:
        got, cn, el = one_step(e, g0, 6 * K + 8)
        u = plan(pkg, h, w, rule=rule)[0].shape[0]
        assert (got == g0).all() and cn == (3 * u, 4 * u, 2 * u, u) and el == 0


SWEEP_RULES = {"ref": (0, 1 << 2), "conway": (1 << 3, (1 << 2) | (1 << 3)),
               "highlife": ((1 << 3) | (1 << 6), (1 << 2) | (1 << 3))}


@pytest.mark.parametrize("seed", range(12))
def test_differential_sweep(pkg, oracle, monkeypatch, seed):
    """test_gpu_copy_pass.test_differential_sweep's generator (three rules, depths 8, 12
    and 16, rows per wavefront 48, 61, 64 and 90, three steps): elide on, elide off and
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
            make(pkg, monkeypatch, h, w, elide=False, **cfg) as noelide, \
            make(pkg, monkeypatch, h, w, skip=False, **cfg) as off:
        engines = (on, noelide, off)
        for e in engines:
            e.load_packed(g0)
        want = g0
        for gens in chunks:
            want = oracle.bp_run(want, w, gens, rule)
            for e in engines:
                e.step(gens)
                assert (e.store_packed() == want).all(), (name, p, h, w, depth, rpw, gens)
        assert on.digest() == oracle.bp_digest(want, w)
        assert counters(on) == counters(noelide)
        assert noelide.activity_elided() == 0 and off.activity_elided() == 0
        assert on.activity_elided() <= on.activity_copied()
        # B/S2 is still when the second step starts: its launch 2 finds every unit held
        assert name != "ref" or on.activity_elided() > 0
        print(name, p, h, w, depth, rpw, chunks, counters(on), on.activity_elided())


def test_seeds_depth_12(pkg, oracle, monkeypatch):
    """Seeds (B2/S), K = 12: a domino explodes while the rest of the field is empty;
    the empty units far from it are held before launch 2 and before the remainder."""
    h, w, depth = 333, 64 * 141 - 37, 12
    g0 = put(empty(h, w), 160, 4500, [(0, 0), (0, 1)])
    pl = plan(pkg, h, w, rule=SEEDS, tb_depth=depth)
    with make(pkg, monkeypatch, h, w, rule=SEEDS, tb_depth=depth) as e, \
            make(pkg, monkeypatch, h, w, elide=False, rule=SEEDS, tb_depth=depth) as off:
        for gens in (2 * depth, 2 * depth + 7, 3 * depth + 3, depth + 8):
            cn, el = both(e, off, oracle, g0, w, gens, SEEDS)
            want, _ = expected_elided(oracle, g0, w, SEEDS, depth, gens, pl)
            assert 0 < el <= want, gens


def test_torus(pkg, oracle, monkeypatch):
    """test_gpu_copy_pass.test_torus' engine (300 x 500, B3/S23 blocks, 300 generations
    against tests/torus_ref.py), elide on against off: the inner engine's field is the
    padded one the wrap kernel leaves, and (P) relies on its normal form."""
    h, w, rule, gens = 300, 500, (1 << 3, (1 << 2) | (1 << 3)), 300
    g0 = blocks_field(h, w, (10, 250, w - 2))  # (the last block wraps around the edge)
    g0[:, -1] &= np.uint64((1 << (w % 64)) - 1)
    bits = torus_ref.unpack(g0, w)
    bits[20:22, 0] = 1  # ... its other half
    start = torus_ref.pack(bits)
    want = torus_ref.torus_run(oracle, start, w, gens, rule, chunk=64)
    seen = {}
    for elide in (True, False):
        clear_switches(monkeypatch)
        if not elide:
            monkeypatch.setenv("GOL_DEV_COPY_ELIDE", "0")
        with pkg.Engine(h, w, rule=rule, semantics=pkg.SEM_TORUS, tb_depth=8, resident=1,
                        handoff=1, halo_depth=64) as e:
            e.load_packed(start)
            e.reset_timing()
            e.step(gens)
            assert (e.store_packed() == want).all()
            assert e.digest() == oracle.bp_digest(want, w)
            seen[elide] = counters(e), e.activity_elided()
    assert seen[True][0] == seen[False][0] and seen[False][1] == 0
    assert 0 < seen[True][1] <= seen[True][0][2]
