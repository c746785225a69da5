"""GPU: the probe pass before a step's first launch (life_probe.hip, DESIGN §4 "Probe
pass") next to the same engine with GOL_DEV_PROBE_PASS=0, against the CPU oracle, and
against a model of which units the pass leaves sure.

The pass runs one generation over line-aligned tiles and marks every unit with a tile
that changes among the tiles meeting its rectangles dilated by K - 1 cells; the first
launch takes every unmarked (sure) unit through on that word and counts it in
Engine.activity_pass_probed(), and every other unit probes in the kernel as it does
without the pass.  So fields and the five older counters equal those of the engine
without the pass, and activity_pass_probed() equals the model's count of sure units:
`sure` restates the condition from the oracle's generations 0 and 1, gol_plan_neighbours'
rectangles and the tile shape the library reports.

Shapes and engine settings are those of test_gpu_still_probe.py.
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
HIGHLIFE = ((1 << 3) | (1 << 6), (1 << 2) | (1 << 3))
K = 16
SWITCHES = ("GOL_DEV_ACTIVITY_SKIP", "GOL_DEV_COPY_THROUGH", "GOL_DEV_STILL_EXIT",
            "GOL_DEV_STILL_PROBE", "GOL_DEV_COPY_PASS", "GOL_DEV_COPY_ELIDE",
            "GOL_DEV_PROBE_PASS")


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


def make(pkg, monkeypatch, h, w, ppass=True, **kw):
    cfg = dict(BASE, rows_per_wave=64, tb_depth=K, device=0)
    cfg.update(kw)
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if not ppass:
        monkeypatch.setenv("GOL_DEV_PROBE_PASS", "0")
    return pkg.Engine(h, w, **cfg)


def plan(pkg, h, w, **kw):
    cfg = dict(BASE, rows_per_wave=64, tb_depth=K)
    cfg.update(kw)
    return pkg.plan_neighbours(h, w, **cfg)[0], pkg.plan_probe_tiles(h, w, **cfg)


def diff_bits(oracle, g0, w, rule):
    g1 = oracle.bp_run(g0, w, 1, rule)
    return np.unpackbits((g0 ^ g1).view(np.uint8), axis=1, bitorder="little")


def may_probe(diff, h, w, depth, rects):
    """test_gpu_still_probe.may_probe: generations 0 and 1 agree on each of the unit's
    rectangles dilated by depth - 1 cells and clipped to the field."""
    d = depth - 1
    ok = set()
    for u in range(rects.shape[0]):
        if not any(diff[max(0, r0 - d):min(h, r1 + d), max(0, 64 * q0 - d):min(w, 64 * q1 + d)].any()
                   for r0, r1, q0, q1 in rects[u] if r1 > r0 and q1 > q0):
            ok.add(u)
    return ok


def unit_tiles(rects, u, h, w, depth, tr, tw):
    """(row chunk, column segment) of the tiles that meet unit u's rectangles dilated
    by depth - 1 cells and clipped to the field."""
    d, out = depth - 1, set()
    for r0, r1, q0, q1 in rects[u].tolist():
        if r1 > r0 and q1 > q0:
            a0, a1 = max(0, r0 - d), min(h, r1 + d)
            c0, c1 = max(0, 64 * q0 - d), min(w, 64 * q1 + d)
            out |= {(i, c) for i in range(a0 // tr, (a1 - 1) // tr + 1)
                    for c in range(c0 // (64 * tw), (c1 - 1) // (64 * tw) + 1)}
    return out


def dirty_tiles(diff, tr, tw):
    rows, cols = np.nonzero(diff)
    return set(zip((rows // tr).tolist(), (cols // (64 * tw)).tolist()))


def sure(diff, h, w, depth, rects, tr, tw, dirty=None):
    """The units none of whose tiles holds a cell that differs between generations 0
    and 1."""
    dirty = dirty_tiles(diff, tr, tw) if dirty is None else dirty
    return {u for u in range(rects.shape[0])
            if not (unit_tiles(rects, u, h, w, depth, tr, tw) & dirty)}


def local_dirty(oracle, g0, w, rule, tiles, tr, tw):
    """Of `tiles`, those that change when evaluated alone, everything outside dead."""
    out = set()
    for i, c in tiles:
        sub = g0[i * tr:(i + 1) * tr, c * tw:(c + 1) * tw].copy()
        sw = min(w, 64 * (c + 1) * tw) - 64 * c * tw
        if (oracle.bp_run(sub, sw, 1, rule) != sub).any():
            out.add((i, c))
    return out


def counters(e):
    c, k = e.activity()
    return (c, k, e.activity_copied(), e.activity_probed(), e.activity_elided())


def one_step(e, g0, gens):
    e.load_packed(g0)
    e.reset_timing()
    e.step(gens)
    return e.store_packed(), counters(e), e.activity_pass_probed()


def both(on, off, oracle, g0, w, gens, rule):
    """One step from g0 on both engines: the fields equal the oracle's, the five older
    counters agree, the engine without the pass counts none.  Returns the counters
    and the pass's count."""
    got, cn, pp = one_step(on, g0, gens)
    ref, co, po = one_step(off, g0, gens)
    want = oracle.bp_run(g0, w, gens, rule)
    assert (got == want).all() and (ref == want).all(), gens
    assert cn == co and po == 0, (gens, cn, co, po)
    assert pp <= cn[3]
    return cn, pp


def blocks_field(h, w):
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
        yield f"blocks-{w}", h, w, pkg.CONWAY, blocks_field(h, w)


@pytest.mark.parametrize("case", range(6))
def test_still_field(pkg, oracle, monkeypatch, case):
    """A still field: every unit is sure, in a step of K and in one of 6 K + 8, with
    the exact counters of test_gpu_still_probe.test_still_field."""
    name, h, w, rule, g0 = list(still_cases(pkg, oracle))[case]
    assert (oracle.bp_run(g0, w, 1, rule) == g0).all() and g0.any(), name
    rects, (tr, tw, ncol, table) = plan(pkg, h, w, rule=rule)
    units = rects.shape[0]
    assert table is not None
    with make(pkg, monkeypatch, h, w, rule=rule) as e, \
            make(pkg, monkeypatch, h, w, ppass=False, rule=rule) as off:
        cn, pp = both(e, off, oracle, g0, w, K, rule)
        assert cn[:4] == (units, 0, 0, units) and pp == units, name
        cn, pp = both(e, off, oracle, g0, w, 6 * K + 8, rule)
        assert cn[:4] == (3 * units, 4 * units, 2 * units, units) and pp == units, name
        assert e.digest() == oracle.bp_digest(g0, w)


def edge_case(pkg, oracle, side):
    """A field whose only change within some unit's tiles shows across a tile edge:
    (h, w, rule, depth, rows_per_wave, g0, unit)."""
    if side in ("left", "right"):
        # Seeds, a vertical domino in the first (last) column of a tile: births in the
        # last (first) column of the tile beside it
        h, w, rule, depth, rpw = 333, 64 * 141 - 37, SEEDS, 12, 64
        col = 64 * 64 if side == "left" else 64 * 64 - 1
        g0 = put(empty(h, w), 100, col, [(0, 0), (1, 0)])
        seg = 0 if side == "left" else 1  # the tile column that sees births only
    else:
        # B3/S23, a blinker in the row above (below) a tile: a birth in the tile's
        # first (last) row.  Row blocks of 63 (65) rows put the first (last) row of a
        # unit's dilated rectangle on that tile's edge
        h, w, rule, depth = 333, 64 * 141 - 37, (1 << 3, (1 << 2) | (1 << 3)), 16
        rpw = 63 if side == "above" else 65
        row = 63 - 15 - 1 if side == "above" else 65 + 15
        g0 = put(empty(h, w), row, 1000, BLINKER)
        seg = None
    return h, w, rule, depth, rpw, g0, seg


@pytest.mark.parametrize("side", ["above", "below", "left", "right"])
def test_tile_edges(pkg, oracle, monkeypatch, side):
    """The evidence of a change lies across a tile edge, on each of the four sides:
    some unit's tiles include the tile that changes and not the tile that holds the
    live cells.  The premise is asserted: the model says that unit is not sure (in the
    vertical cases one such unit is not in may_probe either; in the horizontal ones a
    tile holds whole 64-column words, so a rectangle dilated by K - 1 < 64 cells that
    reaches the cell that changes reaches the tile beside it too), while its tiles
    evaluated alone, with dead neighbours, would pass it."""
    h, w, rule, depth, rpw, g0, seg = edge_case(pkg, oracle, side)
    cfg = dict(rule=rule, tb_depth=depth, rows_per_wave=rpw)
    rects, (tr, tw, ncol, table) = plan(pkg, h, w, **cfg)
    assert table is not None
    diff = diff_bits(oracle, g0, w, rule)
    dirty = dirty_tiles(diff, tr, tw)
    ok = sure(diff, h, w, depth, rects, tr, tw)
    live_rows, live_cols = np.nonzero(np.unpackbits(g0.view(np.uint8), axis=1, bitorder="little"))
    live = set(zip((live_rows // tr).tolist(), (live_cols // (64 * tw)).tolist()))
    found = []
    for u in range(rects.shape[0]):
        tiles = unit_tiles(rects, u, h, w, depth, tr, tw)
        if (tiles & dirty) and not (tiles & live) and \
                not local_dirty(oracle, g0, w, rule, tiles & dirty, tr, tw):
            found.append(u)
    assert found and not (set(found) & ok), side
    if side in ("above", "below"):  # the one whose columns hold the birth
        assert set(found) - may_probe(diff, h, w, depth, rects), side
    with make(pkg, monkeypatch, h, w, **cfg) as e, \
            make(pkg, monkeypatch, h, w, ppass=False, **cfg) as off:
        cn, pp = both(e, off, oracle, g0, w, depth, rule)
        assert pp == len(ok) and cn[3] == len(may_probe(diff, h, w, depth, rects)), side
        assert 0 < pp < rects.shape[0]


def test_change_outside_the_dilated_rectangle(pkg, oracle, monkeypatch):
    """A blinker in a tile of a unit, more than K cells from the unit's rectangles: the
    unit is not sure, yet the kernel's probe takes it through: `probed` counts it,
    `pass_probed` does not."""
    h, w, rule = 333, 64 * 141 - 37, pkg.CONWAY
    g0 = put(empty(h, w), 160, 64 * 63 + 40, BLINKER)  # word 63: strip 1's, tile column 0
    rects, (tr, tw, ncol, table) = plan(pkg, h, w, rule=rule)
    diff = diff_bits(oracle, g0, w, rule)
    ok, may = sure(diff, h, w, K, rects, tr, tw), may_probe(diff, h, w, K, rects)
    assert ok < may and len(may) < rects.shape[0]
    with make(pkg, monkeypatch, h, w, rule=rule) as e, \
            make(pkg, monkeypatch, h, w, ppass=False, rule=rule) as off:
        for gens in (K, 3 * K + 5):
            cn, pp = both(e, off, oracle, g0, w, gens, rule)
            assert cn[3] == len(may) and pp == len(ok), gens


@pytest.mark.parametrize("w", [64 * 126, 64 * 141 - 37])
def test_wake_up(pkg, oracle, monkeypatch, w):
    """test_gpu_still_probe.test_wake_up's field (blocks and two gliders), one step of
    K n generations for n = 1..6: sure units beside units that fail, the counters of
    every launch those of the engine without the pass."""
    h, rule = 525, pkg.CONWAY
    g0 = empty(h, w)
    for r in range(20, h - 2, 64):
        for c in (100, 2000, 4500, 6000, w - 40):
            put(g0, r, c, BLOCK)
    put(g0, 40, 4008, GLIDER)
    put(g0, 168, 4968, GLIDER)
    rects, (tr, tw, ncol, table) = plan(pkg, h, w, rule=rule)
    diff = diff_bits(oracle, g0, w, rule)
    ok, may = sure(diff, h, w, K, rects, tr, tw), may_probe(diff, h, w, K, rects)
    assert 0 < len(ok) <= len(may) < rects.shape[0]
    with make(pkg, monkeypatch, h, w, rule=rule) as e, \
            make(pkg, monkeypatch, h, w, ppass=False, rule=rule) as off:
        for n in range(1, 7):
            cn, pp = both(e, off, oracle, g0, w, K * n, rule)
            assert cn[3] == len(may) and pp == len(ok), n


@pytest.mark.parametrize("name", ["ref", "conway", "highlife"])
def test_soup(pkg, oracle, monkeypatch, name):
    """A p = 0.5 field: every tile changes, no unit is sure, the fields are the
    oracle's."""
    rule = {"ref": pkg.REF_RULE, "conway": pkg.CONWAY, "highlife": HIGHLIFE}[name]
    depth = 12 if name == "highlife" else K
    h, w = 333, 64 * 141 - 37
    g0 = random_field(h, w, 0.5, 11)
    with make(pkg, monkeypatch, h, w, rule=rule, tb_depth=depth) as e, \
            make(pkg, monkeypatch, h, w, ppass=False, rule=rule, tb_depth=depth) as off:
        cn, pp = both(e, off, oracle, g0, w, depth, rule)
        assert pp == 0 and cn[3] == 0
        both(e, off, oracle, g0, w, 3 * depth + 5, rule)


def test_captured_step(pkg, oracle, monkeypatch):
    """A captured step of 40 K + 8 replayed on a still field, a step of K, then the
    same captured step on a field in motion, next to an engine without the pass driven
    through the same sequence: after every step the fields are the oracle's, the five
    older counters agree and the pass's count is the model's.  No word of an earlier
    step survives."""
    h, w, rule, gens = 333, 64 * 141 - 37, pkg.CONWAY, 40 * K + 8
    g0 = empty(h, w)
    for r in range(20, h - 2, 64):
        for c in (100, 4500, w - 40):
            put(g0, r, c, BLOCK)
    g1 = put(g0.copy(), 150, 4400, GLIDER)
    rects, (tr, tw, ncol, table) = plan(pkg, h, w, rule=rule)
    units = rects.shape[0]
    with make(pkg, monkeypatch, h, w, rule=rule) as e, \
            make(pkg, monkeypatch, h, w, ppass=False, rule=rule) as off:

        def step_both(n, want, tag):
            for eng in (e, off):
                eng.step(n)
            assert (e.store_packed() == want).all() and (off.store_packed() == want).all(), tag
            assert counters(e) == counters(off) and off.activity_pass_probed() == 0, tag

        for eng in (e, off):
            eng.load_packed(g0)
            eng.reset_timing()
        for i in range(3):  # plain, capture, replay
            step_both(gens, g0, i)
            assert e.activity_pass_probed() == (i + 1) * units == e.activity_probed()
        step_both(K, g0, "K")
        assert e.activity_pass_probed() == 4 * units
        for eng in (e, off):
            eng.load_packed(g1)
            eng.reset_timing()
        want = g1
        for i in range(2):
            diff = diff_bits(oracle, want, w, rule)
            ok = sure(diff, h, w, K, rects, tr, tw)
            before = e.activity_pass_probed()
            want = oracle.bp_run(want, w, gens, rule)
            step_both(gens, want, ("moving", i))
            assert e.activity_pass_probed() - before == len(ok) < units, i
        # ... and back on the still field
        cn, pp = both(e, off, oracle, g0, w, gens, rule)
        assert pp == units == cn[3]


def test_writes_between_steps(pkg, oracle, monkeypatch):
    """load_packed and write_rect between steps: the next step's pass sees the field
    as written."""
    h, w, rule = 333, 64 * 141 - 37, pkg.CONWAY
    g0 = empty(h, w)
    for r in range(20, h - 2, 64):
        for c in (100, 4500, w - 40):
            put(g0, r, c, BLOCK)
    rects, (tr, tw, ncol, table) = plan(pkg, h, w, rule=rule)
    units = rects.shape[0]
    with make(pkg, monkeypatch, h, w, rule=rule) as e, \
            make(pkg, monkeypatch, h, w, ppass=False, rule=rule) as off:
        cn, pp = both(e, off, oracle, g0, w, 2 * K, rule)
        assert pp == units
        win = put(np.zeros((3, 1), dtype=np.uint64), 0, 0, GLIDER)
        want = g0
        for i, (y, x) in enumerate(((200, 64 * 62 + 30), (60, 64 * 127 + 61))):
            for eng in (e, off):
                eng.write_rect(y, x, win, 3, pkg.RECT_OR)
            want = put(want.copy(), y, x, GLIDER)
            ok = sure(diff_bits(oracle, want, w, rule), h, w, K, rects, tr, tw)
            before = e.activity_pass_probed()
            for eng in (e, off):
                eng.step(2 * K + 3)
            want = oracle.bp_run(want, w, 2 * K + 3, rule)
            assert (e.store_packed() == want).all() and (off.store_packed() == want).all(), i
            assert e.activity_pass_probed() - before == len(ok) < units, i
        assert counters(e) == counters(off) and off.activity_pass_probed() == 0
        cn, pp = both(e, off, oracle, g0, w, K, rule)
        assert pp == units


OFF_CASES = {
    "handoff": dict(tb_depth=8, rows_per_wave=22, handoff=2, streams=1, resident=1),
    "streams": dict(tb_depth=16, streams=2, resident=1),
    "timing": dict(BASE, tb_depth=16, rows_per_wave=64),
    "skip_off": dict(BASE, tb_depth=16, rows_per_wave=64),
    "probe_off": dict(BASE, tb_depth=16, rows_per_wave=64),
    "slot_overflow": dict(BASE, tb_depth=16, rows_per_wave=8),
}


@pytest.mark.parametrize("case", sorted(OFF_CASES))
def test_off_where_no_pass_runs(pkg, oracle, monkeypatch, case):
    """Hand-off plans, multi-stream engines, timed launches, the skip or the probe
    switched off, and a plan whose tiles overflow the table's slots, each next to the
    same engine with GOL_DEV_PROBE_PASS=0: the counter stays 0, the results are the
    oracle's and the five older counters agree."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if case == "skip_off":
        monkeypatch.setenv("GOL_DEV_ACTIVITY_SKIP", "0")
    if case == "probe_off":
        monkeypatch.setenv("GOL_DEV_STILL_PROBE", "0")
    h, w, rule = 600, 64 * 127, pkg.CONWAY
    g0 = empty(h, w)
    for r in range(20, h - 2, 64):
        put(g0, r, 100, BLOCK)
    put(g0, 200, 3000, GLIDER)
    if case == "slot_overflow":
        assert pkg.plan_probe_tiles(h, w, rule=rule, **OFF_CASES[case])[3] is None
    want = oracle.bp_run(g0, w, 16 * 6 + 7, rule)
    seen = {}
    for ppass in (True, False):
        if ppass:
            monkeypatch.delenv("GOL_DEV_PROBE_PASS", raising=False)
        else:
            monkeypatch.setenv("GOL_DEV_PROBE_PASS", "0")
        with pkg.Engine(h, w, rule=rule, device=0, **OFF_CASES[case]) as e:
            e.load_packed(g0)
            e.reset_timing()
            if case == "timing":
                e.set_timing(1)
            e.step(16 * 6 + 7)
            assert (e.store_packed() == want).all(), ppass
            assert e.activity_pass_probed() == 0, ppass
            if case == "slot_overflow":  # the kernel's probe goes on
                assert e.activity_probed() > 0
            seen[ppass] = counters(e)
    assert seen[True] == seen[False]


def test_torus(pkg, oracle, monkeypatch):
    """test_gpu_copy_pass.test_torus' engine (300 x 500, B3/S23 blocks, 300 generations
    against tests/torus_ref.py), the pass on against off: the inner engine takes the
    pass on the padded field the wrap kernel leaves."""
    h, w, rule, gens = 300, 500, (1 << 3, (1 << 2) | (1 << 3)), 300
    g0 = empty(h, w)
    for r in range(20, h - 2, 31):
        for c in (10, 250, w - 1):  # (the last block wraps around the edge)
            put(g0, r, c, [(0, 0), (1, 0)])
            put(g0, r, (c + 1) % w, [(0, 0), (1, 0)])
    want = torus_ref.torus_run(oracle, g0, w, gens, rule, chunk=64)
    assert (want == g0).all()
    seen = {}
    for ppass in (True, False):
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)
        if not ppass:
            monkeypatch.setenv("GOL_DEV_PROBE_PASS", "0")
        with pkg.Engine(h, w, rule=rule, semantics=pkg.SEM_TORUS, tb_depth=8, resident=1,
                        handoff=1, halo_depth=64) as e:
            e.load_packed(g0)
            e.reset_timing()
            e.step(gens)
            assert (e.store_packed() == want).all()
            assert e.digest() == oracle.bp_digest(want, w)
            seen[ppass] = counters(e), e.activity_pass_probed()
    assert seen[True][0] == seen[False][0] and seen[False][1] == 0
    assert 0 < seen[True][1] == seen[True][0][3]
