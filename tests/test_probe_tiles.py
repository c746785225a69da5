"""CPU suite: the probe pass's tile table (plan.cpp build_tile_units; DESIGN §4 "Probe
pass") through the host-only export gol_plan_probe_tiles, against gol_plan_neighbours'
rectangles of the same modelled plan.

Per tile of tile_rows rows x tile_words 64-column words the table lists every unit one
of whose rectangles, dilated by K - 1 cells and clipped to the field, meets the tile
(coverage: an omission would let a unit go through on tiles nobody looked at), and no
unit whose rectangles dilated by K + 1 cells miss it (tightness: a listed unit is
marked whenever the tile changes).  A plan with a tile of more units than slots has
no table and takes no pass.
"""
import numpy as np
import pytest

BASE = dict(resident=1, handoff=1, streams=1)
NONE = 0xFFFFFFFF

SHAPES = {
    "333x126": (333, 64 * 126, dict(BASE, rows_per_wave=64)),
    "333x127": (333, 64 * 127, dict(BASE, rows_per_wave=64)),
    "333x141-37": (333, 64 * 141 - 37, dict(BASE, rows_per_wave=64)),   # the half strip
    "333x156": (333, 64 * 156, dict(BASE, rows_per_wave=64)),
    "589x141-37": (589, 64 * 141 - 37, dict(BASE, rows_per_wave=64)),
    "525x126": (525, 64 * 126, dict(BASE, rows_per_wave=64)),
    "333x141-37-r63": (333, 64 * 141 - 37, dict(BASE, rows_per_wave=63)),
    "65536^2": (65536, 65536, dict()),
    "32768x262144": (32768, 262144, dict()),
}


def listed_pairs(table):
    t, s = np.nonzero(table != NONE)
    return set(zip(t.tolist(), table[t, s].tolist()))


def pairs_of(rects, h, w, d, tr, tw, ncol):
    """(tile, unit) for every tile that meets a rectangle of the unit dilated by d cells
    and clipped to the h x w field."""
    out = set()
    for u in range(rects.shape[0]):
        for r0, r1, q0, q1 in rects[u].tolist():
            if r1 <= r0 or q1 <= q0:
                continue
            a0, a1 = max(0, r0 - d), min(h, r1 + d)
            c0, c1 = max(0, 64 * q0 - d), min(w, 64 * q1 + d)
            for i in range(a0 // tr, (a1 - 1) // tr + 1):
                for c in range(c0 // (64 * tw), (c1 - 1) // (64 * tw) + 1):
                    out.add((i * ncol + c, u))
    return out


@pytest.mark.parametrize("depth", [8, 12, 16])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_coverage_and_tightness(pkg, shape, depth):
    h, w, kw = SHAPES[shape]
    kw = dict(kw, tb_depth=depth)
    rects = pkg.plan_neighbours(h, w, **kw)[0]
    tr, tw, ncol, table = pkg.plan_probe_tiles(h, w, **kw)
    assert table is not None, "a shipped or tested plan without the probe pass"
    assert (tr, tw) == (8, 64) and ncol == -(-((w + 63) // 64) // tw)
    assert table.shape[0] == ncol * -(-h // tr)
    if shape == "333x141-37":  # units of the half strip: two row blocks each
        assert any(r[0][1] > r[0][0] and r[1][1] > r[1][0] for r in rects)
    got = listed_pairs(table)
    assert max(u for _, u in got) < rects.shape[0]
    need = pairs_of(rects, h, w, depth - 1, tr, tw, ncol)
    may = pairs_of(rects, h, w, depth + 1, tr, tw, ncol)
    assert need <= got, sorted(need - got)[:5]
    assert got <= may, sorted(got - may)[:5]
    # every tile has a unit: the rectangles tile the field
    assert len({t for t, _ in got}) == table.shape[0]


def test_slot_overflow_has_no_table(pkg):
    """Row blocks of 8 rows: a tile's K - 1 = 15 rows of dilation reach more blocks
    than there are slots, so the plan has no table (and the engine takes no pass)."""
    h, w = 333, 64 * 141 - 37
    for rpw, want in ((64, True), (16, True), (8, False), (4, False)):
        tr, tw, ncol, table = pkg.plan_probe_tiles(h, w, **dict(BASE, rows_per_wave=rpw, tb_depth=16))
        assert (table is not None) == want, rpw
        assert (tr, tw) == (8, 64)
        assert want or ncol == 0


def test_no_table_without_the_copy_pass(pkg):
    """A hand-off plan never skips: no neighbour lists, no copy pass, no probe pass."""
    kw = dict(tb_depth=8, rows_per_wave=22, handoff=2, streams=1, resident=1)
    assert len(pkg.plan_neighbours(600, 64 * 127, **kw)[2]) == 0
    assert pkg.plan_probe_tiles(600, 64 * 127, **kw)[3] is None


def test_shipped_plans_have_the_table(pkg):
    for h, w, rule in ((65536, 65536, pkg.REF_RULE), (65536, 65536, pkg.CONWAY),
                       (32768, 262144, pkg.REF_RULE)):
        tr, tw, ncol, table = pkg.plan_probe_tiles(h, w, rule=rule)
        assert table is not None and table.shape == (ncol * (h // tr), 8)
        assert int((table != NONE).sum(axis=1).max()) <= 8


def test_torus_uses_the_inner_plan(pkg):
    geo = pkg.torus_geometry(300, 500, tb_depth=8, resident=1, handoff=1, halo_depth=64)
    kw = dict(tb_depth=8, resident=1, handoff=1, halo_depth=64)
    a = pkg.plan_probe_tiles(300, 500, semantics=pkg.SEM_TORUS, **kw)
    b = pkg.plan_probe_tiles(geo["padded_h"], geo["padded_w"], streams=1,
                             **dict(kw, halo_depth=0))
    assert a[:3] == b[:3] and (a[3] is None) == (b[3] is None)
    assert a[3] is None or (a[3] == b[3]).all()
