"""CPU suite: the activity skip's neighbour lists (plan.cpp unit_rects,
build_neighbours) through the host-only model gol_plan_neighbours -- no GPU.

A unit (wavefront) skips a launch of K generations when every unit of its
neighbour list N(U) stored nothing new in the two launches before
(life_stencil.h).  The argument needs the output rectangles of N(U)
to cover U's rectangles dilated by K rows and K lane-group columns, clipped to
the field, and N(U) to hold U.  Row blocks are bottom-up, age-skewed per strip,
and the half strip packs two row blocks per unit, so the lists are not "the 8
around": this sweeps h, w, rows_per_wave, the skew and the half strip on and
off and checks the property for every unit, and that the rectangles tile the
field exactly once.
"""
import numpy as np
import pytest

# widths: one strip; 2 full strips; 2 strips + the half strip with gaps of 1, 15
# and 30 lane groups (test_gpu_halfstrip.py), one of them no multiple of 64; 3 strips
WIDTHS = [1000, 64 * 126, 64 * 127, 64 * 141 - 37, 64 * 156, 64 * 190 + 5]


def check_plan(pkg, h, w, **kw):
    cus = kw.pop("cus", 256)
    m = pkg.plan_model(h, w, cus=cus, **kw)
    rects, offs, ids = pkg.plan_neighbours(h, w, cus=cus, **kw)
    K, ng = m["tb_depth"], (w + 63) // 64
    units = rects.shape[0]
    assert units == m["total_units"]
    if m["handoff"]:
        assert len(ids) == 0  # hand-off plans never skip
        return m
    assert len(ids) > 0 and offs[0] == 0 and offs[-1] == len(ids)
    # the rectangles tile the field: every (row, group) in exactly one of them
    cover = np.zeros((h, ng), dtype=np.int32)
    for u in range(units):
        for r0, r1, q0, q1 in rects[u]:
            if r1 > r0:
                assert 0 <= r0 and r1 <= h and 0 <= q0 < q1 <= ng
                cover[r0:r1, q0:q1] += 1
    assert (cover == 1).all()
    owner = np.full((h, ng), -1, dtype=np.int64)
    for u in range(units):
        for r0, r1, q0, q1 in rects[u]:
            if r1 > r0:
                owner[r0:r1, q0:q1] = u
    for u in range(units):
        nb = ids[offs[u]:offs[u + 1]]
        assert u in nb and (nb < units).all() and len(set(nb.tolist())) == len(nb)
        for r0, r1, q0, q1 in rects[u]:
            if r1 <= r0:
                continue
            need = np.unique(owner[max(0, r0 - K):min(h, r1 + K), max(0, q0 - K):min(ng, q1 + K)])
            missing = set(need.tolist()) - set(nb.tolist())
            assert not missing, (h, w, kw, u, sorted(missing))
    return m


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("h,rpw", [(300, 64), (333, 61), (97, 0), (40, 24)])
def test_neighbours_forced_blocks(pkg, h, w, rpw):
    check_plan(pkg, h, w, rows_per_wave=rpw, handoff=1)
    check_plan(pkg, h, w, rows_per_wave=rpw, handoff=1, tb_depth=16, rule=pkg.CONWAY)


@pytest.mark.parametrize("pairs", ["1", "0"])
@pytest.mark.parametrize("w", WIDTHS[2:5])
def test_neighbours_half_strip_on_off(pkg, monkeypatch, w, pairs):
    monkeypatch.setenv("GOL_DEV_PAIRS", pairs)
    m = check_plan(pkg, 333, w, rows_per_wave=64, handoff=1)
    assert (m["half_units"] > 0) == (pairs == "1")


@pytest.mark.parametrize("w", [64 * 126, 64 * 141 - 37])
@pytest.mark.parametrize("h", [1500, 2011])
def test_neighbours_skewed_blocks(pkg, h, w):
    """Age-skewed blocks (a device of 2 CUs fills one round at this size): the old
    units' longer blocks start at strip-dependent heights."""
    skewed = 0
    for cus in (2, 3):
        for depth in (8, 16):
            m = check_plan(pkg, h, w, cus=cus, handoff=1, tb_depth=depth)
            skewed += m["rows_old"] > 0
    assert skewed > 0


def test_neighbours_skew_off(pkg, monkeypatch):
    monkeypatch.setenv("GOL_DEV_AGE_SKEW", "0")
    m = check_plan(pkg, 1500, 64 * 141, cus=2, handoff=1, tb_depth=16)
    assert m["rows_old"] == 0


def test_handoff_plan_has_no_lists(pkg):
    m = pkg.plan_model(8448, 65536, handoff=2, rule=pkg.CONWAY)
    rects, offs, ids = pkg.plan_neighbours(8448, 65536, handoff=2, rule=pkg.CONWAY)
    assert m["handoff"] == 1 and len(ids) == 0 and rects.shape[0] == m["total_units"]


def test_headline_plan_lists_are_short(pkg):
    """65536^2 B/S2: every unit reads at most a few dozen streaks (one per lane)."""
    rects, offs, ids = pkg.plan_neighbours(65536, 65536)
    n = np.diff(offs.astype(np.int64))
    assert len(ids) > 0 and n.min() >= 1 and n.max() <= 64
