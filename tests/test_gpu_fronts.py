"""GPU: signals of speed 1 -- one cell per generation, the fastest a radius-1 rule
allows and the speed DESIGN §4 argues from -- through still units: the skip,
copy-through, the still probe, the copy pass, the probe pass and the twin test all
decide from "nothing changed within K cells", and gliders (c/4) and soups (c/2 at
most) would pass a dilation of half that.

Fuses (rule_ref.py): a one-cell-wide line is still in its interior under B/S2 and,
if diagonal, under B3/S23, and loses its end cells one per generation, so the
units it lies in go quiet and a front reaches them at exactly speed 1; the field
after g generations is a formula.  The burning end is aimed at a row-block seam,
a strip seam, a unit corner and the half strip from every direction, starting
3K + d cells away for d = 0 .. K + 1, so the launch and the generation within it
in which the front arrives take every value, whatever the off-by-one convention.

Two plans of the skip kind of test_gpu_activity.py (one stream, classic blocks):
  64-row blocks  that file's plan.  A unit's neighbour list holds the whole blocks
      above and below, which a front needs 64 generations to cross, so the unit
      the front enters is awake long before: tight for what compares cells (the
      probes' K - 1), not for the lists.
  15-row blocks  K - 1 rows: the list of a unit reaches exactly two blocks up, the
      second of which ends K rows away, and the front crosses a block within one
      launch.  Here the model of test_gpu_activity.py (`expected`, from the oracle)
      has the entered unit skip the very launch before the front arrives (across a
      row seam, a corner and into the half strip; not through a block's side, where
      the front comes along the list's own blocks), and a list dilated by K - 1
      rows instead of K leaves a cell alive that should be dead
      (profiles/r16/mutants.txt).  Columns are dilated by K lane groups, 64 K
      cells, so no front is tight sideways.

Flood (one cell -> the Chebyshev ball) and erosion (a full field with holes, B/S8)
send the same fronts through the generic kernels, K = 12 and 8.  The last tests
run the fronts where nothing skips: the resident kernel, hand-off blocks, groups
of stripes at several halo depths and the torus.
"""
import numpy as np
import pytest

import rule_ref as rr
from test_gpu_activity import WIDTHS, expected, make, one_step, plan
from torus_ref import pack, roll_run

pytestmark = pytest.mark.gpu

H, K = 333, 16
OFFSETS = range(K + 2)
DIAGONALS = [(1, 1), (1, -1), (-1, 1), (-1, -1)]
VERTICALS, HORIZONTALS = [(1, 0), (-1, 0)], [(0, 1), (0, -1)]
RULES = {"B/S2": rr.REF_RULE, "B3/S23": rr.CONWAY}
SEQUENCE = [K, K, 3 * K + 5, K]


def owner(rects, r, c):
    us = [u for u in range(rects.shape[0]) for r0, r1, q0, q1 in rects[u]
          if r0 <= r < r1 and q0 <= c // 64 < q1]
    assert len(us) == 1, (r, c, us)
    return us[0]


def targets(rects, kind, rule):
    """[(direction, (row, column))]: the first cell the front kills past the seam."""
    full = [u for u in range(rects.shape[0]) if rects[u][1][1] <= rects[u][1][0]]
    pairs = [u for u in range(rects.shape[0]) if u not in full]
    # the row-block seam nearest the middle, in strip 0; the block below it
    r0s = sorted({int(rects[u][0][0]) for u in full if rects[u][0][2] == 0})
    R = min((r for r in r0s if r > 0), key=lambda r: abs(r - H // 2))
    below = [rects[u][0] for u in full if rects[u][0][0] == R and rects[u][0][2] == 0][0]
    mid = int(R + (min(below[1], H) - R) // 2)
    C = 64 * min(int(rects[u][0][2]) for u in full if rects[u][0][2] > 0)  # strip 0 | the next
    orth = rule == rr.REF_RULE
    if kind == "row":
        dirs = DIAGONALS + (VERTICALS if orth else [])
        return [((dr, dc), (R if dr > 0 else R - 1, 2000)) for dr, dc in dirs]
    if kind == "strip":
        dirs = DIAGONALS + (HORIZONTALS if orth else [])
        return [((dr, dc), (mid, C if dc > 0 else C - 1)) for dr, dc in dirs]
    if kind == "corner":
        return [((dr, dc), (R if dr > 0 else R - 1, C if dc > 0 else C - 1)) for dr, dc in DIAGONALS]
    assert kind == "half" and pairs
    # the half strip's columns; its unit of two row blocks nearest the middle ends at
    # Rp: fronts moving up enter it there, fronts moving down enter the unit after the
    # next (a front that started inside the two-block unit would keep every unit that
    # lists it awake, and with 64-row blocks that is every unit above)
    q0, q1 = int(rects[pairs[0]][0][2]), int(rects[pairs[0]][0][3])
    Rp = min((int(rects[u][1][1]) for u in pairs), key=lambda r: abs(r - H // 2))
    rows = sorted(int(r[0]) for u in range(rects.shape[0]) for r in rects[u]
                  if r[1] > r[0] and r[2] == q0)
    Rn = [r for r in rows if r > Rp][0]
    out = []
    for dr, dc in DIAGONALS + (VERTICALS + HORIZONTALS if orth else []):
        r = mid if dr == 0 else Rn if dr > 0 else Rp - 1
        c = 32 * (q0 + q1) if dc == 0 else 64 * q0 if dc > 0 else 64 * q1 - 1
        out.append(((dr, dc), (r, c)))
    return out


def scenario(pkg, rpw, kind, rule):
    w = WIDTHS[2] if kind == "half" else WIDTHS[0]
    pl = plan(pkg, H, w, rule=rule, rows_per_wave=rpw, tb_depth=K)
    return w, pl, targets(pl[0], kind, rule)


def skips_before_arrival(oracle, field, w, rule, pl, u, start):
    """Input condition: the model lets unit u skip the launch before the one in which
    the front's first cell inside it dies (generation start + 1).  Returns that and
    the model's skip count over one step of 6K generations."""
    model = expected(oracle, field, w, rule, K, 6, pl)
    n = start // K  # generation start + 1 is computed by launch n (0-based)
    assert 3 <= n <= 5
    return u in model[n - 1], sum(len(s) for s in model)


@pytest.mark.parametrize("kind", ["row", "strip", "corner", "half"])
@pytest.mark.parametrize("name", sorted(RULES))
@pytest.mark.parametrize("rpw", [64, K - 1])
def test_fuse_fronts(pkg, oracle, monkeypatch, model_plans, rpw, name, kind):
    rule = RULES[name]
    w, pl, tg = scenario(pkg, rpw, kind, rule)
    units = pl[0].shape[0]
    hits, least, cases = [], None, 0
    # the oracle's model costs more than the GPU's work: with 64-row blocks, where it
    # only bounds the skip count, at the ends of the sweep and around d = K
    model_at = OFFSETS if rpw < 64 else (0, K - 1, K, K + 1)
    with make(pkg, monkeypatch, H, w, rule=rule, rows_per_wave=rpw) as e, \
            make(pkg, monkeypatch, H, w, skip=False, rule=rule, rows_per_wave=rpw) as off:
        for direction, (tr, tc) in tg:
            u = owner(pl[0], tr, tc)
            for d in OFFSETS:
                start = 3 * K + d
                field, after, n = rr.fuse_towards(H, w, tr, tc, direction, start)
                assert n > 2 * (start + 2), "the other end must not reach the target first"
                tag = (name, rpw, kind, direction, d)
                # one long step
                got, (c, k) = one_step(e, field, 6 * K + 8)
                ref, (co, ko) = one_step(off, field, 6 * K + 8)
                want = after(6 * K + 8)
                assert (got == want).all(), tag
                assert (ref == want).all() and ko == 0 and c + k == co == 7 * units, tag
                assert k > 0, tag
                if d in model_at:
                    hit, model = skips_before_arrival(oracle, field, w, rule, pl, u, start)
                    assert k <= model, (tag, k, model)
                    if hit:
                        hits.append((direction, d))
                least = k if least is None else min(least, k)
                # several steps: the per-step decisions meet a front that has moved
                for eng in (e, off):
                    eng.load_packed(field)
                    eng.reset_timing()
                    done = 0
                    for gens in SEQUENCE:
                        eng.step(gens)
                        done += gens
                        assert (eng.store_packed() == after(done)).all(), (tag, done, eng is e)
                # only the step of 3K + 5 has a third launch, the first that may skip
                assert e.activity()[1] <= units and off.activity()[1] == 0, tag
                cases += 1
    print(name, rpw, kind, f"{cases} fields, least skipped {least}, entered unit skips the "
          f"launch before arrival at (direction, d):", hits)
    if rpw == 64 or kind == "strip":
        # the block above (below) is on the unit's list and takes the front 4 launches to
        # cross; so are the neighbouring strips, K lane groups wide: a front that comes in
        # through a block's side has been on the list for longer still
        assert not hits
    else:
        # d = K - 2 and K - 1: the cell dies in the last generations of the fourth launch,
        # the front was 2K + 1 rows or more away when the unit skipped the third
        assert {d for _, d in hits} == {K - 2, K - 1}, hits


FRONT_W = WIDTHS[0]


@pytest.mark.parametrize("depth", [12, 8])
def test_flood_front(pkg, oracle, monkeypatch, model_plans, depth):
    """One cell near the top left corner under B12345678/S012345678: 4200 generations
    take the front down every row block and over the strip seam.  Ahead of it dead
    units skip, behind it full ones."""
    h, w, r, c = H, FRONT_W, 10, 100
    field, after = rr.flood(h, w, r, c)
    pl = plan(pkg, h, w, rule=rr.FLOOD, tb_depth=depth)
    seam = 64 * min(int(q) for q in pl[0][:, 0, 2] if q > 0)
    assert c + 4200 > seam + 64 and r + 4200 > h
    with make(pkg, monkeypatch, h, w, rule=rr.FLOOD, tb_depth=depth) as e, \
            make(pkg, monkeypatch, h, w, skip=False, rule=rr.FLOOD, tb_depth=depth) as off:
        assert e.tb_depth == depth
        # the front inside the first block, across the row seams, just over the strip seam
        for gens in (3 * depth + 5, 150, seam - c + depth // 2, 4200):
            got, (cc, k) = one_step(e, field, gens)
            ref, (co, ko) = one_step(off, field, gens)
            want = after(gens)
            assert (got == want).all() and (ref == want).all(), (depth, gens)
            assert e.digest() == oracle.bp_digest(want, w)
            assert k > 0 and ko == 0 and cc + k == co, (depth, gens, cc, k, co)
        assert not rr.unpack(want, w).all() and rr.unpack(want, w)[:, :seam + 64].all()


@pytest.mark.parametrize("depth", [12, 8])
def test_erosion_front(pkg, oracle, monkeypatch, model_plans, depth):
    """B/S8: a full field with a one-cell hole on a unit corner and a hole across a
    lane-group boundary; the dead regions grow at speed 1 into full, still units."""
    h, w = H, FRONT_W
    pl = plan(pkg, h, w, rule=rr.EROSION, tb_depth=depth)
    seam = 64 * min(int(q) for q in pl[0][:, 0, 2] if q > 0)
    holes = [(128, 129, seam, seam + 1), (250, 253, 6000, 6070)]
    field, after = rr.eroded(h, w, holes)
    with make(pkg, monkeypatch, h, w, rule=rr.EROSION, tb_depth=depth) as e, \
            make(pkg, monkeypatch, h, w, skip=False, rule=rr.EROSION, tb_depth=depth) as off:
        for gens in (5, depth, 3 * depth + 1, 6 * depth + 7, (h + 1) // 2 + 3):
            got, (cc, k) = one_step(e, field, gens)
            ref, (co, ko) = one_step(off, field, gens)
            want = after(gens)
            assert (got == want).all() and (ref == want).all(), (depth, gens)
            assert e.digest() == oracle.bp_digest(want, w)
            assert ko == 0 and cc + k == co
        assert not want.any() and after((h + 1) // 2 - 1).any()
        # and step by step, so that each step starts where a front stands
        for eng in (e, off):
            eng.load_packed(field)
            done = 0
            for gens in (5, depth, 3 * depth + 1, depth):
                eng.step(gens)
                done += gens
                assert (eng.store_packed() == after(done)).all(), (depth, done)


# ---- the same fronts where nothing skips ---------------------------------------------------

SMALL = (200, 300)
NO_SKIP = {
    "resident": dict(resident=2),
    "handoff": dict(tb_depth=8, rows_per_wave=22, handoff=2, streams=1, resident=1),
}
STEPS = [1, 15, 16, 17, 40]


def small_cases():
    h, w = SMALL
    out = {
        "fuse_v": (rr.REF_RULE,) + rr.fuse(h, w, 0, 131, h, rr.VERTICAL),
        "fuse_h": (rr.REF_RULE,) + rr.fuse(h, w, 77, 3, w - 5, rr.HORIZONTAL),
        "fuse_d": (rr.CONWAY,) + rr.fuse(h, w, 0, 60, h, rr.DIAGONAL),
        "fuse_a": (rr.CONWAY,) + rr.fuse(h, w, 2, 250, h - 2, rr.ANTIDIAGONAL),
        "flood": (rr.FLOOD,) + rr.flood(h, w, 99, 63),
        "erosion": (rr.EROSION,) + rr.eroded(h, w, [(100, 101, 64, 65), (30, 33, 120, 200)]),
    }
    return out


@pytest.mark.parametrize("case", sorted(small_cases()))
@pytest.mark.parametrize("engine", sorted(NO_SKIP))
def test_fronts_without_skip(pkg, oracle, engine, case):
    h, w = SMALL
    rule, field, after = small_cases()[case]
    cfg = dict(NO_SKIP[engine])
    if engine == "handoff" and rule not in (rr.REF_RULE, rr.CONWAY):
        cfg.update(tb_depth=12, rows_per_wave=30)  # the generic rules' hand-off depth
    with pkg.Engine(h, w, rule=rule, device=0, **cfg) as e:
        assert e.handoff == (engine == "handoff")
        assert (e.resident is not None) == (engine == "resident")
        e.load_packed(field)
        done = 0
        for gens in STEPS:
            e.step(gens)
            done += gens
            want = after(done)
            assert (e.store_packed() == want).all(), (engine, case, done)
            assert e.digest() == oracle.bp_digest(want, w)
        assert e.activity()[1] == 0


def seam_fuses(h, w, first, last, start):
    """Two B/S2 fuses in one field: an end that moves down column 190 and kills cell
    (first, 190), the first row below the first stripe seam, in generation start + 1,
    and one that moves up column 120 and kills (last - 1, 120), the last row above
    the last seam, in the same generation.  Returns (field, after, cells): the two
    target cells."""
    fa, aa, _ = rr.fuse_towards(h, w, first, 190, (1, 0), start)
    fb, ab, _ = rr.fuse_towards(h, w, last - 1, 120, (-1, 0), start)
    return fa | fb, (lambda g: aa(g) | ab(g)), [(first, 190), (last - 1, 120)]


@pytest.mark.parametrize("overlap", [0, 1, 2])
@pytest.mark.parametrize("halo", [1, 7, 16, 64])
@pytest.mark.parametrize("n", [2, 3])
def test_fronts_across_stripe_seams(pkg, oracle, n, halo, overlap):
    """Groups of n stripes.  A flood seed in the last row above a stripe seam.  B/S2
    fuse ends that start 1, about halo / 2, halo, halo + 1 and halo + 2 rows before
    a seam, one moving down and one moving up, so that an end crosses the seam in
    the first exchange round, at its last generation, and in the next rounds; the
    steps end 8 generations or more after the crossing, and the target cells and
    the rows behind them are checked to have burnt."""
    h, w = SMALL
    steps = (2, halo + 3, 6)
    with pkg.Group(h, w, n, rule=rr.FLOOD, halo_depth=halo, exchange_overlap=overlap) as g:
        seam = g.members[1].row0
        assert 0 < seam < h and all(m.halo_depth == halo for m in g.members)
        field, after = rr.flood(h, w, seam - 1, 190)
        g.load_packed(field)
        done = 0
        for gens in steps:
            g.step(gens)
            done += gens
            want = after(done)
            assert (g.store_packed() == want).all(), (n, halo, overlap, "flood", done)
            assert g.digest() == oracle.bp_digest(want, w)
        cells = rr.unpack(want, w)
        assert cells[seam - 1 + done, 190] and not cells[seam + done, 190]  # radius `done`
    with pkg.Group(h, w, n, rule=rr.REF_RULE, halo_depth=halo, exchange_overlap=overlap) as g:
        first, last = g.members[1].row0, g.members[-1].row0
        for start in sorted({1, halo // 2 + 1, halo, halo + 1, halo + 2}):
            field, after, targets = seam_fuses(h, w, first, last, start)
            total = sum(steps)
            assert total >= start + 1 + 8
            for r, c in targets:  # the formula: alive until generation start, dead after
                assert rr.unpack(after(start), w)[r, c] and not rr.unpack(after(start + 1), w)[r, c]
            g.load_packed(field)
            done = 0
            for gens in steps:
                g.step(gens)
                done += gens
                want = after(done)
                assert (g.store_packed() == want).all(), (n, halo, overlap, start, done)
                assert g.digest() == oracle.bp_digest(want, w)
            # the ends crossed their seams: total - start rows beyond have burnt
            got, was, past = rr.unpack(g.store_packed(), w), rr.unpack(field, w), total - start
            assert was[first:first + past + 1, 190].all() and not got[first:first + past, 190].any()
            assert was[last - past - 1:last, 120].all() and not got[last - past:last, 120].any()


def test_fronts_on_the_torus(pkg, oracle):
    """A flood seed next to the corner grows into the ball in torus distance; a
    diagonal fuse that lies across both wraps burns like any other (np.roll
    reference): the end that starts at cell 0 passes the row wrap at cell 30, the
    end that starts at cell 89 the column wrap at cell 50."""
    h, w = 130, 200
    field, after = rr.flood(h, w, 1, 197, torus=True)
    with pkg.Engine(h, w, rule=rr.FLOOD, device=0, semantics=pkg.SEM_TORUS) as e:
        e.load_packed(field)
        done = 0
        for gens in (1, 16, 23, 30):
            e.step(gens)
            done += gens
            assert (e.store_packed() == after(done)).all(), done
        assert done > h // 2 and not rr.unpack(after(done), w).all()
    i = np.arange(90)
    line = np.zeros((h, w), dtype=np.uint8)
    line[(100 + i) % h, (150 + i) % w] = 1
    start = pack(line)
    for rule in (rr.REF_RULE, rr.CONWAY):
        with pkg.Engine(h, w, rule=rule, device=0, semantics=pkg.SEM_TORUS) as e:
            e.load_packed(start)
            want = start
            for gens in (1, 16, 25):
                e.step(gens)
                want = roll_run(want, w, gens, rule)
                assert (e.store_packed() == want).all(), (rr.rule_name(rule), gens)
            k = i[42:90 - 42]  # cells 42 .. 47: past cell 30 and short of cell 50
            assert (100 + 42) % h < 100 and (150 + 47) % w > 150
            ends = np.zeros((h, w), dtype=np.uint8)
            ends[(100 + k) % h, (150 + k) % w] = 1
            assert (want == pack(ends)).all()
