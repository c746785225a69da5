"""Host: tests/call_model.py -- the numpy model of the public calls against plain
references, and the program generator against the floors that keep the GPU sweep
(test_gpu_call_sequences.py) from passing without reaching the states it is for.

The floors are per kind and rule, over 24 programs: the share of programs with a step
that starts on a fixed point the host has seen (a "fixed candidate"), with two such steps
and no call between them, with a writer onto such a point, and with a step on a field in
motion.  They come from the model alone; the GPU file asserts the engines' own counters
on top.  GOL_CALLSEQ_COVERAGE=1 writes the facts per program to
profiles/call_sequences/coverage.json.
"""
import json
import os
import random

import numpy as np
import pytest

import call_model as cm
import rule_ref as rr
import torus_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVERAGE = os.path.join(ROOT, "profiles", "call_sequences", "coverage.json")
PROGRAMS = 24
GLIDER = cm.WINDOWS["glider"]


def field(h, w, cells):
    g = np.zeros((h, w), dtype=np.uint8)
    for r, c in cells:
        g[r, c] = 1
    return g


# ---- 1. the model against plain references


@pytest.mark.parametrize("rule", [cm.REF_RULE, cm.CONWAY, cm.HIGHLIFE], ids=rr.rule_name)
@pytest.mark.parametrize("h,w", [(1, 1), (9, 65), (37, 130), (64, 64)])
def test_step(oracle, rule, h, w):
    cells = rr.random_cells(h, w, h * 7 + w)
    m = cm.Model(oracle, cells, rule)
    t = cm.Model(oracle, cells, rule, torus=True)
    done = 0
    for g in (1, 2, 5, 17, 70):
        m.step(g)
        t.step(g)
        done += g
        assert (m.cells == rr.numpy_run(cells, done, rule)).all(), (h, w, done)
        want = torus_ref.unpack(torus_ref.roll_run(torus_ref.pack(cells), w, done, rule), w)
        assert (t.cells == want).all(), (h, w, done)
    assert m.is_fixed() == bool((rr.numpy_run(m.cells, 1, rule) == m.cells).all())
    assert m.digest() == tuple(oracle.bp_digest(torus_ref.pack(m.cells), w))
    if h > 5:
        parts = [m.digest_rows(0, 3), m.digest_rows(3, h - 5), m.digest_rows(h - 2, 2)]
        assert sum(p[0] for p in parts) == m.digest()[0]
        assert sum(p[1] for p in parts) & 0xFFFFFFFFFFFFFFFF == m.digest()[1]


@pytest.mark.parametrize("torus", [False, True])
def test_rect_ops(oracle, torus):
    """write_rect, read_rect and density against a loop over the cells."""
    h, w = 23, 150
    rng = np.random.default_rng(5)
    m = cm.Model(oracle, rr.random_cells(h, w, 2), cm.CONWAY, torus=torus)
    spots = [(0, 0, 3, 3), (h - 5, w - 70, 5, 70), (7, 60, 6, 9)]
    if torus:
        spots += [(h - 2, 10, 5, 8), (3, w - 3, 4, 70), (h - 1, w - 1, h, w)]
    for y, x, rh, rw in spots:
        for op in range(4):
            win = rng.integers(0, 2, (rh, rw), dtype=np.uint8)
            want = m.cells.copy()
            for i in range(rh):
                for j in range(rw):
                    r, c = (y + i) % h, (x + j) % w
                    d, s = int(want[r, c]), int(win[i, j])
                    want[r, c] = (s, d | s, d ^ s, d & (1 - s))[op]
            m.write_rect(y, x, win, op)
            assert (m.cells == want).all(), (y, x, rh, rw, op)
            got = torus_ref.unpack(m.read_rect(y, x, rh, rw), rw)
            cnt = m.density(y, x, rh, rw, 2, 7)
            for i in range(rh):
                for j in range(rw):
                    assert got[i, j] == want[(y + i) % h, (x + j) % w]
            loop = np.zeros_like(cnt)
            for i in range(rh):
                for j in range(rw):
                    loop[i // 2, j // 7] += got[i, j]
            assert (cnt == loop).all()
    if not torus:
        with pytest.raises(AssertionError):
            m.write_rect(h - 1, 0, GLIDER, cm.RECT_OR)


def brute(run, start, max_gens, lag, every, finish):
    """gol_step_until_periodic by keeping every generation: the first check generation
    g = c * every <= max_gens whose field equals generation g - lag's, the least divisor
    d of lag with generation g + d equal to g's, the number of checks made."""
    gens = [start]
    for _ in range(max_gens + lag):
        gens.append(run(gens[-1], 1))
    checks, last = 0, None
    for g in range(every, max_gens + 1, every):
        checks += 1
        last = g
        if (gens[g - lag] == gens[g]).all():
            p = min(d for d in range(1, lag + 1) if lag % d == 0 and (gens[g + d] == gens[g]).all())
            extra = 0 if lag == 1 else max(d for d in range(1, lag) if lag % d == 0 and d <= p)
            end = gens[g + (max_gens - g) % p] if finish else gens[g]
            return dict(period=p, advanced=g, checks=checks, extra_generations=extra, field=end,
                        slot=gens[g - lag])
    return dict(period=0, advanced=max_gens, checks=checks, extra_generations=0,
                field=gens[max_gens], slot=None if last is None else gens[last - lag])


UNTIL = [
    # name, h, w, torus, cells, lag, every, max, period, advanced
    ("blinker", 9, 9, False, [(4, 3), (4, 4), (4, 5)], 2, 0, 300, 2, 64),
    ("blinker-lag4", 9, 9, False, [(4, 3), (4, 4), (4, 5)], 4, 5, 300, 2, 5),
    ("blinker-lag1", 9, 9, False, [(4, 3), (4, 4), (4, 5)], 1, 3, 20, 0, 20),
    ("block", 9, 70, False, [(4, 63), (4, 64), (5, 63), (5, 64)], 4, 4, 100, 1, 4),
    ("glider-torus", 8, 8, True, [(0, 1), (1, 2), (2, 0), (2, 1), (2, 2)], 32, 0, 500, 32, 64),
    ("glider-dies", 12, 12, False, [(0, 1), (1, 2), (2, 0), (2, 1), (2, 2)], 1, 7, 300, 1, None),
    ("r-pentomino", 60, 60, False, [(30, 31), (30, 32), (31, 30), (31, 31), (32, 31)], 6, 16, 100, 0, 100),
    ("nothing-to-check", 9, 9, False, [(4, 3), (4, 4), (4, 5)], 2, 64, 63, 0, 63),
]


@pytest.mark.parametrize("finish", [False, True])
@pytest.mark.parametrize("case", UNTIL, ids=[c[0] for c in UNTIL])
def test_until_periodic(oracle, case, finish):
    name, h, w, torus, cells, lag, every, max_gens, period, advanced = case
    start = field(h, w, cells)
    m = cm.Model(oracle, start, cm.CONWAY, torus=torus)
    m.snapshot()
    run = ((lambda f, n: torus_ref.unpack(torus_ref.roll_run(torus_ref.pack(f), w, n, cm.CONWAY), w))
           if torus else (lambda f, n: rr.numpy_run(f, n, cm.CONWAY)))
    want = brute(run, start, max_gens, lag, every or -(-lag // 64) * 64, finish)
    got = m.until_periodic(max_gens, lag, every, finish)
    assert want["period"] == period and (advanced is None or want["advanced"] == advanced), want
    if name == "glider-torus":
        assert period == 4 * h
    for k in ("period", "advanced", "checks", "extra_generations"):
        assert got[k] == want[k], (name, k, got[k], want[k])
    assert (got["field"] == want["field"]).all() and (m.cells == want["field"]).all(), name
    if want["slot"] is None:
        assert got["slot"] is None and m.slot is None
    else:
        assert (m.slot == want["slot"]).all() and (got["slot"] == want["slot"]).all()
        assert m.diff() == int((want["field"] != want["slot"]).sum())
        assert m.same() == (m.diff() == 0)


def test_snapshot_slot(oracle):
    m = cm.Model(oracle, field(20, 20, [(5, 5), (5, 6), (5, 7)]), cm.CONWAY)
    m.snapshot()
    assert m.same() and m.diff() == 0
    m.step(1)
    assert not m.same() and m.diff() == 4
    m.write_rect(0, 0, GLIDER, cm.RECT_XOR)
    assert m.diff() == 9
    m.restore()
    assert m.same() and m.cells.sum() == 3
    m.step(2)
    assert m.same() and not m.is_fixed()


# ---- 2. the generator


def test_lattice_is_still(oracle):
    """The B3/S23 start field is a fixed point, under HighLife too, on every shape."""
    shapes = [(333, 8987), (130, 64 * 126 - 63), (400, 64 * 156), (300, 500), (130, 192), (257, 320),
              (1500, 500)]
    for h, w in shapes:
        g = cm.lattice(h, w)
        assert g.any()
        for rule in (cm.CONWAY, cm.HIGHLIFE):
            for torus in (False, True):
                assert cm.Model(oracle, g, rule, torus=torus).is_fixed(), (h, w, rule, torus)
    assert not cm.Model(oracle, cm.lattice(333, 8987, [(50, 3000)]), cm.CONWAY).is_fixed()


def test_programs_repeat(pkg):
    hot = cm.plan_hot(pkg)
    for kind in cm.KINDS:
        rule = cm.KINDS[kind]["rules"][-1][0]
        a, b = cm.case_program(kind, rule, 3, hot), cm.case_program(kind, rule, 3, hot)
        assert cm.format_ops(a["ops"]) == cm.format_ops(b["ops"]) and a["start"] == b["start"]
        assert a["cfg"] == b["cfg"] and (a["h"], a["w"]) == (b["h"], b["w"])
        c = cm.case_program(kind, rule, 4, hot)
        assert cm.format_ops(a["ops"]) != cm.format_ops(c["ops"])


def test_window_positions(pkg):
    """60 % of the windows lie within 2 cells of a hot coordinate on an axis (here: at
    least half), every class of hot coordinate is met, and on a torus a third (here: a
    quarter at least) wrap an edge."""
    hot = cm.plan_hot(pkg)
    c = cm.case_program("skip16", cm.CONWAY, 0, hot)
    h, w, H = c["h"], c["w"], c["hot"]
    assert {"edge", "tile", "seam"} <= set(H["rows"]) and {"edge", "word", "seam"} <= set(H["cols"])
    rnd = random.Random(1)
    near, met = 0, set()
    for _ in range(2000):
        wh, ww = rnd.choice([(2, 2), (3, 3), (5, 5), (4, 70)])
        y, x = cm.draw_position(rnd, h, w, wh, ww, H, False)
        assert 0 <= y <= h - wh and 0 <= x <= w - ww
        ys, xs = (y, y + wh - 1, y + wh // 2), (x, x + ww - 1, x + ww // 2)
        hit = False
        for axis, vals, at in (("rows", H["rows"], ys), ("cols", H["cols"], xs)):
            for k, vs in vals.items():
                if any(abs(a - v) <= 2 for a in at for v in vs):
                    met.add((axis, k))
                    hit = True
        near += hit
    assert near >= 1000, near
    assert met == {(a, k) for a in ("rows", "cols") for k in H[a]}, met
    wraps = 0
    for _ in range(2000):
        y, x = cm.draw_position(rnd, 300, 500, 3, 3, cm.hot_coordinates(300, 500), True)
        assert 0 <= y < 300 and 0 <= x < 500
        wraps += y + 3 > 300 or x + 3 > 500
    assert wraps >= 500, wraps


# kind, rule -> floors as shares of the programs: a fixed candidate, a run of two, a writer
# onto a seen fixed point
FLOORS = {
    ("skip16", cm.REF_RULE): (3 / 4, 1 / 2, 1 / 2),
    ("skip8", cm.REF_RULE): (3 / 4, 1 / 2, 1 / 2),
    ("skip16", cm.CONWAY): (1 / 3, 1 / 5, 1 / 5),
    ("skip12", cm.HIGHLIFE): (1 / 3, 1 / 5, 1 / 5),
}
_coverage = {}


@pytest.mark.parametrize("kind,rule", sorted(FLOORS), ids=[f"{k}-{rr.rule_name(r)}" for k, r in sorted(FLOORS)])
def test_generator_floors(pkg, oracle, kind, rule):
    hot = cm.plan_hot(pkg)
    K = cm.KINDS[kind]["K"]
    rows, ops_drawn, names = [], set(), set()
    for seed in range(PROGRAMS):
        c = cm.case_program(kind, rule, seed, hot)
        assert 4 <= sum(1 for op in c["ops"] if op[0] in ("step", "sync")) and c["K"] == K
        m = cm.Model(oracle, cm.make_field(oracle, c["start"], c["h"], c["w"]), rule)
        facts = cm.program_facts(cm.run_program(m, c["ops"]), K)
        ops_drawn |= {op[4] for op in c["ops"] if op[0] == "write"}
        names |= {op[0] for op in c["ops"]} | {op[3] for op in c["ops"] if op[0] == "write"}
        rows.append(dict(kind=kind, rule=rr.rule_name(rule), seed=seed, h=c["h"], w=c["w"],
                         ops=len(c["ops"]), **facts))
    n = len(rows)
    cand, run2, seen = FLOORS[(kind, rule)]
    share = lambda key, least: sum(r[key] >= least for r in rows)  # noqa: E731
    got = (share("fixed_candidates", 1), share("longest_run", 2), share("seen_writes", 1))
    print(kind, rr.rule_name(rule), "of", n, "programs: candidate, run of two, seen write:", got)
    assert got[0] >= cand * n and got[1] >= run2 * n and got[2] >= seen * n, got
    # every program steps a field in motion (so at least 4 of 5 do)
    assert share("moving_steps", 1) == n >= 0.8 * n
    # a write that leaves the field as it was occurs; all four ops and every window do
    assert sum(r["noop_writes"] for r in rows) >= 1
    assert ops_drawn == {0, 1, 2, 3}
    want = {"block", "blinker", "glider", "eraser", "restore", "snapshot", "load", "until",
            "init_random", "load_ascii", "act", "set_timing", "reset_timing", "store", "digest",
            "read", "density", "digest_rows", "same", "diff", "rewrite"}
    if rule == cm.REF_RULE:
        want.add("bar")
    assert want <= names, want - names
    # two writers in a row occur, and some program has more graphable lengths than the
    # graph cache's 8 slots hold on two starting buffers
    assert sum(r["writer_pairs"] for r in rows) >= 3
    assert max(r["lengths"] for r in rows) >= 5
    _coverage[f"{kind} {rr.rule_name(rule)}"] = rows
    if os.environ.get("GOL_CALLSEQ_COVERAGE") == "1" and len(_coverage) == len(FLOORS):
        os.makedirs(os.path.dirname(COVERAGE), exist_ok=True)
        with open(COVERAGE, "w") as f:
            json.dump(_coverage, f, indent=1, sort_keys=True)
            f.write("\n")
