"""GPU: the activity skip (life_stencil.h) against the CPU oracle, against
the same engine with the skip switched off (GOL_DEV_ACTIVITY_SKIP=0 at create),
and against a model of which units may skip.

A unit (wavefront) leaves a launch out when every unit of its neighbour list
stored nothing new in the two launches before, within one gol_step.  The model
(`expected`) restates that from the oracle's fields, the units' rectangles and
their neighbour lists (gol_plan_neighbours, the host model of the same plan): a
unit is quiet at launch n when the oracle's generation nK equals generation nK - 1
on its rectangles.  The kernel may call a quiet unit "changed" (it also compares
up to 7 rows below its block), never the reverse, so the engine skips at most
what the model skips, and exactly that where nothing lives next to a block's
lower edge.

Every engine here streams (resident = 1) classic blocks (handoff = 1) of about
64 rows on one stream, the only plans that skip; the widths give 2 full strips
and the half-strip gaps of test_gpu_halfstrip.py (1, 15 and 30 lane groups).
"""
import re
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BASE = dict(resident=1, handoff=1, streams=1)
# 2 full strips; + the half strip with gaps of 1, 15 (no multiple of 64) and 30 groups
WIDTHS = [64 * 126, 64 * 127, 64 * 141 - 37, 64 * 156]
GLIDER = [(0, 1), (1, 2), (2, 0), (2, 1), (2, 2)]  # moves (+1, +1) every 4 generations
BLOCK = [(0, 0), (0, 1), (1, 0), (1, 1)]
BLINKER = [(0, 0), (0, 1), (0, 2)]


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


def make(pkg, monkeypatch, h, w, skip=True, **kw):
    cfg = dict(BASE, rows_per_wave=64, tb_depth=16, device=0)
    cfg.update(kw)
    if skip:
        monkeypatch.delenv("GOL_DEV_ACTIVITY_SKIP", raising=False)
    else:
        monkeypatch.setenv("GOL_DEV_ACTIVITY_SKIP", "0")
    return pkg.Engine(h, w, **cfg)


def plan(pkg, h, w, **kw):
    cfg = dict(BASE, rows_per_wave=64, tb_depth=16)
    cfg.update(kw)
    return pkg.plan_neighbours(h, w, **cfg)


def expected(oracle, g0, w, rule, K, launches, pl):
    """Units the model lets skip, per launch of one step of K * launches generations
    from g0: [set of unit ids], from the oracle's fields."""
    rects, offs, ids = pl
    units = rects.shape[0]
    streak = np.zeros(units, dtype=np.int64)
    g = g0
    out = []
    for n in range(launches):
        prev = oracle.bp_run(g, w, K - 1, rule)
        g = oracle.bp_run(prev, w, 1, rule)
        diff = g != prev
        quiet = np.ones(units, dtype=bool)
        for u in range(units):
            for r0, r1, q0, q1 in rects[u]:
                if r1 > r0 and diff[r0:r1, q0:q1].any():
                    quiet[u] = False
        skip = set()
        if n >= 1:
            skip = {u for u in range(units) if (streak[ids[offs[u]:offs[u + 1]]] >= 2).all()}
            assert all(quiet[u] for u in skip)  # the argument of DESIGN §4
        out.append(skip)
        streak = np.where(quiet, np.minimum(streak + 1, 255), 0)
    return out


def one_step(e, g0, gens):
    e.load_packed(g0)
    e.reset_timing()
    e.step(gens)
    got = e.store_packed()
    return got, e.activity()


@pytest.mark.parametrize("w", WIDTHS)
def test_frozen_field(pkg, oracle, monkeypatch, w):
    """B/S2, p = 0.5: still after ~7 generations.  Two launches compute, the rest skip."""
    h, K = 333, 16
    g0 = oracle.bp_random(h, w, 3)
    with make(pkg, monkeypatch, h, w) as e:
        units = plan(pkg, h, w)[0].shape[0]
        got, (c, k) = one_step(e, g0, 2 * K)
        assert (c, k) == (2 * units, 0)
        got, (c, k) = one_step(e, g0, 6 * K + 8)
        want = oracle.bp_run(g0, w, 6 * K + 8)
        assert (got == want).all() and e.digest() == oracle.bp_digest(want, w)
        # still by generation 15: launches 1 and 2 end quiet, 3 to 6 skip, the
        # remainder computes
        model = expected(oracle, g0, w, oracle.REF_RULE, K, 6, plan(pkg, h, w))
        assert [len(s) for s in model] == [0, 0] + [units] * 4
        assert (c, k) == (3 * units, 4 * units)
        # from the fixed point: launches 1 and 2 compute, 3 to 6 skip
        got, (c, k) = one_step(e, want, 6 * K + 8)
        assert (got == want).all() and (c, k) == (3 * units, 4 * units)
    with make(pkg, monkeypatch, h, w, skip=False) as e:
        got, (c, k) = one_step(e, g0, 6 * K + 8)
        assert (got == want).all() and (c, k) == (7 * units, 0)


@pytest.mark.parametrize("w", [64 * 126, 64 * 141 - 37])
def test_wake_up(pkg, oracle, monkeypatch, w):
    """B3/S23: 2x2 blocks in otherwise empty tiles, gliders that cross a row-block
    boundary together with a strip boundary (column 4032: strip 0 | strip 1, or the
    half strip) and, at the second width, the half strip's other boundary (column
    4992).  One gol_step of 16 n generations from the start for n = 1..12, so every
    16th generation is compared with full history; the glider leaves its corner
    tile for an interior one, whose larger neighbourhood wakes up units that
    had skipped: the count of computing units rises."""
    h, K, rule = 525, 16, pkg.CONWAY
    g0 = empty(h, w)
    for r in range(20, h - 2, 64):
        for c in (100, 2000, 4500, 6000, w - 40):
            put(g0, r, c, BLOCK)
    put(g0, 40, 4008, GLIDER)
    put(g0, 168, 4968, GLIDER)
    pl = plan(pkg, h, w, rule=rule)
    units = pl[0].shape[0]
    model = expected(oracle, g0, w, rule, K, 12, pl)
    with make(pkg, monkeypatch, h, w, rule=rule) as e, \
            make(pkg, monkeypatch, h, w, skip=False, rule=rule) as off:
        skipped = [0]
        for n in range(1, 13):
            got, (c, k) = one_step(e, g0, K * n)
            ref, (co, ko) = one_step(off, g0, K * n)
            want = oracle.bp_run(g0, w, K * n, rule)
            assert (got == want).all() and (ref == want).all(), f"after {K * n} generations"
            assert c + k == n * units and (co, ko) == (n * units, 0)
            assert k <= sum(len(s) for s in model[:n])
            skipped.append(k)
    per_launch = np.diff(skipped)  # units that skipped launch n
    print("skipped per launch", per_launch.tolist(), "model", [len(s) for s in model])
    assert skipped[-1] > 0 and (per_launch[:2] == 0).all() and (per_launch[2:] > 0).all()
    assert (per_launch[2:] < units).all()
    # The kernel's "changed" holds wherever the model's does, so by induction its
    # streaks are at most the model's and the units it skips are a subset of the
    # model's sets; with equal counts at every launch they are those sets.  Then a
    # unit that skipped launch n and is not in the set of a later launch has
    # computed again.
    assert per_launch.tolist() == [len(s) for s in model]
    woken = [u for n in range(2, 11) for u in model[n] - model[n + 1]]
    assert woken, "no unit wakes up in this scenario"


def test_wake_up_skewed_blocks(pkg, oracle, monkeypatch, model_plans):
    """The same on a plan the planner skews (the first-dispatched units' blocks are
    longer, so the row blocks of neighbouring strips start at different heights)
    with the half strip: blocks everywhere, gliders scattered so that some cross
    row-block and strip boundaries wherever those lie."""
    h, w, K, rule = 16000, 64 * 141 - 37, 16, pkg.CONWAY
    rnd = np.random.default_rng(5)
    g0 = empty(h, w)
    for r in range(10, h - 4, 97):
        for c in range(30, w - 4, 1013):
            put(g0, r, c, BLOCK)
    for _ in range(60):
        r, c = int(rnd.integers(0, (h - 60) // 97)), int(rnd.integers(0, (w - 60) // 1013))
        put(g0, 10 + 97 * r + 30, 30 + 1013 * c + 40, GLIDER)
    cfg = dict(rule=rule, rows_per_wave=0)
    with make(pkg, monkeypatch, h, w, **cfg) as e, make(pkg, monkeypatch, h, w, skip=False, **cfg) as off:
        assert e.age_skew is not None and e.columns[1] > 0 and not e.handoff
        got, (c, k) = one_step(e, g0, 9 * K)
        ref, (co, ko) = one_step(off, g0, 9 * K)
        want = oracle.bp_run(g0, w, 9 * K, rule)
        assert (got == want).all() and (ref == want).all()
        assert c > 0 and k > 0 and ko == 0 and c + k == co


def test_period_2(pkg, oracle, monkeypatch):
    """A blinker alone in a tile: s(t) != s(t - 1) there for ever, so its unit and
    the units that list it never skip; everything else does."""
    h, w, K, rule, n = 333, 64 * 141 - 37, 16, pkg.CONWAY, 8
    g0 = put(empty(h, w), 160, 4500, BLINKER)  # the half strip, rows 128..191
    pl = plan(pkg, h, w, rule=rule)
    rects, offs, ids = pl
    units = rects.shape[0]
    owner = [u for u in range(units) for r0, r1, q0, q1 in rects[u]
             if r0 <= 160 < r1 and q0 <= 4500 // 64 < q1]
    assert len(owner) == 1
    awake = {u for u in range(units) if owner[0] in ids[offs[u]:offs[u + 1]]}
    assert 1 < len(awake) < units
    model = expected(oracle, g0, w, rule, K, n, pl)
    assert all(s == set(range(units)) - awake for s in model[2:])
    with make(pkg, monkeypatch, h, w, rule=rule) as e:
        got, (c, k) = one_step(e, g0, K * n)
        assert (got == oracle.bp_run(g0, w, K * n, rule)).all()
        assert k == (n - 2) * (units - len(awake)) and c + k == n * units


def test_settles_mid_launch(pkg, oracle, monkeypatch):
    """Patterns that become still lifes 1 and 2 generations into the first launch
    (an L of 3 cells -> block, a row of 4 -> beehive): that launch already ends
    quiet, and everything skips from the third on."""
    h, w, K, rule, n = 333, 64 * 127, 16, pkg.CONWAY, 10
    g0 = empty(h, w)
    put(g0, 30, 300, [(0, 0), (0, 1), (1, 0)])
    put(g0, 200, 5000, [(0, 0), (0, 1), (0, 2), (0, 3)])
    pl = plan(pkg, h, w, rule=rule)
    units = pl[0].shape[0]
    model = expected(oracle, g0, w, rule, K, n, pl)
    assert all(len(s) == units for s in model[2:])
    with make(pkg, monkeypatch, h, w, rule=rule) as e:
        got, (c, k) = one_step(e, g0, K * n + 8)
        assert (got == oracle.bp_run(g0, w, K * n + 8, rule)).all()
        assert (c, k) == (3 * units, (n - 2) * units)


@pytest.mark.parametrize("w", [64 * 141 - 37, 64 * 126 + 1])
def test_edges(pkg, oracle, monkeypatch, w):
    """Quiet (blocks) and active (blinkers) tiles on all four borders, in the corners
    and in the last, masked lane group; a height that is no multiple of the block."""
    h, K, rule, n = 64 * 9 + 13, 16, pkg.CONWAY, 6
    g0 = empty(h, w)
    for r, c in ((0, 0), (0, w - 2), (h - 2, 0), (h - 2, w - 2), (0, 5000), (h - 2, 2500),
                 (400, 0), (150, w - 2)):
        put(g0, r, c, BLOCK)
    for r, c in ((1, 2000), (h - 2, 6000), (300, 0), (500, w - 3)):
        put(g0, r, c, BLINKER)
    pl = plan(pkg, h, w, rule=rule)
    units = pl[0].shape[0]
    model = expected(oracle, g0, w, rule, K, n, pl)
    want_k = sum(len(s) for s in model)
    assert 0 < want_k < (n - 2) * units
    with make(pkg, monkeypatch, h, w, rule=rule) as e, \
            make(pkg, monkeypatch, h, w, skip=False, rule=rule) as off:
        got, (c, k) = one_step(e, g0, K * n + 7)
        ref, (co, ko) = one_step(off, g0, K * n + 7)
        want = oracle.bp_run(g0, w, K * n + 7, rule)
        assert (got == want).all() and (ref == want).all()
        assert (c, k) == ((n + 1) * units - want_k, want_k) and ko == 0


def test_step_shapes(pkg, oracle, monkeypatch):
    """gens < 4K (plain launches), repeated steps of one size (the replayed graph),
    and a load between two steps that puts a glider into a tile that had been quiet."""
    h, w, K, rule = 333, 64 * 141 - 37, 16, pkg.CONWAY
    g0 = empty(h, w)
    for r in range(20, h - 2, 64):
        for c in (100, 4500, w - 40):
            put(g0, r, c, BLOCK)
    units = plan(pkg, h, w, rule=rule)[0].shape[0]
    with make(pkg, monkeypatch, h, w, rule=rule) as e:
        got, (c, k) = one_step(e, g0, 3 * K)  # plain path: the third launch skips
        assert (got == g0).all() and (c, k) == (2 * units, units)
        got, (c, k) = one_step(e, g0, 3 * K + 7)
        assert (got == g0).all() and (c, k) == (3 * units, units)
        e.load_packed(g0)
        e.reset_timing()
        for i in range(3):  # capture, then two replays
            e.step(5 * K)
            assert (e.store_packed() == g0).all()
            assert e.activity() == (2 * units * (i + 1), 3 * units * (i + 1))
        g1 = put(g0.copy(), 150, 4400, GLIDER)
        e.load_packed(g1)
        want = g1
        for i in range(3):
            e.step(5 * K)
            want = oracle.bp_run(want, w, 5 * K, rule)
            assert (e.store_packed() == want).all(), f"step {i} after the load"
        c, k = e.activity()
        assert k < 3 * units * 6 and c + k == 5 * units * 6
        # timing on: plain launches that all compute, and the counters say so
        e.load_packed(g1)
        e.reset_timing()
        e.set_timing(1)
        e.step(5 * K)
        assert (e.store_packed() == oracle.bp_run(g1, w, 5 * K, rule)).all()
        assert e.activity() == (5 * units, 0)
        e.set_timing(0)


OFF_CASES = {
    "handoff": dict(tb_depth=8, rows_per_wave=22, handoff=2, streams=1, resident=1),
    "streams": dict(tb_depth=16, streams=2, resident=1),
    "resident": dict(),
    "rank_1_of_1": dict(tb_depth=16, rank=0, nranks=1, handoff=1),
}


@pytest.mark.parametrize("case", sorted(OFF_CASES))
def test_off_where_it_must_be_off(pkg, oracle, monkeypatch, case):
    """Hand-off plans, multi-stream engines, the resident kernel and a stripe engine
    that is the only rank never skip; results are unchanged.  (Two ranks:
    test_rank_engines_never_skip.)"""
    monkeypatch.delenv("GOL_DEV_ACTIVITY_SKIP", raising=False)
    h, w = (512, 4096) if case == "resident" else (600, 64 * 127)
    rule = pkg.CONWAY
    cfg = dict(OFF_CASES[case])
    if case == "rank_1_of_1":
        cfg["transport"] = lambda up, dn: (None, None)
    g0 = empty(h, w)
    for r in range(20, h - 2, 64):
        put(g0, r, 100, BLOCK)
    put(g0, 200, 3000, GLIDER)
    with pkg.Engine(h, w, rule=rule, device=0, **cfg) as e:
        if case == "handoff":
            assert e.handoff
        if case == "resident":
            assert e.resident is not None
        got, (c, k) = one_step(e, g0, 16 * 6)
        assert (got == oracle.bp_run(g0, w, 16 * 6, rule)).all()
        assert k == 0


def test_rank_engines_never_skip(pkg, oracle, monkeypatch):
    """Two rank engines of one field over an in-process loopback transport (each
    rank's gol_step in a thread of its own; the boundary rows change hands at a
    barrier): mostly still stripes with a glider that crosses the seam, several
    halo rounds, against the oracle; no unit skips."""
    monkeypatch.delenv("GOL_DEV_ACTIVITY_SKIP", raising=False)
    h, w, rule, world, gens = 600, 64 * 127, pkg.CONWAY, 2, 16 * 9 + 5
    g0 = empty(h, w)
    for r in range(20, h - 2, 64):
        for c in (100, 4500):
            put(g0, r, c, BLOCK)
    put(g0, 280, 3000, GLIDER)  # rows 280.. -> crosses row 300 after 80 generations
    sent = [None] * world
    gate = threading.Barrier(world, timeout=60)
    out, errs = [None] * world, []

    def transport(rank):
        def xchg(up, dn):
            sent[rank] = (up, dn)
            gate.wait()
            got = (sent[rank - 1][1] if rank > 0 else None,
                   sent[rank + 1][0] if rank + 1 < world else None)
            gate.wait()
            return got
        return xchg

    def run(rank):
        try:
            with pkg.Engine(h, w, rule=rule, device=0, rank=rank, nranks=world, tb_depth=16,
                            handoff=1, halo_depth=32, transport=transport(rank)) as e:
                e.load_packed(g0[e.row0:e.row0 + e.rows])
                e.step(gens)
                out[rank] = (e.row0, e.store_packed(), e.activity())
        except Exception as ex:  # noqa: BLE001
            errs.append(ex)
            gate.abort()

    ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    want = oracle.bp_run(g0, w, gens, rule)
    assert (want != g0).any()
    for row0, got, (c, k) in out:
        assert (got == want[row0:row0 + got.shape[0]]).all()
        assert k == 0


def _dev_kernels(pkg):
    blob = open(pkg.LIB_PATH, "rb").read()
    return re.search(rb"life_tb_kernelILi\d+ELi\dELi\dELb\dELi\dELb1E", blob) is not None


@pytest.mark.parametrize("switch", ["GOL_DEV_PASSES=2", "GOL_DEV_PASSES=3",
                                    "GOL_DEV_XCD_SHIFT=01230123:1"])
def test_dev_switches_turn_it_off(pkg, oracle, monkeypatch, switch):
    """Dev build only.  An engine that may run multi-pass launches rotates four field
    buffers, so "the buffer the launch before last wrote" is not the one a launch
    writes -- also on a plan that falls back to single passes (here: more units
    than one round holds); and the per-XCD row shift moves block boundaries the
    neighbour lists do not model.  Neither may skip: B/S2, frozen, 6K + 8 generations."""
    if not _dev_kernels(pkg):
        pytest.skip("multi-pass kernels and the row shift are in the dev build only "
                    "(GOL_LIB=.../libgol_dev.so)")
    monkeypatch.delenv("GOL_DEV_ACTIVITY_SKIP", raising=False)
    name, val = switch.split("=")
    monkeypatch.setenv(name, val)
    passes = name == "GOL_DEV_PASSES"
    h, w = (18 * 1150, 64 * 126) if passes else (3000, 64 * 126)
    g0 = oracle.bp_random(h, w, 11)
    with pkg.Engine(h, w, device=0, tb_depth=K_DEV, rows_per_wave=18 if passes else 0,
                    **BASE) as e:
        if passes:
            assert e.passes == 1  # the plan fell back to single passes
        got, (c, k) = one_step(e, g0, 6 * K_DEV + 8)
        assert (got == oracle.bp_run(g0, w, 6 * K_DEV + 8)).all()
        assert c > 0 and k == 0


K_DEV = 16

SWEEP_RULES = {"ref": (0, 1 << 2), "conway": (1 << 3, (1 << 2) | (1 << 3)),
               "highlife": ((1 << 3) | (1 << 6), (1 << 2) | (1 << 3))}


@pytest.mark.parametrize("seed", range(24))
def test_differential_sweep(pkg, oracle, monkeypatch, seed):
    """Seeded sweep: B/S2, B3/S23 and HighLife at densities 0.02 to 0.5, skip on
    against skip off against the oracle, over several steps."""
    rnd = np.random.default_rng(1000 + seed)
    name = sorted(SWEEP_RULES)[seed % 3]
    rule = SWEEP_RULES[name]
    p = [0.02, 0.05, 0.12, 0.3, 0.5][int(rnd.integers(5))]
    h = int(rnd.integers(130, 700))
    w = int(rnd.choice(WIDTHS + [3000, 64 * 190 + 5])) - int(rnd.integers(0, 64))
    depth = 12 if name == "highlife" else int(rnd.choice([8, 16]))
    rpw = int(rnd.choice([48, 61, 64, 90]))
    chunks = [int(rnd.choice([3 * depth, 5 * depth + 3, 8 * depth, 4 * depth + 1])) for _ in range(3)]
    g0 = random_field(h, w, p, seed)
    cfg = dict(rule=rule, tb_depth=depth, rows_per_wave=rpw)
    with make(pkg, monkeypatch, h, w, **cfg) as on, make(pkg, monkeypatch, h, w, skip=False, **cfg) as off:
        on.load_packed(g0)
        off.load_packed(g0)
        want = g0
        for gens in chunks:
            on.step(gens)
            off.step(gens)
            want = oracle.bp_run(want, w, gens, rule)
            a, b = on.store_packed(), off.store_packed()
            assert (a == want).all() and (b == want).all(), (name, p, h, w, depth, rpw, gens)
        assert on.digest() == oracle.bp_digest(want, w)
        assert off.activity()[1] == 0
        # B/S2 is still when the second step starts: its third launch skips
        assert name != "ref" or on.activity()[1] > 0
        print(name, p, h, w, depth, rpw, chunks, "activity", on.activity())
