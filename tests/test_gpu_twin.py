"""GPU: the probe pass leaves the rows that both field buffers already hold
(life_probe.hip, DESIGN §4 "Probe pass: rows both buffers hold"), next to the same
engine with GOL_DEV_TWIN=0 and with GOL_DEV_PROBE_PASS=0, against the CPU oracle.

The last launch of a step records per unit whether it left its output rows equal to its
input rows (twin[U]); the tile kernel of the next step's probe pass stores no tile
that keeps its state and all of whose owners have that word, and counts it in
Engine.activity_pass_kept().  Every other writer of the field withdraws the record.
After every step the three fields are the oracle's, the six older counters of the
engine with the switch off are those of the engine with it on (the engine without the
probe pass agrees on five and counts no pass_probed, as in test_gpu_probe_pass.py),
and the two reference engines keep nothing.

`Trio` models the count from the oracle's generations, gol_plan_neighbours' rectangles
and lists and the tile shape the library reports: a tile is kept iff generations 0 and
1 of the step agree on it, it has an owner, and every owner was calm (every streak of
its list >= 1) in the last launch of the step before, or took the probe's quiet exit
where that step was one launch.  The kernel's streaks are at most the model's
(test_gpu_copy_elide.py): a unit compares the rows it stores and, past its last row,
some rows of the next row block, fewer than one block of 64 rows.  So the model is
evaluated twice, on the unit's rectangles (an upper bound) and on the rectangles
grown by 64 rows up and down (a lower bound); the count lies between the two, which
are equal on every still field and wherever motion stays a block away from the units
that decide.

Shapes, fields and engine settings are those of test_gpu_probe_pass.py.
"""
import numpy as np
import pytest

import test_gpu_copy_elide as ce
import test_gpu_probe_pass as pp
import torus_ref

pytestmark = pytest.mark.gpu

K = pp.K
CONWAY = (1 << 3, (1 << 2) | (1 << 3))
SWITCHES = pp.SWITCHES + ("GOL_DEV_TWIN",)
PAD = 64  # rows_per_wave: a unit's comparison ends less than one block past its rows


def clear_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def make3(pkg, monkeypatch, h, w, **kw):
    """(twin on, GOL_DEV_TWIN=0, GOL_DEV_PROBE_PASS=0); the switches are read at create."""
    cfg = dict(pp.BASE, rows_per_wave=64, tb_depth=K, device=0)
    cfg.update(kw)
    out = []
    for env in (None, "GOL_DEV_TWIN", "GOL_DEV_PROBE_PASS"):
        clear_switches(monkeypatch)
        if env:
            monkeypatch.setenv(env, "0")
        out.append(pkg.Engine(h, w, **cfg))
    clear_switches(monkeypatch)
    return out


def six(e):
    c, k = e.activity()
    return (c, k, e.activity_copied(), e.activity_probed(), e.activity_elided(),
            e.activity_pass_probed())


def streaks(oracle, g0, w, rule, depth, launches, rects, pad):
    """test_gpu_copy_elide.streaks_after with the rectangles grown by `pad` rows."""
    h, units = g0.shape[0], rects.shape[0]
    streak = np.zeros(units, dtype=np.int64)
    g, out = g0, []
    for _ in range(launches):
        prev = oracle.bp_run(g, w, depth - 1, rule)
        g = oracle.bp_run(prev, w, 1, rule)
        diff = g != prev
        quiet = np.ones(units, dtype=bool)
        for u in range(units):
            for r0, r1, q0, q1 in rects[u]:
                if r1 > r0 and diff[max(0, r0 - pad):min(h, r1 + pad), q0:q1].any():
                    quiet[u] = False
        streak = np.where(quiet, np.minimum(streak + 1, 255), 0)
        out.append(streak.copy())
    return out


class Trio:
    """Three engines driven through the same calls, the oracle's field and the model of
    twin[] (lower and upper bound; None: the record is withdrawn)."""

    def __init__(self, pkg, oracle, monkeypatch, h, w, rule, depth=K, **kw):
        self.pkg, self.oracle, self.h, self.w, self.rule, self.depth = pkg, oracle, h, w, rule, depth
        cfg = dict(rule=rule, tb_depth=depth, **kw)
        self.pl = pkg.plan_neighbours(h, w, **dict(pp.BASE, rows_per_wave=64, **cfg))
        self.rects = self.pl[0]
        self.units = self.rects.shape[0]
        tr, tw, ncol, table = pkg.plan_probe_tiles(h, w, **dict(pp.BASE, rows_per_wave=64, **cfg))
        assert table is not None
        self.tr, self.tw = tr, tw
        # the tiles that hold field rows, from the tile shape the library reports
        self.tiles = [(i, c) for i in range((h + tr - 1) // tr)
                      for c in range(((w + 63) // 64 + tw - 1) // tw)]
        assert len(self.tiles) == table.shape[0] and ncol == ((w + 63) // 64 + tw - 1) // tw
        self.owners = {t: set() for t in self.tiles}
        for u in range(self.units):
            for t in pp.unit_tiles(self.rects, u, h, w, 1, tr, tw):
                self.owners[t].add(u)
        assert all(self.owners.values())
        self.engines = make3(pkg, monkeypatch, h, w, **cfg)
        self.want = None
        self.twin = None  # (lower, upper) sets of units
        self.last = [six(e) for e in self.engines]
        self.kept = 0

    def close(self):
        for e in self.engines:
            e.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def load(self, g0):
        for e in self.engines:
            e.load_packed(g0)
        self.want, self.twin = g0.copy(), None

    def still(self):
        return (self.oracle.bp_run(self.want, self.w, 1, self.rule) == self.want).all()

    def twin_after(self, g0, gens):
        """twin[] as the last launch of a step of `gens` from g0 leaves it."""
        d = self.depth
        launches, rem = gens // d, gens % d
        out = []
        for pad in (PAD, 0):
            if launches >= 1 and (rem or launches >= 2):
                # a remainder reads the streaks of the last depth-d launch, a depth-d
                # launch those of the launch before it
                n = launches if rem else launches - 1
                st = streaks(self.oracle, g0, self.w, self.rule, d, n, self.rects, pad)
                out.append(ce.listed(self.pl, st[n - 1], 1))
            elif launches == 1:
                # one launch: the units that took the probe's quiet exit, the sure ones
                # (lower) or all that the kernel's probe may pass (upper)
                diff = pp.diff_bits(self.oracle, g0, self.w, self.rule)
                out.append(pp.sure(diff, self.h, self.w, d, self.rects, self.tr, self.tw)
                           if pad else pp.may_probe(diff, self.h, self.w, d, self.rects))
            else:
                return None  # fewer than d generations: no launch that probes
        return tuple(out)

    def kept_bounds(self):
        if self.twin is None:
            return 0, 0
        diff = pp.diff_bits(self.oracle, self.want, self.w, self.rule)
        dirty = pp.dirty_tiles(diff, self.tr, self.tw)
        clean = [t for t in self.tiles if t not in dirty]
        return tuple(sum(1 for t in clean if self.owners[t] <= tw) for tw in self.twin)

    def check(self, tag, kept=None):
        """Fields, counters and the kept count of what ran since the last check."""
        on, off, nopass = self.engines
        for e in self.engines:
            assert (e.store_packed() == self.want).all(), tag
        now = [six(e) for e in self.engines]
        delta = [tuple(a - b for a, b in zip(n, l)) for n, l in zip(now, self.last)]
        self.last = now
        assert delta[0] == delta[1], (tag, delta)
        assert delta[0][:5] == delta[2][:5] and delta[2][5] == 0, (tag, delta)
        assert off.activity_pass_kept() == 0 and nopass.activity_pass_kept() == 0, tag
        got = on.activity_pass_kept() - self.kept
        self.kept += got
        if kept is not None:
            lo, hi = kept
            print(tag, "kept", got, "model", lo, hi, "of", len(self.tiles))
            assert lo <= got <= hi, (tag, got, lo, hi)
        return delta[0], got

    def step(self, gens, tag=""):
        # (a step of fewer than `depth` generations has no depth-`depth` launch, so no pass)
        bounds = self.kept_bounds() if gens >= self.depth else (0, 0)
        start = self.want
        for e in self.engines:
            e.step(gens)
        self.want = self.oracle.bp_run(start, self.w, gens, self.rule)
        self.twin = self.twin_after(start, gens)
        return self.check((tag, gens), bounds)


def blocks(h, w, cols=(100, 4500, -40)):
    g0 = pp.empty(h, w)
    for r in range(20, h - 2, 64):
        for c in cols:
            pp.put(g0, r, c if c >= 0 else w + c, pp.BLOCK)
    return g0


def wake_up_field(h, w):
    g0 = blocks(h, w, (100, 2000, 4500, 6000, -40))
    pp.put(g0, 40, 4008, pp.GLIDER)
    pp.put(g0, 168, 4968, pp.GLIDER)
    return g0


# ---- 1. still fields


@pytest.mark.parametrize("case", range(6))
def test_still_field(pkg, oracle, monkeypatch, case):
    """test_gpu_probe_pass.still_cases: nothing is kept in the first step after the
    load, every tile in every later step, whatever the step's last launch was; the six
    counters of each step are those test_still_field pins there and in
    test_gpu_copy_elide.py."""
    name, h, w, rule, g0 = list(pp.still_cases(pkg, oracle))[case]
    with Trio(pkg, oracle, monkeypatch, h, w, rule) as t:
        u, n = t.units, len(t.tiles)
        t.load(g0)
        assert t.still() and g0.any()
        pins = {K: (u, 0, 0, u, 0, u), 6 * K + 8: (3 * u, 4 * u, 2 * u, u, 2 * u, u),
                2 * K: (2 * u, 0, u, u, u, u)}
        for i, gens in enumerate((K, 6 * K + 8, 6 * K + 8, K, 2 * K)):
            cn, kept = t.step(gens, name)
            assert cn == pins[gens], (name, gens)
            assert kept == (0 if i == 0 else n), (name, gens)
        assert t.engines[0].digest() == oracle.bp_digest(g0, w)
        assert t.engines[0].activity_pass_kept() == 4 * n
        t.engines[0].reset_timing()
        assert t.engines[0].activity_pass_kept() == 0


# ---- 2. a stale twin must not pass


def settles_at(oracle, rule, t):
    """test_gpu_copy_elide.settles_between for one t: a 6 x 6 box whose first
    generation with s(t) == s(t + 1) is t."""
    for seed in range(200):
        box = np.random.default_rng(7000 + seed).random((6, 6)) < 0.5
        cells = [(int(r), int(c)) for r, c in zip(*np.nonzero(box))]
        g = pp.put(pp.empty(64, 64), 29, 29, cells)
        for i in range(t + 1):
            nxt = oracle.bp_run(g, 64, 1, rule)
            if (nxt == g).all():
                break
            g = nxt
        else:
            continue
        if i == t:
            return cells
    raise AssertionError("no pattern found")


# (generations of the first step, generation at which the pattern goes still): the last
# launch -- a remainder of one launch and of two, a depth-K launch with the copy pass
# (index 1) and without (index 2) -- starts 1 to 3 generations before that
STALE = [(K + 8, K + 1), (2 * K, K + 2), (K + 3, K + 3), (3 * K, 2 * K + 1), (2 * K + 8, 2 * K + 3)]


@pytest.mark.parametrize("gens,t_still", STALE)
def test_stale_twin(pkg, oracle, monkeypatch, gens, t_still):
    """A B3/S23 pattern across a row-block seam that goes still 1-3 generations into
    the last launch of the first step: its units compute in that launch and end it
    quiet, the other buffer holds the cells from before.  In the step of K that follows
    every tile keeps its state; the pattern's tiles must store all the same."""
    h, w, rule = 525, 64 * 141 - 37, CONWAY
    cells = settles_at(oracle, rule, t_still)
    with Trio(pkg, oracle, monkeypatch, h, w, rule) as t:
        rects = t.rects
        top = next(x for x in range(t.units) if rects[x][0][2] > 0 and 64 <= rects[x][0][1] < h - 64
                   and rects[x][1][1] <= rects[x][1][0])
        seam, q0, q1 = int(rects[top][0][1]), int(rects[top][0][2]), int(rects[top][0][3])
        g0 = blocks(h, w, (100, -40))
        pp.put(g0, seam - 3, 64 * ((q0 + q1) // 2), cells)
        first = gens - gens % K if gens % K else gens - K  # where the last launch starts
        a, b = oracle.bp_run(g0, w, first, rule), oracle.bp_run(g0, w, gens, rule)
        assert 1 <= t_still - first <= 3 and (oracle.bp_run(b, w, 1, rule) == b).all()
        changed = {x for x in range(t.units) for r0, r1, c0, c1 in rects[x]
                   if r1 > r0 and (a[r0:r1, c0:c1] != b[r0:r1, c0:c1]).any()}
        assert changed
        t.load(g0)
        t.step(gens, "settling")
        lo, hi = t.twin
        assert not (changed & hi) and lo, "the pattern's units computed in the last launch"
        assert t.still()
        stale = [x for x in t.tiles if t.owners[x] & changed]
        lo_n, hi_n = t.kept_bounds()
        assert 0 < lo_n <= hi_n <= len(t.tiles) - len(stale)
        cn, kept = t.step(K, "after")
        assert cn[3] == t.units == cn[5]  # every unit sure: nobody stores the tiles' rows later


# ---- 3. every writer clears the flag


def kept_everything(t, g0):
    t.load(g0)
    t.step(2 * K + 8, "warm")
    cn, kept = t.step(K, "warm")
    assert kept == len(t.tiles)


@pytest.mark.parametrize("writer", ["write_rect", "load_packed", "load_ascii", "init_random"])
def test_writer_clears(pkg, oracle, monkeypatch, writer):
    """From a still field on which every tile is kept: a writer of the field, then a
    step of K.  The field is the oracle's and nothing is kept."""
    h, w, rule = 333, 64 * 141 - 37, CONWAY
    g0 = blocks(h, w)
    other = blocks(h, w, (300, 3000, 7000))
    with Trio(pkg, oracle, monkeypatch, h, w, rule) as t:
        kept_everything(t, g0)
        if writer == "write_rect":
            # a block into an empty tile: still after the write, so only the withdrawn
            # record makes the tile store
            win = pp.put(np.zeros((2, 1), dtype=np.uint64), 0, 0, pp.BLOCK)
            for e in t.engines:
                e.write_rect(200, 2000, win, 2, pkg.RECT_OR)
            t.want = pp.put(t.want.copy(), 200, 2000, pp.BLOCK)
        elif writer == "load_packed":
            for e in t.engines:
                e.load_packed(other)
            t.want = other.copy()
        elif writer == "load_ascii":
            with pkg.Engine(h, w, rule=rule, device=0, tb_depth=K, **pp.BASE) as src:
                src.load_packed(other)
                text = src.store_ascii(h * (w + 1))
            for e in t.engines:
                e.load_ascii(text)
            t.want = other.copy()
        else:
            for e in t.engines:
                e.init_random(5)
            t.want = oracle.bp_random(h, w, 5)
        t.twin = None
        assert writer == "init_random" or t.still()
        cn, kept = t.step(K, writer)
        assert kept == 0
        if writer != "init_random":  # ... and the record is back
            cn, kept = t.step(K, writer)
            assert kept == len(t.tiles)


def test_timed_step_clears(pkg, oracle, monkeypatch):
    """A timed step of K between two steps, blocks and a glider: its launches are not
    activity launches and leave the glider's old cells in the other buffer."""
    h, w, rule = 333, 64 * 141 - 37, CONWAY
    g0 = pp.put(blocks(h, w), 150, 4400, pp.GLIDER)
    with Trio(pkg, oracle, monkeypatch, h, w, rule) as t:
        t.load(g0)
        t.step(2 * K + 8, "warm")
        cn, kept = t.step(K, "warm")
        assert 0 < kept < len(t.tiles)
        for e in t.engines:
            e.set_timing(1)
            e.step(K)
            e.set_timing(0)
        t.want = oracle.bp_run(t.want, w, K, rule)
        t.twin = None
        t.check("timed")
        cn, kept = t.step(K, "after")
        assert kept == 0
        cn, kept = t.step(K, "again")
        assert kept > 0


def test_torus_keeps_nothing(pkg, oracle, monkeypatch):
    """test_gpu_probe_pass.test_torus' engine, a still object across the edge: the wrap
    kernel writes the ghost cells before every round, so the inner engine's record is
    withdrawn every time and nothing is ever kept."""
    h, w, rule = 300, 500, CONWAY
    g0 = pp.empty(h, w)
    for r in range(20, h - 2, 31):
        for c in (10, 250, w - 1):
            pp.put(g0, r, c, [(0, 0), (1, 0)])
            pp.put(g0, r, (c + 1) % w, [(0, 0), (1, 0)])
    assert (torus_ref.torus_run(oracle, g0, w, 64, rule, chunk=64) == g0).all()
    seen = []
    for env in (None, "GOL_DEV_TWIN", "GOL_DEV_PROBE_PASS"):
        clear_switches(monkeypatch)
        if env:
            monkeypatch.setenv(env, "0")
        with pkg.Engine(h, w, rule=rule, semantics=pkg.SEM_TORUS, tb_depth=8, resident=1,
                        handoff=1, halo_depth=64) as e:
            e.load_packed(g0)
            e.reset_timing()
            for gens in (300, 64, 8):
                e.step(gens)
                assert (e.store_packed() == g0).all(), (env, gens)
            assert e.activity_pass_kept() == 0
            seen.append(six(e))
    assert seen[0] == seen[1] and seen[0][:5] == seen[2][:5] and seen[2][5] == 0
    assert seen[0][5] > 0


# ---- 4. step shapes


SHAPES = [K + 8, K + 3, 2 * K, 3 * K, 40 * K, K, K - 4, K + 8, 3 * K + 5, 5 * K + 3, K, 7]


@pytest.mark.parametrize("field", ["still", "wake_up"])
def test_step_shapes(pkg, oracle, monkeypatch, field):
    """The last launch a remainder of one launch and of two (3 = 2 + 1), a depth-K
    launch at 2K, 3K and 40K, the step's only launch (K), no probing launch at all (fewer
    than K generations), on the plain path (under 4K generations) and on the captured
    one, each followed by a step that shows what the record says."""
    h, w, rule = 525, 64 * 141 - 37, CONWAY
    g0 = blocks(h, w, (100, 2000, 4500, 6000, -40)) if field == "still" else wake_up_field(h, w)
    with Trio(pkg, oracle, monkeypatch, h, w, rule) as t:
        t.load(g0)
        n, prev = len(t.tiles), None
        for gens in SHAPES:
            cn, kept = t.step(gens, field)
            if field == "still":
                assert kept == (n if prev is not None and prev >= K and gens >= K else 0), (prev, gens)
            prev = gens
        assert field == "still" or t.kept > 0


def test_captured_step(pkg, oracle, monkeypatch):
    """A captured step of 40 K + 8 replayed five times on a still field, then on the
    wake-up field, then on the still field again with a step of K in between."""
    h, w, rule, gens = 525, 64 * 126, CONWAY, 40 * K + 8
    g0 = blocks(h, w, (100, 2000, 4500, 6000, -40))
    g1 = wake_up_field(h, w)
    with Trio(pkg, oracle, monkeypatch, h, w, rule) as t:
        u, n = t.units, len(t.tiles)
        t.load(g0)
        for i in range(5):
            cn, kept = t.step(gens, ("still", i))
            assert cn == (3 * u, 38 * u, 2 * u, u, 2 * u, u) and kept == (n if i else 0)
        t.load(g1)
        for i in range(2):
            cn, kept = t.step(gens, ("wake-up", i))
            assert kept == 0 if i == 0 else 0 < kept < n
        t.load(g0)
        cn, kept = t.step(gens, "still again")
        assert kept == 0
        cn, kept = t.step(K, "K")
        assert kept == n
        cn, kept = t.step(gens, "after K")
        assert cn == (3 * u, 38 * u, 2 * u, u, 2 * u, u) and kept == n


# ---- 5. a moving field


@pytest.mark.parametrize("w", [64 * 126, 64 * 141 - 37])
def test_wake_up(pkg, oracle, monkeypatch, w):
    """The wake-up field launch by launch (steps of K), then in longer steps: kept
    tiles beside tiles that store and tiles that change."""
    h, rule = 525, CONWAY
    with Trio(pkg, oracle, monkeypatch, h, w, rule) as t:
        t.load(wake_up_field(h, w))
        for i, gens in enumerate([K] * 6 + [2 * K, 2 * K + 7, 3 * K, K + 3]):
            cn, kept = t.step(gens, i)
            assert (kept > 0) == (i > 0), i
            assert kept < len(t.tiles)


@pytest.mark.parametrize("name", ["ref", "conway", "highlife"])
def test_soup(pkg, oracle, monkeypatch, name):
    """A p = 0.5 soup under the three rules, step after step."""
    rule = {"ref": pkg.REF_RULE, "conway": CONWAY, "highlife": pp.HIGHLIFE}[name]
    depth = 12 if name == "highlife" else K
    h, w = 333, 64 * 141 - 37
    with Trio(pkg, oracle, monkeypatch, h, w, rule, depth=depth) as t:
        t.load(pp.random_field(h, w, 0.5, 11))
        for gens in (3 * depth + 5, 2 * depth, depth, depth + 8):
            t.step(gens, name)
        # B/S2 is still after a few generations; the other two never are
        assert (t.kept > 0) == (name == "ref")


# ---- 6. off where it must be off


OFF = dict(pp.OFF_CASES, copy_pass_off=dict(pp.BASE, tb_depth=16, rows_per_wave=64),
           twin_off=dict(pp.BASE, tb_depth=16, rows_per_wave=64))


@pytest.mark.parametrize("case", sorted(OFF))
def test_off(pkg, oracle, monkeypatch, case):
    """test_gpu_probe_pass.OFF_CASES, GOL_DEV_COPY_PASS=0 and GOL_DEV_TWIN=0: three steps
    on a still field, the oracle's field and nothing kept."""
    clear_switches(monkeypatch)
    env = {"skip_off": "GOL_DEV_ACTIVITY_SKIP", "probe_off": "GOL_DEV_STILL_PROBE",
           "copy_pass_off": "GOL_DEV_COPY_PASS", "twin_off": "GOL_DEV_TWIN"}.get(case)
    if env:
        monkeypatch.setenv(env, "0")
    h, w, rule = 600, 64 * 127, CONWAY
    g0 = pp.empty(h, w)
    for r in range(20, h - 2, 64):
        pp.put(g0, r, 100, pp.BLOCK)
    with pkg.Engine(h, w, rule=rule, device=0, **OFF[case]) as e:
        e.load_packed(g0)
        e.reset_timing()
        if case == "timing":
            e.set_timing(1)
        for gens in (16 * 6 + 7, 16 * 2, 16):
            e.step(gens)
            assert (e.store_packed() == g0).all(), gens
        assert e.activity_pass_kept() == 0
        if case in ("copy_pass_off", "twin_off"):  # the probe pass itself goes on
            assert e.activity_pass_probed() > 0
