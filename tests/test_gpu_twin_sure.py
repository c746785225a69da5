"""GPU: probe-pass tiles that a remainder launch proved still leave before their field
loads (life_probe.hip, DESIGN §4 "Sure tiles"), next to the same engine with
GOL_DEV_TWIN_SURE=0, with GOL_DEV_TWIN=0 and with GOL_DEV_PROBE_PASS=0, against the CPU
oracle.

Where a step ends with a remainder launch (fewer than K generations since the last
depth-K launch wrote the streaks), a unit that launch finds calm keeps its state for
one more generation, and the calm kernel writes twin[U] = 2 instead of 1.  A tile of
the next step's probe pass all of whose owners have a 2 counts as kept and in
Engine.activity_pass_sure() and returns without a field load.  The field, the six older
counters and activity_pass_kept() are those of the engine with the switch off, which
loads every tile.

`Quad` is test_gpu_twin.Trio with that fourth engine.  The model: a tile is sure iff
Trio's model keeps it and the step before ended with a remainder launch; Trio's lower
and upper bounds carry over unchanged.

Shapes, fields and engine settings are those of test_gpu_probe_pass.py and
test_gpu_twin.py.
"""
import numpy as np
import pytest

import rule_ref as rr
import test_gpu_probe_pass as pp
import test_gpu_twin as tw

K = tw.K
CONWAY = tw.CONWAY
SWITCH = "GOL_DEV_TWIN_SURE"


class Quad(tw.Trio):
    """Trio's three engines (the first with the sure exit on) and one with
    GOL_DEV_TWIN_SURE=0, driven through the same calls."""

    def __init__(self, pkg, oracle, monkeypatch, h, w, rule, depth=K, **kw):
        monkeypatch.delenv(SWITCH, raising=False)
        super().__init__(pkg, oracle, monkeypatch, h, w, rule, depth=depth, **kw)
        cfg = dict(pp.BASE, rows_per_wave=64, tb_depth=depth, device=0, rule=rule)
        cfg.update(kw)
        monkeypatch.setenv(SWITCH, "0")
        self.nosure = pkg.Engine(h, w, **cfg)
        monkeypatch.delenv(SWITCH, raising=False)
        self.last_nosure = tw.six(self.nosure)
        self.kept_nosure = 0
        self.sure = 0
        self.rem = False  # the step before ended with a remainder launch

    def close(self):
        super().close()
        self.nosure.close()

    def load(self, g0):
        super().load(g0)
        self.nosure.load_packed(g0)
        self.rem = False

    def each(self):
        return self.engines + [self.nosure]

    def check(self, tag, kept=None, sure=None):
        """Trio.check, then the fourth engine against the first: field, the six older
        counters, pass_kept; pass_sure is 0 on all but the first.  Returns Trio's pair
        and the first engine's sure count since the last check."""
        cn, got = super().check(tag, kept)
        assert (self.nosure.store_packed() == self.want).all(), tag
        now = tw.six(self.nosure)
        delta = tuple(a - b for a, b in zip(now, self.last_nosure))
        self.last_nosure = now
        assert delta == cn, (tag, delta, cn)
        k = self.nosure.activity_pass_kept() - self.kept_nosure
        self.kept_nosure += k
        assert k == got, (tag, k, got)
        for e in self.engines[1:] + [self.nosure]:
            assert e.activity_pass_sure() == 0, tag
        s = self.engines[0].activity_pass_sure() - self.sure
        self.sure += s
        assert s <= got, (tag, s, got)
        if sure is not None:
            lo, hi = sure
            print(tag, "sure", s, "model", lo, hi, "of", len(self.tiles))
            assert lo <= s <= hi, (tag, s, lo, hi)
        return cn, got, s

    def step(self, gens, tag=""):
        bounds = self.kept_bounds() if gens >= self.depth else (0, 0)
        sure = bounds if self.rem else (0, 0)
        start = self.want
        for e in self.each():
            e.step(gens)
        self.want = self.oracle.bp_run(start, self.w, gens, self.rule)
        self.twin = self.twin_after(start, gens)
        self.rem = gens >= self.depth and gens % self.depth != 0
        return self.check((tag, gens), bounds, sure)


# ---- 0. plumbing, without a GPU


def test_accessor_and_switch_plumbing(pkg):
    """The accessor is exported, declared in the header's list and bound with the
    signature of its siblings; the switch is read by the library."""
    assert "gol_activity_pass_sure" in pkg.EXPORTS
    L = pkg.lib()
    assert L.gol_activity_pass_sure.argtypes == L.gol_activity_pass_kept.argtypes
    assert hasattr(pkg.Engine, "activity_pass_sure")
    # a null engine is an error, not a crash
    assert L.gol_activity_pass_sure(None, None) != 0


gpu = pytest.mark.gpu


# ---- 1. still fields


@gpu
@pytest.mark.parametrize("case", range(6))
def test_still_field(pkg, oracle, monkeypatch, case):
    """test_gpu_probe_pass.still_cases.  Every tile is sure in exactly the steps that
    follow a step ending in a remainder (6K + 8: one launch of 8; 6K + 3: two launches,
    2 + 1); none after the load, after 2K (a depth-K launch writes 1) and after a step
    of K (the held writer).  The six counters are test_gpu_twin.test_still_field's
    pins; 6K + 3 has one more remainder launch than 6K + 8, copied and elided."""
    name, h, w, rule, g0 = list(pp.still_cases(pkg, oracle))[case]
    with Quad(pkg, oracle, monkeypatch, h, w, rule) as t:
        u, n = t.units, len(t.tiles)
        t.load(g0)
        assert t.still() and g0.any()
        pins = {K: (u, 0, 0, u, 0, u), 6 * K + 8: (3 * u, 4 * u, 2 * u, u, 2 * u, u),
                6 * K + 3: (4 * u, 4 * u, 3 * u, u, 3 * u, u), 2 * K: (2 * u, 0, u, u, u, u)}
        steps = (6 * K + 8, 6 * K + 8, 6 * K + 3, 2 * K, 6 * K + 8, K, K)
        want_sure = (0, n, n, n, 0, n, 0)
        for i, gens in enumerate(steps):
            cn, kept, sure = t.step(gens, name)
            assert cn == pins[gens], (name, i, gens, cn)
            assert kept == (0 if i == 0 else n), (name, i, gens)
            assert sure == want_sure[i], (name, i, gens, sure)
        assert t.engines[0].digest() == oracle.bp_digest(g0, w)
        assert t.engines[0].activity_pass_sure() == 4 * n
        t.engines[0].reset_timing()
        assert t.engines[0].activity_pass_sure() == 0 == t.engines[0].activity_pass_kept()


# ---- 2. a stale or insufficient proof must not pass


# test_gpu_twin.STALE (the pattern goes still 1 to 3 generations into the first step's
# last launch: its units compute there), and patterns that go still before the
# remainder starts at t1, r + 1 .. K generations before the step's end and earlier: at
# t1 - 1 (the last generation at which the last depth-K launch still finds it calm),
# t1 - 2, t1 - 3 and K before the end; and exactly at t1 and at t1 + 1 (r and r - 1
# before the end: not calm).  (settles_at's seeds hold no pattern for 15, 25, 31 or 32.)
STALE = tw.STALE + [(3 * K + 8, 3 * K - 1), (3 * K + 8, 3 * K - 3), (3 * K + 8, 2 * K + 3),
                    (3 * K + 8, 3 * K + 1), (2 * K + 8, 2 * K - 2), (2 * K + 8, K + 8),
                    (K + 8, K), (K + 3, K), (K + 3, K - 2), (K + 3, 3)]


@gpu
@pytest.mark.parametrize("gens,t_still", STALE)
def test_stale_proof(pkg, oracle, monkeypatch, gens, t_still):
    """test_gpu_twin.test_stale_twin's field: blocks and a B3/S23 pattern across a
    row-block seam that goes still at generation t_still of a first step of `gens`.
    The field is still after that step, so every tile would be kept by its content;
    the tiles of the units that were not calm in the last launch must load (and store),
    and no tile is sure after a step whose last launch was a depth-K launch."""
    h, w, rule = 525, 64 * 141 - 37, CONWAY
    cells = tw.settles_at(oracle, rule, t_still)
    with Quad(pkg, oracle, monkeypatch, h, w, rule) as t:
        rects = t.rects
        top = next(x for x in range(t.units) if rects[x][0][2] > 0 and 64 <= rects[x][0][1] < h - 64
                   and rects[x][1][1] <= rects[x][1][0])
        seam, q0, q1 = int(rects[top][0][1]), int(rects[top][0][2]), int(rects[top][0][3])
        g0 = tw.blocks(h, w, (100, -40))
        pp.put(g0, seam - 3, 64 * ((q0 + q1) // 2), cells)
        t1 = gens - gens % K if gens % K else gens - K  # where the last launch starts
        b = oracle.bp_run(g0, w, gens, rule)
        assert (oracle.bp_run(b, w, 1, rule) == b).all()
        t.load(g0)
        t.step(gens, "settling")
        assert t.still()
        lo, hi = t.kept_bounds()
        n = len(t.tiles)
        if gens % K == 0:
            assert not t.rem
        elif t_still < t1:
            # s(t1) == s(t1 - 1) everywhere: every unit is calm, every tile sure
            assert t.rem and lo == hi == n
        else:
            assert t.rem and 0 < lo <= hi < n
        cn, kept, sure = t.step(K, "after")
        assert cn[3] == t.units == cn[5]
        assert sure == kept if gens % K else sure == 0


# ---- 3. motion beside still units


@gpu
@pytest.mark.parametrize("w", [64 * 126, 64 * 141 - 37])
def test_wake_up(pkg, oracle, monkeypatch, w):
    """test_gpu_twin.wake_up_field (blocks and two gliders) through steps that end in a
    remainder and steps that do not: sure tiles beside tiles that load and tiles that
    change, the gliders entering units whose tiles were sure the step before."""
    h, rule = 525, CONWAY
    with Quad(pkg, oracle, monkeypatch, h, w, rule) as t:
        t.load(tw.wake_up_field(h, w))
        n = len(t.tiles)
        for i, gens in enumerate([K + 8, K + 8, K + 3, 2 * K, K + 1, 3 * K + 5, K, 2 * K + 7, K + 8]):
            before = t.rem
            cn, kept, sure = t.step(gens, i)
            assert (sure > 0) == before, (i, gens, sure)
            assert sure < n


@gpu
@pytest.mark.parametrize("gens,d", [(K + 8, 0), (K + 8, K), (2 * K - 1, 0), (2 * K - 1, 7),
                                    (2 * K - 1, K - 1), (2 * K - 1, K), (2 * K - 1, K + 1)])
def test_front_arrives(pkg, oracle, monkeypatch, gens, d):
    """A speed-1 front (rule_ref.fuse_towards, a diagonal fuse under B3/S23, as in
    test_gpu_fronts.py) burning down towards a row-block seam three blocks and d cells
    away, in steps of K + 8 and of 2K - 1 (a remainder of K - 1 = 12 + 2 + 1, the proof's
    tight case: no generation of slack): the tile at the seam is sure while the front
    is more than two blocks away (the model's lower bound, which takes a block of 64
    rows more than the lists, says so) and changes in a later step.
    The fuse's other end burns up from the bottom border, 500 rows below."""
    h, w, rule = 64 * 14 - 3, 64 * 126, CONWAY
    with Quad(pkg, oracle, monkeypatch, h, w, rule) as t:
        R = 64 * 5
        assert any(int(t.rects[u][0][0]) == R for u in range(t.units))
        tr, tc, start = R, 2000, 3 * 64 + d
        field, after, length = rr.fuse_towards(h, w, tr, tc, (1, 1), start)
        assert length > start + 500
        tile = (tr // t.tr, (tc // 64) // t.tw)
        rows = slice(tile[0] * t.tr, (tile[0] + 1) * t.tr)
        words = slice(tile[1] * t.tw, (tile[1] + 1) * t.tw)
        t.load(field)
        was_sure = entered = False
        for i in range((start + 2 * K) // gens + 2):
            own = t.twin is not None and t.rem and t.owners[tile] <= t.twin[0]
            before = t.want
            cn, kept, sure = t.step(gens, (d, i))
            assert (t.want == after((i + 1) * gens)).all()
            changed = (before[rows, words] != t.want[rows, words]).any()
            if own and not changed:
                was_sure = True
                assert sure > 0
            elif was_sure and changed:
                entered = True
        assert was_sure and entered, (gens, d)


# ---- 4. every writer withdraws, the generic rule, the off switches


def sure_everything(t, g0):
    t.load(g0)
    t.step(2 * K + 8, "warm")
    cn, kept, sure = t.step(K + 8, "warm")
    assert kept == sure == len(t.tiles)


@gpu
@pytest.mark.parametrize("writer", ["write_rect", "load_packed", "load_ascii", "init_random"])
def test_writer_clears(pkg, oracle, monkeypatch, writer):
    """test_gpu_twin.test_writer_clears from a field on which every tile is sure: a
    writer of the field, then a step of K + 8.  Nothing is kept and nothing is sure; the
    step after that has all of it back."""
    h, w, rule = 333, 64 * 141 - 37, CONWAY
    g0 = tw.blocks(h, w)
    other = tw.blocks(h, w, (300, 3000, 7000))
    with Quad(pkg, oracle, monkeypatch, h, w, rule) as t:
        sure_everything(t, g0)
        if writer == "write_rect":
            win = pp.put(np.zeros((2, 1), dtype=np.uint64), 0, 0, pp.BLOCK)
            for e in t.each():
                e.write_rect(200, 2000, win, 2, pkg.RECT_OR)
            t.want = pp.put(t.want.copy(), 200, 2000, pp.BLOCK)
        elif writer == "load_packed":
            for e in t.each():
                e.load_packed(other)
            t.want = other.copy()
        elif writer == "load_ascii":
            with pkg.Engine(h, w, rule=rule, device=0, tb_depth=K, **pp.BASE) as src:
                src.load_packed(other)
                text = src.store_ascii(h * (w + 1))
            for e in t.each():
                e.load_ascii(text)
            t.want = other.copy()
        else:
            for e in t.each():
                e.init_random(5)
            t.want = oracle.bp_random(h, w, 5)
        t.twin, t.rem = None, False
        cn, kept, sure = t.step(K + 8, writer)
        assert kept == 0 == sure
        if writer != "init_random":
            cn, kept, sure = t.step(K + 8, writer)
            assert kept == sure == len(t.tiles)


@gpu
def test_timed_and_short_steps_clear(pkg, oracle, monkeypatch):
    """A timed step and a step of fewer than K generations between two steps: neither
    is an activity step with a probing launch, both withdraw the record."""
    h, w, rule = 333, 64 * 141 - 37, CONWAY
    with Quad(pkg, oracle, monkeypatch, h, w, rule) as t:
        sure_everything(t, tw.blocks(h, w))
        for e in t.each():
            e.set_timing(1)
            e.step(K + 8)
            e.set_timing(0)
        t.twin, t.rem = None, False
        t.check("timed")
        cn, kept, sure = t.step(K + 8, "after timed")
        assert kept == 0 == sure
        cn, kept, sure = t.step(K - 4, "short")
        assert kept == 0 == sure
        cn, kept, sure = t.step(K + 8, "after short")
        assert kept == 0 == sure
        cn, kept, sure = t.step(K + 8, "again")
        assert kept == sure == len(t.tiles)


@gpu
def test_generic_rule(pkg, oracle, monkeypatch):
    """HighLife (the generic kernel, K = 12) on a block field, and on a soup that never
    settles."""
    h, w, depth = 333, 64 * 141 - 37, 12
    with Quad(pkg, oracle, monkeypatch, h, w, pp.HIGHLIFE, depth=depth) as t:
        n = len(t.tiles)
        t.load(tw.blocks(h, w))
        want = (0, n, n, 0, 0, n)
        for i, gens in enumerate((depth + 8, 2 * depth + 3, 2 * depth, depth, 3 * depth + 1, depth + 1)):
            cn, kept, sure = t.step(gens, "highlife")
            assert sure == want[i] and kept == (n if i else 0), (i, gens)
        t.load(pp.random_field(h, w, 0.5, 11))
        for gens in (depth + 8, 2 * depth + 5, depth + 1):
            cn, kept, sure = t.step(gens, "soup")
            assert sure == 0


@gpu
@pytest.mark.parametrize("env", [SWITCH, "GOL_DEV_TWIN", "GOL_DEV_PROBE_PASS", "GOL_DEV_COPY_PASS"])
def test_off(pkg, oracle, monkeypatch, env):
    """Each switch that turns the feature off, on a still field through steps that end
    in remainders: the oracle's field and pass_sure = 0."""
    tw.clear_switches(monkeypatch)
    monkeypatch.delenv(SWITCH, raising=False)
    monkeypatch.setenv(env, "0")
    h, w, rule = 600, 64 * 127, CONWAY
    g0 = pp.empty(h, w)
    for r in range(20, h - 2, 64):
        pp.put(g0, r, 100, pp.BLOCK)
    with pkg.Engine(h, w, rule=rule, device=0, **dict(pp.BASE, tb_depth=K, rows_per_wave=64)) as e:
        e.load_packed(g0)
        e.reset_timing()
        for gens in (6 * K + 7, 2 * K + 3, K + 8):
            e.step(gens)
            assert (e.store_packed() == g0).all(), gens
        assert e.activity_pass_sure() == 0
        if env == SWITCH:  # the twin test itself goes on
            assert e.activity_pass_kept() > 0
    monkeypatch.delenv(env, raising=False)
