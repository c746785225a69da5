"""GPU: a step that the host knows starts from a fixed point replays a short graph
(step.cpp step_single_launches, DESIGN §4 "Short step"), next to the same engine with
GOL_DEV_SHORT_STEP=0, against the CPU oracle.

gol_sync reads twin[] where a step has run since it last looked.  twin_ok set and a 2
in every unit's word (written before a remainder launch, test_gpu_twin_sure.py) say
that the whole field equals its generation before.  Until a writer withdraws that, a
captured step with 5 or more depth-K launches leaves out the stencil kernels of
launches 4 .. n, each of which would exit on one load, and runs one wavefront in their
place that repeats their test and adds n - 3 to the counter they add 1 to each.
Engine.activity_short_steps() counts such steps on the host.  The field, the six older
counters, pass_kept and pass_sure are those of the engine with the switch off.

Shapes, fields and engine settings are those of test_gpu_probe_pass.py and
test_gpu_twin.py.
"""
import numpy as np
import pytest

import test_gpu_probe_pass as pp
import test_gpu_twin as tw
import torus_ref

K = tw.K
CONWAY = tw.CONWAY
SWITCH = "GOL_DEV_SHORT_STEP"
LONG = 6 * K + 8  # 7 launches: the buffers swap from step to step, both graphs replay
gpu = pytest.mark.gpu


def eight(e):
    return tw.six(e) + (e.activity_pass_kept(), e.activity_pass_sure())


class Pair:
    """The engine with the short step (first) and with GOL_DEV_SHORT_STEP=0, driven
    through the same calls, and the oracle's field."""

    def __init__(self, pkg, oracle, monkeypatch, h, w, rule, mode=None, **kw):
        self.oracle, self.h, self.w, self.rule = oracle, h, w, rule
        cfg = dict(pp.BASE, rows_per_wave=64, tb_depth=K, device=0, rule=rule)
        cfg.update(kw)
        tw.clear_switches(monkeypatch)
        monkeypatch.delenv("GOL_DEV_TWIN_SURE", raising=False)
        self.engines = []
        for v in (mode, "0"):
            monkeypatch.delenv(SWITCH, raising=False)
            if v is not None:
                monkeypatch.setenv(SWITCH, v)
            self.engines.append(pkg.Engine(h, w, **cfg))
        monkeypatch.delenv(SWITCH, raising=False)
        self.on, self.off = self.engines
        self.want = None
        self.last = [eight(e) for e in self.engines]
        self.short = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for e in self.engines:
            e.close()

    def load(self, g0):
        for e in self.engines:
            e.load_packed(g0)
        self.want = g0.copy()

    def sync(self):
        for e in self.engines:
            e.sync()

    def check(self, tag):
        """Fields against the oracle, the eight counters of what ran since the last
        check against the engine with the switch off; returns them and the short
        steps counted since."""
        for e in self.engines:
            assert (e.store_packed() == self.want).all(), tag
        now = [eight(e) for e in self.engines]
        delta = [tuple(a - b for a, b in zip(n, l)) for n, l in zip(now, self.last)]
        self.last = now
        assert delta[0] == delta[1], (tag, delta)
        assert self.off.activity_short_steps() == 0, tag
        s = self.on.activity_short_steps() - self.short
        self.short += s
        return delta[0], s

    def step(self, gens, tag="", sync=False):
        for e in self.engines:
            e.step(gens)
        if sync:
            self.sync()
        self.want = self.oracle.bp_run(self.want, self.w, gens, self.rule)
        return self.check((tag, gens))


def glider_field(h, w):
    return pp.put(tw.blocks(h, w), 150, 4400, pp.GLIDER)


# ---- 0. plumbing, without a GPU


def test_accessor_and_switch_plumbing(pkg):
    assert "gol_activity_short_steps" in pkg.EXPORTS
    L = pkg.lib()
    assert L.gol_activity_short_steps.argtypes == L.gol_activity_pass_kept.argtypes
    assert hasattr(pkg.Engine, "activity_short_steps")
    assert L.gol_activity_short_steps(None, None) != 0


# ---- 1. still fields


@gpu
@pytest.mark.parametrize("case", range(6))
def test_still_field(pkg, oracle, monkeypatch, case):
    """test_gpu_probe_pass.still_cases: load, a step of 6K + 8, sync, then three steps of
    6K + 8 and one of 7K + 3 with no further sync.  Exactly the steps after the sync are
    short; the counters of every step are test_gpu_twin.test_still_field's pins (7K + 3:
    one more skipped launch and one more remainder launch than 6K + 8).  7 and 9
    launches: the buffers swap from step to step, so both starting buffers' short
    graphs are captured and replayed."""
    name, h, w, rule, g0 = list(pp.still_cases(pkg, oracle))[case]
    with Pair(pkg, oracle, monkeypatch, h, w, rule) as t:
        u = int(pkg.plan_neighbours(h, w, **dict(pp.BASE, rows_per_wave=64, rule=rule,
                                                 tb_depth=K))[0].shape[0])
        tr, twd, ncol, table = pkg.plan_probe_tiles(h, w, **dict(pp.BASE, rows_per_wave=64, rule=rule,
                                                                 tb_depth=K))
        n = table.shape[0]
        pins = {LONG: (3 * u, 4 * u, 2 * u, u, 2 * u, u), 7 * K + 3: (4 * u, 5 * u, 3 * u, u, 3 * u, u)}
        t.load(g0)
        cn, short = t.step(LONG, name, sync=True)
        assert cn == pins[LONG] + (0, 0) and short == 0, (name, cn, short)
        for i, gens in enumerate((LONG, LONG, LONG, 7 * K + 3)):
            cn, short = t.step(gens, (name, i))
            assert cn == pins[gens] + (n, n), (name, i, cn)
            assert short == 1, (name, i)
        assert t.on.digest() == oracle.bp_digest(g0, w)
        assert t.on.activity_short_steps() == 4
        t.on.reset_timing()
        assert t.on.activity_short_steps() == 0
        t.last[0] = eight(t.on)
        t.short = 0
        cn, short = t.step(LONG, "after reset")
        assert short == 1


# ---- 2. not seen, not short


@gpu
def test_not_seen_not_short(pkg, oracle, monkeypatch):
    h, w, rule = 333, 64 * 141 - 37, CONWAY
    with Pair(pkg, oracle, monkeypatch, h, w, rule) as t:
        t.load(tw.blocks(h, w))
        # no gol_sync between the steps (store_packed and the counters wait, they do
        # not look)
        for i in range(3):
            cn, short = t.step(LONG, ("unseen", i))
            assert short == 0
        t.sync()
        # fewer than 5 depth-K launches, captured (4K + 8) and plain (2K + 8)
        for gens in (4 * K + 8, 2 * K + 8, K + 3):
            cn, short = t.step(gens, "few", sync=True)
            assert short == 0
        cn, short = t.step(LONG, "armed")
        assert short == 1
        # a step that ends with a depth-K launch writes 1: it runs short (the flag
        # holds), a sync after it sees nothing new, and the flag stays
        cn, short = t.step(6 * K, "6K", sync=True)
        assert short == 1
        cn, short = t.step(LONG, "after 6K")
        assert short == 1
        # a write, then 6K and a sync: twin is 1, the flag does not come back
        t.load(tw.blocks(h, w))
        cn, short = t.step(6 * K, "6K from a load", sync=True)
        assert short == 0
        cn, short = t.step(6 * K, "6K again", sync=True)
        assert short == 0
        cn, short = t.step(LONG, "value 1", sync=True)
        assert short == 0
        cn, short = t.step(LONG, "value 2")
        assert short == 1
        # timing on: no graph at all; the timed step withdraws the flag
        for e in t.engines:
            e.set_timing(8)
        cn, short = t.step(LONG, "timed", sync=True)
        assert short == 0
        for e in t.engines:
            e.set_timing(0)
        cn, short = t.step(LONG, "after timed")
        assert short == 0
        t.sync()
        cn, short = t.step(LONG, "seen again")
        assert short == 1


# ---- 3. every writer withdraws


WRITERS = ["load_packed", "load_ascii", "init_random", "write_rect", "snapshot_restore", "short_step"]


@gpu
@pytest.mark.parametrize("writer", WRITERS)
def test_writer_withdraws(pkg, oracle, monkeypatch, writer):
    """After the observation (one short step proves it was made), a writer puts a field
    with a glider in place, or a step of fewer than K generations runs.  The next step
    is full and the oracle's, and a sync on the moving field does not arm the flag."""
    h, w, rule = 333, 64 * 141 - 37, CONWAY
    g0, g1 = tw.blocks(h, w), glider_field(h, w)
    with Pair(pkg, oracle, monkeypatch, h, w, rule) as t:
        if writer == "snapshot_restore":
            t.load(g1)
            for e in t.engines:
                e.snapshot()
        t.load(g0)
        t.step(LONG, "warm", sync=True)
        cn, short = t.step(LONG, "armed", sync=True)
        assert short == 1
        if writer == "load_packed":
            t.load(g1)
        elif writer == "load_ascii":
            with pkg.Engine(h, w, rule=rule, device=0, tb_depth=K, **pp.BASE) as src:
                src.load_packed(g1)
                text = src.store_ascii(h * (w + 1))
            for e in t.engines:
                e.load_ascii(text)
            t.want = g1.copy()
        elif writer == "init_random":
            for e in t.engines:
                e.init_random(5)
            t.want = oracle.bp_random(h, w, 5)
        elif writer == "write_rect":
            win = pp.put(np.zeros((3, 1), dtype=np.uint64), 0, 0, pp.GLIDER)
            for e in t.engines:
                e.write_rect(150, 4400, win, 3, pkg.RECT_OR)
            t.want = g1.copy()
        elif writer == "snapshot_restore":
            for e in t.engines:
                e.snapshot_restore()
            t.want = g1.copy()
        else:
            cn, short = t.step(K - 4, "short step")
            assert short == 0
        cn, short = t.step(LONG, (writer, 0), sync=True)
        assert short == 0, writer
        cn, short = t.step(LONG, (writer, 1), sync=True)
        # (after the step of K - 4 the field is still: that sync saw it again)
        assert short == (1 if writer == "short_step" else 0), writer
        cn, short = t.step(LONG, (writer, 2))
        assert short == (1 if writer == "short_step" else 0), writer


@gpu
def test_torus_and_composite_never(pkg, oracle, monkeypatch):
    """A torus engine (the wrap withdraws the record before every round) and an engine
    of two stripes on two streams: still fields, synced steps, no short step."""
    tw.clear_switches(monkeypatch)
    monkeypatch.delenv(SWITCH, raising=False)
    h, w, rule = 300, 500, CONWAY
    g0 = pp.empty(h, w)
    for r in range(20, h - 2, 31):
        for c in (10, 250, w - 1):
            pp.put(g0, r, c, [(0, 0), (1, 0)])
            pp.put(g0, r, (c + 1) % w, [(0, 0), (1, 0)])
    assert (torus_ref.torus_run(oracle, g0, w, 64, rule, chunk=64) == g0).all()
    with pkg.Engine(h, w, rule=rule, semantics=pkg.SEM_TORUS, tb_depth=8, resident=1,
                    handoff=1, halo_depth=64) as e:
        e.load_packed(g0)
        for gens in (300, 300, 64 * 7 + 3):
            e.step(gens)
            e.sync()
            assert (e.store_packed() == g0).all(), gens
        assert e.activity_short_steps() == 0
    h, w = 600, 64 * 127
    g0 = tw.blocks(h, w)
    with pkg.Engine(h, w, rule=rule, device=0, tb_depth=16, streams=2, resident=1) as e:
        e.load_packed(g0)
        for i in range(3):
            e.step(LONG)
            e.sync()
            assert (e.store_packed() == g0).all(), i
        assert e.activity_short_steps() == 0


# ---- 4. not a fixed point


@gpu
@pytest.mark.parametrize("what", ["blinker", "glider"])
def test_not_a_fixed_point(pkg, oracle, monkeypatch, what):
    """A still field and one blinker, or one glider far from every edge: some unit is
    never calm, so five synced steps arm nothing."""
    h, w, rule = 525, 64 * 141 - 37, CONWAY
    g0 = tw.blocks(h, w, (100, 2000, 6000, -40))
    pp.put(g0, 200, 4400, pp.BLINKER if what == "blinker" else pp.GLIDER)
    with Pair(pkg, oracle, monkeypatch, h, w, rule) as t:
        t.load(g0)
        for i, gens in enumerate((LONG, LONG, 7 * K + 3, LONG, 5 * K + 1)):
            cn, short = t.step(gens, (what, i), sync=True)
            assert short == 0, (what, i)
        assert not (oracle.bp_run(t.want, w, 1, rule) == t.want).all()


# ---- 5. the error code


@gpu
def test_error_code(pkg, oracle, monkeypatch):
    """GOL_DEV_SHORT_STEP=2 takes the short graph unseen.  On a still field that is
    exact.  On the glider field the node's test fails: gol_sync returns GOL_ESTATE and
    names the cause, and the engine takes a fresh load and steps it rightly."""
    h, w, rule = 333, 64 * 141 - 37, CONWAY
    g0, g1 = tw.blocks(h, w), glider_field(h, w)
    with Pair(pkg, oracle, monkeypatch, h, w, rule, mode="2") as t:
        t.load(g0)
        cn, short = t.step(LONG, "forced, still", sync=True)
        assert short == 1
        for e in t.engines:
            e.load_packed(g1)
        t.on.step(LONG)
        with pytest.raises(pkg.GolError) as err:
            t.on.sync()
        assert err.value.status == pkg.GOL_ESTATE and "short step" in str(err.value)
        t.on.sync()  # reported once
        t.load(g1)
        t.last[0] = eight(t.on)
        t.short = t.on.activity_short_steps()
        cn, short = t.step(4 * K + 5, "after the error", sync=True)
        assert short == 0
        cn, short = t.step(K + 3, "after the error", sync=True)
        assert short == 0
