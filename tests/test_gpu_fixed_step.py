"""GPU: on a proven fixed point a step is one kernel (step.cpp step_single_launches,
life_copy.hip life_still_step_kernel, DESIGN §4 "Fixed step"), next to the same engine
with GOL_DEV_FIXED_STEP=0 (the short graph, 11 kernels) and with GOL_DEV_SHORT_STEP=0
(every kernel of the step), against the CPU oracle.

After every step the three engines hold the oracle's field, the eight counters moved
alike, and Engine.activity_state() is identical word for word: what the one kernel
leaves is what the step's kernels leave, the words of the skip's own state included.
Engine.activity_fixed_steps() counts the steps that took the path, on the host.

Shapes, fields and engine settings are those of test_gpu_short_step.py.
"""
import numpy as np
import pytest

import test_gpu_probe_pass as pp
import test_gpu_short_step as ss
import test_gpu_twin as tw
import torus_ref

K = tw.K
CONWAY = tw.CONWAY
FIXED, SHORT = "GOL_DEV_FIXED_STEP", "GOL_DEV_SHORT_STEP"
LONG = ss.LONG  # 6K + 8, 7 launches
gpu = pytest.mark.gpu


class Trio:
    """The engine as shipped (or with GOL_DEV_FIXED_STEP=mode), with
    GOL_DEV_FIXED_STEP=0 and with GOL_DEV_SHORT_STEP=0, driven through the same calls,
    and the oracle's field."""

    def __init__(self, pkg, oracle, monkeypatch, h, w, rule, mode=None, **kw):
        self.oracle, self.h, self.w, self.rule, self.mode = oracle, h, w, rule, mode
        cfg = dict(pp.BASE, rows_per_wave=64, tb_depth=K, device=0, rule=rule)
        cfg.update(kw)
        tw.clear_switches(monkeypatch)
        monkeypatch.delenv("GOL_DEV_TWIN_SURE", raising=False)
        self.engines = []
        for env in ({FIXED: mode} if mode else {}, {FIXED: "0"}, {SHORT: "0"}):
            monkeypatch.delenv(FIXED, raising=False)
            monkeypatch.delenv(SHORT, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            self.engines.append(pkg.Engine(h, w, **cfg))
        monkeypatch.delenv(FIXED, raising=False)
        monkeypatch.delenv(SHORT, raising=False)
        self.on, self.graph, self.full = self.engines
        self.want = None
        self.rebase()

    def rebase(self):
        self.last = [ss.eight(e) for e in self.engines]
        self.short = self.on.activity_short_steps()
        self.fixed = self.on.activity_fixed_steps()
        self.short_graph = self.graph.activity_short_steps()

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
        """Fields against the oracle; the eight counters of what ran since the last
        check, alike on the three engines; the short steps of the first two alike; the
        activity state identical.  Returns the counters, the short and the fixed steps
        counted since."""
        for e in self.engines:
            assert (e.store_packed() == self.want).all(), tag
        now = [ss.eight(e) for e in self.engines]
        delta = [tuple(a - b for a, b in zip(n, l)) for n, l in zip(now, self.last)]
        self.last = now
        assert delta[0] == delta[1] == delta[2], (tag, delta)
        assert self.full.activity_short_steps() == 0, tag
        assert self.full.activity_fixed_steps() == 0 and self.graph.activity_fixed_steps() == 0, tag
        s = self.on.activity_short_steps() - self.short
        sg = self.graph.activity_short_steps() - self.short_graph
        # (GOL_DEV_FIXED_STEP=2 takes the path unseen, where no short graph would run)
        assert s == sg or self.mode == "2", (tag, s, sg)
        self.short += s
        self.short_graph += sg
        f = self.on.activity_fixed_steps() - self.fixed
        self.fixed += f
        st = [e.activity_state() for e in self.engines]
        for name, other in (("fixed step off", st[1]), ("short step off", st[2])):
            assert st[0].shape == other.shape, tag
            bad = np.nonzero(st[0] != other)[0]
            assert bad.size == 0, (tag, name, bad[:8].tolist(), st[0][bad[:8]].tolist(),
                                   other[bad[:8]].tolist())
        return delta[0], s, f

    def step(self, gens, tag="", sync=False, still=False):
        for e in self.engines:
            e.step(gens)
        if sync:
            self.sync()
        if not still:  # (a fixed point stays: the caller has checked that it is one)
            self.want = self.oracle.bp_run(self.want, self.w, gens, self.rule)
        return self.check((tag, gens))


def counts(pkg, h, w, rule):
    cfg = dict(pp.BASE, rows_per_wave=64, rule=rule, tb_depth=K)
    u = int(pkg.plan_neighbours(h, w, **cfg)[0].shape[0])
    n = pkg.plan_probe_tiles(h, w, **cfg)[3].shape[0]
    return u, n


def pin(pkg, gens, u, n):
    """gol_plan_still_step as the eight counters of a step over u units and n tiles."""
    fx = pkg.plan_still_step(K, gens)
    return (fx["computed"] * u, (fx["skipped"] + fx["busy0_add"]) * u, fx["copied"] * u,
            fx["probed"] * u, fx["elided"] * u, fx["pass_probed"] * u,
            fx["kept_passes"] * n, fx["sure_passes"] * n)


# ---- 1. still fields


@gpu
@pytest.mark.parametrize("case", range(6))
def test_still_field(pkg, oracle, monkeypatch, case):
    """test_gpu_probe_pass.still_cases.  Every step after the sync is a fixed step while
    the steps end with a remainder launch; the step of 6K is one too and leaves twin at
    1, so the step after it is a short one whose probe pass finds no sure tile; a sync
    after that step sees the 2s again.  7, 7, 9, 6, 6, 7 launches: both buffers start a
    fixed step."""
    name, h, w, rule, g0 = list(pp.still_cases(pkg, oracle))[case]
    assert (oracle.bp_run(g0, w, 1, rule) == g0).all(), name
    u, n = counts(pkg, h, w, rule)
    assert pin(pkg, LONG, u, n) == (3 * u, 4 * u, 2 * u, u, 2 * u, u, n, n)
    assert pin(pkg, 7 * K + 3, u, n) == (4 * u, 5 * u, 3 * u, u, 3 * u, u, n, n)
    with Trio(pkg, oracle, monkeypatch, h, w, rule) as t:
        t.load(g0)
        cn, short, fixed = t.step(LONG, name, sync=True, still=True)
        assert cn == pin(pkg, LONG, u, n)[:6] + (0, 0) and (short, fixed) == (0, 0), (name, cn)
        for i, gens in enumerate((LONG, LONG, 7 * K + 3, 5 * K + 1, 6 * K)):
            cn, short, fixed = t.step(gens, (name, i), still=True)
            assert cn == pin(pkg, gens, u, n), (name, i, cn)
            assert (short, fixed) == (1, 1), (name, i, short, fixed)
        cn, short, fixed = t.step(LONG, (name, "after 6K"), still=True)
        assert cn == pin(pkg, LONG, u, n)[:6] + (n, 0), (name, cn)
        assert (short, fixed) == (1, 0), name
        t.sync()
        cn, short, fixed = t.step(LONG, (name, "seen again"), still=True)
        assert cn == pin(pkg, LONG, u, n) and (short, fixed) == (1, 1), (name, cn)
        assert t.on.digest() == oracle.bp_digest(g0, w)
        assert t.on.activity_fixed_steps() == 6 and t.on.activity_short_steps() == 7
        t.on.reset_timing()
        assert t.on.activity_fixed_steps() == 0 and t.on.activity_pass_sure() == 0
        assert t.on.activity_pass_kept() == 0


# ---- 2. what a fixed step leaves is a valid start


@gpu
def test_motion_after_fixed_steps(pkg, oracle, monkeypatch):
    h, w, rule = 333, 64 * 141 - 37, CONWAY
    g0 = tw.blocks(h, w)
    with Trio(pkg, oracle, monkeypatch, h, w, rule) as t:
        t.load(g0)
        t.step(LONG, "warm", sync=True, still=True)
        for i, gens in enumerate((LONG, 7 * K + 3)):
            cn, short, fixed = t.step(gens, ("fixed", i), still=True)
            assert fixed == 1
        win = pp.put(np.zeros((3, 1), dtype=np.uint64), 0, 0, pp.GLIDER)
        for e in t.engines:
            e.write_rect(150, 4400, win, 3, pkg.RECT_OR)
        t.want = ss.glider_field(h, w)
        for i, gens in enumerate((LONG, 2 * K + 8, 7 * K + 3)):
            cn, short, fixed = t.step(gens, ("moving", i), sync=True)
            assert (short, fixed) == (0, 0), i
        assert t.on.activity_fixed_steps() == 2


# ---- 3. every writer withdraws


@gpu
@pytest.mark.parametrize("writer", ss.WRITERS)
def test_writer_withdraws(pkg, oracle, monkeypatch, writer):
    """test_gpu_short_step.test_writer_withdraws' writers, after one fixed step: the step
    after the writer is not fixed, and every step is the oracle's."""
    h, w, rule = 333, 64 * 141 - 37, CONWAY
    g0, g1 = tw.blocks(h, w), ss.glider_field(h, w)
    with Trio(pkg, oracle, monkeypatch, h, w, rule) as t:
        if writer == "snapshot_restore":
            t.load(g1)
            for e in t.engines:
                e.snapshot()
        t.load(g0)
        t.step(LONG, "warm", sync=True, still=True)
        cn, short, fixed = t.step(LONG, "armed", sync=True, still=True)
        assert (short, fixed) == (1, 1)
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
            cn, short, fixed = t.step(K - 4, "short step", still=True)
            assert (short, fixed) == (0, 0)
        cn, short, fixed = t.step(LONG, (writer, 0), sync=True)
        assert (short, fixed) == (0, 0), writer
        cn, short, fixed = t.step(LONG, (writer, 1))
        # (after the step of K - 4 the field is still: that sync saw it again)
        assert short == fixed == (1 if writer == "short_step" else 0), writer


# ---- 4. never taken


@gpu
def test_torus_and_composite_never(pkg, oracle, monkeypatch):
    """test_gpu_short_step's torus engine and its engine of two stripes on two streams:
    still fields, synced steps, no fixed step, and no activity state to read."""
    tw.clear_switches(monkeypatch)
    monkeypatch.delenv(SHORT, raising=False)
    monkeypatch.delenv(FIXED, raising=False)
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
        assert e.activity_fixed_steps() == 0 and e.activity_short_steps() == 0
        with pytest.raises(pkg.GolError) as err:
            e.activity_state()
        assert err.value.status == pkg.GOL_ESTATE
    h, w = 600, 64 * 127
    g0 = tw.blocks(h, w)
    with pkg.Engine(h, w, rule=rule, device=0, tb_depth=16, streams=2, resident=1) as e:
        e.load_packed(g0)
        for i in range(3):
            e.step(LONG)
            e.sync()
            assert (e.store_packed() == g0).all(), i
        assert e.activity_fixed_steps() == 0
        with pytest.raises(pkg.GolError) as err:
            e.activity_state()
        assert err.value.status == pkg.GOL_ESTATE


@gpu
def test_timed_step_never(pkg, oracle, monkeypatch):
    """set_timing(8): no graph and no fixed step; the timed step withdraws the host's
    word, and a sync after an untimed step brings it back."""
    h, w, rule = 333, 64 * 141 - 37, CONWAY
    with Trio(pkg, oracle, monkeypatch, h, w, rule) as t:
        t.load(tw.blocks(h, w))
        t.step(LONG, "warm", sync=True, still=True)
        cn, short, fixed = t.step(LONG, "armed", still=True)
        assert (short, fixed) == (1, 1)
        for e in t.engines:
            e.set_timing(8)
        cn, short, fixed = t.step(LONG, "timed", sync=True, still=True)
        assert (short, fixed) == (0, 0)
        for e in t.engines:
            e.set_timing(0)
        cn, short, fixed = t.step(LONG, "after timed", still=True)
        assert (short, fixed) == (0, 0)
        t.sync()
        cn, short, fixed = t.step(LONG, "seen again", still=True)
        assert (short, fixed) == (1, 1)
        # fewer than 5 depth-K launches: neither short nor fixed
        cn, short, fixed = t.step(4 * K + 8, "4K + 8", still=True)
        assert (short, fixed) == (0, 0)


# ---- 5. the switch


@gpu
def test_switch_off(pkg, oracle, monkeypatch):
    """GOL_DEV_FIXED_STEP=0: no fixed step, and the short steps of the parent (Trio.check
    holds the second engine to that after every step; here on the engine alone).
    GOL_DEV_TWIN_SURE=0 and GOL_DEV_STILL_EXIT=0 switch the short step off and this
    path with it."""
    h, w, rule = 333, 64 * 141 - 37, CONWAY
    g0 = tw.blocks(h, w)
    tw.clear_switches(monkeypatch)
    monkeypatch.delenv(SHORT, raising=False)
    monkeypatch.delenv(FIXED, raising=False)
    for env, want_short in (({FIXED: "0"}, 3), ({"GOL_DEV_TWIN_SURE": "0"}, 0),
                            ({"GOL_DEV_STILL_EXIT": "0"}, 0), ({SHORT: "0"}, 0)):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with pkg.Engine(h, w, **dict(pp.BASE, rows_per_wave=64, tb_depth=K, device=0, rule=rule)) as e:
            e.load_packed(g0)
            e.step(LONG)
            e.sync()
            for gens in (LONG, 7 * K + 3, LONG):
                e.step(gens)
            assert (e.store_packed() == g0).all(), env
            assert e.activity_fixed_steps() == 0, env
            assert e.activity_short_steps() == want_short, env
        for k in env:
            monkeypatch.delenv(k, raising=False)


# ---- 6. the error status


@gpu
def test_error_status(pkg, oracle, monkeypatch):
    """GOL_DEV_FIXED_STEP=2 takes the path after every step that ended with a remainder
    launch, whatever the host has seen.  On a still field that is exact.  On the glider
    field, loaded after such a step, the kernel's test fails (the load withdrew twin_ok):
    it writes nothing, gol_sync returns GOL_ESTATE once and names the cause, and the
    engine takes a fresh load and steps it rightly.  An error status, never a fault."""
    h, w, rule = 333, 64 * 141 - 37, CONWAY
    g0, g1 = tw.blocks(h, w), ss.glider_field(h, w)
    with Trio(pkg, oracle, monkeypatch, h, w, rule, mode="2") as t:
        t.load(g0)
        cn, short, fixed = t.step(LONG, "unseen, first", still=True)
        assert fixed == 0
        cn, short, fixed = t.step(LONG, "unseen, second", still=True)
        assert fixed == 1
        for e in t.engines:
            e.load_packed(g1)
        before = t.on.activity_state()
        t.on.step(LONG)
        with pytest.raises(pkg.GolError) as err:
            t.on.sync()
        assert err.value.status == pkg.GOL_ESTATE and "short step" in str(err.value)
        t.on.sync()  # reported once
        assert (t.on.activity_state() == before).all()  # the kernel wrote nothing
        t.load(g1)
        t.rebase()
        cn, short, fixed = t.step(LONG, "after the error", sync=True)
        assert (short, fixed) == (0, 0)
        cn, short, fixed = t.step(4 * K + 5, "after the error", sync=True)
        assert (short, fixed) == (0, 0)
