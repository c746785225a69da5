"""GPU: pending fixed steps (step.cpp flush_still, csrc/still_pending.h, DESIGN §4 "Fixed
step").  Consecutive fixed steps only book their effect on the host; one
life_still_step_kernel with the sums runs when somebody looks at the activity state or
the error word, or enqueues work that does.

Four engines go through the same calls: the engine as shipped, the one with
GOL_DEV_FIXED_STEP=0 (the short graph), the one with GOL_DEV_SHORT_STEP=0 (every kernel
of every step) -- test_gpu_fixed_step.Trio -- and the one with GOL_DEV_FIXED_DEFER=0 (one
kernel per fixed step).  After a run of steps with no call between them they hold the
oracle's field, the eight counters moved alike and Engine.activity_state() is identical
word for word; Engine.activity_fixed_launches() tells one kernel from n.

Shapes and fields are those of test_gpu_fixed_step.py / test_gpu_probe_pass.py.
"""
import numpy as np
import pytest

import test_gpu_fixed_step as fs
import test_gpu_probe_pass as pp
import test_gpu_short_step as ss
import test_gpu_twin as tw

K = fs.K
CONWAY = fs.CONWAY
LONG = fs.LONG  # 6K + 8, 7 launches: the buffers swap
DEFER = "GOL_DEV_FIXED_DEFER"
gpu = pytest.mark.gpu

# lengths of a run's steps but the last: 7, 8, 6 and 11 launches; the last is 6K, whose
# last launch has depth K and leaves twin at 1
RUN = (LONG, LONG + 1, 5 * K + 3, 8 * K + 15)


class Quad(fs.Trio):
    """Trio and a fourth engine with GOL_DEV_FIXED_DEFER=0 (and the Trio's mode)."""

    def __init__(self, pkg, oracle, monkeypatch, h, w, rule, mode=None, **kw):
        super().__init__(pkg, oracle, monkeypatch, h, w, rule, mode=mode, **kw)
        cfg = dict(pp.BASE, rows_per_wave=64, tb_depth=K, device=0, rule=rule)
        cfg.update(kw)
        monkeypatch.setenv(DEFER, "0")
        if mode:
            monkeypatch.setenv(fs.FIXED, mode)
        self.each = pkg.Engine(h, w, **cfg)
        monkeypatch.delenv(DEFER, raising=False)
        monkeypatch.delenv(fs.FIXED, raising=False)
        self.engines.append(self.each)
        self.rebase()

    def check(self, tag):
        out = super().check(tag)
        # the fourth engine went through every call of the first: all of it alike
        assert ss.eight(self.each) == ss.eight(self.on), tag
        assert self.each.activity_fixed_steps() == self.on.activity_fixed_steps(), tag
        assert self.each.activity_short_steps() == self.on.activity_short_steps(), tag
        a, b = self.on.activity_state(), self.each.activity_state()
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (tag, "one kernel per step", bad[:8].tolist(), a[bad[:8]].tolist(),
                               b[bad[:8]].tolist())
        return out

    def launches(self):
        return self.on.activity_fixed_launches(), self.each.activity_fixed_launches()

    def quiet(self, lengths):
        """Steps with no call between them."""
        for gens in lengths:
            for e in self.engines:
                e.step(gens)


def add(pins):
    return tuple(sum(p[i] for p in pins) for i in range(8))


def armed(pkg, oracle, monkeypatch, g0=None, mode=None):
    """test_gpu_fixed_step's blocks field after a synced step: the next step is fixed."""
    h, w, rule = 333, 64 * 141 - 37, CONWAY
    t = Quad(pkg, oracle, monkeypatch, h, w, rule, mode=mode)
    t.load(tw.blocks(h, w) if g0 is None else g0)
    t.step(LONG, "warm", sync=True, still=True)
    return t


# ---- 0. the switch, without a GPU


def test_plumbing(pkg):
    assert hasattr(pkg.Engine, "activity_fixed_launches")
    assert "gol_activity_fixed_launches" in pkg.EXPORTS


# ---- 1. runs of steps


@gpu
@pytest.mark.parametrize("n,odd,case", [(2, 0, 0), (2, 1, 3), (3, 0, 4), (3, 1, 1), (17, 0, 5),
                                        (17, 1, 2)])
def test_run_of_steps(pkg, oracle, monkeypatch, n, odd, case):
    """n steps with no call between them, of differing lengths, the last of 6K.  odd: one
    fixed step of 7 launches goes before, so that the run starts on the other buffer."""
    name, h, w, rule, g0 = list(pp.still_cases(pkg, oracle))[case]
    assert (oracle.bp_run(g0, w, 1, rule) == g0).all(), name
    u, tiles = fs.counts(pkg, h, w, rule)
    with Quad(pkg, oracle, monkeypatch, h, w, rule) as t:
        t.load(g0)
        t.step(LONG, name, sync=True, still=True)
        if odd:
            cn, short, fixed = t.step(LONG, (name, "odd"), still=True)
            assert (short, fixed) == (1, 1)
        l0 = t.launches()
        lengths = [RUN[i % len(RUN)] for i in range(n - 1)] + [6 * K]
        t.quiet(lengths)
        assert t.launches() == (l0[0], l0[1] + n), name  # (host counts: no flush yet)
        cn, short, fixed = t.check((name, "run", n))
        assert cn == add([fs.pin(pkg, g, u, tiles) for g in lengths]), (name, cn)
        assert (short, fixed) == (n, n), (name, short, fixed)
        assert t.launches() == (l0[0] + 1, l0[1] + n), name
        # the 6K step left twin at 1: the next step is a short one, not fixed
        cn, short, fixed = t.step(LONG, (name, "after 6K"), still=True)
        assert (short, fixed) == (1, 0), name
        assert t.launches() == (l0[0] + 1, l0[1] + n), name
        assert t.on.digest() == oracle.bp_digest(g0, w)


# ---- 2. every flush point


GETTERS = ["activity", "activity_copied", "activity_probed", "activity_elided",
           "activity_pass_probed", "activity_pass_kept", "activity_pass_sure"]
POINTS = ["sync"] + GETTERS + ["activity_state", "reset_timing", "step_K", "step_past_6K",
                               "load_packed", "write_rect", "snapshot_compare", "set_timing"]


@gpu
@pytest.mark.parametrize("point", POINTS)
def test_flush_point(pkg, oracle, monkeypatch, point):
    """Two steps pending, then the call: one kernel, and everything as on the engines
    that ran every step's kernels."""
    h, w = 333, 64 * 141 - 37
    g1 = ss.glider_field(h, w)
    with armed(pkg, oracle, monkeypatch) as t:
        l0 = t.launches()
        t.quiet((LONG, 7 * K + 3))
        assert t.launches() == (l0[0], l0[1] + 2)
        fixed_steps, moving = 2, False
        if point in ("sync", "activity_state", "reset_timing") or point in GETTERS:
            for e in t.engines:
                getattr(e, point)()
            if point == "reset_timing":
                assert t.launches() == (0, 0)
                assert t.on.activity_fixed_steps() == 0
                t.rebase()
                l0, fixed_steps = (-1, -2), 0
        elif point == "step_K":
            t.quiet((K,))
        elif point == "step_past_6K":
            t.quiet((6 * K,))  # fixed, pending with the two
            assert t.launches() == (l0[0], l0[1] + 3)
            t.quiet((LONG,))  # twin is 1: a short step, whose kernels read the state
            l0, fixed_steps = (l0[0], l0[1] + 1), 3
        elif point == "load_packed":
            t.load(g1)
            moving = True
        elif point == "write_rect":
            win = pp.put(np.zeros((3, 1), dtype=np.uint64), 0, 0, pp.GLIDER)
            for e in t.engines:
                e.write_rect(150, 4400, win, 3, pkg.RECT_OR)
            t.want = g1.copy()
            moving = True
        elif point == "snapshot_compare":
            for e in t.engines:
                e.snapshot()
            assert t.launches() == (l0[0], l0[1] + 2)  # (a copy of field words)
            for e in t.engines:
                assert e.snapshot_same()
        elif point == "set_timing":
            for e in t.engines:
                e.set_timing(8)
            assert t.launches() == (l0[0], l0[1] + 2)  # (touches no stream)
            t.quiet((LONG,))  # a timed step is no fixed step: its launches flush
        assert t.launches() == (l0[0] + 1, l0[1] + 2), point
        cn, short, fixed = t.check(point)
        assert fixed == fixed_steps, (point, fixed)
        assert t.launches() == (l0[0] + 1, l0[1] + 2), point
        if point == "set_timing":
            for e in t.engines:
                e.set_timing(0)
        if moving:
            for i, gens in enumerate((LONG, 2 * K + 8, 7 * K + 3)):
                cn, short, fixed = t.step(gens, (point, "moving", i), sync=True)
                assert (short, fixed) == (0, 0), (point, i)
        else:
            # the field is still what it was, and a sync sees it so again
            t.sync()
            t.step(LONG, (point, "again"), sync=True, still=True)
            cn, short, fixed = t.step(LONG, (point, "fixed again"), still=True)
            assert (short, fixed) == (1, 1), point


@gpu
def test_close_with_steps_pending(pkg, oracle, monkeypatch):
    """close() drops pending steps; the next engine starts clean, over and over."""
    h, w, rule = 333, 64 * 141 - 37, CONWAY
    g0 = tw.blocks(h, w)
    tw.clear_switches(monkeypatch)
    for k in (fs.FIXED, fs.SHORT, DEFER):
        monkeypatch.delenv(k, raising=False)
    cfg = dict(pp.BASE, rows_per_wave=64, tb_depth=K, device=0, rule=rule)
    for i in range(4):
        e = pkg.Engine(h, w, **cfg)
        e.load_packed(g0)
        e.step(LONG)
        e.sync()
        assert e.activity_fixed_launches() == 0 and e.activity_fixed_steps() == 0, i
        e.step(LONG)
        e.step(7 * K + 3)
        assert e.activity_fixed_steps() == 2 and e.activity_fixed_launches() == 0, i
        if i == 3:
            assert (e.store_packed() == g0).all()
            e.sync()
            assert e.activity_fixed_launches() == 1
        e.close()


# ---- 3. readers of the field


@gpu
def test_field_readers(pkg, oracle, monkeypatch):
    """With steps pending the field is the fixed point, in whichever buffer."""
    h, w = 333, 64 * 141 - 37
    with armed(pkg, oracle, monkeypatch) as t:
        g0 = t.want
        for lengths in ((LONG, 7 * K + 3), (LONG,)):  # ends on either buffer
            t.quiet(lengths)
            assert (t.on.store_packed() == g0).all()
            t.quiet(lengths)
            assert t.on.digest() == oracle.bp_digest(g0, w)
            t.quiet(lengths)
            win = t.on.read_rect(0, 4480, 40, 130)
            for e in t.engines[1:]:
                assert (e.read_rect(0, 4480, 40, 130) == win).all()
            assert win.any()
            t.sync()
            cn, short, fixed = t.check(("readers", lengths))
            assert fixed == 3 * len(lengths)


# ---- 4. a proof that fails


@gpu
def test_failed_proof(pkg, oracle, monkeypatch):
    """test_gpu_fixed_step.test_error_status with two steps pending: the one kernel's
    test fails as the first step's would, it writes the error word alone, the next sync
    returns GOL_ESTATE once, and the engine goes on as after the single step."""
    h, w = 333, 64 * 141 - 37
    g0, g1 = tw.blocks(h, w), ss.glider_field(h, w)
    with Quad(pkg, oracle, monkeypatch, h, w, CONWAY, mode="2") as t:
        t.load(g0)
        cn, short, fixed = t.step(LONG, "unseen, first", still=True)
        assert fixed == 0
        t.quiet((LONG, 7 * K + 3))
        cn, short, fixed = t.check("unseen, two pending")
        assert fixed == 2
        for e in t.engines:
            e.load_packed(g1)
        for e in (t.on, t.each):
            before = e.activity_state()
            l0 = e.activity_fixed_launches()
            e.step(LONG)
            e.step(7 * K + 3)
            with pytest.raises(pkg.GolError) as err:
                e.sync()
            assert err.value.status == pkg.GOL_ESTATE and "short step" in str(err.value)
            e.sync()  # reported once
            assert (e.activity_state() == before).all()  # the kernels wrote nothing
            assert e.activity_fixed_launches() - l0 == (1 if e is t.on else 2)
        t.load(g1)
        t.rebase()
        cn, short, fixed = t.step(LONG, "after the error", sync=True)
        assert (short, fixed) == (0, 0)
        cn, short, fixed = t.step(4 * K + 5, "after the error", sync=True)
        assert (short, fixed) == (0, 0)
