"""GPU: seeded programs of public calls on settling fields (tests/call_model.py) through
every engine kind that remembers something between calls, against the numpy model.

What an engine remembers so that a still field costs less -- streaks, copy-through,
twin[], the host's still_seen / twin_two, the short graph, pending fixed steps, the cache
of captured step graphs; halo_fresh, the ghosts and the per-stripe snapshot slots on the
other kinds -- is right only if every writer of the field withdraws its part of it.  The
hand-written tests put one call between two steps; here call orders are drawn: two
writers in a row, writes at tile edges and unit seams of a field the host has seen still,
restores of a moving snapshot onto a fixed point, a dozen graphable lengths through one
engine.  The field is the contract: nothing is asserted of the counters but the sums that
show the still machinery ran (and that it never ran with GOL_DEV_ACTIVITY_SKIP=0).

Checks happen only where the program has a reader and after its last op, so "no look
between steps" stays what the program says.  GOL_CALLSEQ_CHECK_EVERY=1 compares the field
after every op (to localise a failure by hand), GOL_CALLSEQ_SCALE=n runs n times the
seeds.  test_call_model_host.py holds the model's own tests and the generator's floors.
"""
import os

import numpy as np
import pytest

import call_model as cm
import torus_ref

pytestmark = pytest.mark.gpu

SCALE = max(1, int(os.environ.get("GOL_CALLSEQ_SCALE", "1")))
CHECK_EVERY = os.environ.get("GOL_CALLSEQ_CHECK_EVERY") == "1"
SKIP_SWITCH = "GOL_DEV_ACTIVITY_SKIP"
SNAPSHOT_OPS = ("snapshot", "restore", "same", "diff", "until")
HOST_COUNTS = ("activity_short_steps", "activity_fixed_steps", "activity_fixed_launches")

CASES = [(kind, rule, seed) for kind, spec in cm.KINDS.items() for rule, n in spec["rules"]
         for seed in range(n * SCALE)]
# Programs beyond the seeds above that once failed, kept by name (kind, rule, seed) with
# one line on what was stale.  None so far.
REGRESSIONS = []
CASES += [c for c in REGRESSIONS if c not in CASES]
# (kind, rule, seed) -> the counters of the program's engines, for test_still_machinery_ran
_results = {}


class Failure(AssertionError):
    pass


def clear_dev_switches(monkeypatch, autotune_off=True):
    for name in list(os.environ):
        if name.startswith("GOL_DEV_") and name != "GOL_DEV_AUTOTUNE":
            monkeypatch.delenv(name, raising=False)
    if autotune_off:
        monkeypatch.setenv("GOL_DEV_AUTOTUNE", "0")
    else:
        monkeypatch.delenv("GOL_DEV_AUTOTUNE", raising=False)


def make_engines(pkg, monkeypatch, case):
    """The engine as shipped and, for the kinds with the still machinery, the one created
    under GOL_DEV_ACTIVITY_SKIP=0 (the switches are read at create)."""
    h, w, rule, kind = case["h"], case["w"], case["rule"], case["kind"]
    clear_dev_switches(monkeypatch, autotune_off=kind != "default")
    if kind == "group":
        return [pkg.Group(h, w, 3, rule=rule, **case["cfg"])]
    engines = [pkg.Engine(h, w, rule=rule, device=0, **case["cfg"])]
    if cm.KINDS[kind].get("skip"):
        monkeypatch.setenv(SKIP_SWITCH, "0")
        engines.append(pkg.Engine(h, w, rule=rule, device=0, **case["cfg"]))
        monkeypatch.delenv(SKIP_SWITCH)
    return engines


def members(e):
    return getattr(e, "members", [e])


def engine_op(pkg, oracle, e, op, case, first, window):
    """One op on one engine; a reader's answer in the model's form."""
    name, w = op[0], case["w"]
    group = hasattr(e, "members")
    if name == "step":
        e.step(op[1])
    elif name == "sync":
        e.sync()
    elif name == "write":
        _, y, x, win, o = op
        e.write_rect(y, x, torus_ref.pack(cm.WINDOWS[win]), cm.WINDOWS[win].shape[1], o)
    elif name == "rewrite":
        _, y, x, rh, rw = op
        e.write_rect(y, x, window, rw, pkg.RECT_SET)
    elif name == "load":
        e.load_packed(torus_ref.pack(cm.make_field(oracle, op[1], case["h"], w)))
    elif name == "load_ascii":
        e.load_ascii(oracle.bp_unpack(torus_ref.pack(cm.make_field(oracle, op[1], case["h"], w)), w))
    elif name == "init_random":
        e.init_random(op[1])
    elif name == "snapshot":
        e.snapshot()
    elif name == "restore":
        e.snapshot_restore()
    elif name == "same":
        return e.snapshot_same()
    elif name == "diff":
        return e.snapshot_diff()
    elif name == "until":
        r = e.step_until_periodic(*op[1:])
        return dict(period=r.period, advanced=r.advanced, checks=r.checks,
                    extra_generations=r.extra_generations, lag=r.lag, check_every=r.check_every,
                    slot_diff=e.snapshot_diff(), field=e.store_packed())
    elif name == "store":
        return e.store_packed()
    elif name == "digest":
        return tuple(e.digest())
    elif name == "digest_rows":
        parts = [m.digest_rows(op[1], op[2]) for m in members(e)]
        return sum(p[0] for p in parts), sum(p[1] for p in parts) & 0xFFFFFFFFFFFFFFFF
    elif name == "read":
        return e.read_rect(*op[1:])
    elif name == "density":
        return e.density(*op[1:])
    elif name == "act":
        getter = op[1]
        if getter == "activity_state" and (group or not first):
            getter = "activity"  # (the state's words exist only where the skip is on)
        for m in members(e):
            getattr(m, getter)()
    elif name == "set_timing":
        for m in members(e):
            m.set_timing(op[1])
    elif name == "reset_timing":
        for m in members(e):
            m.reset_timing()
    else:
        raise AssertionError(op)
    return None


def equal(name, got, want, model):
    if name == "until":
        keys = ("period", "advanced", "checks", "extra_generations", "lag", "check_every")
        if any(got[k] != want[k] for k in keys):
            return False
        if want["slot"] is not None and got["slot_diff"] != model.diff():
            return False
        return bool((got["field"] == torus_ref.pack(want["field"])).all())
    if isinstance(want, np.ndarray):
        return got.shape == want.shape and bool((got == want).all())
    return got == want


def brief(v):
    if isinstance(v, dict):
        return {k: brief(x) for k, x in v.items() if k not in ("field", "slot")}
    if isinstance(v, np.ndarray):
        return f"array{v.shape} sum {int(np.asarray(v, dtype=np.uint64).sum() & np.uint64(0xFFFFFFFF))}"
    return v


def run_case(pkg, oracle, monkeypatch, case):
    """The program on the model and the engines.  Returns the model's facts and, per
    engine, the activity counters summed over the program."""
    kind, rule, ops = case["kind"], case["rule"], case["ops"]
    model = cm.Model(oracle, cm.make_field(oracle, case["start"], case["h"], case["w"]), rule,
                     torus=case["torus"])
    engines = make_engines(pkg, monkeypatch, case)
    group = kind == "group"
    host = [dict.fromkeys(HOST_COUNTS, 0) for _ in engines]
    records = []

    def fail(i, what):
        raise Failure(f"{kind} {cm.RULE_NAMES[rule]} seed {case['seed']} ({case['h']} x {case['w']}, "
                      f"{case['cfg']}), op {i}: {what}\nstart {case['start']}\n{cm.format_ops(ops, i)}")

    def call(i, n, fn, *args):
        try:
            return fn(*args)
        except pkg.GolError as ex:
            fail(i, f"engine {n} raised {ex}")

    try:
        for n, e in enumerate(engines):
            call(-1, n, e.load_packed, model.packed())
        for i, op in enumerate(ops):
            name = op[0]
            if group and name in SNAPSHOT_OPS:
                # a partitioned field's answer is a collective one: GOL_ESTATE, nothing done
                for m in engines[0].members:
                    with pytest.raises(pkg.GolError) as err:
                        engine_op(pkg, oracle, m, op, case, True, None)
                    if err.value.status != pkg.GOL_ESTATE:
                        fail(i, f"a group member raised {err.value}")
                continue
            window = model.read_rect(*op[1:]) if name == "rewrite" else None
            if name == "reset_timing" and not group:
                for n, e in enumerate(engines):  # (host counts: no look)
                    for k in HOST_COUNTS:
                        host[n][k] += getattr(e, k)()
            want, rec = cm.run_op(model, op)
            records.append(rec)
            for n, e in enumerate(engines):
                got = call(i, n, engine_op, pkg, oracle, e, op, case, n == 0, window)
                if name in cm.READERS and not equal(name, got, want, model):
                    fail(i, f"engine {n} answers {brief(got)}, the model {brief(want)}")
            if CHECK_EVERY:
                for n, e in enumerate(engines):
                    if not (call(i, n, e.store_packed) == model.packed()).all():
                        fail(i, f"engine {n} holds another field")
        last = len(ops) - 1
        for n, e in enumerate(engines):
            call(last, n, e.sync)  # (a GOL_ESTATE here: the fixed step's proof failed)
            got = call(last, n, e.store_packed)
            if not (got == model.packed()).all():
                bad = np.argwhere(got != model.packed())
                fail(last, f"engine {n} ends on another field: {len(bad)} words differ, the first "
                           f"at row {bad[0][0]} word {bad[0][1]}")
            if tuple(call(last, n, e.digest)) != model.digest():
                fail(last, f"engine {n}'s digest differs")
        counters = []
        if not group:
            for n, e in enumerate(engines):
                c = {k: host[n][k] + getattr(e, k)() for k in HOST_COUNTS}
                c["skipped"] = e.activity()[1]
                counters.append(c)
    finally:
        for e in engines:
            e.close()
    return cm.program_facts(records, case["K"]), counters


def check_counters(case, facts, counters):
    """Per program: the fixed steps are at most the steps that start on a fixed point, and
    with GOL_DEV_ACTIVITY_SKIP=0 nothing of the still machinery runs."""
    if not cm.KINDS[case["kind"]].get("skip"):
        return
    on, off = counters
    assert on["activity_fixed_steps"] <= facts["fixed_start"], (case["kind"], case["seed"], on, facts)
    assert on["activity_fixed_steps"] <= on["activity_short_steps"], on
    assert off == dict.fromkeys(off, 0), (case["kind"], case["seed"], off)


@pytest.mark.parametrize("kind,rule,seed", CASES,
                         ids=[f"{k}-{cm.RULE_NAMES[r]}-{s}" for k, r, s in CASES])
def test_program(pkg, oracle, monkeypatch, model_plans, kind, rule, seed):
    case = cm.case_program(kind, rule, seed, cm.plan_hot(pkg))
    facts, counters = run_case(pkg, oracle, monkeypatch, case)
    check_counters(case, facts, counters)
    _results[(kind, rule, seed)] = (facts, counters)


SKIP_KINDS = [(k, r) for k, spec in cm.KINDS.items() if spec.get("skip") for r, _ in spec["rules"]]


@pytest.mark.parametrize("kind,rule", SKIP_KINDS, ids=[f"{k}-{cm.RULE_NAMES[r]}" for k, r in SKIP_KINDS])
def test_still_machinery_ran(pkg, oracle, monkeypatch, model_plans, kind, rule):
    """The input condition from the engines, summed over the seeds of a kind and rule:
    units skipped, steps replayed the short graph, steps ran as fixed steps, and fixed
    steps shared a kernel.  (Programs test_program has run in this session are not run
    again.)"""
    seeds = dict(cm.KINDS[kind]["rules"])[rule]
    total = dict.fromkeys(HOST_COUNTS + ("skipped",), 0)
    for seed in range(seeds):
        if (kind, rule, seed) not in _results:
            case = cm.case_program(kind, rule, seed, cm.plan_hot(pkg))
            _results[(kind, rule, seed)] = run_case(pkg, oracle, monkeypatch, case)
        on = _results[(kind, rule, seed)][1][0]
        for k in total:
            total[k] += on[k]
    print(kind, cm.RULE_NAMES[rule], total)
    assert total["skipped"] > 0, total
    assert total["activity_short_steps"] > 0, total
    assert total["activity_fixed_steps"] > 0, total
    assert total["activity_fixed_launches"] < total["activity_fixed_steps"], total


# ---- the cache of captured step graphs


def turnover_lengths(K):
    """Ten graphable lengths: more than the cache's 8 slots, whatever the buffers' parity."""
    return [4 * K + 1, 4 * K + 5, 5 * K + 3, 6 * K, 6 * K + 8, 7 * K + 3, 8 * K, 8 * K + 15, 9 * K + 2,
            10 * K + 7]


@pytest.mark.parametrize("rule", [cm.CONWAY, cm.REF_RULE], ids=["B3/S23", "B/S2"])
def test_graph_cache_turnover(pkg, oracle, monkeypatch, model_plans, rule):
    """Three rounds of the ten lengths through one skip16 engine (and its twin with
    GOL_DEV_ACTIVITY_SKIP=0), the field checked against the oracle after every step: the
    second and third rounds replay lengths whose graph was evicted and captured again in
    another state.
    B3/S23: (a) a lattice with two gliders; (b) the still lattice with a sync after every
    step, so that short and fixed keys mix in; a glider is written; (c) the lengths
    backwards, each twice, then forwards.
    B/S2: a 0.5 soup that settles in the first round; the second round syncs after every
    step, the third does not."""
    K, h, w = 16, 333, 64 * 141 - 37
    case = dict(kind="skip16", rule=rule, h=h, w=w, cfg=dict(cm.BASE, tb_depth=K, rows_per_wave=64))
    model = cm.Model(oracle, cm.lattice(h, w, [(40, 4008), (168, 4968)]) if rule == cm.CONWAY
                     else cm.make_field(oracle, ("random", 11), h, w), rule)
    engines = make_engines(pkg, monkeypatch, case)
    try:
        def load():
            for e in engines:
                e.load_packed(model.packed())

        def round_(tag, sync, order=1, twice=False):
            for g in [g for g in turnover_lengths(K)[::order] for _ in range(2 if twice else 1)]:
                model.step(g)
                for n, e in enumerate(engines):
                    e.step(g)
                    if sync:
                        e.sync()
                    assert (e.store_packed() == model.packed()).all(), (tag, g, n)

        load()
        assert not model.is_fixed()
        round_("a", False)
        if rule == cm.CONWAY:
            model.load(cm.lattice(h, w))
            load()
        assert model.is_fixed()
        round_("b", True)
        on = engines[0]
        assert on.activity_short_steps() > 0 and on.activity_fixed_steps() > 0
        if rule == cm.CONWAY:
            win = cm.WINDOWS["glider"]
            model.write_rect(150, 4400, win, cm.RECT_OR)
            for e in engines:
                e.write_rect(150, 4400, torus_ref.pack(win), 3, pkg.RECT_OR)
            assert not model.is_fixed()
        fixed = on.activity_fixed_steps()
        # backwards first: the lengths round (b) used last are still cached (the LRU
        # cache misses every time on ten lengths in a circle); each twice, so that a
        # length of an odd number of launches starts on either buffer
        round_("c, backwards", False, -1, twice=True)
        round_("c", False)
        if rule == cm.CONWAY:
            assert on.activity_fixed_steps() == fixed  # (a field in motion: never)
        for e in engines:
            e.sync()
            assert tuple(e.digest()) == model.digest()
        off = engines[1]
        assert off.activity_short_steps() == 0 and off.activity()[1] == 0
    finally:
        for e in engines:
            e.close()
