"""GPU: what a sequence of steps leaves behind, call by call, against a recorded trace
(tests/golden/step_trace.json).

The single-stream step issues its kernels from one schedule (csrc/step_plan.h, DESIGN §4
"The step's schedule").  This test holds the schedule's outcome fixed across every switch
of the activity skip: after each call of a fixed list it compares, exactly, the eight
activity counters, the short and fixed step counts, a CRC of the activity state's words
and the field's digest with the recorded ones.  The still field's digests are also the
CPU oracle's, so the record cannot hold a wrong field.

The call list walks every way a step is issued: 3 (a remainder alone), K, 2K + 1,
4K - 1 (the longest step issued directly), 4K (the shortest captured one), 6K + 8 and
6K + K - 1 (the longest remainder chain: 12, 2, 1 at K = 16); after a sync, 6K + 8 twice
(short graph, then the fixed step on the still field), 5K (ends at depth K) and 6K + 8.

Run as a script, the file prints the trace as JSON (the way the record was made).
"""
import functools
import json
import os
import sys
import zlib

import pytest

import test_gpu_probe_pass as pp
import test_gpu_twin as tw
from test_gpu_short_step import eight

pytestmark = pytest.mark.gpu

H, W = 64 * 9 + 13, 9023
DEPTHS = (16, 7)
FIELDS = ("still", "glider")
RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_trace.json")
SWITCHES = tw.SWITCHES + ("GOL_DEV_TWIN_SURE", "GOL_DEV_SHORT_STEP", "GOL_DEV_FIXED_STEP")
# (name, environment, timing interval)
SETTINGS = [("default", {}, 0)] + [
    (f"{name}={v}", {name: v}, 0)
    for name, v in (("GOL_DEV_COPY_THROUGH", "1"), ("GOL_DEV_COPY_PASS", "0"),
                    ("GOL_DEV_COPY_ELIDE", "0"), ("GOL_DEV_STILL_PROBE", "0"),
                    ("GOL_DEV_PROBE_PASS", "0"), ("GOL_DEV_TWIN", "0"),
                    ("GOL_DEV_TWIN_SURE", "0"), ("GOL_DEV_STILL_EXIT", "0"),
                    ("GOL_DEV_SHORT_STEP", "0"), ("GOL_DEV_FIXED_STEP", "0"))
] + [("set_timing(8)", {}, 8)]


def calls(K):
    """The steps, None = sync()."""
    return (3, K, 2 * K + 1, 4 * K - 1, 4 * K, 6 * K + 8, 6 * K + K - 1, None,
            6 * K + 8, 6 * K + 8, 5 * K, 6 * K + 8)


@functools.lru_cache(maxsize=None)
def field(name):
    g0 = pp.blocks_field(H, W)
    return pp.put(g0, 40, 40, pp.GLIDER) if name == "glider" else g0


class environment:
    """The activity skip's switches as `env` says, every other one at its default, and
    the cost models' plans; the caller's environment comes back on exit."""

    def __init__(self, env):
        self.env = dict(env, GOL_DEV_AUTOTUNE="0")

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in SWITCHES + ("GOL_DEV_AUTOTUNE",)}
        for k in self.saved:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def trace(pkg, name, K, env, timing):
    """One engine through the call list: a record of 13 numbers after every call."""
    out = []
    with environment(env):  # the switches are read at create
        e = pkg.Engine(H, W, **dict(pp.BASE, rows_per_wave=64, tb_depth=K, device=0, rule=pkg.CONWAY))
    with e:
        if timing:
            e.set_timing(timing)
        e.load_packed(field(name))
        for g in calls(K):
            if g is None:
                e.sync()
            else:
                e.step(g)
            out.append(list(eight(e)) + [e.activity_short_steps(), e.activity_fixed_steps(),
                                         zlib.crc32(e.activity_state().tobytes())] + list(e.digest()))
    return out


def traces(pkg, name, K):
    return {f"{name}/K{K}/{s}": trace(pkg, name, K, env, timing) for s, env, timing in SETTINGS}


@functools.lru_cache(maxsize=None)
def record():
    with open(RECORD) as f:
        return json.load(f)


@pytest.mark.parametrize("K", DEPTHS)
@pytest.mark.parametrize("name", FIELDS)
def test_step_trace(pkg, oracle, model_plans, name, K):
    want = record()
    g0 = field(name)
    still = oracle.bp_digest(g0, W) if name == "still" else None
    if still:
        assert (oracle.bp_run(g0, W, 1, pkg.CONWAY) == g0).all()
    for s, env, timing in SETTINGS:
        key = f"{name}/K{K}/{s}"
        got = trace(pkg, name, K, env, timing)
        for i, (g, rec) in enumerate(zip(calls(K), got)):
            print(key, g, rec)
            if still:
                assert tuple(rec[-2:]) == tuple(still), (key, i, g)
        assert got == want[key], key
    # the default engine took both paths the fixed point opens
    rec = want[f"still/K{K}/default"]
    assert rec[-1][8] >= 2 and rec[-1][9] >= 1


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as entry

    pkg = entry.load_package()
    out = {}
    for name in FIELDS:
        for K in DEPTHS:
            out.update(traces(pkg, name, K))
    print(json.dumps(out, separators=(",", ":")))
