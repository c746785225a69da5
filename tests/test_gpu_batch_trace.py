"""GPU suite: population traces of a batch (BatchEngine.step_trace,
gol_batch_step_trace) -- every sample of every field, exactly, against batch_trace_ref's
plain numpy, whose conditions test_batch_trace_host.py checks."""
import ctypes

import numpy as np
import pytest

import batch_ref
import batch_rules_ref
import batch_trace_ref
import rule_ref
from batch_trace_ref import CASES, CASE_IDS, STILL

pytestmark = pytest.mark.gpu


def sem_of(pkg, torus):
    return pkg.SEM_TORUS if torus else pkg.SEM_GLOBAL


def check_call(pkg, b, got, want_live, want_final, gens, every):
    """One step_trace call on batch b: the trace, the fields it left and its counters."""
    assert got.dtype == np.uint32 and got.shape == want_live.shape
    bad = np.argwhere(got != want_live)
    assert bad.size == 0, [(int(s), int(f), int(got[s, f]), int(want_live[s, f]))
                           for s, f in bad[:8]]
    wrong = np.argwhere((b.store_packed() != batch_ref.pack(want_final)).any(axis=(1, 2))).ravel()
    assert wrong.size == 0, wrong[:8].tolist()
    plan = batch_trace_ref.plan(gens, every, b.launch_generations)
    r = b.last_trace
    assert (r.every, r.samples, r.launches) == (every, plan["samples"], plan["launches"])


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_random_cases(pkg, i):
    h, w, n, rule, torus, gens, every, p = CASES[i]
    cells, live, final = batch_trace_ref.case(i)
    with pkg.BatchEngine(n, h, w, rule=rule, device=0, semantics=sem_of(pkg, torus)) as b:
        b.load_packed(batch_ref.pack(cells))
        check_call(pkg, b, b.step_trace(gens, every), live, final, gens, every)


@pytest.mark.parametrize("cap", ["1", "every", "2every+1"])
@pytest.mark.parametrize("i", [1, 2], ids=[CASE_IDS[1], CASE_IDS[2]])
def test_launch_seams(pkg, monkeypatch, i, cap):
    h, w, n, rule, torus, gens, every, p = CASES[i]
    cells, live, final = batch_trace_ref.case(i)
    cap = {"1": 1, "every": every, "2every+1": 2 * every + 1}[cap]
    monkeypatch.setenv("GOL_DEV_BATCH_LAUNCH_GENS", str(cap))
    with pkg.BatchEngine(n, h, w, rule=rule, device=0, semantics=sem_of(pkg, torus)) as b:
        assert b.launch_generations == cap
        b.load_packed(batch_ref.pack(cells))
        check_call(pkg, b, b.step_trace(gens, every), live, final, gens, every)
        assert b.last_trace.launches == -(-(gens // every) // max(1, cap // every)) > 1


def lane_sum_shapes():
    out = []
    for lpf in (1, 2, 4, 8, 16, 32, 64):
        for wq in [lpf] + ([lpf // 2 + 1] if lpf >= 4 else []):
            out.append((wq, min(2 * (64 // lpf) + 1, 33)))
    return out + [(2, 4 * 32 + 3)]  # five wavefronts: a second workgroup


@pytest.mark.parametrize("wq,n", lane_sum_shapes())
def test_lane_sum(pkg, wq, n):
    """A still rule, so every sample is the initial count: per-lane counts that differ
    between neighbouring lanes and neighbouring fields, in both planes of a word."""
    h, w = 8, 64 * wq
    cells = batch_trace_ref.lane_sum_cells(wq, n)
    want = np.repeat(cells.sum(axis=(1, 2), dtype=np.uint32)[None, :], 2, axis=0)
    with pkg.BatchEngine(n, h, w, rule=STILL, device=0) as b:
        geo = pkg.batch_geometry(n, h, w)
        assert geo["lanes_per_field"] >= wq > geo["lanes_per_field"] // 2
        b.load_packed(batch_ref.pack(cells))
        check_call(pkg, b, b.step_trace(2, 1), want, cells, 2, 1)


@pytest.mark.parametrize("h,w,n", [(64, 4096, 2), (64, 64, 65)])
def test_full_fields(pkg, h, w, n):
    cells = np.ones((n, h, w), dtype=np.uint8)
    with pkg.BatchEngine(n, h, w, rule=STILL, device=0) as b:
        b.load_packed(batch_ref.pack(cells))
        got = b.step_trace(3, 1)
        check_call(pkg, b, got, np.full((3, n), h * w, dtype=np.uint32), cells, 3, 1)


def test_rule_per_field(pkg):
    h, w, n, rule, torus, _, _, p = CASES[1]
    gens, every = 24, 2
    cells = batch_trace_ref.case(1)[0]
    birth, survive = batch_rules_ref.random_rules(n, seed=h * 1000 + w)
    live, final = batch_trace_ref.trace_ref(cells, gens, every, (birth, survive), torus)
    assert len({tuple(live[:, f].tolist()) for f in range(n)}) == n  # no two fields alike
    with pkg.BatchEngine(n, h, w, rule=rule, device=0, semantics=sem_of(pkg, torus)) as b:
        b.set_rules(birth, survive)
        b.load_packed(batch_ref.pack(cells))
        check_call(pkg, b, b.step_trace(gens, every), live, final, gens, every)
        b.drop_rules()
        _, _, _, _, _, g1, e1, _ = CASES[1]
        b.load_packed(batch_ref.pack(cells))
        check_call(pkg, b, b.step_trace(g1, e1), *batch_trace_ref.case(1)[1:], g1, e1)


def test_strides_and_forms(pkg):
    h, w, n, rule, torus, gens, every, p = CASES[0]
    cells, live, final = batch_trace_ref.case(0)
    start = batch_ref.pack(cells)
    L = pkg.lib()
    with pkg.BatchEngine(n, h, w, rule=rule, device=0, semantics=sem_of(pkg, torus)) as b:
        # a wider stride: the extra columns keep the sentinel
        b.load_packed(start)
        buf = np.full((gens, n + 5), 0xDEADBEEF, dtype=np.uint32)
        r = pkg.BatchTrace(struct_size=ctypes.sizeof(pkg.BatchTrace))
        assert L.gol_batch_step_trace(b._h, gens, every, buf.ctypes.data, n + 5,
                                      ctypes.byref(r)) == pkg.GOL_OK
        assert (buf[:, :n] == live).all() and (buf[:, n:] == 0xDEADBEEF).all()
        assert (r.every, r.samples, r.launches) == (every, gens, 1)
        assert (b.store_packed() == batch_ref.pack(final)).all()

        # the tensor form, from the same start
        import torch
        b.load_packed(start)
        t = b.step_trace_tensor(gens, every)
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
        assert tuple(t.shape) == (gens, n)
        assert (t.cpu().numpy().view(np.uint32) == live).all()
        assert (b.store_packed() == batch_ref.pack(final)).all()
        # ... with the wider stride on the device
        b.load_packed(start)
        wide = torch.full((gens, n + 5), 0x5EADBEEF, dtype=torch.int32, device=t.device)
        torch.cuda.current_stream(wide.device).synchronize()
        assert L.gol_batch_step_trace_device(b._h, gens, every, wide.data_ptr(), n + 5,
                                             ctypes.byref(r)) == pkg.GOL_OK
        wide = wide.cpu().numpy().view(np.uint32)
        assert (wide[:, :n] == live).all() and (wide[:, n:] == 0x5EADBEEF).all()

        # two calls in a row: each counts from its own start
        b.load_packed(start)
        first = b.step_trace(15, 1)
        second = b.step_trace(gens - 15, 1)
        assert (np.concatenate([first, second]) == live).all()
        assert second.shape == (gens - 15, n) and b.last_trace.samples == gens - 15

        # generations < every: no sample, the fields stepped, one launch
        b.load_packed(start)
        none = b.step_trace(3, 4)
        assert none.shape == (0, n) and none.dtype == np.uint32
        assert (b.last_trace.samples, b.last_trace.launches) == (0, 1)
        assert (b.store_packed() == batch_ref.pack(batch_ref.run(cells, 3, rule, torus))).all()
        assert tuple(b.step_trace_tensor(3, 4).shape) == (0, n)
        assert (b.store_packed() == batch_ref.pack(batch_ref.run(cells, 6, rule, torus))).all()

        # generations == 0: nothing run
        b.load_packed(start)
        assert b.step_trace(0, 1).shape == (0, n)
        assert (b.last_trace.samples, b.last_trace.launches) == (0, 0)
        assert L.gol_batch_step_trace(b._h, 0, 7, None, 0, ctypes.byref(r)) == pkg.GOL_OK
        assert (b.store_packed() == start).all()


def test_rejections_leave_the_batch_alone(pkg):
    h, w, n = 8, 8, 130
    L = pkg.lib()
    size = ctypes.sizeof(pkg.BatchTrace)
    with pkg.BatchEngine(n, h, w, rule=rule_ref.CONWAY, device=0) as b:
        b.load_packed(batch_ref.pack(batch_trace_ref.case(0)[0]))
        before = b.digest()
        buf = np.full((4, n), 7, dtype=np.uint32)
        ok = pkg.BatchTrace(struct_size=size)
        cases = [
            ("batch", (None, 4, 1, buf.ctypes.data, n, ctypes.byref(ok))),
            ("out", (b._h, 4, 1, buf.ctypes.data, n, None)),
            ("struct_size", (b._h, 4, 1, buf.ctypes.data, n,
                             ctypes.byref(pkg.BatchTrace(struct_size=size - 1)))),
            ("struct_size", (b._h, 4, 1, buf.ctypes.data, n,
                             ctypes.byref(pkg.BatchTrace(struct_size=0)))),
            ("every", (b._h, 4, 0, buf.ctypes.data, n, ctypes.byref(ok))),
            ("every", (b._h, 2 ** 20, 65537, buf.ctypes.data, n, ctypes.byref(ok))),
            ("sample_stride", (b._h, 4, 1, buf.ctypes.data, n - 1, ctypes.byref(ok))),
            ("sample_stride", (b._h, 4, 1, buf.ctypes.data, 0, ctypes.byref(ok))),
            ("live", (b._h, 4, 1, None, n, ctypes.byref(ok))),
            ("representable", (b._h, 4, 1, buf.ctypes.data, 2 ** 62, ctypes.byref(ok))),
            ("representable", (b._h, 2 ** 40, 1, buf.ctypes.data, 2 ** 30, ctypes.byref(ok))),
        ]
        for fn in (L.gol_batch_step_trace, L.gol_batch_step_trace_device):
            for word, args in cases:
                assert fn(*args) == pkg.GOL_EINVAL, word
                assert word in L.gol_last_error().decode(), word
        for bad_every in (0, 65537, 1.5):
            with pytest.raises(pkg.GolError):
                b.step_trace(4, bad_every)
            with pytest.raises(pkg.GolError):
                b.step_trace_tensor(4, bad_every)
        after = b.digest()
        assert (after[0] == before[0]).all() and (after[1] == before[1]).all()
        assert (buf == 7).all()
