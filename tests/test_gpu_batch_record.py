"""GPU suite: recorded rollouts of a batch (BatchEngine.step_record,
gol_batch_step_record) -- every word of every frame, exactly, against batch_record_ref's
plain numpy, whose conditions test_batch_record_host.py checks."""
import ctypes

import numpy as np
import pytest

import batch_ref
import batch_record_ref
import batch_rules_ref
import batch_trace_ref
import rule_ref
from batch_record_ref import CASES, CASE_IDS, STILL

pytestmark = pytest.mark.gpu

SENTINEL = np.uint64(0xDEADBEEFCAFEF00D)


def sem_of(pkg, torus):
    return pkg.SEM_TORUS if torus else pkg.SEM_GLOBAL


def check_call(pkg, b, got, want_frames, want_final, gens, every):
    """One step_record call on batch b: the frames, the fields it left (all n of them)
    and its counters."""
    assert got.dtype == np.uint64 and got.shape == want_frames.shape
    bad = np.argwhere(got != want_frames)
    assert bad.size == 0, [(tuple(int(v) for v in k), hex(int(got[tuple(k)])),
                            hex(int(want_frames[tuple(k)]))) for k in bad[:8]]
    wrong = np.argwhere((b.store_packed() != batch_ref.pack(want_final)).any(axis=(1, 2))).ravel()
    assert wrong.size == 0, wrong[:8].tolist()
    plan = batch_trace_ref.plan(gens, every, b.launch_generations)
    r = b.last_record
    assert (r.every, r.samples, r.launches) == (every, plan["samples"], plan["launches"])


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_random_cases(pkg, i):
    h, w, n, rule, torus, gens, every, p, first, count = CASES[i]
    cells, frames, final = batch_record_ref.case(i)
    with pkg.BatchEngine(n, h, w, rule=rule, device=0, semantics=sem_of(pkg, torus)) as b:
        b.load_packed(batch_ref.pack(cells))
        check_call(pkg, b, b.step_record(gens, every, first, count), frames, final, gens, every)


@pytest.mark.parametrize("cap", ["1", "every", "2every+1"])
@pytest.mark.parametrize("i", [1, 2], ids=[CASE_IDS[1], CASE_IDS[2]])
def test_launch_seams(pkg, monkeypatch, i, cap):
    h, w, n, rule, torus, gens, every, p, first, count = CASES[i]
    cells, frames, final = batch_record_ref.case(i)
    cap = {"1": 1, "every": every, "2every+1": 2 * every + 1}[cap]
    monkeypatch.setenv("GOL_DEV_BATCH_LAUNCH_GENS", str(cap))
    with pkg.BatchEngine(n, h, w, rule=rule, device=0, semantics=sem_of(pkg, torus)) as b:
        assert b.launch_generations == cap
        b.load_packed(batch_ref.pack(cells))
        check_call(pkg, b, b.step_record(gens, every, first, count), frames, final, gens, every)
        assert b.last_record.launches == -(-(gens // every) // max(1, cap // every)) > 1


def placement_shapes():
    """test_gpu_batch_trace.lane_sum_shapes(), restated: every lanes_per_field with a full
    and a partial word count, and five wavefronts."""
    out = []
    for lpf in (1, 2, 4, 8, 16, 32, 64):
        for wq in [lpf] + ([lpf // 2 + 1] if lpf >= 4 else []):
            out.append((wq, min(2 * (64 // lpf) + 1, 33)))
    return out + [(2, 4 * 32 + 3)]  # five wavefronts: a second workgroup


@pytest.mark.parametrize("wq,n", placement_shapes())
def test_placement(pkg, wq, n):
    """A still rule, so every sample is the loaded words: each word of each row of each
    field of the window at its address under padded strides, and no other word written."""
    h, w, samples = 8, 64 * wq, 2
    first, count = (1, n - 2) if n >= 3 else (0, n)
    words = batch_ref.pack(batch_ref.random_batch(n, h, w, seed=1000 * wq + n, p=.5))
    rs = wq + 1
    fs = h * rs + 3
    ss = count * fs + 5
    want = np.full(samples * ss + 7, SENTINEL, dtype=np.uint64)
    for s in range(samples):
        for j in range(count):
            for r in range(h):
                at = s * ss + j * fs + r * rs
                want[at:at + wq] = words[first + j, r]
    L = pkg.lib()
    with pkg.BatchEngine(n, h, w, rule=STILL, device=0) as b:
        geo = pkg.batch_geometry(n, h, w)
        assert geo["lanes_per_field"] >= wq > geo["lanes_per_field"] // 2
        b.load_packed(words)
        r = pkg.BatchRecord(struct_size=ctypes.sizeof(pkg.BatchRecord))
        # the host form
        buf = np.full(want.shape, SENTINEL, dtype=np.uint64)
        assert L.gol_batch_step_record(b._h, samples, 1, first, count, buf.ctypes.data, ss, fs,
                                       rs, ctypes.byref(r)) == pkg.GOL_OK
        assert (r.every, r.samples, r.launches) == (1, samples, 1)
        bad = np.flatnonzero(buf != want)
        assert bad.size == 0, [(int(k), hex(int(buf[k])), hex(int(want[k]))) for k in bad[:8]]
        # the device form: the kernel's own stores under the padded strides
        import torch
        dev = torch.full((want.size,), int(SENTINEL.astype(np.int64)), dtype=torch.int64,
                         device="cuda:0")
        torch.cuda.current_stream(dev.device).synchronize()
        assert L.gol_batch_step_record_device(b._h, samples, 1, first, count, dev.data_ptr(), ss,
                                              fs, rs, ctypes.byref(r)) == pkg.GOL_OK
        got = dev.cpu().numpy().view(np.uint64)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, [(int(k), hex(int(got[k])), hex(int(want[k]))) for k in bad[:8]]
        assert (b.store_packed() == words).all()


@pytest.mark.parametrize("torus", [False, True], ids=["dead", "torus"])
@pytest.mark.parametrize("w", [1, 63, 65, 130])
def test_last_word_mask(pkg, w, torus):
    """All cells live under the still rule: bits at columns >= w are 0 in every frame
    (the kernel stores its registers unmasked: they must hold valid columns only, on a
    torus too, whose ghost column w is set only in the copy a pass ingests)."""
    n, h = 5, 9
    cells = np.ones((n, h, w), dtype=np.uint8)
    want = batch_ref.pack(cells)
    with pkg.BatchEngine(n, h, w, rule=STILL, device=0, semantics=sem_of(pkg, torus)) as b:
        b.load_packed(want)
        got = b.step_record(3, 1)
        assert not (got[..., -1] >> np.uint64(w % 64)).any()
        check_call(pkg, b, got, np.repeat(want[None], 3, axis=0), cells, 3, 1)


def test_rule_per_field(pkg):
    h, w, n, rule, torus, gens, every, p, first, count = CASES[1]
    cells = batch_record_ref.case(1)[0]
    birth, survive = batch_rules_ref.random_rules(n, seed=h * 1000 + w)
    frames, final = batch_record_ref.record_ref(cells, gens, every, (birth, survive), torus,
                                                first, count)
    assert (frames != batch_record_ref.case(1)[1]).any()  # the rules matter
    with pkg.BatchEngine(n, h, w, rule=rule, device=0, semantics=sem_of(pkg, torus)) as b:
        b.set_rules(birth, survive)
        b.load_packed(batch_ref.pack(cells))
        check_call(pkg, b, b.step_record(gens, every, first, count), frames, final, gens, every)
        b.drop_rules()
        b.load_packed(batch_ref.pack(cells))
        check_call(pkg, b, b.step_record(gens, every, first, count),
                   *batch_record_ref.case(1)[1:], gens, every)


def test_forms_agree(pkg):
    h, w, n, rule, torus, gens, every, p, first, count = CASES[2]
    cells, frames, final = batch_record_ref.case(2)
    start = batch_ref.pack(cells)
    with pkg.BatchEngine(n, h, w, rule=rule, device=0, semantics=sem_of(pkg, torus)) as b:
        b.load_packed(start)
        host = b.step_record(gens, every, first, count)
        check_call(pkg, b, host, frames, final, gens, every)
        import torch
        if not torch.cuda.is_available():
            return
        b.load_packed(start)
        t = b.step_record_tensor(gens, every, first, count)
        assert t.dtype == torch.int64 and t.is_cuda and t.is_contiguous()
        assert tuple(t.shape) == host.shape
        check_call(pkg, b, t.cpu().numpy().view(np.uint64), host, final, gens, every)
        # the window defaults to the whole batch
        b.load_packed(start)
        whole = b.step_record(gens, every)
        assert whole.shape == (gens // every, n, h, b.wq)
        assert (whole[:, first:first + count] == frames).all()
        # two calls in a row: each counts from its own start
        b.load_packed(start)
        one = b.step_record(2 * every, every, first, count)
        two = b.step_record(every, every, first, count)
        assert (np.concatenate([one, two]) == frames).all()


def test_nothing_to_record(pkg):
    h, w, n, rule, torus, gens, every, p, first, count = CASES[0]
    cells = batch_record_ref.case(0)[0]
    start = batch_ref.pack(cells)
    L = pkg.lib()
    r = pkg.BatchRecord(struct_size=ctypes.sizeof(pkg.BatchRecord))
    with pkg.BatchEngine(n, h, w, rule=rule, device=0, semantics=sem_of(pkg, torus)) as b:
        # count == 0: the fields are stepped and nothing is recorded (any pointer, any stride)
        b.load_packed(start)
        none = b.step_record(5, 1, 7, 0)
        assert none.shape == (5, 0, h, 1) and none.dtype == np.uint64
        assert (b.last_record.every, b.last_record.samples, b.last_record.launches) == (1, 5, 1)
        after5 = batch_ref.pack(batch_ref.run(cells, 5, rule, torus))
        assert (b.store_packed() == after5).all()
        buf = np.full(16, SENTINEL, dtype=np.uint64)
        b.load_packed(start)
        assert L.gol_batch_step_record(b._h, 5, 1, n, 0, buf.ctypes.data, 0, 0, 0,
                                       ctypes.byref(r)) == pkg.GOL_OK
        assert L.gol_batch_step_record_device(b._h, 0, 1, n, 0, None, 0, 0, 0,
                                              ctypes.byref(r)) == pkg.GOL_OK
        assert (buf == SENTINEL).all() and (b.store_packed() == after5).all()

        # generations < every: no sample, the fields stepped, one launch
        b.load_packed(start)
        none = b.step_record(3, 4)
        assert none.shape == (0, n, h, 1)
        assert (b.last_record.samples, b.last_record.launches) == (0, 1)
        assert (b.store_packed() == batch_ref.pack(batch_ref.run(cells, 3, rule, torus))).all()
        b.load_packed(start)
        assert L.gol_batch_step_record(b._h, 3, 4, 0, n, None, 0, 0, 0,
                                       ctypes.byref(r)) == pkg.GOL_OK
        assert (r.every, r.samples, r.launches) == (4, 0, 1)
        assert (b.store_packed() == batch_ref.pack(batch_ref.run(cells, 3, rule, torus))).all()

        # generations == 0: nothing run
        b.load_packed(start)
        assert b.step_record(0, 1).shape == (0, n, h, 1)
        assert (b.last_record.samples, b.last_record.launches) == (0, 0)
        assert L.gol_batch_step_record(b._h, 0, 7, 0, n, None, 0, 0, 0,
                                       ctypes.byref(r)) == pkg.GOL_OK
        assert (b.store_packed() == start).all()


def test_rejections_leave_the_batch_alone(pkg):
    h, w, n = 9, 65, 70
    wq = 2
    L = pkg.lib()
    size = ctypes.sizeof(pkg.BatchRecord)
    fs, c = h * wq, 10
    with pkg.BatchEngine(n, h, w, rule=rule_ref.CONWAY, device=0) as b:
        b.load_packed(batch_ref.pack(batch_record_ref.case(2)[0]))
        before = b.store_packed()
        buf = np.full(4 * c * fs, SENTINEL, dtype=np.uint64)
        p = buf.ctypes.data
        ok = pkg.BatchRecord(struct_size=size)
        o = ctypes.byref(ok)
        cases = [
            ("batch", (None, 4, 1, 0, c, p, c * fs, fs, wq, o)),
            ("out", (b._h, 4, 1, 0, c, p, c * fs, fs, wq, None)),
            ("struct_size", (b._h, 4, 1, 0, c, p, c * fs, fs, wq,
                             ctypes.byref(pkg.BatchRecord(struct_size=size - 1)))),
            ("struct_size", (b._h, 4, 1, 0, c, p, c * fs, fs, wq,
                             ctypes.byref(pkg.BatchRecord(struct_size=0)))),
            ("every", (b._h, 4, 0, 0, c, p, c * fs, fs, wq, o)),
            ("every", (b._h, 2 ** 20, 65537, 0, c, p, c * fs, fs, wq, o)),
            ("first + count", (b._h, 4, 1, n - c + 1, c, p, c * fs, fs, wq, o)),
            ("first + count", (b._h, 4, 1, n + 1, 0, p, c * fs, fs, wq, o)),
            ("first + count", (b._h, 4, 1, 2 ** 64 - 1, 2, p, c * fs, fs, wq, o)),
            ("row_stride_words < ceil", (b._h, 4, 1, 0, c, p, c * fs, fs, wq - 1, o)),
            ("field_stride_words < h", (b._h, 4, 1, 0, c, p, c * fs, fs - 1, wq, o)),
            ("field_stride_words < h", (b._h, 4, 1, 0, c, p, c * fs, fs, 2 ** 62, o)),
            ("sample_stride_words < count", (b._h, 4, 1, 0, c, p, c * fs - 1, fs, wq, o)),
            ("sample_stride_words < count", (b._h, 4, 1, 0, c, p, c * fs, 2 ** 62, wq, o)),
            ("frames", (b._h, 4, 1, 0, c, None, c * fs, fs, wq, o)),
            ("representable", (b._h, 4, 1, 0, c, p, 2 ** 62, fs, wq, o)),
            ("representable", (b._h, 2 ** 40, 1, 0, c, p, 2 ** 30, fs, wq, o)),
            # the order: an earlier check speaks first
            ("out", (b._h, 4, 0, n, c, None, 0, 0, 0, None)),
            ("struct_size", (b._h, 4, 0, n, c, None, 0, 0, 0,
                             ctypes.byref(pkg.BatchRecord(struct_size=1)))),
            ("every", (b._h, 4, 0, n, c, None, 0, 0, 0, o)),
            ("first + count", (b._h, 4, 1, n, c, None, 0, 0, 0, o)),
            ("row_stride_words < ceil", (b._h, 4, 1, 0, c, None, 0, 0, 0, o)),
            ("field_stride_words < h", (b._h, 4, 1, 0, c, None, 0, 0, wq, o)),
            ("sample_stride_words < count", (b._h, 4, 1, 0, c, None, 0, fs, wq, o)),
        ]
        for fn in (L.gol_batch_step_record, L.gol_batch_step_record_device):
            for word, args in cases:
                assert fn(*args) == pkg.GOL_EINVAL, word
                assert word in L.gol_last_error().decode(), (word, L.gol_last_error().decode())
        assert (ok.every, ok.samples, ok.launches) == (0, 0, 0)
        for bad in ({"every": 0}, {"every": 65537}, {"every": 1.5}, {"first": n, "count": 1},
                    {"first": -1}, {"count": n + 1}):
            with pytest.raises(pkg.GolError):
                b.step_record(4, **bad)
            with pytest.raises(pkg.GolError):
                b.step_record_tensor(4, **bad)
        assert (b.store_packed() == before).all()
        assert (buf == SENTINEL).all()


def test_record_then_step(pkg):
    h, w, n, rule, torus, gens, every, p, first, count = CASES[3]
    cells = batch_record_ref.case(3)[0]
    g1, g2 = 13, 9
    sem = sem_of(pkg, torus)
    with pkg.BatchEngine(n, h, w, rule=rule, device=0, semantics=sem) as a, \
            pkg.BatchEngine(n, h, w, rule=rule, device=0, semantics=sem) as b:
        a.load_packed(batch_ref.pack(cells))
        b.load_packed(batch_ref.pack(cells))
        a.step_record(g1, every, 2, 5)
        a.step(g2)
        b.step(g1 + g2)
        got, want = a.store_packed(), b.store_packed()
        assert (got == want).all()
        assert (want == batch_ref.pack(batch_ref.run(cells, g1 + g2, rule, torus))).all()
