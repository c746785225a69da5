"""CPU suite: the rollout reference (batch_record_ref.py) against the population-trace
reference, the conditions the GPU cases rest on, the cell helpers pack_cells /
unpack_cells, and gol_batch_step_record's host-only side: the exported symbols and the
argument checks that never touch a GPU."""
import ctypes

import numpy as np
import pytest

import batch_ref
import batch_record_ref
import batch_rules_ref
import batch_trace_ref
import rule_ref
from batch_record_ref import CASES, CASE_IDS


def popcount(words):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).reshape(
        words.shape + (64,)).sum(axis=-1, dtype=np.uint64)


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_case_conditions(i):
    """What the GPU cases rest on, on the reference alone: at every sample at least half of
    the recorded fields differ from their previous sample (the start is sample -1), so a
    repeated, late or early frame cannot pass; where there is a tail the last frame is not
    the final state, so a tail that is recorded or not run cannot pass."""
    h, w, n, rule, torus, gens, every, p, first, count = CASES[i]
    cells, frames, final = batch_record_ref.case(i)
    assert frames.dtype == np.uint64
    assert frames.shape == (gens // every, count, h, (w + 63) // 64)
    prev = batch_ref.pack(cells[first:first + count])
    for s in range(frames.shape[0]):
        moved = int((frames[s] != prev).any(axis=(1, 2)).sum())
        assert 2 * moved >= count, (s, moved, count)
        prev = frames[s]
    if gens % every:
        assert (frames[-1] != batch_ref.pack(final[first:first + count])).any()
    # bits at columns >= w are 0 in the reference's frames
    if w % 64:
        assert not (frames[..., -1] >> np.uint64(w % 64)).any()


def test_least_moving_case():
    """(the figure the conditions were chosen at: 6 of 10 fields, B/S2's sparse case)"""
    least = 1.0
    for i, c in enumerate(CASES):
        cells, frames, _ = batch_record_ref.case(i)
        prev = batch_ref.pack(cells[c[8]:c[8] + c[9]])
        for s in range(frames.shape[0]):
            least = min(least, (frames[s] != prev).any(axis=(1, 2)).sum() / c[9])
            prev = frames[s]
    assert least == 0.6


def test_cases_cover_the_geometries(pkg):
    geo = [pkg.batch_geometry(c[2], c[0], c[1]) for c in CASES]
    assert {g["rows_in_regs"] for g in geo} == {8, 16, 32, 64}
    assert {g["lanes_per_field"] for g in geo} >= {1, 2, 4, 64}
    assert {c[4] for c in CASES} == {False, True}
    assert {c[5] % c[6] for c in CASES} >= {0, 2, 3}
    # a window that starts and ends inside a wavefront and spans three of them
    def spans_three(c, g):
        fpw, first, end = g["fields_per_wave"], c[8], c[8] + c[9]
        return first % fpw and end % fpw and (end - 1) // fpw - first // fpw + 1 >= 3
    assert any(spans_three(c, g) for c, g in zip(CASES, geo))
    # whole batches, windows strictly inside one, and wavefronts with no field in the window
    assert any(c[8] == 0 and c[9] == c[2] for c in CASES)
    assert any(c[8] > 0 and c[8] + c[9] < c[2] for c in CASES)
    assert any(c[8] >= g["fields_per_wave"] or (c[2] - 1) // g["fields_per_wave"] >
               (c[8] + c[9] - 1) // g["fields_per_wave"] for c, g in zip(CASES, geo))
    assert {c[3] for c in CASES} == {rule_ref.REF_RULE, rule_ref.CONWAY, batch_record_ref.B36S23}


@pytest.mark.parametrize("torus", [False, True], ids=["dead", "torus"])
def test_reference_agrees_with_the_trace_reference(torus):
    n, h, w, gens, every = 7, 9, 70, 14, 3
    cells = batch_ref.random_batch(n, h, w, seed=31, p=.4)
    birth, survive = batch_rules_ref.random_rules(n, seed=5)
    for rules in ((birth, survive), rule_ref.CONWAY):
        live, final_t = batch_trace_ref.trace_ref(cells, gens, every, rules, torus)
        frames, final = batch_record_ref.record_ref(cells, gens, every, rules, torus)
        assert frames.shape == (gens // every, n, h, 2)
        assert (popcount(frames).sum(axis=(2, 3)) == live).all()
        assert (final == final_t).all()
        # a window is a slice of the whole record, and the final fields do not depend on it
        part, final_w = batch_record_ref.record_ref(cells, gens, every, rules, torus, 2, 3)
        assert (part == frames[:, 2:5]).all() and (final_w == final).all()


def test_reference_edge_shapes():
    cells = batch_ref.random_batch(3, 8, 8, seed=1)
    frames, final = batch_record_ref.record_ref(cells, 2, 3, rule_ref.CONWAY)
    assert frames.shape == (0, 3, 8, 1)
    assert (final == batch_ref.run(cells, 2, rule_ref.CONWAY)).all()
    frames, final = batch_record_ref.record_ref(cells, 0, 1, rule_ref.CONWAY)
    assert frames.shape == (0, 3, 8, 1) and (final == cells).all()
    frames, final = batch_record_ref.record_ref(cells, 2, 1, batch_record_ref.STILL, False, 1, 0)
    assert frames.shape == (2, 0, 8, 1) and (final == cells).all()
    frames, final = batch_record_ref.record_ref(cells, 2, 1, batch_record_ref.STILL)
    assert (frames == batch_ref.pack(cells)[None]).all() and (final == cells).all()


@pytest.mark.parametrize("w", [1, 63, 64, 65, 130])
def test_pack_and_unpack_cells(pkg, w):
    cells = batch_ref.random_batch(5, 7, w, seed=w)
    words = pkg.pack_cells(cells)
    assert words.dtype == np.uint64 and words.shape == (5, 7, (w + 63) // 64)
    assert (words == batch_ref.pack(cells)).all()
    back = pkg.unpack_cells(words, w)
    assert back.dtype == np.uint8 and back.shape == cells.shape and (back == cells).all()
    # any leading shape: frames [samples, count, h, wq], one field [h, wq]
    stack = np.stack([cells, 1 - cells])
    assert (pkg.pack_cells(stack) == np.stack([words, batch_ref.pack(1 - cells)])).all()
    assert (pkg.unpack_cells(pkg.pack_cells(stack), w) == stack).all()
    assert (pkg.unpack_cells(words[2], w) == cells[2]).all()
    assert (pkg.pack_cells(cells[2]) == words[2]).all()
    # all cells live: the padding bits of the last word stay 0
    full = pkg.pack_cells(np.ones((2, 3, w), dtype=np.uint8))
    assert int(popcount(full).sum()) == 2 * 3 * w


def einval(pkg, status):
    assert status == pkg.GOL_EINVAL
    msg = pkg.lib().gol_last_error().decode()
    assert msg
    return msg


def test_library_exports_the_calls_and_rejects_a_null_batch(pkg):
    """(the checks that need a batch are in test_gpu_batch_record.py)"""
    L = pkg.lib()
    assert ctypes.sizeof(pkg.BatchRecord) == 24
    assert {"gol_batch_step_record", "gol_batch_step_record_device"} <= set(pkg.EXPORTS)
    buf = np.zeros(8, dtype=np.uint64)
    for name in ("gol_batch_step_record", "gol_batch_step_record_device"):
        fn = getattr(L, name)
        out = pkg.BatchRecord(struct_size=ctypes.sizeof(pkg.BatchRecord))
        assert "batch" in einval(pkg, fn(None, 10, 1, 0, 1, buf.ctypes.data, 8, 8, 1,
                                         ctypes.byref(out)))
        assert "batch" in einval(pkg, fn(None, 10, 1, 0, 1, buf.ctypes.data, 8, 8, 1, None))
        assert (out.every, out.samples, out.launches) == (0, 0, 0)
