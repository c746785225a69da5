"""CPU suite: the batch reference (batch_ref.py) against the two references the project
already trusts, and gol_batch's host-only side: the fixed geometry and the argument
checks, which never touch a GPU."""
import numpy as np
import pytest

import batch_ref
import rule_ref
import torus_ref

RULES = [rule_ref.REF_RULE, rule_ref.CONWAY, (0b1001000, 0b1100), (1, 0), rule_ref.FLOOD]
KNOBS = ["tb_depth", "halo_depth", "rows_per_wave", "handoff", "streams", "strip_lanes",
         "word_planes", "resident", "exchange_overlap"]


@pytest.mark.parametrize("rule", RULES, ids=rule_ref.rule_name)
@pytest.mark.parametrize("h,w", [(1, 1), (1, 64), (3, 2), (5, 7), (9, 65), (17, 130)])
def test_batch_ref_is_numpy_run_field_by_field(h, w, rule):
    cells = batch_ref.random_batch(4, h, w, seed=h * 1000 + w)
    got = batch_ref.run(cells, 5, rule)
    for i in range(cells.shape[0]):
        assert (got[i] == rule_ref.numpy_run(cells[i], 5, rule)).all(), i


@pytest.mark.parametrize("rule", RULES, ids=rule_ref.rule_name)
@pytest.mark.parametrize("h,w", [(1, 1), (1, 64), (3, 2), (2, 2), (64, 1), (5, 7), (9, 65)])
def test_batch_ref_torus_is_roll_run_field_by_field(h, w, rule):
    cells = batch_ref.random_batch(4, h, w, seed=h * 1000 + w + 1)
    got = batch_ref.pack(batch_ref.run(cells, 5, rule, torus=True))
    words = batch_ref.pack(cells)
    for i in range(cells.shape[0]):
        assert (got[i] == torus_ref.roll_run(words[i], w, 5, rule)).all(), i


def test_batch_ref_pack_is_the_canonical_packing():
    cells = batch_ref.random_batch(3, 9, 130, seed=3)
    words = batch_ref.pack(cells)
    for i in range(3):
        assert (words[i] == torus_ref.pack(cells[i])).all()
    assert (batch_ref.unpack(words, 130) == cells).all()


def expected_geometry(n, h, w):
    wq = -(-w // 64)
    lpf = 1
    while lpf < wq:
        lpf *= 2
    rows = min(r for r in (8, 16, 32, 64) if r >= h)
    fpw = 64 // lpf
    return {"lanes_per_field": lpf, "fields_per_wave": fpw, "rows_in_regs": rows,
            "waves": -(-n // fpw)}


# (h, w) -> lanes_per_field, fields_per_wave, rows_in_regs, written out
CONTRACT = {(1, 1): (1, 64, 8), (8, 64): (1, 64, 8), (9, 65): (2, 32, 16), (17, 130): (4, 16, 32),
            (33, 200): (4, 16, 64), (64, 4096): (64, 1, 64)}


@pytest.mark.parametrize("h,w", sorted(CONTRACT))
@pytest.mark.parametrize("sem", ["global", "torus"])
def test_batch_geometry_is_the_contract(pkg, h, w, sem):
    lpf, fpw, rows = CONTRACT[(h, w)]
    for n in (1, fpw, fpw + 1):
        g = pkg.batch_geometry(n, h, w, semantics=pkg.SEM_TORUS if sem == "torus" else pkg.SEM_GLOBAL)
        assert g == expected_geometry(n, h, w)
        assert (g["lanes_per_field"], g["fields_per_wave"], g["rows_in_regs"]) == (lpf, fpw, rows)
        assert g["waves"] == (1 if n <= fpw else 2)


def einval(pkg, fn):
    with pytest.raises(pkg.GolError) as ei:
        fn()
    assert ei.value.status == pkg.GOL_EINVAL
    msg = pkg.lib().gol_last_error().decode()
    assert msg
    return msg


BAD_SHAPES = [(0, 8, 8), (1, 0, 8), (1, 8, 0), (1, 65, 8), (1, 8, 4097)]


@pytest.mark.parametrize("n,h,w", BAD_SHAPES)
def test_batch_rejects_bad_shapes_without_a_gpu(pkg, n, h, w):
    msg = einval(pkg, lambda: pkg.batch_geometry(n, h, w))
    assert msg == einval(pkg, lambda: pkg.BatchEngine(n, h, w))
    if h == 65 or w == 4097:
        assert "gol_create" in msg


def test_batch_rejects_too_many_lanes(pkg):
    assert pkg.batch_geometry(2 ** 31, 8, 64)["waves"] == 2 ** 25
    assert "gol_create" in einval(pkg, lambda: pkg.batch_geometry(2 ** 31 + 1, 8, 64))
    assert pkg.batch_geometry(2 ** 25, 8, 4096)["waves"] == 2 ** 25
    einval(pkg, lambda: pkg.batch_geometry(2 ** 25 + 1, 8, 4096))


def test_batch_rejects_ref_stripes_and_bad_rules(pkg):
    einval(pkg, lambda: pkg.batch_geometry(4, 8, 8, semantics=pkg.SEM_REF_STRIPES))
    einval(pkg, lambda: pkg.BatchEngine(4, 8, 8, semantics=pkg.SEM_REF_STRIPES))
    einval(pkg, lambda: pkg.batch_geometry(4, 8, 8, rule=(512, 0)))
    einval(pkg, lambda: pkg.BatchEngine(4, 8, 8, rule=(0, 512)))


@pytest.mark.parametrize("knob", KNOBS)
def test_batch_has_no_plan_knobs(pkg, knob):
    einval(pkg, lambda: pkg.batch_geometry(4, 8, 8, **{knob: 1}))
    # the same through gol_batch_create, which returns before it touches a GPU
    import ctypes
    cfg = pkg.make_config(**{knob: 2})
    handle = ctypes.c_void_p()
    assert pkg.lib().gol_batch_create(4, 8, 8, ctypes.byref(cfg), ctypes.byref(handle)) == pkg.GOL_EINVAL
    assert pkg.lib().gol_last_error() and not handle.value


def test_batch_launch_cap_switch_is_checked_before_the_gpu(pkg, monkeypatch):
    monkeypatch.setenv("GOL_DEV_BATCH_LAUNCH_GENS", "0")
    einval(pkg, lambda: pkg.BatchEngine(4, 8, 8))
