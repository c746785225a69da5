"""GPU: every bit of the two rule masks through the generic kernels (rule32_total's
mask sum, life_stencil.h), against the plain numpy reference of rule_ref.py.

The 18 rules with one mask bit set give each bit on its own; B3/S23 with one bit
flipped keeps the field active, so the fused depths meet every neighbour count
with that bit's outcome for many generations.  Each rule runs on the streaming
kernels of depth 1, 8 (classic blocks), 12 (hand-off blocks) and 16, on the
resident kernel and on a torus engine; 40 x 4100 crosses a strip seam and ends in
a ragged word.  The start fields hold every (alive, count) pair and every flipped
bit shows at every generation count compared (test_rule_ref_host.py, whose
checks run again here).  Fields and digests are compared exactly.
"""
import subprocess

import numpy as np
import pytest

import rule_ref as rr
from test_rule_ref_host import (ALL_RULES, DEPTHS, SHAPES, check_census, check_differs,
                                reference, start_cells)
from torus_ref import pack, roll_run

pytestmark = pytest.mark.gpu

STREAM = dict(resident=1, streams=1)
ENGINES = {
    "d1": dict(STREAM, tb_depth=1),
    "d8": dict(STREAM, tb_depth=8, handoff=1),
    "d12h": dict(STREAM, tb_depth=12, handoff=2, rows_per_wave=30),
    "d16": dict(STREAM, tb_depth=16),
    "res": dict(resident=2, tb_depth=16),
}
assert sorted(c["tb_depth"] for c in ENGINES.values()) == sorted(DEPTHS + [16])


def run(e, oracle, w, start, want, depth):
    """load, step(1), step(depth + 3); field and digest after each."""
    e.load_packed(start)
    done = 0
    for gens in (1, depth + 3):
        e.step(gens)
        done += gens
        got = e.store_packed()
        assert (got == want[done]).all(), f"after {done} generations"
        assert e.digest() == oracle.bp_digest(want[done], w), f"digest after {done} generations"


@pytest.mark.parametrize("rule", ALL_RULES, ids=rr.rule_name)
def test_rule_bits(pkg, oracle, model_plans, rule):
    for shape in sorted(SHAPES):
        h, w, _ = SHAPES[shape]
        check_census(shape)
        if rule in rr.CONWAY_XOR:
            check_differs(shape, rule)
        start, want = pack(start_cells(shape)), reference(shape, rule)
        for name, cfg in ENGINES.items():
            with pkg.Engine(h, w, rule=rule, device=0, **cfg) as e:
                assert name == "res" or e.tb_depth == cfg["tb_depth"], name
                assert e.handoff == (name == "d12h"), name
                assert (e.resident is not None) == (name == "res"), name
                try:
                    run(e, oracle, w, start, want, cfg["tb_depth"])
                except AssertionError as ex:
                    raise AssertionError(f"{rr.rule_name(rule)} {shape} {name}: {ex}") from None
    # the torus: the same start field with its edges joined, against the wrapped numpy step
    h, w, _ = SHAPES["130x200"]
    start = pack(start_cells("130x200"))
    with pkg.Engine(h, w, rule=rule, device=0, semantics=pkg.SEM_TORUS) as e:
        depth = e.tb_depth
        want = {1: roll_run(start, w, 1, rule)}
        want[depth + 4] = roll_run(want[1], w, depth + 3, rule)
        if rule in rr.CONWAY_XOR:  # (a border cell of a one-bit rule may not tell)
            assert (want[1] != reference("130x200", rule)[1]).any(), "the wrap does not show"
        run(e, oracle, w, start, want, depth)


def cli(pkg, d, h, w, gens, data, *args):
    (d / "data.txt").write_bytes(data)
    (d / "grid_size_data.txt").write_text(f"{h} {w} {gens}")
    return subprocess.run([pkg.CLI_PATH, "--dir", str(d), *args], capture_output=True, text=True,
                          timeout=120)


def test_cli_rule_strings(pkg, tmp_path):
    """gol --rule B.../S...: every digit 0..8 on either side, both letter cases, against
    numpy_run; malformed rules end with status 2 and `bad rule` before any GPU call."""
    h, w, gens = 33, 70, 5
    cells = rr.random_cells(h, w, 6)
    data = b"".join(bytes(np.where(r, 49, 48).astype(np.uint8)) + b"\n" for r in cells)
    for text, rule in (("B1357/S02468", (0b010101010, 0b101010101)),
                       ("b0248/s1", (0b100010101, 0b000000010))):
        assert rr.rule_name(rule).lower() == text.lower()
        r = cli(pkg, tmp_path, h, w, gens, data, "--rule", text)
        assert r.returncode == 0, r.stderr
        want = rr.numpy_run(cells, gens, rule)
        assert want.any() and (want != rr.numpy_run(cells, gens, rr.CONWAY)).any()
        assert (tmp_path / "output.txt").read_bytes() == \
            b"".join(bytes(np.where(r, 49, 48).astype(np.uint8)) + b"\n" for r in want), text
    (tmp_path / "output.txt").unlink()
    for text in ("B9/S", "B3S23", "3/23", "B3/"):
        r = cli(pkg, tmp_path, h, w, gens, data, "--rule", text)
        assert r.returncode == 2 and "bad rule" in r.stderr, (text, r.returncode, r.stderr)
        assert not (tmp_path / "output.txt").exists()
