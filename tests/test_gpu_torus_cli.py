"""`gol --torus`: the reference program's files and output.txt format with the
field's opposite edges joined, byte for byte against the torus reference of
torus_ref.py unpacked to ASCII."""
import subprocess

import pytest

import torus_ref

H, W, GENS = 1500, 500, 6


def setup_dir(tmp_path, ref_data):
    (tmp_path / "data.txt").write_bytes(ref_data)
    (tmp_path / "grid_size_data.txt").write_text(f"{H} {W} {GENS}")
    return tmp_path


def run_cli(pkg, d, *args):
    return subprocess.run([pkg.CLI_PATH, "--dir", str(d), *args], capture_output=True, text=True,
                          timeout=300)


def test_torus_flag_conflicts_and_help(pkg, tmp_path, ref_data):
    """No GPU needed: --help names --torus, and it is rejected with --ref-ranks and
    with --gpus / --stripes above 1 before anything is read."""
    r = run_cli(pkg, tmp_path, "--help")
    assert r.returncode == 0 and "--torus" in r.stderr
    d = setup_dir(tmp_path, ref_data)
    for extra in (["--ref-ranks", "2"], ["--gpus", "2"], ["--stripes", "3"],
                  ["--gpus", "1", "--stripes", "2"]):
        r = run_cli(pkg, d, "--torus", *extra)
        assert r.returncode == 2 and "--torus" in r.stderr, extra
        assert not (d / "output.txt").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("rule_arg,rule", [(None, (0, 1 << 2)),
                                           ("conway", (1 << 3, (1 << 2) | (1 << 3)))])
def test_cli_torus_matches_reference(pkg, oracle, tmp_path, ref_data, rule_arg, rule):
    d = setup_dir(tmp_path, ref_data)
    r = run_cli(pkg, d, "--torus", *(["--rule", rule_arg] if rule_arg else []))
    assert r.returncode == 0, r.stderr
    start = oracle.bp_pack(ref_data, H, W)
    want = torus_ref.torus_run(oracle, start, W, GENS, rule)
    assert (d / "output.txt").read_bytes() == oracle.bp_unpack(want, W)
    # the wrap shows: the dead-border run differs
    assert not (want == oracle.bp_run(start, W, GENS, rule)).all()
    lines = r.stdout.splitlines()
    assert lines[0] == "Process 0 wrote data to the file." and len(lines) == 2


@pytest.mark.gpu
def test_cli_torus_with_one_gpu_one_stripe(pkg, oracle, tmp_path, ref_data):
    """--gpus 1 --stripes 1 are the torus engine's own values."""
    d = setup_dir(tmp_path, ref_data)
    r = run_cli(pkg, d, "--torus", "--gpus", "1", "--stripes", "1", "--halo-depth", "4")
    assert r.returncode == 0, r.stderr
    want = torus_ref.torus_run(oracle, oracle.bp_pack(ref_data, H, W), W, GENS, (0, 1 << 2))
    assert (d / "output.txt").read_bytes() == oracle.bp_unpack(want, W)
