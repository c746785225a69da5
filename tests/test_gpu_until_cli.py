"""GPU: `gol --until-periodic LAG[:EVERY]` writes the output.txt the run without the
flag writes, and reports the generation and period in one extra line."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

H, W = 100, 90


def run_cli(pkg, oracle, tmp_path, name, epochs, *flags):
    d = tmp_path / name
    d.mkdir()
    (d / "grid_size_data.txt").write_text(f"{H} {W} {epochs}\n")
    (d / "data.txt").write_bytes(oracle.bp_unpack(oracle.bp_random(H, W, 6), W))
    r = subprocess.run([pkg.CLI_PATH, "--dir", str(d), "--rule", "conway", *flags],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return (d / "output.txt").read_bytes(), r.stdout.splitlines()


def plain(lines):
    return [ln for ln in lines if not ln.startswith("Total time")]


def test_until_periodic_flag(pkg, oracle, tmp_path):
    assert os.path.exists(pkg.CLI_PATH)
    epochs = 1003  # past generation 576, where the field has period 6; (1003 - 576) % 6 = 1
    want = oracle.bp_unpack(oracle.bp_run(oracle.bp_random(H, W, 6), W, epochs, oracle.CONWAY), W)
    base, base_lines = run_cli(pkg, oracle, tmp_path, "base", epochs)
    got, lines = run_cli(pkg, oracle, tmp_path, "until", epochs, "--until-periodic", "6")
    assert base == want and got == want
    extra = [ln for ln in lines if "eriod" in ln]
    assert extra == ["Period 6 from generation 576 on (lag 6, checked every 64 generations)."]
    assert not [ln for ln in base_lines if "eriod" in ln]
    assert plain([ln for ln in lines if ln not in extra]) == plain(base_lines)
    # LAG:EVERY, and a limit the field does not settle within
    got, lines = run_cli(pkg, oracle, tmp_path, "short", 200, "--until-periodic", "6:32")
    assert got == oracle.bp_unpack(oracle.bp_run(oracle.bp_random(H, W, 6), W, 200, oracle.CONWAY), W)
    assert [ln for ln in lines if "eriod" in ln] == [
        "No period dividing 6 within 200 generations (checked every 32)."]


def test_until_periodic_needs_one_engine(pkg, tmp_path):
    for flags in (["--ref-ranks", "2"], ["--gpus", "1"], ["--stripes", "2"]):
        r = subprocess.run([pkg.CLI_PATH, "--dir", str(tmp_path), "--until-periodic", "6", *flags],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--until-periodic" in r.stderr
    r = subprocess.run([pkg.CLI_PATH, "--until-periodic", "x"], capture_output=True, text=True)
    assert r.returncode == 2 and "LAG[:EVERY]" in r.stderr
