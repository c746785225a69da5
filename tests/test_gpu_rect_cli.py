"""`gol --paste FILE@Y,X[:op]` and `gol --window Y,X,H,W`: the CLI's region I/O
against the binding's write_rect / read_rect on the same field."""
import subprocess

import numpy as np
import pytest

import torus_ref

H, W, GENS = 1500, 500, 6
PATTERN = ["0110", "1100", "0101"]  # 3 x 4, pasted at an odd offset


def setup_dir(tmp_path, ref_data, gens=GENS):
    (tmp_path / "data.txt").write_bytes(ref_data)
    (tmp_path / "grid_size_data.txt").write_text(f"{H} {W} {gens}")
    (tmp_path / "p.txt").write_text("".join(line + "\n" for line in PATTERN))
    return tmp_path


def run_cli(pkg, d, *args):
    return subprocess.run([pkg.CLI_PATH, "--dir", str(d), *args], capture_output=True, text=True,
                          timeout=300)


def test_help_and_bad_options(pkg, tmp_path, ref_data):
    """No GPU needed: --help names both options; a malformed option value or paste
    file ends the program before anything runs."""
    r = run_cli(pkg, tmp_path, "--help")
    assert r.returncode == 0 and "--paste" in r.stderr and "--window" in r.stderr
    d = setup_dir(tmp_path, ref_data)
    for extra in (["--paste", "p.txt"], ["--paste", f"{d}/p.txt@1"], ["--paste", f"{d}/p.txt@1,2:and"],
                  ["--window", "1,2,3"], ["--window", "1,2,3,x"]):
        r = run_cli(pkg, d, *extra)
        assert r.returncode == 2 and extra[0] in r.stderr, extra
    for name, text in (("ragged.txt", "010\n01\n"), ("letters.txt", "010\n0a0\n"), ("empty.txt", "")):
        (d / name).write_text(text)
        r = run_cli(pkg, d, "--paste", f"{d}/{name}@0,0")
        assert r.returncode == 1 and "gol error 1" in r.stderr and name in r.stderr
    r = run_cli(pkg, d, "--paste", f"{d}/missing.txt@0,0")
    assert r.returncode == 1 and "missing.txt" in r.stderr
    assert not (d / "output.txt").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("torus", [False, True], ids=["dead_border", "torus"])
def test_cli_paste_and_window_match_the_binding(pkg, oracle, tmp_path, ref_data, torus):
    d = setup_dir(tmp_path, ref_data)
    pat = np.array([[int(c) for c in line] for line in PATTERN], dtype=np.uint8)
    y, x = (H - 2, W - 3) if torus else (701, 61)  # torus: across the corner
    wy, wx, wh, ww = (H - 9, W - 70, 20, 131) if torus else (695, 31, 17, 129)
    extra = ["--torus"] if torus else []
    r = run_cli(pkg, d, "--rule", "conway", *extra, "--paste", f"{d}/p.txt@{y},{x}:xor",
                "--paste", f"{d}/p.txt@3,5", "--window", f"{wy},{wx},{wh},{ww}")
    assert r.returncode == 0, r.stderr
    with pkg.Engine(H, W, rule=pkg.CONWAY, device=0,
                    semantics=pkg.SEM_TORUS if torus else pkg.SEM_GLOBAL) as e:
        e.load_ascii(ref_data)
        e.write_rect(y, x, torus_ref.pack(pat), 4, pkg.RECT_XOR)
        e.write_rect(3, 5, torus_ref.pack(pat), 4, pkg.RECT_SET)
        e.step(GENS)
        win = e.read_rect(wy, wx, wh, ww)
    want = oracle.bp_unpack(win, ww)
    assert len(want) == wh * (ww + 1)
    assert (d / "output.txt").read_bytes() == want
    assert r.stdout.splitlines()[0] == "Process 0 wrote data to the file."
    # the window alone replaces an older, longer output.txt
    (d / "output.txt").write_bytes(b"x" * (len(want) + 100))
    r = run_cli(pkg, d, "--rule", "conway", *extra, "--paste", f"{d}/p.txt@{y},{x}:xor",
                "--paste", f"{d}/p.txt@3,5", "--window", f"{wy},{wx},{wh},{ww}")
    assert r.returncode == 0 and (d / "output.txt").read_bytes() == want


@pytest.mark.gpu
def test_cli_paste_outside_the_field(pkg, tmp_path, ref_data):
    d = setup_dir(tmp_path, ref_data)
    r = run_cli(pkg, d, "--paste", f"{d}/p.txt@{H - 2},0")
    assert r.returncode == 1 and "gol error 1" in r.stderr and "outside" in r.stderr
    r = run_cli(pkg, d, "--ref-ranks", "3", "--paste", f"{d}/p.txt@0,0")
    assert r.returncode == 1 and "gol error 6" in r.stderr
