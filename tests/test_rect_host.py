"""CPU suite for the region I/O (gol_read_rect / gol_write_rect / gol_density): the
host-only blit gol_rect_blit against numpy, its argument checks, and the shared
word gather and merge of rect_blit.h under the host sanitizers (no GPU needed)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import torus_ref

CSRC = os.path.join(ROOT, "mpi-game-of-life_amd", "csrc")
OFFS = (0, 1, 31, 32, 63)
COLS = (1, 2, 63, 64, 65, 127, 128, 129, 200)


def np_blit(src_bits, sx, dst_bits, dx, cols, op):
    s = src_bits[:, sx:sx + cols]
    d = dst_bits[:, dx:dx + cols]
    out = dst_bits.copy()
    out[:, dx:dx + cols] = (s, d | s, d ^ s, d & (1 - s))[op]
    return out


@pytest.mark.parametrize("so", OFFS)
@pytest.mark.parametrize("do", OFFS)
def test_rect_blit_matches_numpy(pkg, so, do):
    """Every (sx mod 64, dx mod 64), width, op and 1..3 rows: the blitted bits, and
    every destination bit outside [dx, dx + cols) unchanged."""
    rng = np.random.default_rng(100 * so + do)
    for cols in COLS:
        for op in (pkg.RECT_SET, pkg.RECT_OR, pkg.RECT_XOR, pkg.RECT_CLEAR):
            for rows in (1, 2, 3):
                sx, dx = 64 + so, 128 + do
                sw, dw = (sx + cols + 63) // 64, (dx + cols + 63) // 64 + 1
                src = rng.integers(0, 2, (rows, sw * 64), dtype=np.uint8)
                dst = rng.integers(0, 2, (rows, dw * 64), dtype=np.uint8)
                got = torus_ref.pack(dst)
                pkg.rect_blit(torus_ref.pack(src), sx, got, dx, rows, cols, op)
                want = np_blit(src, sx, dst, dx, cols, op)
                assert (torus_ref.unpack(got, dw * 64) == want).all(), (cols, op, rows)


def test_rect_blit_rejects_bad_args(pkg):
    L = pkg.lib()
    a = np.zeros((2, 2), dtype=np.uint64)
    b = np.ones((2, 2), dtype=np.uint64)
    # bits [70, 140) need 3 words per row
    assert L.gol_rect_blit(a.ctypes.data, 2, 70, b.ctypes.data, 2, 0, 2, 70, 0) == pkg.GOL_EINVAL
    assert L.gol_rect_blit(a.ctypes.data, 2, 0, b.ctypes.data, 2, 70, 2, 70, 0) == pkg.GOL_EINVAL
    assert L.gol_rect_blit(a.ctypes.data, 0, 0, b.ctypes.data, 2, 0, 2, 1, 0) == pkg.GOL_EINVAL
    assert L.gol_rect_blit(a.ctypes.data, 2, 0, b.ctypes.data, 2, 0, 2, 64, 4) == pkg.GOL_EINVAL
    assert L.gol_rect_blit(None, 2, 0, b.ctypes.data, 2, 0, 2, 64, 0) == pkg.GOL_EINVAL
    assert pkg.lib().gol_last_error()
    assert (b == 1).all()
    with pytest.raises(pkg.GolError) as ei:
        pkg.rect_blit(a, 0, b, 0, 2, 64, op=7)
    assert ei.value.status == pkg.GOL_EINVAL and "op" in str(ei.value)
    # nothing to do is not an error
    assert L.gol_rect_blit(a.ctypes.data, 2, 0, b.ctypes.data, 2, 0, 0, 64, 0) == pkg.GOL_OK
    assert L.gol_rect_blit(a.ctypes.data, 2, 0, b.ctypes.data, 2, 0, 2, 0, 0) == pkg.GOL_OK
    assert (b == 1).all()


def test_rect_ops_are_the_header_enum(pkg):
    hdr = open(os.path.join(ROOT, "include", "gol.h")).read()
    for name, val in (("SET", pkg.RECT_SET), ("OR", pkg.RECT_OR), ("XOR", pkg.RECT_XOR),
                      ("CLEAR", pkg.RECT_CLEAR)):
        assert f"GOL_RECT_{name} = {val}" in hdr


def test_rect_blit_under_sanitizers(tmp_path):
    """rect_blit.h against a per-bit loop, as a stand-alone program under ASan + UBSan
    (built and run like the torus gather sweep)."""
    if os.environ.get("GOL_ASAN_SUITE"):
        cxx, link = "/opt/rocm/lib/llvm/bin/clang++", ["-shared-libasan"]
    else:
        cxx, link = shutil.which("g++"), ["-static-libasan", "-static-libubsan"]
    assert cxx and os.path.exists(cxx), "no host C++ compiler"
    exe = tmp_path / "sweep"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", *link, f"-I{CSRC}",
                    os.path.join(ROOT, "tests", "rect_blit_sweep.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ")
