"""CPU suite for the torus engines (GOL_SEM_TORUS): the host-only entry points
gol_torus_geometry and gol_torus_pad, the wrap rule's word gather under the host
sanitizers, and the tests' own torus reference (no GPU needed)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import torus_ref

CSRC = os.path.join(ROOT, "mpi-game-of-life_amd", "csrc")
RULES = {"B/S2": (0, 1 << 2), "B3/S23": (1 << 3, (1 << 2) | (1 << 3)),
         "B36/S23": ((1 << 3) | (1 << 6), (1 << 2) | (1 << 3))}


@pytest.mark.parametrize("h,w", [(1, 1), (1, 64), (3, 5), (5, 63), (7, 64), (9, 65), (4, 130),
                                 (37, 500)])
@pytest.mark.parametrize("G", [1, 16, 70, 130])
def test_torus_pad_is_modular_indexing(pkg, h, w, G):
    """Padded cell (y, x) = bits[(y - G) % h, (x - 64 Gx) % w], for ghost depths
    below and above h and w; bits past padded_w are 0."""
    rng = np.random.default_rng(1000 * h + w)
    bits = rng.integers(0, 2, (h, w), dtype=np.uint8)
    Gx = (G + 63) // 64
    field = torus_ref.pack(bits)
    # junk at columns >= w of the caller's last word must not show
    if w % 64:
        field = field.copy()
        field[:, -1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(w % 64)
    out = pkg.torus_pad(field, w, G, Gx)
    pw = w + 128 * Gx
    assert out.shape == (h + 2 * G, (w + 63) // 64 + 2 * Gx)
    got = torus_ref.unpack(out, out.shape[1] * 64)
    yy, xx = np.mgrid[0:h + 2 * G, 0:pw]
    assert (got[:, :pw] == bits[(yy - G) % h, (xx - 64 * Gx) % w]).all()
    assert not got[:, pw:].any()
    # the tests' own padding agrees (64 Gx columns left and right)
    assert (got[:, :pw] == torus_ref.wrap_pad(bits, G, 64 * Gx)).all()


def test_torus_pad_rejects_bad_args(pkg):
    a = np.zeros((4, 2), dtype=np.uint64)
    out = np.zeros((6, 3), dtype=np.uint64)
    L = pkg.lib()
    assert L.gol_torus_pad(a.ctypes.data, 2, 4, 100, 1, 1, out.ctypes.data, 3) == pkg.GOL_EINVAL
    assert L.gol_torus_pad(a.ctypes.data, 1, 4, 100, 1, 1, out.ctypes.data, 4) == pkg.GOL_EINVAL
    assert L.gol_torus_pad(None, 2, 4, 100, 1, 1, out.ctypes.data, 4) == pkg.GOL_EINVAL
    assert L.gol_torus_pad(a.ctypes.data, 2, 0, 100, 1, 1, out.ctypes.data, 4) == pkg.GOL_EINVAL


@pytest.mark.parametrize("h,w", [(1, 1), (1, 64), (64, 64), (37, 500), (1500, 500), (4096, 4096),
                                 (6140, 100), (6200, 4096), (65536, 65536)])
@pytest.mark.parametrize("rule", list(RULES))
def test_torus_geometry_auto(pkg, h, w, rule):
    g = pkg.torus_geometry(h, w, rule=RULES[rule])
    G = g["round_gens"]
    assert g["ghost_rows"] == G
    assert 64 * g["ghost_words"] >= G and g["ghost_words"] == (G + 63) // 64
    assert g["padded_h"] == h + 2 * G
    assert g["padded_w"] == w + 128 * g["ghost_words"]
    # the auto value: a positive multiple of the inner engine's streaming depth K
    # (what the planner reports for the padded field), at most 256 (128 above 2^25
    # cells), and at most min(h, w) / 4 where that is above K
    K = pkg.plan_model(g["padded_h"], g["padded_w"], rule=RULES[rule], streams=1)["tb_depth"]
    assert G > 0 and G % K == 0, (G, K)
    assert G <= (256 if h * w <= 1 << 25 else 128) and (G <= min(h, w) // 4 or G <= 2 * K)
    # the planner's view of a torus config is the inner engine's plan
    m = pkg.plan_model(h, w, rule=RULES[rule], semantics=pkg.SEM_TORUS)
    assert (m["tb_depth"], m["halo_depth"]) == (K, G)
    assert m["rows_hi"] == g["padded_h"]


@pytest.mark.parametrize("G", [1, 5, 64, 65, 200])
def test_torus_geometry_explicit_round(pkg, G):
    g = pkg.torus_geometry(257, 320, halo_depth=G)
    assert g["round_gens"] == g["ghost_rows"] == G
    assert g["ghost_words"] == (G + 63) // 64
    assert (g["padded_h"], g["padded_w"]) == (257 + 2 * G, 320 + 128 * g["ghost_words"])


def test_torus_geometry_rejects(pkg):
    """The GOL_EINVALs of gol_create for a torus config, with a message."""
    for kw in ({"streams": 2}, {"word_planes": 4}, {"halo_depth": 1 << 17}, {"tb_depth": 3},
               {"semantics": pkg.SEM_GLOBAL}):
        with pytest.raises(pkg.GolError) as ei:
            pkg.torus_geometry(100, 100, **kw)
        assert ei.value.status == pkg.GOL_EINVAL and str(ei.value).split(": ", 1)[1]
    for h, w in ((0, 10), (10, 0)):
        with pytest.raises(pkg.GolError) as ei:
            pkg.torus_geometry(h, w)
        assert ei.value.status == pkg.GOL_EINVAL
    with pytest.raises(pkg.GolError) as ei:
        pkg.torus_geometry(100, 100, streams=2)
    assert "stream" in str(ei.value)
    # semantics values past GOL_SEM_TORUS are still rejected
    with pytest.raises(pkg.GolError) as ei:
        pkg.plan_model(100, 100, semantics=3)
    assert ei.value.status == pkg.GOL_EINVAL


def test_torus_rejected_by_rank_entry_points(pkg):
    """Rank engines, groups and the round schedule are dead-border only; they say
    so before touching a GPU."""
    with pytest.raises(pkg.GolError) as ei:
        pkg.round_schedule(1000, 1000, 0, 2, 64, semantics=pkg.SEM_TORUS)
    assert ei.value.status == pkg.GOL_EINVAL
    with pytest.raises(pkg.GolError) as ei:
        pkg.Engine(1000, 1000, semantics=pkg.SEM_TORUS, rank=0, nranks=2, uid=b"\0" * 128)
    assert ei.value.status == pkg.GOL_EINVAL
    with pytest.raises(pkg.GolError) as ei:
        pkg.Engine(1000, 1000, semantics=pkg.SEM_TORUS, rank=0, nranks=2,
                   transport=lambda up, dn: (None, None))
    assert ei.value.status == pkg.GOL_EINVAL
    with pytest.raises(pkg.GolError) as ei:
        pkg.Group(1000, 1000, 2, semantics=pkg.SEM_TORUS)
    assert ei.value.status == pkg.GOL_EINVAL
    for kw in ({"streams": 2}, {"word_planes": 4}):
        with pytest.raises(pkg.GolError) as ei:
            pkg.Engine(100, 100, semantics=pkg.SEM_TORUS, **kw)
        assert ei.value.status == pkg.GOL_EINVAL


def test_wrap_gather_under_sanitizers(tmp_path):
    """The header gather against a per-bit loop, w in 1..200 and ghost depths up to
    130, as a stand-alone program under ASan + UBSan."""
    # the sanitizer runtimes are linked statically, so the program does not care
    # what else the loader brings in first; under tools/asan_cpu_suite.sh, which
    # preloads clang's shared runtime into every child, it links against that one
    if os.environ.get("GOL_ASAN_SUITE"):
        cxx, link = "/opt/rocm/lib/llvm/bin/clang++", ["-shared-libasan"]
    else:
        cxx, link = shutil.which("g++"), ["-static-libasan", "-static-libubsan"]
    assert cxx and os.path.exists(cxx), "no host C++ compiler"
    exe = tmp_path / "sweep"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", *link, f"-I{CSRC}",
                    os.path.join(ROOT, "tests", "torus_gather_sweep.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ")


@pytest.mark.parametrize("h,w", [(1, 1), (1, 7), (2, 3), (5, 64), (9, 65), (33, 130)])
@pytest.mark.parametrize("rule", list(RULES))
def test_reference_recipe_equals_roll(oracle, h, w, rule):
    """The GPU tests' reference (wrapped padding + the dead-border oracle + crop)
    against the np.roll torus."""
    rng = np.random.default_rng(h * 131 + w)
    start = torus_ref.pack(rng.integers(0, 2, (h, w), dtype=np.uint8))
    for gens in (1, 17):
        want = torus_ref.roll_run(start, w, gens, RULES[rule])
        assert (torus_ref.torus_run(oracle, start, w, gens, RULES[rule]) == want).all()
        assert (torus_ref.torus_run(oracle, start, w, gens, RULES[rule], chunk=5) == want).all()
