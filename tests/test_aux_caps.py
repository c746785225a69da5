"""CPU: every case of tests/aux_cases.py crosses the threshold it claims to cross.

The grid caps of the auxiliary kernels, the snapshot compare's tile shape and
rect_stage's keep limit are read out of the sources with regular expressions (as
tests/test_stage_logic.py reads the stencil's immediates); a pattern that no longer
matches fails the test.  Whoever raises a cap or reshapes a tile has to enlarge the
cases of tests/test_gpu_aux_scale.py with it: below the cap a case runs only the first
trip of the kernel's grid-stride loop, which every small test runs already.

Each test prints the item counts next to the caps (pytest -s, or -rP).
"""
import os
import re

import numpy as np

import aux_cases as ac
import torus_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpi-game-of-life_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def launcher_trips():
    """launcher name -> wavefronts or threads (= items) per trip of its kernel's loop:
    grid_for(items, per_block, cap) launches at most `cap` workgroups of 256 threads,
    and a workgroup takes per_block items per trip (256: one per thread, 4: one per
    wavefront)."""
    src = source("life_aux.hip")
    assert re.search(r"dim3 grid_for\(int64_t items, int64_t per_block, int64_t cap\)", src)
    out = {}
    bodies = re.split(r"\nhipError_t launch_(\w+)\(", src)
    for name, body in zip(bodies[1::2], bodies[2::2]):
        m = re.search(r"grid_for\((.*?),\s*(\d+),\s*(\d+)\)", body)
        if not m:
            continue
        per_block, cap = int(m.group(2)), int(m.group(3))
        assert per_block in (256, 256 // 64), (name, per_block)
        assert "dim3(256)" in body and "dim3(64" not in body, name
        out[name] = per_block * cap
    return out


def trips_of(name):
    t = launcher_trips()
    assert name in t, f"no grid_for(...) found in launch_{name}"
    return t[name]


def snap_consts():
    hdr = source("life_internal.h")
    c = {k: int(v) for k, v in
         re.findall(r"constexpr int (kWavesPerBlock|kCopyTileRows|kCopyTileWords) = (\d+);", hdr)}
    assert set(c) == {"kWavesPerBlock", "kCopyTileRows", "kCopyTileWords"}, c
    m = re.search(r"life_snap_diff_kernel,\s*dim3\(\(unsigned\)min\(blocks,\s*\(int64_t\)(\d+)\)\),"
                  r"\s*dim3\(64 \* kWavesPerBlock\)", source("life_snap.hip"))
    assert m, "the diff launch's workgroup cap was not found in life_snap.hip"
    c["diff_blocks"] = int(m.group(1))
    c["diff_trip"] = c["diff_blocks"] * c["kWavesPerBlock"]  # tiles per trip
    return c


def stage_keep():
    m = re.search(r"constexpr size_t kRectStageKeep = (\d+)u << (\d+);", source("engine.cpp"))
    assert m, "kRectStageKeep was not found in engine.cpp"
    assert re.search(r"if \(bytes > kRectStageKeep\) \{\s*HIP_TRY\(hipMalloc\(&s->p, bytes\)\);",
                     source("engine.cpp"))
    return int(m.group(1)) << int(m.group(2))


def test_every_pattern_matches():
    t = launcher_trips()
    for name in ("rect_read", "rect_write", "density", "ascii_pack", "ascii_unpack", "torus_wrap"):
        assert name in t, name
        print(f"launch_{name}: {t[name]} items per trip")
    c = snap_consts()
    print("snapshot compare:", c)
    print("kRectStageKeep:", stage_keep())
    # the increments the second trips take
    aux, snap = source("life_aux.hip"), source("life_snap.hip")
    assert len(re.findall(r"k \+= nwaves\)", aux)) == 3  # ascii pack, unpack, density
    assert len(re.findall(r"k \+= \(int64_t\)gridDim\.x \* blockDim\.x\)", aux)) == 5
    assert re.search(r"tile < \(uint32_t\)a\.ntile; tile \+= nwaves\)", snap)


def test_case1_snapshot_tiles():
    c, s = snap_consts(), ac.SNAP
    tr, tw, trip = c["kCopyTileRows"], c["kCopyTileWords"], c["diff_trip"]
    nwords = ac.cdiv(s.w, 64)
    ntile = ac.snap_tiles(s.h, nwords, tr, tw)
    print(f"case 1: {ntile} tiles, {trip} per trip")
    assert ntile > trip
    assert ac.cdiv(nwords, tw) == 2 and s.h % tr, "two tile columns, a partial last tile row"
    assert nwords % tw == 1, "the second tile column is the row's last word, the one SnapArgs::mask meets"
    for tile, (y, x) in s.flips:
        assert y < s.h and x < s.w
        assert ac.snap_tile_of(y, x, nwords, tr, tw) == tile, (tile, y, x)
    tiles = [t for t, _ in s.flips]
    assert {0, trip - 1, trip, trip + 1, ntile - 2, ntile - 1} <= set(tiles)
    assert any(x >= 64 * tw for _, (_, x) in s.flips) and any(x < 64 * tw for _, (_, x) in s.flips)
    y, x, rh, rw = s.second_trip_window
    assert y + rh <= s.h and x + rw <= s.w
    assert ac.snap_tile_of(y, 0, nwords, tr, tw) >= trip, "the window lies in second-trip tiles"
    assert x < 64 * tw < x + rw


def test_case2_rect_items():
    r = ac.RECT
    cap_r, cap_w = trips_of("rect_read"), trips_of("rect_write")
    for kind, kw in r.kinds.items():
        torus = kw.get("semantics") == 2
        for win in [r.window] + ([r.torus_window] if torus else []):
            ps = ac.pieces(torus, r.h, r.w, *win)
            reads = [ac.rect_read_items(rn, cn) for _, _, rn, cn, _, _ in ps]
            writes = [ac.rect_write_items(c0, rn, cn) for _, c0, rn, cn, _, _ in ps]
            print(f"case 2 {kind} {win}: read {reads} / {cap_r}, write {writes} / {cap_w}")
            assert max(reads) > cap_r and max(writes) > cap_w
            assert max(ac.stage_bytes_rect(rn, cn) for _, _, rn, cn, _, _ in ps) <= stage_keep()
    assert len(ac.pieces(True, r.h, r.w, *r.torus_window)) == 4, "both seams"
    y, x, rh, rw = r.window
    assert y + rh <= r.h and x + rw <= r.w and x % 64 and (x + rw) % 64


def test_case3_density_items():
    r = ac.RECT
    cap = trips_of("density")
    by, bx = r.second_trip_block
    for win in ((0, 0, r.h, r.w), r.window):
        y, x, rh, rw = win
        for (b_y, b_x), why in r.blocks.items():
            items, nchunk = ac.density_items(x, rw, 0, rh, b_y)
            print(f"case 3 {win} blocks {b_y} x {b_x}: {items} items, {nchunk} chunks ({why})")
            assert nchunk >= 2, "more than 64 lane groups: a block fed from several chunks"
            assert ac.stage_bytes_density(rh, rw, b_y, b_x) <= stage_keep()
        items, _ = ac.density_items(x, rw, 0, rh, by)
        print(f"case 3 {win} blocks {by} x {bx}: {items} / {cap}")
        assert items > cap
        assert bx > 64 * 64, "a block wider than a chunk"
    # the seam window's large piece
    ps = ac.pieces(True, r.h, r.w, *r.torus_window)
    assert max(ac.density_items(c0, cn, wr, rn, r.seam_block[0])[1] for _, c0, rn, cn, wr, _ in ps) >= 2


def test_case4_staging_bytes():
    s, keep = ac.STAGE, stage_keep()
    y, x, rh, rw = s.window
    assert y + rh <= s.h and x + rw <= s.w
    b = ac.stage_bytes_rect(rh, rw)
    print(f"case 4 window: {b} bytes staged / {keep} kept")
    assert b > keep
    y, x, rh, rw, by, bx = s.density
    b = ac.stage_bytes_density(rh, rw, by, bx)
    print(f"case 4 density: {b} bytes staged / {keep} kept")
    assert b > keep
    y, x, rh, rw = s.small
    assert ac.stage_bytes_rect(rh, rw) <= keep


def test_case5_ascii_items():
    a = ac.ASCII
    for name in ("ascii_pack", "ascii_unpack"):
        cap = trips_of(name)
        items = ac.ascii_items(a.h, a.w)
        print(f"case 5 {name}: {items} / {cap}")
        assert items > cap
        ng = ac.ascii_items(1, a.w)
        assert ac.ascii_item_of(a.bad_row, ng - 1, a.w) >= cap, "the line end's check"
        assert ac.ascii_item_of(a.ones_from, 0, a.w) >= cap and a.ones_from < a.h


def test_case6_wrap_items(pkg):
    w_, cap = ac.WRAP, trips_of("torus_wrap")
    geo = pkg.torus_geometry(w_.h, w_.w, halo_depth=w_.kw["halo_depth"])
    assert (geo["ghost_rows"], geo["ghost_words"]) == (w_.ghost_rows, w_.ghost_words)
    items, ghost = ac.torus_wrap_items(w_.h, w_.w, w_.ghost_rows, w_.ghost_words)
    print(f"case 6: {items} items ({ghost} of the ghost rows) / {cap}")
    assert items > cap
    assert cap < ghost, "the second trip holds every side word of the interior rows"
    c = snap_consts()
    tiles = ac.snap_tiles(w_.h, ac.cdiv(w_.w, 64), c["kCopyTileRows"], c["kCopyTileWords"])
    print(f"case 6 snapshot view: {tiles} tiles / {c['diff_trip']} (one trip)")
    y, x, rh, rw = w_.corner
    assert y + rh > w_.h and x + rw > w_.w, "the window crosses the corner"


def test_case7_composite_tiles(pkg):
    c, s = snap_consts(), ac.COMPOSITE
    tr, tw, trip = c["kCopyTileRows"], c["kCopyTileWords"], c["diff_trip"]
    n = s.kw["streams"]
    spans = [pkg.rank_rows(s.h, n, r) for r in range(n)]
    starts = [r0 for r0, _ in spans]
    nwords = ac.cdiv(s.w, 64)
    for leaf, (r0, rows) in enumerate(spans):
        ntile = ac.snap_tiles(rows, nwords, tr, tw)
        print(f"case 7 leaf {leaf}: rows [{r0}, {r0 + rows}), {ntile} tiles / {trip}")
        assert ntile > trip
    flips = ac.composite_flips(s.h, s.w, starts, tr, tw)
    cells = [cell for _, _, cell in flips]
    assert len(set(cells)) == len(cells)
    for leaf, (r0, rows) in enumerate(spans):
        mine = [(t, cell) for lf, t, cell in flips if lf == leaf]
        assert all(r0 <= y < r0 + rows and 0 <= x < s.w for _, (y, x) in mine)
        assert sum(t >= trip for t, _ in mine) >= 2 and sum(t < trip for t, _ in mine) >= 1
    b = starts[1]
    assert {b - 1, b} <= {y for y, _ in cells}


def test_packed_window_references():
    """aux_cases.packed_window / placed_window (case 4's references on packed words)
    against the cell-by-cell crop and paste of torus_ref on a small field."""
    rng = np.random.default_rng(7)
    h, w = 9, 333
    bits = rng.integers(0, 2, (h, w), dtype=np.uint8)
    words = torus_ref.pack(bits)
    for y, x, rh, rw in ((0, 0, h, w), (1, 31, 7, 200), (2, 64, 3, 128), (0, 63, 9, 270),
                         (3, 5, 2, 1), (0, 300, 9, 33), (4, 192, 1, 141)):
        want = torus_ref.pack(bits[y:y + rh, x:x + rw])
        assert (ac.packed_window(words, y, x, rh, rw) == want).all(), (y, x, rh, rw)
        win = rng.integers(0, 1 << 63, (rh, ac.cdiv(rw, 64) + 1), dtype=np.uint64)  # junk beyond rw
        cells = np.zeros((rh, w), dtype=np.uint8)
        cells[:, x:x + rw] = torus_ref.unpack(win, rw)
        assert (ac.placed_window(win, x, rw, words.shape[1]) == torus_ref.pack(cells)).all()


def test_gpu_file_references():
    """The numpy references of tests/test_gpu_aux_scale.py (crop, paste, block_sums,
    ascii_text, first_diff) against index-by-index models on a small field whose windows
    cross the seams."""
    import test_gpu_aux_scale as t

    rng = np.random.default_rng(8)
    h, w = 23, 201
    bits = rng.integers(0, 2, (h, w), dtype=np.uint8)
    for y, x, rh, rw in ((0, 0, h, w), (3, 5, 7, 100), (20, 190, 10, 50), (22, 200, 23, 201),
                         (0, 150, 5, 201), (18, 0, 23, 3)):
        win, words = t.random_window(rng, rh, rw)
        assert win.shape == (rh, rw) and (torus_ref.unpack(words, rw) == win).all()
        ix = np.ix_((y + np.arange(rh)) % h, (x + np.arange(rw)) % w)
        assert (t.crop(bits, y, x, rh, rw) == bits[ix]).all()
        for op in (0, 2):
            want = bits.copy()
            want[ix] = win if op == 0 else bits[ix] ^ win
            assert (t.paste(bits, y, x, win, op) == want).all(), (y, x, rh, rw, op)
        for by, bx in ((1, 1), (1, 64), (8, 8), (16, 100), (64, 64), (rh, rw), (3, 7)):
            want = np.array([[win[i:i + by, j:j + bx].sum() for j in range(0, rw, bx)]
                             for i in range(0, rh, by)])
            assert (t.block_sums(win, by, bx) == want).all(), (by, bx)
    text = t.ascii_text(bits)
    assert text == b"".join(bytes(48 + int(c) for c in row) + b"\n" for row in bits)
    assert t.first_diff(text, text) is None and t.first_diff(text, text[:-1]) == -1
    other = bytearray(text)
    other[777] ^= 1
    assert t.first_diff(bytes(other), text) == 777


def batch_launcher_trips():
    """launcher name -> items per trip of its kernel's loop in life_batch_aux.hip, as
    launcher_trips() for life_aux.hip: batch_grid(items, per_block, cap)."""
    src = source("life_batch_aux.hip")
    assert re.search(r"dim3 batch_grid\(int64_t items, int64_t per_block, int64_t cap\)", src)
    out = {}
    bodies = re.split(r"\nhipError_t launch_batch_(\w+)\(", src)
    for name, body in zip(bodies[1::2], bodies[2::2]):
        m = re.search(r"batch_grid\((.*?),\s*(\d+),\s*(\d+)\)", body)
        if not m:
            continue
        per_block, cap = int(m.group(2)), int(m.group(3))
        assert per_block in (256, 256 // 64), (name, per_block)
        assert "dim3(256)" in body, name
        out[name] = (m.group(1).strip(), per_block * cap)
    return out


def test_batch_codec_patterns_match():
    t = batch_launcher_trips()
    assert set(t) >= {"load", "store", "init_random", "digest"}, sorted(t)
    # the item counts the formulas of aux_cases.py restate
    assert t["load"][0] == t["store"][0] == "count * g.h * g.wq"
    assert t["init_random"][0] == "g.n * g.h * g.wq" and t["digest"][0] == "count"
    for name in ("load", "store", "init_random", "digest"):
        print(f"launch_batch_{name}: {t[name][1]} items per trip")
    src = source("life_batch_aux.hip")
    # the increments the second trips take: load, store, init_random; digest
    assert len(re.findall(r"k \+= \(int64_t\)gridDim\.x \* blockDim\.x\)", src)) == 3
    assert len(re.findall(r"for \(int64_t i = wave0; i < count; i \+= nwaves\)", src)) == 1
    assert re.search(r"nwaves = \(\(int64_t\)gridDim\.x \* blockDim\.x\) >> 6;", src)


def test_case8_batch_codec_items(pkg):
    c, t = ac.BATCH_CODEC, batch_launcher_trips()
    geo = pkg.batch_geometry(c.n, c.h, c.w)
    assert (geo["lanes_per_field"], geo["fields_per_wave"]) == (16, 4)
    assert geo["lanes_per_field"] > ac.cdiv(c.w, 64), "padding lanes"
    items = ac.batch_codec_items(c.n, c.h, c.w)
    for name in ("load", "store", "init_random"):
        cap = t[name][1]
        print(f"case 8 {name}: {items} / {cap}")
        assert items > cap
        f, r, q = ac.batch_field_of_word(cap, c.h, c.w)
        print(f"case 8 {name}: the second trip starts at field {f}, row {r}, word {q}")
        assert f == c.boundary[1] and 0 < r < c.h, "the trips' border lies inside a field"
        assert c.boundary == (f - 1, f, f + 1) and f + 1 < c.n - 1
    cap = t["store"][1]
    first, count = c.sub
    assert first < c.boundary[1] < first + count <= c.n
    assert ac.batch_codec_items(count, c.h, c.w) <= cap
    first, count = c.sub_trip
    sub = ac.batch_codec_items(count, c.h, c.w)
    print(f"case 8 sub-range store: {sub} / {cap}")
    assert sub > cap and first > 0 and first + count < c.n
    f, r, q = ac.batch_field_of_word(cap, c.h, c.w)
    assert first + f < first + count


def test_case9_batch_digest_items(pkg):
    c, t = ac.BATCH_DIGEST, batch_launcher_trips()
    cap = t["digest"][1]
    items = ac.batch_digest_items(c.n)
    print(f"case 9 digest: {items} / {cap}")
    assert items > cap
    first, count = c.sub
    assert first < cap < first + count <= c.n, "the slice crosses the whole call's border"
    assert ac.batch_digest_items(count) <= cap
    assert pkg.batch_geometry(c.n, c.h, c.w)["lanes_per_field"] == 2


def test_rule_pairs_batch_is_one_trip():
    """Why the suite's largest batch before cases 8 and 9 was not enough: its words land
    exactly on the cap, and digest was never called on it."""
    c, t = ac.RULE_PAIRS, batch_launcher_trips()
    items = ac.batch_codec_items(c.n, c.h, c.w)
    for name in ("load", "store"):
        print(f"test_every_rule_pair_once {name}: {items} / {t[name][1]}")
        assert items <= t[name][1]
