"""CPU: the case list of tests/batch_lattice.py meets every class of the batch kernels'
lane setup with every other, and its restatements agree with the library and the oracle.

rows_in_regs and lanes_per_field come from gol_batch_geometry (host only), not from the
restatement.  The lane-setup expressions are read out of life_batch.h and
life_batch_until.h with regular expressions, as tests/test_aux_caps.py reads the grid
caps: a pattern that no longer matches fails the test, and whoever rewrites the setup
has to revisit the classes of batch_lattice.py.
"""
import os
import re

import numpy as np
import pytest

import batch_lattice as bl
import batch_ref
import batch_rules_ref
import batch_until_ref
import rule_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpi-game-of-life_amd", "csrc")
BOUNDARIES = ("global", "torus")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.fixture(scope="module")
def geo(pkg):
    """case -> {boundary: gol_batch_geometry}."""
    sems = {"global": pkg.SEM_GLOBAL, "torus": pkg.SEM_TORUS}
    return {c: {b: pkg.batch_geometry(c.n, c.h, c.w, semantics=sems[b]) for b in BOUNDARIES}
            for c in bl.CASES}


def test_the_lists_are_the_issue_s():
    assert bl.H == [1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64]
    assert bl.WQ == [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64]
    assert len(bl.CASES) == len({(c.h, c.w) for c in bl.CASES}) == 544
    assert len(bl.UNTIL_CASES) == len(bl.H) * len(bl.WQ) == 224
    assert all(1 <= c.h <= 64 and 1 <= c.w <= 4096 and c.n >= 1 for c in bl.CASES)
    print(f"{len(bl.CASES)} cases, {sum(c.n * c.h * c.w for c in bl.CASES)} cells")


def test_restatement_agrees_with_batch_geometry(geo):
    for c in bl.CASES:
        for b in BOUNDARIES:
            assert geo[c][b] == {"lanes_per_field": bl.lanes_per_field(c.w),
                                 "fields_per_wave": bl.fields_per_wave(c.w),
                                 "rows_in_regs": bl.rows_in_regs(c.h),
                                 "waves": bl.waves(c.n, c.w)}, (c, b)


def test_kernel_constants_are_the_restated_ones():
    hdr = source("life_batch.h")
    m = re.search(r"constexpr int kBatchRowsList\[\] = \{([\d, ]+)\};", hdr)
    assert m and tuple(int(x) for x in m.group(1).split(",")) == bl.ROWS_LIST
    m = re.search(r"constexpr int kBatchWaves = (\d+);", hdr)
    assert m and int(m.group(1)) == bl.BATCH_WAVES
    cpp = source("batch.cpp")
    assert re.search(r"while \(s->lpf < s->wq\) \{\s*s->lpf \*= 2;\s*s->lpf_shift \+= 1;", cpp)
    assert re.search(r"s->rows = 8;\s*while \(s->rows < h\) s->rows \*= 2;", cpp)


# the lane setup, line by line: what batch_lattice.py's classes are derived from
SETUP = [
    r"const int q = lane & \(lpf - 1\);",
    r"const int64_t f = \(wave << \(6 - a\.lpf_shift\)\) \+ \(lane >> a\.lpf_shift\);",
    r"const bool live = q < a\.wq && f < a\.n;",
    r"const bool first = q == 0, last_lane = q == a\.wq - 1;",
    r"b\.inner_l = first \? 0u : ~0u;",
    r"b\.inner_r = last_lane \? 0u : ~0u;",
    r"const uint64_t m = live \? \(last_lane \? a\.lastmask : ~0ull\) : 0ull;",
    r"b\.partner = 4 \* \(first \? lane \+ a\.wq - 1 : last_lane \? lane - \(a\.wq - 1\) : lane\);",
    r"const uint32_t cl = \(uint32_t\)\(a\.w - 1\) & 63u, cg = \(uint32_t\)a\.w & 63u;",
    r"b\.send_hi = \(last_lane && \(cl & 1u\)\) \? ~0u : 0u;",
    r"b\.lshl = 31u - \(cl >> 1\);",
    r"b\.wfull = cg == 0u \? ~0u : 0u;",
    r"b\.gm\[0\] = \(last_lane && cg != 0u && !\(cg & 1u\)\) \? 1u << \(cg >> 1\) : 0u;",
    r"b\.gm\[1\] = \(last_lane && \(cg & 1u\)\) \? 1u << \(cg >> 1\) : 0u;",
]


@pytest.mark.parametrize("name,fn", [("life_batch.h", "batch_run"),
                                     ("life_batch_until.h", "batch_until_run")])
def test_lane_setup_is_the_one_the_classes_restate(name, fn):
    src = source(name)
    at = src.find(f"void {fn}(const Batch")
    assert at > 0, f"{fn} was not found in {name}"
    body = src[at:]
    for pat in SETUP:
        assert len(re.findall(pat, body)) == 1, (name, pat)
    # the until kernel's place at the schedule's events repeats field and liveness
    if fn == "batch_until_run":
        place = src[src.find("BatchUntilPlace batch_until_place("):at]
        assert re.search(r"p\.f = \(wave << \(6 - a\.lpf_shift\)\) \+ \(lane >> a\.lpf_shift\);", place)
        assert re.search(r"p\.head = q == 0 && p\.f < a\.n;", place)
        assert re.search(r"p\.live = q < a\.wq && p\.f < a\.n;", place)
        assert re.search(r"p\.off = wave \* \(int64_t\)a\.h \* 64 \+ lane;", place)


def test_row_and_word_expressions():
    hdr, until = source("life_batch.h"), source("life_batch_until.h")
    # the pass: which steps run, what step R and step h ingest
    assert re.search(r"for \(int t = 1; t <= R; \+\+t\) \{\s*if \(t <= h\) \{", hdr)
    assert re.search(r"if \(t < R\) \{\s*in = x\[t\];.*\n\s*\} else \{\s*in\.v\[0\] = in\.v\[1\] = 0u;", hdr)
    assert re.search(r"if constexpr \(TORUS\) \{\s*if \(t == h\) in = top;", hdr)
    assert re.search(r"if constexpr \(TORUS\) \{\s*if \(t == h\) last = y;", hdr)
    assert re.search(r"const uint32_t wl = from_last << b\.lshl;", hdr)
    assert re.search(r"const uint32_t wr = from_first & b\.wfull;", hdr)
    # the internal order
    assert re.search(r"const int64_t v = f >> \(6 - lpf_shift\);\s*"
                     r"const int64_t l = \(\(f & \(\(64 >> lpf_shift\) - 1\)\) << lpf_shift\) \+ q;\s*"
                     r"return \(v \* h \+ r\) \* 64 \+ l;", hdr)
    # the until kernel's per-field ballot
    assert re.search(r"p\.fmask = \(lpf == 64 \? ~0ull : \(1ull << lpf\) - 1ull\) << "
                     r"\(lane & ~\(lpf - 1\)\);", until)
    assert re.search(r"const bool eq = \(__ballot\(d != 0u\) & p\.fmask\) == 0ull;", until)
    assert re.search(r"if \(wave >= a\.waves\) return;", hdr)
    assert re.search(r"if \(wave >= u\.a\.waves\) return;", until)


def test_phase_table():
    """lane_setup() on the six phases, written out (the table of batch_lattice.py)."""
    want = {1: (0, False, 31, 1, (1, 0)), 2: (1, True, 31, 2, (0, 1)),
            33: (32, False, 15, 33, (1, 16)), 62: (61, True, 1, 62, (0, 31)),
            63: (62, False, 0, 63, (1, 31)), 64: (63, True, 0, 0, None)}
    assert tuple(sorted(want)) == bl.PHASES
    for wq in bl.WQ:
        for p, (cl, hi, lshl, cg, ghost) in want.items():
            s = bl.lane_setup(bl.width(wq, p))
            assert (s["cl"], s["send_hi"], s["lshl"], s["cg"], s["ghost"]) == (cl, hi, lshl, cg, ghost)
            assert s["wfull"] == (ghost is None)
            assert bl.phase(bl.width(wq, p)) == p and bl.words(bl.width(wq, p)) == wq
    got = [bl.lane_setup(bl.width(1, p)) for p in bl.PHASES]
    assert {s["lshl"] for s in got} == {31, 15, 1, 0}
    assert {s["ghost"] for s in got} == {(1, 0), (0, 1), (1, 16), (0, 31), (1, 31), None}
    assert any(s["lshl"] == 0 and not s["send_hi"] for s in got), "lshl = 0 with the even plane"


def pairs(cases, geo):
    return {(geo[c][b]["rows_in_regs"], geo[c][b]["lanes_per_field"], b)
            for c in cases for b in BOUNDARIES}


def test_every_rows_lanes_pair_under_both_boundaries(geo):
    want = {(R, lpf, b) for R in bl.ROWS_LIST for lpf in bl.LPF_LIST for b in BOUNDARIES}
    assert len(want) == 2 * 28
    assert pairs(bl.CASES, geo) == want
    assert pairs(bl.UNTIL_CASES, geo) == want


def test_every_row_class_with_one_lane_and_with_several(geo):
    for cases in (bl.CASES, bl.UNTIL_CASES):
        for R in bl.ROWS_LIST:
            for cls, h in (("full", R), ("last_dead", R - 1), ("least", bl.least_h(R))):
                assert cls in bl.row_classes(h) and bl.rows_in_regs(h) == R
                lpfs = {geo[c]["global"]["lanes_per_field"] for c in cases if c.h == h}
                assert 1 in lpfs and len(lpfs - {1}) == len(bl.LPF_LIST) - 1, (R, cls, lpfs)
        for h in (2, 3):
            lpfs = {geo[c]["global"]["lanes_per_field"] for c in cases if c.h == h}
            assert lpfs == set(bl.LPF_LIST), h


def test_every_lane_class_occurs(geo):
    for lpf in bl.LPF_LIST:
        wqs = {bl.words(c.w) for c in bl.cases_of(lpf)}
        assert wqs == {wq for wq in bl.WQ if bl.lanes_per_field(64 * wq) == lpf}
        assert lpf in wqs
        if lpf >= 4:
            assert lpf // 2 + 1 in wqs and lpf - 1 in wqs
            assert "most_padding" in bl.lane_classes(lpf // 2 + 1)
            assert "one_padding" in bl.lane_classes(lpf - 1)
        assert bl.lane_classes(lpf) == {"full"}


def test_every_phase_with_every_lanes_per_field_with_and_without_padding(geo):
    for lpf in bl.LPF_LIST:
        for until in (False, True):
            cases = bl.cases_of(lpf, until)
            assert all(geo[c]["global"]["lanes_per_field"] == lpf for c in cases)
            assert {bl.phase(c.w) for c in cases} == set(bl.PHASES), (lpf, until)
        cases = bl.cases_of(lpf)
        padded = {bl.phase(c.w) for c in cases if bl.padding_lanes(c.w) > 0}
        exact = {bl.phase(c.w) for c in cases if bl.padding_lanes(c.w) == 0}
        assert exact == set(bl.PHASES), lpf
        assert padded == (set(bl.PHASES) if lpf >= 4 else set()), lpf
        # every (wq, phase) pair, at each of the four heights of part 2
        for h in bl.PART2_H:
            got = {(bl.words(c.w), bl.phase(c.w)) for c in cases if c.h == h}
            assert len(got) == len({bl.words(c.w) for c in cases}) * len(bl.PHASES), (lpf, h)


def test_field_counts(geo):
    for c in bl.CASES:
        g = geo[c]["global"]
        if g["fields_per_wave"] > 1:
            assert c.n % g["fields_per_wave"] != 0, c  # the last wavefront is partly filled
        assert c.n >= 3, c
    for lpf in bl.LPF_LIST:
        for cases in (bl.cases_of(lpf), bl.cases_of(lpf, until=True)):
            big = [c for c in cases if geo[c]["global"]["waves"] > bl.BATCH_WAVES]
            assert len(big) == 1 and (big[0].h, bl.words(big[0].w)) == bl.BIG[lpf]
            # a second workgroup, whose trailing wavefronts return at once
            assert geo[big[0]]["global"]["waves"] % bl.BATCH_WAVES != 0
    assert {bl.rows_in_regs(h) for h, _ in bl.BIG.values()} == set(bl.ROWS_LIST)


def test_rule_tables_put_flood_beside_the_empty_rule():
    for k, c in enumerate(bl.CASES):
        birth, survive = bl.rule_table(c, k)
        assert birth.shape == survive.shape == (c.n,)
        fpw = bl.fields_per_wave(c.w)
        if fpw >= 2:
            assert bl.flood_beside_empty(birth, survive, fpw), c
    # every rule of the list meets every lanes_per_field
    for lpf in bl.LPF_LIST:
        seen = set()
        for k, c in enumerate(bl.CASES):
            if bl.lanes_per_field(c.w) == lpf:
                birth, survive = bl.rule_table(c, k)
                seen |= set(zip(birth.tolist(), survive.tolist()))
        assert seen >= set(batch_rules_ref.MIXED), lpf
    assert not bl.flood_beside_empty(*batch_rules_ref.cycled(64), 64)


@pytest.mark.parametrize("h,w", [(1, 1), (3, 70), (7, 64), (9, 129), (5, 520)])
def test_codec_restatements_are_the_oracle_s(oracle, h, w):
    n, seed, first = 5, 1234567, 3
    got = bl.synthetic_fields(first, n, h, w, seed)
    live, hsh = bl.digests(got)
    assert got.dtype == live.dtype == hsh.dtype == np.uint64
    for i in range(n):
        want = oracle.bp_random(h, w, seed + first + i)
        assert (got[i] == want).all(), i
        assert (int(live[i]), int(hsh[i])) == oracle.bp_digest(want, w), i
    other = batch_ref.pack(batch_ref.random_batch(n, h, w, seed=5, p=.2))
    live, hsh = bl.digests(other)
    for i in range(n):
        assert (int(live[i]), int(hsh[i])) == oracle.bp_digest(other[i], w), i
    assert bl.last_mask(w) == np.uint64((1 << (w % 64)) - 1 if w % 64 else 2 ** 64 - 1)


@pytest.mark.parametrize("torus", [False, True], ids=["dead", "torus"])
def test_until_ref_rules_is_until_ref_field_by_field(torus):
    n, h, w, max_g, lag, every = 26, 7, 9, 12, 4, 5
    cells = batch_ref.random_batch(n, h, w, seed=3, p=.35)
    birth, survive = batch_rules_ref.cycled(n)
    period, generation, final = batch_until_ref.until_ref_rules(cells, max_g, lag, every, birth,
                                                                survive, torus)
    assert (period != 0).any() and (period == 0).any()
    for i in range(n):
        p, g, f = batch_until_ref.until_ref(cells[i:i + 1], max_g, lag, every,
                                            (int(birth[i]), int(survive[i])), torus)
        assert (period[i], generation[i]) == (p[0], g[0]), i
        assert (final[i] == f[0]).all(), i
    same = batch_until_ref.until_ref_rules(cells, max_g, lag, every, np.full(n, rule_ref.CONWAY[0]),
                                           np.full(n, rule_ref.CONWAY[1]), torus)
    want = batch_until_ref.until_ref(cells, max_g, lag, every, rule_ref.CONWAY, torus)
    assert all((a == b).all() for a, b in zip(same, want))
