"""CPU: the plain numpy reference (rule_ref.py) against the formulas of its builders,
the oracle against it for every mask bit, and the input conditions of the GPU tests
that use both (test_gpu_rule_bits.py, test_gpu_fronts.py import them from here, so
that none of their cases can pass on a field that never exercises its rule).
"""
import functools

import numpy as np
import pytest

import rule_ref as rr
from torus_ref import pack, roll_run, unpack

# ---- what test_gpu_rule_bits.py runs: its shapes, start fields and generation counts ---

SHAPES = {"130x200": (130, 200, 1), "40x4100": (40, 4100, 2)}  # h, w, default_rng seed
DEPTHS = [1, 8, 12, 16]
# every engine steps 1 generation, then depth + 3 more
GENS = sorted({1} | {1 + d + 3 for d in DEPTHS})
ALL_RULES = rr.ONE_BIT + rr.CONWAY_XOR
MIN_CENSUS = 20    # cells of each (alive, neighbour count) kind in a start field
# A floor, not a measured margin: enough cells that tell a CONWAY_XOR rule from B3/S23 at each
# later checked count for a wrong outcome of the flipped bit to show in many places (the fields
# here differ in 254 cells or more on 130 x 200 and 1878 or more on 40 x 4100; the tests print it)
MIN_DIFFER = 100


@functools.lru_cache(maxsize=None)
def start_cells(shape):
    h, w, seed = SHAPES[shape]
    cells = rr.random_cells(h, w, seed)
    cells.setflags(write=False)
    return cells


@functools.lru_cache(maxsize=None)
def reference(shape, rule):
    """{generations: packed field} of numpy_run from the shape's start field, at GENS."""
    cells, out, done = start_cells(shape), {}, 0
    for g in GENS:
        cells = rr.numpy_run(cells, g - done, rule)
        done = g
        out[g] = pack(cells)
        out[g].setflags(write=False)
    return out


def check_census(shape):
    """Every (alive, count 0..8) pair occurs in the start field, so that a wrong
    outcome for any one of them changes the first generation."""
    c = rr.census(start_cells(shape))
    assert c.min() >= MIN_CENSUS, c.tolist()
    return int(c.min())


def check_differs(shape, rule):
    """At every generation count checked, the rule's field is not B3/S23's: the
    flipped bit has mattered (and goes on mattering inside the fused steps)."""
    own, conway = reference(shape, rule), reference(shape, rr.CONWAY)
    h, w, _ = SHAPES[shape]
    n = [int((unpack(own[g], w) != unpack(conway[g], w)).sum()) for g in GENS]
    # after one generation: exactly the start field's cells of the flipped bit's kind
    db, ds = rule[0] ^ rr.CONWAY[0], rule[1] ^ rr.CONWAY[1]
    kind = rr.census(start_cells(shape))[1 if ds else 0, (db | ds).bit_length() - 1]
    assert GENS[0] == 1 and n[0] == kind >= MIN_CENSUS, (rr.rule_name(rule), n[0], kind)
    assert min(n[1:]) >= MIN_DIFFER, (rr.rule_name(rule), dict(zip(GENS, n)))
    return min(n[1:])


def test_rule_lists():
    assert len(set(rr.ONE_BIT)) == 18 and len(set(rr.CONWAY_XOR)) == 18
    assert all(bin(b).count("1") + bin(s).count("1") == 1 for b, s in rr.ONE_BIT)
    assert all(bin(b ^ rr.CONWAY[0]).count("1") + bin(s ^ rr.CONWAY[1]).count("1") == 1
               for b, s in rr.CONWAY_XOR)
    assert all(0 <= b < 512 and 0 <= s < 512 for b, s in ALL_RULES)
    assert rr.rule_name(rr.FLOOD) == "B12345678/S012345678"
    assert rr.rule_name(rr.EROSION) == "B/S8" and rr.rule_name(rr.CONWAY) == "B3/S23"


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_start_fields_hold_every_count(shape):
    print(shape, "least (alive, count) census", check_census(shape))


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_flipped_bits_show_at_every_checked_generation(shape):
    least = min(check_differs(shape, rule) for rule in rr.CONWAY_XOR)
    print(shape, "least number of cells that differ from B3/S23", least)


def test_numpy_run_known_answers():
    """numpy_run itself: blinker, block and glider under B3/S23, the B/S2 patterns of
    test_oracle.py, and the wrapped step of torus_ref.roll_run away from the border."""
    def cells(rows):
        return np.array([[c == "#" for c in r] for r in rows], dtype=np.uint8)
    blinker = cells([".....", ".....", ".###.", ".....", "....."])
    assert (rr.numpy_run(blinker, 1, rr.CONWAY) == blinker.T).all()
    assert (rr.numpy_run(blinker, 2, rr.CONWAY) == blinker).all()
    assert (rr.numpy_run(blinker, 1, rr.REF_RULE) ==
            cells([".....", ".....", "..#..", ".....", "....."])).all()
    block = cells(["....", ".##.", ".##.", "...."])
    assert (rr.numpy_run(block, 9, rr.CONWAY) == block).all()
    assert not rr.numpy_run(block, 1, rr.REF_RULE).any()
    g = np.zeros((12, 12), dtype=np.uint8)
    g[1:4, 1:4] = cells([".#.", "..#", "###"])
    assert (rr.numpy_run(g, 4, rr.CONWAY) == np.roll(np.roll(g, 1, 0), 1, 1)).all()
    # a field with an empty margin of more than `gens` cells evolves alike on a torus
    big = np.zeros((40, 50), dtype=np.uint8)
    big[10:30, 10:40] = rr.random_cells(20, 30, 4)
    for rule in (rr.CONWAY, (0b101010, 0b010101011)):
        assert (pack(rr.numpy_run(big, 9, rule)) == roll_run(pack(big), 50, 9, rule)).all()


# ---- the builders' formulas -------------------------------------------------------------

FORMULA_GENS = [1, 7, 16, 33]


def agree(field, after, w, rule, burn_out):
    """The formula equals numpy_run at FORMULA_GENS and, where the pattern dies in
    generation `burn_out`, there and one generation on."""
    for g in FORMULA_GENS + ([burn_out, burn_out + 1] if burn_out else []):
        want = rr.run_packed(field, w, g, rule)
        assert (after(g) == want).all(), (rr.rule_name(rule), g)
    if burn_out:
        assert after(burn_out - 1).any() and not after(burn_out).any()


@pytest.mark.parametrize("step", rr.ORIENTATIONS)
@pytest.mark.parametrize("rule", [rr.REF_RULE, rr.CONWAY], ids=rr.rule_name)
def test_fuse_formula(rule, step):
    if rule == rr.CONWAY and 0 in step:
        # horizontal and vertical lines give births under B3/S23: not a fuse
        field, after = rr.fuse(60, 90, 20, 20, 9, step)
        assert (after(1) != rr.run_packed(field, 90, 1, rule)).any()
        return
    h, w, L = 97, 131, 81
    r, c = (5, 120) if step == rr.ANTIDIAGONAL else (5, 7)
    field, after = rr.fuse(h, w, r, c, L, step)
    assert rr.unpack(field, w).sum() == L
    agree(field, after, w, rule, (L + 1) // 2)
    # an even length burns out too, one generation earlier than the odd one above
    field, after = rr.fuse(h, w, r, c, L - 1, step)
    agree(field, after, w, rule, (L - 1) // 2)


@pytest.mark.parametrize("rule", [rr.REF_RULE, rr.CONWAY], ids=rr.rule_name)
def test_fuse_corner_to_corner(rule):
    """Lines that touch the border at both ends: the two diagonals of a square field,
    and (B/S2) a full row and a full column."""
    n = 71
    for r, c, step in ((0, 0, rr.DIAGONAL), (0, n - 1, rr.ANTIDIAGONAL)):
        field, after = rr.fuse(n, n, r, c, n, step)
        agree(field, after, n, rule, (n + 1) // 2)
    if rule == rr.REF_RULE:
        for r, c, step in ((n - 1, 0, rr.HORIZONTAL), (0, 0, rr.VERTICAL), (0, n - 1, rr.VERTICAL)):
            field, after = rr.fuse(n, n, r, c, n, step)
            agree(field, after, n, rule, (n + 1) // 2)


@pytest.mark.parametrize("direction", [(1, 1), (1, -1), (-1, 1), (-1, -1), (0, 1), (0, -1),
                                       (1, 0), (-1, 0)])
def test_fuse_towards(direction):
    """The end that moves in `direction` reaches the target when the builder says."""
    h, w, tr, tc, start = 80, 90, 40, 45, 13
    field, after, n = rr.fuse_towards(h, w, tr, tc, direction, start)
    bit = lambda f: int(rr.unpack(f, w)[tr, tc])  # noqa: E731
    assert n > 2 * (start + 2) and bit(field) == 1
    assert bit(after(start)) == 1 and bit(after(start + 1)) == 0
    for g in (1, start, start + 1, 33):
        assert (after(g) == rr.run_packed(field, w, g, rr.REF_RULE)).all()
    assert rr.fuse_towards(h, w, tr, tc, direction, start, limit=30)[2] == 30


def test_flood_formula():
    h, w = 61, 150
    for r, c in ((30, 70), (0, 0), (60, 149), (3, 140)):
        field, after = rr.flood(h, w, r, c)
        agree(field, after, w, rr.FLOOD, None)
        full = max(r, h - 1 - r, c, w - 1 - c)
        assert rr.unpack(after(full), w).all() and not rr.unpack(after(full - 1), w).all()
        assert (after(full) == rr.run_packed(field, w, full, rr.FLOOD)).all()
    # in torus distance, against the wrapped numpy step
    field, after = rr.flood(h, w, 2, 145, torus=True)
    for g in (1, 7, 16, 33, 76):
        assert (after(g) == roll_run(field, w, g, rr.FLOOD)).all(), g
    assert rr.unpack(after(75), w).all() and not rr.unpack(after(74), w).all()


def test_erosion_formula():
    h, w = 70, 140
    holes = [(20, 21, 30, 31), (40, 47, 100, 103), (0, 2, 60, 61)]
    field, after = rr.eroded(h, w, holes)
    assert rr.unpack(field, w).sum() == h * w - 1 - 21 - 2
    agree(field, after, w, rr.EROSION, None)
    last = max(g for g in range(36) if after(g).any())
    for g in (last, last + 1, 36):
        assert (after(g) == rr.run_packed(field, w, g, rr.EROSION)).all(), g
    # no holes: the field dies from the border alone, in ceil(min(h, w) / 2) generations
    field, after = rr.eroded(h, w, [])
    agree(field, after, w, rr.EROSION, 35)
    assert after(34).any() and not after(35).any()


# ---- the oracle, for every bit -----------------------------------------------------------

ORACLE_SHAPES = [(37, 131), (64, 193)]
RANDOM_RULES = [tuple(int(x) for x in np.random.default_rng(400 + i).integers(0, 512, 2))
                for i in range(20)]
PINNED = ALL_RULES + [rr.FLOOD, rr.EROSION] + RANDOM_RULES


@pytest.mark.parametrize("rule", PINNED, ids=rr.rule_name)
def test_oracle_bitpacked_equals_numpy(oracle, rule):
    """bp_run, which every GPU test of a generic rule trusts, against numpy_run after
    12 generations and after each of the first three."""
    for i, (h, w) in enumerate(ORACLE_SHAPES):
        cells = rr.random_cells(h, w, 10 + i)
        g0 = pack(cells)
        for gens in (1, 2, 3, 12):
            got = oracle.bp_run(g0, w, gens, rule)
            assert (got == pack(rr.numpy_run(cells, gens, rule))).all(), (h, w, gens)


@pytest.mark.parametrize("rule", [rr.CONWAY_XOR[1], rr.CONWAY_XOR[4], rr.CONWAY_XOR[5],
                                  rr.CONWAY_XOR[9], rr.CONWAY_XOR[14], RANDOM_RULES[0]],
                         ids=rr.rule_name)
def test_oracle_ref_stripes_equals_numpy(oracle, rule):
    """bp_ref_stripes at P = 3: each rank's extended stripe (oracle.ref_stripe, pinned
    by test_oracle.py) evolves alone under numpy_run and keeps its own rows."""
    P, gens = 3, 12
    for i, (h, w) in enumerate(ORACLE_SHAPES):
        cells = rr.random_cells(h, w, 30 + i)
        want = np.zeros_like(cells)
        for r in range(P):
            s, n = oracle.ref_stripe(h, P, r)
            lo, hi = r * (h // P), h if r == P - 1 else (r + 1) * (h // P)
            want[lo:hi] = rr.numpy_run(cells[s:s + n], gens, rule)[lo - s:hi - s]
        assert (oracle.bp_ref_stripes(pack(cells), w, gens, P, rule) == pack(want)).all()
        # the stripes' dead seams show: this is not the whole field's evolution
        assert (pack(want) != pack(rr.numpy_run(cells, gens, rule))).any()
