"""A third reference, in plain integer numpy, and fields whose future is a formula
(test_rule_ref_host.py, test_gpu_rule_bits.py, test_gpu_fronts.py).

numpy_run is independent of the oracle (oracle/gol_oracle.c) and of
torus_ref.roll_run: a dead border by zero padding, the eight shifted slices
summed, the rule read off the two 9-bit masks.  Only pack / unpack are shared.

The rule lists name every mask bit on its own (ONE_BIT) and inside a rule that
stays active for many generations (CONWAY_XOR), so that the generic kernels see
every neighbour count with every outcome.

The builders give fields with an exact signal of speed 1 -- one cell per
generation, the fastest anything moves under a radius-1 rule, and the speed the
activity skip's dilation is argued from:

  fuse     a one-cell-wide line.  Under B/S2 (any of the 4 orientations) and under
           B3/S23 (the 2 diagonal ones) its interior is still and nothing is born
           beside it; its end cells die, one per generation and end: after g
           generations the cells with index in [g, L - g) are left.
  flood    B12345678/S012345678: one cell grows into the Chebyshev ball of radius
           g, clipped to the field (on a torus: the ball in torus distance).
  erosion  B/S8: a full field with rectangular holes keeps the cells further than
           g cells from the border and from every hole.
"""
import numpy as np

from torus_ref import pack, unpack

REF_RULE = (0, 1 << 2)                          # B/S2
CONWAY = (1 << 3, (1 << 2) | (1 << 3))          # B3/S23
FLOOD = (0x1FE, 0x1FF)                          # B12345678/S012345678
EROSION = (0, 1 << 8)                           # B/S8

# the 18 rules with exactly one mask bit set: B0/S ... B8/S, B/S0 ... B/S8
ONE_BIT = [(1 << n, 0) for n in range(9)] + [(0, 1 << n) for n in range(9)]
# B3/S23 with one of its 18 bits flipped
CONWAY_XOR = ([(CONWAY[0] ^ (1 << n), CONWAY[1]) for n in range(9)] +
              [(CONWAY[0], CONWAY[1] ^ (1 << n)) for n in range(9)])


def rule_name(rule):
    b, s = rule
    return ("B" + "".join(str(n) for n in range(9) if b >> n & 1) +
            "/S" + "".join(str(n) for n in range(9) if s >> n & 1))


def counts(bits):
    """Live neighbours of every cell of uint8 / int [h, w] cells, dead beyond the border."""
    h, w = bits.shape
    p = np.zeros((h + 2, w + 2), dtype=np.int64)
    p[1:-1, 1:-1] = bits
    return (p[:-2, :-2] + p[:-2, 1:-1] + p[:-2, 2:] + p[1:-1, :-2] + p[1:-1, 2:] +
            p[2:, :-2] + p[2:, 1:-1] + p[2:, 2:])


def numpy_run(bits, gens, rule):
    """uint8 [h, w] cells after `gens` generations of (birth, survive), dead border."""
    birth, survive = rule
    alive = np.asarray(bits).astype(np.int64)
    for _ in range(gens):
        n = counts(alive)
        alive = (((birth >> n) & 1) & ~alive | ((survive >> n) & 1) & alive) & 1
    return alive.astype(np.uint8)


def run_packed(words, w, gens, rule):
    """numpy_run on a packed uint64 field of w columns."""
    return pack(numpy_run(unpack(words, w), gens, rule))


def random_cells(h, w, seed, p=0.5):
    return (np.random.default_rng(seed).random((h, w)) < p).astype(np.uint8)


def census(bits):
    """[2, 9] array: how many dead / alive cells have 0..8 live neighbours."""
    n = counts(bits)
    out = np.zeros((2, 9), dtype=np.int64)
    for a in (0, 1):
        out[a] = np.bincount(n[np.asarray(bits) == a], minlength=9)
    return out


# ---- fields whose future is a formula -------------------------------------------------

# a fuse's orientation: the step from cell i to cell i + 1
HORIZONTAL, VERTICAL, DIAGONAL, ANTIDIAGONAL = (0, 1), (1, 0), (1, 1), (1, -1)
ORIENTATIONS = [HORIZONTAL, VERTICAL, DIAGONAL, ANTIDIAGONAL]


def _set(h, w, rows, cols):
    g = np.zeros((h, (w + 63) // 64), dtype=np.uint64)
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    assert ((rows >= 0) & (rows < h) & (cols >= 0) & (cols < w)).all()
    np.bitwise_or.at(g, (rows, cols // 64), np.uint64(1) << (cols % 64).astype(np.uint64))
    return g


def fuse(h, w, r, c, length, step):
    """A line of `length` cells from (r, c), cell i at (r, c) + i * step.  Returns
    (field, after): the packed field and after(g), the packed field g generations
    on under B/S2 (any step) or B3/S23 (diagonal steps): cells [g, length - g)."""
    dr, dc = step
    i = np.arange(length)

    def after(g):
        k = i[g:max(g, length - g)]
        return _set(h, w, r + k * dr, c + k * dc)
    return after(0), after


def fuse_towards(h, w, tr, tc, direction, start, limit=None):
    """A fuse whose burning end moves in `direction` (dr, dc; it may point up or
    left) and stands `start` cells before (tr, tc) at generation 0, so that cell
    (tr, tc) dies in generation start + 1.  The line runs on past (tr, tc) to the
    border, or for `limit` cells.  Returns (field, after, length)."""
    dr, dc = direction
    r, c = tr - start * dr, tc - start * dc
    n = limit or max(h, w)
    for d, x, m in ((dr, r, h), (dc, c, w)):
        if d > 0:
            n = min(n, m - x)
        elif d < 0:
            n = min(n, x + 1)
    assert n > 0, "the fuse starts outside the field"
    field, after = fuse(h, w, r, c, n, direction)
    return field, after, n


def flood(h, w, r, c, torus=False):
    """One cell at (r, c).  Returns (field, after): after(g) is the Chebyshev ball
    of radius g about it, clipped to the field, or in torus distance."""
    def after(g):
        dy, dx = np.abs(np.arange(h) - r), np.abs(np.arange(w) - c)
        if torus:
            dy, dx = np.minimum(dy, h - dy), np.minimum(dx, w - dx)
        return pack(((dy[:, None] <= g) & (dx[None, :] <= g)).astype(np.uint8))
    return after(0), after


def eroded(h, w, holes):
    """A full field but for `holes`, rectangles (r0, r1, c0, c1) of dead cells
    [r0, r1) x [c0, c1).  Returns (field, after): under B/S8 a cell lasts g
    generations when no dead cell -- hole or beyond the border -- is within g."""
    def after(g):
        a = np.zeros((h, w), dtype=np.uint8)
        if 2 * g < h and 2 * g < w:
            a[g:h - g, g:w - g] = 1
        for r0, r1, c0, c1 in holes:
            a[max(r0 - g, 0):r1 + g, max(c0 - g, 0):c1 + g] = 0
        return pack(a)
    return after(0), after
