"""The cases of tests/test_gpu_aux_scale.py, and why each is large enough.

The auxiliary kernels (region I/O, density, ASCII codec, torus wrap in life_aux.hip,
the snapshot compare in life_snap.hip, the batch codec in life_batch_aux.hip: cases 8 and
9) walk their work items with a grid-stride loop
over a capped grid: trip t of the loop handles the items [t C, (t + 1) C) with C the
number of threads (or wavefronts) the capped grid holds.  A case belongs here if its
item count is above C, so that the loop's increment runs, or if it stages more bytes
than engine.cpp's rect_stage keeps between calls.

This module holds the shapes, the cells the GPU test plants, and the kernels' own
item-count formulas restated in Python; tests/test_aux_caps.py reads the caps out of
the sources and checks every claim made here on the CPU.  All engines are 2-plane
(lane groups of one 64-column word), the shipped build.
"""
from types import SimpleNamespace as NS

import numpy as np

PLANES = 2
GROUP_COLS = 32 * PLANES  # columns of a lane group


def cdiv(a, b):
    return -(-a // b)


# ---- work items per launch: the formulas of the launchers and of leaf_read /
# leaf_write / leaf_density (one launch per non-wrapping piece of a leaf's region)

def rect_read_items(rows, cols):
    """launch_rect_read: one thread per word of the compact window."""
    return rows * cdiv(cols, 64)


def rect_write_items(x, rows, cols):
    """launch_rect_write: one thread per lane group that holds a column of the piece."""
    return rows * ((x + cols - 1) // GROUP_COLS - x // GROUP_COLS + 1)


def density_items(x, cols, wrow0, rows, by):
    """launch_density: (work items, column chunks of 64 lane groups); one wavefront per
    item = up to 32 rows of one block row x one chunk."""
    rpi = min(by, 32)
    nchunk = ((x + cols - 1) // GROUP_COLS - x // GROUP_COLS + 64) // 64
    nbr = (wrow0 + rows - 1) // by - wrow0 // by + 1
    return nbr * cdiv(by, rpi) * nchunk, nchunk


def ascii_items(rows, w):
    """launch_ascii_pack / _unpack: one wavefront per (row, lane group)."""
    return rows * cdiv(cdiv(w, 64), PLANES // 2)


def ascii_item_of(row, group, w):
    return row * cdiv(cdiv(w, 64), PLANES // 2) + group


def torus_wrap_items(h, w, ghost_rows, ghost_words):
    """launch_torus_wrap: (items, those of the 2 G ghost rows); the interior rows' side
    words follow the ghost rows'."""
    wq_pad = (w + 128 * ghost_words + 63) // 64
    ghost = 2 * ghost_rows * wq_pad
    return ghost + h * (wq_pad - (w >> 6)), ghost


def snap_tiles(rows, nwords, tile_rows, tile_words):
    """launch_snap_compare: tiles of a leaf's view (rows x nwords stored words)."""
    return cdiv(rows, tile_rows) * cdiv(nwords, tile_words)


def snap_tile_of(row, col, nwords, tile_rows, tile_words):
    """The tile that holds cell (row, col) of the view: column segments fastest."""
    return (row // tile_rows) * cdiv(nwords, tile_words) + (col // 64) // tile_words


def stage_bytes_rect(rows, cols):
    """leaf_read / leaf_write: the compact window of one cut."""
    return rows * cdiv(cols, 64) * 8


def stage_bytes_density(rh, rw, by, bx):
    """leaf_density: one uint32 per block."""
    return cdiv(rh, by) * cdiv(rw, bx) * 4


def torus_pieces(h, w, y, x, rh, rw):
    """torus.cpp torus_pieces: the non-wrapping pieces (field row, field column, rows,
    columns, window row, window column) of a window that may cross the seams."""
    h0, w0 = min(rh, h - y), min(rw, w - x)
    return [(r0, c0, rn, cn, wr, wc)
            for r0, rn, wr in ((y, h0, 0), (0, rh - h0, h0))
            for c0, cn, wc in ((x, w0, 0), (0, rw - w0, w0)) if rn and cn]


def pieces(torus, h, w, y, x, rh, rw):
    return torus_pieces(h, w, y, x, rh, rw) if torus else [(y, x, rh, rw, 0, 0)]


# ---- packed-word references for windows too large to unpack (case 4): bit j of word
# q of a row = column 64 q + j

def packed_window(words, y, x, rh, rw):
    """The rh x rw window at (y, x) of a packed field as packed words: a shift-and-or of
    neighbouring words, the last word masked to rw columns."""
    ww, q0, s = cdiv(rw, 64), x // 64, x % 64
    out = words[y:y + rh, q0:q0 + ww].copy()
    if s:
        nxt = words[y:y + rh, q0 + 1:q0 + ww + 1]
        out >>= np.uint64(s)
        out[:, :nxt.shape[1]] |= nxt << np.uint64(64 - s)
    if rw % 64:
        out[:, -1] &= np.uint64((1 << (rw % 64)) - 1)
    return out


def placed_window(win, x, rw, wq):
    """The packed window `win` (its bits beyond rw ignored) as rows of wq field words
    with the window's column 0 at field column x, zero elsewhere."""
    ww, q0, s = cdiv(rw, 64), x // 64, x % 64
    a = np.ascontiguousarray(win[:, :ww], dtype=np.uint64).copy()
    if rw % 64:
        a[:, -1] &= np.uint64((1 << (rw % 64)) - 1)
    out = np.zeros((a.shape[0], wq), dtype=np.uint64)
    out[:, q0:q0 + ww] = a << np.uint64(s)
    if s:
        n = min(ww, wq - q0 - 1)
        out[:, q0 + 1:q0 + 1 + n] |= a[:, :n] >> np.uint64(64 - s)
    return out


# ---- the cases

# Case 1: snapshot compare on one leaf.  65 words per row = 2 tile columns, 6,151 tile
# rows (the last of 3 rows), 12,302 tiles: the diff kernel's 8,192 wavefronts take a
# second trip for the tiles from 8,192 on, i.e. for the rows from 32,768 on.  The
# default engine: at h >= 32768 gol_create chooses between one stream and two stripes
# from the device's plan, and on an MI355X this shape runs on one stream (the GPU test
# asserts it; two stripes of 24,60x rows would hold 6,152 tiles each and stay under
# the cap, and case 7 is the composite engine).
SNAP = NS(
    h=49203, w=4160, kw=dict(),
    # (tile, cell): both column segments; the second is the row's last word (columns
    # 4,096-4,159), the one the compare masks
    flips=[(0, (3, 17)), (8191, (32767, 4159)), (8192, (32768, 0)), (8193, (32768, 4096)),
           (12299, (49199, 4130)), (12300, (49200, 4095)), (12301, (49202, 4159))],
    second_trip_window=(40000, 1000, 300, 3100),  # crosses the tile columns' border
)

# Case 2: rectangle read and write, and case 3: density on the same fields.  The
# window has 8,200 x 257 = 2,107,400 words and lane groups; the torus window crosses
# both seams and its large piece has 8,295 x 258.
RECT = NS(
    h=8300, w=16500,
    kinds={"default": dict(), "torus": dict(semantics=2)},
    window=(37, 31, 8200, 16400),
    torus_window=(8300 - 5, 16500 - 37, 8300, 16500),
    # density blocks (by, bx) -> what the block is here for
    blocks={
        (1, 5000): "8,200 x 5 chunk items: a second trip, blocks that span chunks",
        (8, 8): "the joined path with atomics, in every chunk",
        (64, 64): "one key per lane over all 64 lanes",
        (37, 4100): "runs of equal keys that cross a wavefront's end",
        (40, 4096): "with x = 31 every block edge falls inside a lane group",
        (8200, 16400): "one block added up from thousands of wavefronts",
    },
    second_trip_block=(1, 5000),
    seam_block=(37, 4100),
)

# Case 4: transient staging.  The window's compact form has 363 x 23,200 words =
# 67,372,800 bytes and the 4,100 x 4,100 counts 67,240,000, both above 64 MiB.
STAGE = NS(
    h=23300, w=23300,
    window=(3, 31, 23200, 23200),
    density=(0, 0, 4100, 4100, 1, 1),
    small=(1, 1, 5, 70),
)

# Case 5: ASCII codec.  1,100 x 65 = 71,500 items; row 1,050's line end is checked by
# item 68,314, and the rows from 1,009 on are packed wholly in the second trip.
ASCII = NS(h=1100, w=4100, kw=dict(streams=1), bad_row=1050, ones_from=1009)

# Case 6: torus wrap.  2 x 256 x 4,104 ghost-row words + 64 x 9 side words =
# 2,101,824: the second trip holds the tail of the bottom ghost rows and every left
# and right ghost word of the interior rows.  The snapshot compare of this engine sees
# 64 rows x 4,096 words = 8 x 64 tiles, far below the diff kernel's cap: it checks the
# torus view (word offset tGx), not a second trip.
WRAP = NS(h=64, w=262100, kw=dict(semantics=2, halo_depth=256), ghost_rows=256, ghost_words=4,
          corner=(60, 262090, 8, 20))

# Case 7: composite engine, two stripes of case 1's rows each.
COMPOSITE = NS(h=98403, w=4160, kw=dict(streams=2))


def composite_flips(h, w, row_starts, tile_rows=8, tile_words=64):
    """Case 7's cells as (leaf, tile of the leaf, (y, x)): just above and just below
    every stripe boundary, and in each leaf's second trip (leaf row >= 32,768), in both
    tile columns.  row_starts: the stripes' first rows."""
    ends = list(row_starts[1:]) + [h]
    out = []
    for leaf, (r0, r1) in enumerate(zip(row_starts, ends)):
        cells = [(r0, 63), (r1 - 1, w - 1), (r0 + 32768, 64), (r0 + 40001, w - 2), (r1 - 1, 0)]
        for y, x in cells:
            out.append((leaf, snap_tile_of(y - r0, x, cdiv(w, 64), tile_rows, tile_words), (y, x)))
    return out


# ---- the batch codec kernels (life_batch_aux.hip): items per launch

def batch_codec_items(count, h, w):
    """launch_batch_load / _store / _init_random: one thread per canonical word of the
    fields of the call."""
    return count * h * cdiv(w, 64)


def batch_digest_items(count):
    """launch_batch_digest: one wavefront per field."""
    return count


def batch_field_of_word(k, h, w):
    """(field, row, word) of canonical word k of a batch."""
    per = h * cdiv(w, 64)
    return k // per, (k % per) // cdiv(w, 64), k % cdiv(w, 64)


# Case 8: batch load, store and init_random.  4,100 x 64 x 9 = 2,361,600 words, 18.9 MB;
# 9 words per row in 16 lanes per field, so 7 padding lanes per field and 4 fields per
# wavefront.  Word 2,097,152, the second trip's first, is word 8 of row 56 of field 3,640.
# `sub`: a store_packed(first, count) of one trip (1,100 x 576 = 633,600 words) that reads
# fields on both sides of field 3,640; `sub_trip`: one of more than a trip's words
# (3,700 x 576 = 2,131,200), which starts in its first trip and ends in its second.
BATCH_CODEC = NS(n=4100, h=64, w=520, seed=61, gens=3, boundary=(3639, 3640, 3641),
                 sub=(3000, 1100), sub_trip=(200, 3700), sampled_others=32)

# Case 9: batch digest.  33,000 fields of 3 x 70 (2 words per row, 2 lanes per field),
# one wavefront each: the fields from 32,768 on are the second trip's.
BATCH_DIGEST = NS(n=33000, h=3, w=70, seed=62, sub=(32000, 1000))

# The largest batch of the suite before these cases (test_gpu_batch_rules.py
# test_every_rule_pair_once): exactly one trip of words.
RULE_PAIRS = NS(n=262144, h=8, w=8)
