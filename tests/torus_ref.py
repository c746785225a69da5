"""What a torus does, for the torus tests (test_torus_host.py, test_gpu_torus*.py).

Two independent references on packed uint64 fields (bit j of word q = column 64q+j):

  torus_run   the recipe: for g generations pad the field by g wrapped cells on
              every side in numpy, run the oracle's dead-border bp_run for g
              generations and crop.  The dead border's error moves one cell per
              generation, so it ends exactly at the crop.  Fast (the oracle is
              bit-packed and threaded); what the GPU tests compare against.
  roll_run    plain numpy: neighbour counts by np.roll, one generation at a time.
              Slow; checks the recipe and the small GPU cases.
"""
import numpy as np


def pack(bits):
    """uint8 [h, w] cells -> uint64 [h, ceil(w/64)] packed words."""
    h, w = bits.shape
    wq = (w + 63) // 64
    b = np.zeros((h, wq * 64), dtype=np.uint8)
    b[:, :w] = bits
    return np.packbits(b.reshape(h, wq, 64), axis=2, bitorder="little").view(np.uint64).reshape(h, wq)


def unpack(words, w):
    """uint64 [h, >= ceil(w/64)] packed words -> uint8 [h, w] cells."""
    a = np.ascontiguousarray(words, dtype=np.uint64)
    h = a.shape[0]
    return np.unpackbits(a.view(np.uint8).reshape(h, -1), axis=1, bitorder="little")[:, :w].copy()


def wrap_pad(bits, gy, gx_left, gx_right=None):
    """Cells [h, w] -> [h + 2 gy, gx_left + w + gx_right], each taken from
    (y mod h, x mod w)."""
    h, w = bits.shape
    gx_right = gx_left if gx_right is None else gx_right
    ys = np.arange(-gy, h + gy) % h
    xs = np.arange(-gx_left, w + gx_right) % w
    return bits[np.ix_(ys, xs)]


def torus_run(oracle, words, w, gens, rule, chunk=None):
    """The recipe, `chunk` generations at a time (default: all at once)."""
    bits = unpack(words, w)
    h = bits.shape[0]
    left = gens
    while left > 0:
        g = min(left, chunk or left)
        padded = oracle.bp_run(pack(wrap_pad(bits, g, g)), w + 2 * g, g, rule)
        bits = unpack(padded, w + 2 * g)[g:g + h, g:g + w]
        left -= g
    return pack(bits)


def roll_run(words, w, gens, rule):
    """np.roll torus, one generation at a time."""
    bits = unpack(words, w).astype(np.int32)
    birth, survive = rule
    for _ in range(gens):
        n = sum(np.roll(np.roll(bits, dy, 0), dx, 1)
                for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))
        born = ((birth >> n) & 1) & (1 - bits)
        stay = ((survive >> n) & 1) & bits
        bits = (born | stay).astype(np.int32)
    return pack(bits.astype(np.uint8))
