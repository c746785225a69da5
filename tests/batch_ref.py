"""What a batch does, for the batch tests (test_batch_host.py, test_gpu_batch.py).

A plain-numpy runner over [n, h, w] uint8 cells, independent of the library, of the
oracle and of the other references' code: a dead border by zero padding or a torus by
np.roll, the eight neighbours summed, the rule read off the two 9-bit masks, all n
fields at once and none touching another.  test_batch_host.py pins it field by field
to rule_ref.numpy_run (dead border) and torus_ref.roll_run (torus).
"""
import numpy as np

OFFSETS = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]


def neighbours(cells, torus):
    """Live neighbours of every cell of uint8 [n, h, w] cells."""
    n, h, w = cells.shape
    if torus:
        return sum(np.roll(cells, (dy, dx), axis=(1, 2)) for dy, dx in OFFSETS)
    p = np.zeros((n, h + 2, w + 2), dtype=cells.dtype)
    p[:, 1:-1, 1:-1] = cells
    return sum(p[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy, dx in OFFSETS)


def run(cells, gens, rule, torus=False):
    """uint8 [n, h, w] cells after `gens` generations of (birth, survive)."""
    birth, survive = rule
    born = np.array([(birth >> k) & 1 for k in range(9)], dtype=np.uint8)
    stays = np.array([(survive >> k) & 1 for k in range(9)], dtype=np.uint8)
    alive = np.asarray(cells).astype(np.uint8)
    for _ in range(gens):
        k = neighbours(alive, torus)
        alive = np.where(alive == 1, stays[k], born[k])
    return alive


def random_batch(n, h, w, seed, p=0.5):
    return (np.random.default_rng(seed).random((n, h, w)) < p).astype(np.uint8)


def pack(cells):
    """uint8 [n, h, w] cells -> uint64 [n, h, ceil(w/64)] canonical packed words."""
    n, h, w = cells.shape
    wq = (w + 63) // 64
    b = np.zeros((n, h, wq * 64), dtype=np.uint8)
    b[:, :, :w] = cells
    return np.packbits(b.reshape(n, h, wq, 64), axis=3, bitorder="little").view(np.uint64).reshape(n, h, wq)


def unpack(words, w):
    """uint64 [n, h, >= ceil(w/64)] packed words -> uint8 [n, h, w] cells."""
    a = np.ascontiguousarray(words, dtype=np.uint64)
    n, h = a.shape[:2]
    return np.unpackbits(a.view(np.uint8).reshape(n, h, -1), axis=2, bitorder="little")[:, :, :w].copy()
