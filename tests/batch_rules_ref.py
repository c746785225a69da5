"""What a batch with per-field rules does, for its tests (test_batch_rules_host.py,
test_gpu_batch_rules.py).

A plain-numpy runner over [n, h, w] uint8 cells like batch_ref.run, with a rule per field:
birth and survive are arrays [n] of 9-bit masks, spread to per-field 9-entry tables that
np.take_along_axis reads at every cell's neighbour count (batch_ref.neighbours).
test_batch_rules_host.py pins it field by field to batch_ref.run.
"""
import numpy as np

import batch_ref
import rule_ref

B36S23 = (0b1001000, 0b1100)
B0 = (1, 0)
# the rule list of the mixed-rule tests: field i takes rule i mod len(MIXED)
MIXED = rule_ref.ONE_BIT + [rule_ref.REF_RULE, rule_ref.CONWAY, rule_ref.FLOOD, B0,
                            (0x1FF, 0x1FF), (0, 0)]


def tables(masks):
    """uint8 [n, 9]: bit k of masks[i] at [i, k]."""
    m = np.asarray(masks, dtype=np.uint32)
    return ((m[:, None] >> np.arange(9, dtype=np.uint32)[None, :]) & 1).astype(np.uint8)


def run(cells, gens, birth, survive, torus=False):
    """uint8 [n, h, w] cells after `gens` generations, field i under (birth[i], survive[i])."""
    alive = np.asarray(cells).astype(np.uint8)
    n, h, w = alive.shape
    born, stays = tables(birth), tables(survive)
    assert born.shape == (n, 9) and stays.shape == (n, 9)
    for _ in range(gens):
        k = batch_ref.neighbours(alive, torus).reshape(n, h * w).astype(np.int64)
        b = np.take_along_axis(born, k, axis=1)
        s = np.take_along_axis(stays, k, axis=1)
        alive = np.where(alive.reshape(n, h * w) == 1, s, b).reshape(n, h, w)
    return alive


def cycled(n, rules=MIXED):
    """(birth, survive) uint32 [n]: field i takes rules[i mod len(rules)]."""
    r = np.array([rules[i % len(rules)] for i in range(n)], dtype=np.uint32).reshape(n, 2)
    return r[:, 0].copy(), r[:, 1].copy()


def random_rules(n, seed):
    """(birth, survive) uint32 [n], seeded random 9-bit masks."""
    r = np.random.default_rng(seed).integers(0, 512, size=(2, n), dtype=np.uint32)
    return r[0].copy(), r[1].copy()
