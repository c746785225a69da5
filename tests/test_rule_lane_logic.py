"""The per-lane rule network (RULE_LANE, life_rule_lane.h), checked exhaustively on the CPU.

rule32_lane computes a cell's next state from the 9-cell total T = H3(r-2) + H3(r-1) +
H3(r) and the lane's own masks with a multiplexer tree of v_bitop3.  This test reads the
immediates from the header and evaluates the network bit by bit for every triple of H3
sums and both values of `alive` (an alive cell is part of its row's H3, so alive with a
middle H3 of 0 cannot occur), under one-bit, empty, full, named and random rules: the
result must be bit n of the mask that `alive` selects, n = T - alive.
"""
import itertools
import os
import re

import numpy as np
import pytest

import rule_ref
from test_stage_logic import bitop3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpi-game-of-life_amd", "csrc")
LANE_NAMES = ["kLaneT2", "kLaneT3", "kLaneLeaf", "kLaneSel0", "kLaneSel1", "kLaneSel2", "kLaneSel3"]


def luts(name):
    src = open(os.path.join(CSRC, name)).read()
    return {m.group(1): int(m.group(2), 16)
            for m in re.finditer(r"constexpr uint32_t (k\w+) = 0x([0-9A-Fa-f]+);", src)}


def rules():
    rng = np.random.default_rng(950)
    rand = [tuple(int(v) for v in rng.integers(0, 512, size=2)) for _ in range(200)]
    return (rule_ref.ONE_BIT + [(0, 0), (0x1FF, 0x1FF), rule_ref.REF_RULE, rule_ref.CONWAY] + rand)


def network(L, S, a, b, e, alive, birth, survive):
    """rule32_lane on one bit: a, b, e = (sum, carry) of H3(r-2), H3(r-1), H3(r)."""
    s0 = bitop3(S["kXor3"], a[0], b[0], e[0])
    k0 = bitop3(S["kMaj"], a[0], b[0], e[0])
    p = bitop3(S["kXor3"], a[1], b[1], e[1])
    mj = bitop3(S["kMaj"], a[1], b[1], e[1])
    x = p ^ k0
    t2 = bitop3(L["kLaneT2"], p, k0, mj)
    t3 = bitop3(L["kLaneT3"], p, k0, mj)
    B = [(birth >> k) & 1 for k in range(9)]
    Sv = [(survive >> k) & 1 for k in range(9)]
    B = B + [0]
    leaf = [B[0]] + [bitop3(L["kLaneLeaf"], alive, Sv[v - 1], B[v]) for v in range(1, 10)]
    m = [bitop3(L["kLaneSel0"], s0, leaf[2 * j + 1], leaf[2 * j]) for j in range(5)]
    lo = bitop3(L["kLaneSel1"], x, m[1], m[0])
    hi = bitop3(L["kLaneSel1"], x, m[3], m[2])
    low8 = bitop3(L["kLaneSel2"], t2, hi, lo)
    return bitop3(L["kLaneSel3"], t3, m[4], low8)


def test_header_names_its_immediates():
    L = luts("life_rule_lane.h")
    assert sorted(L) == sorted(LANE_NAMES)
    src = open(os.path.join(CSRC, "life_rule_lane.h")).read()
    for name in LANE_NAMES:
        assert "lop3<%s>" % name in src, name


def test_lane_network_matches_every_rule():
    L, S = luts("life_rule_lane.h"), luts("life_stencil.h")
    cases = 0
    all_rules = rules()
    assert len(all_rules) == 18 + 4 + 200
    for ha, hb, he in itertools.product(range(4), repeat=3):
        for alive in (0, 1):
            if alive and hb == 0:
                continue
            a, b, e = ((h & 1, h >> 1) for h in (ha, hb, he))
            T = ha + hb + he
            n = T - alive
            for birth, survive in all_rules:
                want = ((survive if alive else birth) >> n) & 1
                got = network(L, S, a, b, e, alive, birth, survive)
                assert got == want, (ha, hb, he, alive, rule_ref.rule_name((birth, survive)))
            cases += 1
    assert cases == 64 + 48


@pytest.mark.parametrize("v", range(10))
def test_every_total_selects_its_own_leaf(v):
    """With one-hot leaves the tree returns the leaf of T and no other."""
    L, S = luts("life_rule_lane.h"), luts("life_stencil.h")
    seen = 0
    for ha, hb, he in itertools.product(range(4), repeat=3):
        a, b, e = ((h & 1, h >> 1) for h in (ha, hb, he))
        T = ha + hb + he
        # dead cell: leaf_T = B(T), T <= 8; alive cell: leaf_T = S(T - 1), T >= 1
        if v <= 8:
            assert network(L, S, a, b, e, 0, 1 << v, 0) == int(T == v)
        if v >= 1 and hb > 0:
            assert network(L, S, a, b, e, 1, 0, 1 << (v - 1)) == int(T == v)
        seen += T == v
    assert seen > 0
