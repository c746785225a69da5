"""The cases of tests/test_gpu_batch_lattice.py, and why each is there.

The batch kernels (life_batch.h batch_run, life_batch_until.h batch_until_run and their
RULE_LANE instantiations in life_batch_rules.h) share one lane setup, which branches on
a field's geometry (h, w) in three independent ways.  This module restates those
classes in Python and builds the list of (h, w, n) cases from them;
tests/test_batch_lattice_host.py checks on the CPU, against gol_batch_geometry, that the
list meets every class with every other, and reads the setup's expressions out of the
two headers so that whoever rewrites them has to come back here.

Rows.  rows_in_regs R is the least of 8, 16, 32, 64 that is >= h.  The pass of batch_pass
runs steps t = 1 .. R under `t <= h`; the classes of h within an R:
  full      h = R      step R is taken: `in` is the constant 0 (t == R), or `top` on a torus
  last_dead h = R - 1  the last register row is the dead row (read, never written)
  least     R / 2 + 1  (1 for R = 8) the most steps left out
and h = 2 and 3: on a torus the rows above and below a row coincide (h = 2) or are the
row itself (h = 1), the smallest field on which they differ has 3 rows.

Lanes.  lanes_per_field lpf is the least power of two >= wq = ceil(w / 64); a field's
lanes q >= wq are padding lanes (cm = 0, no loads, no stores).  lpf sets lpf_shift in
batch_word_index, the partner address 4 * (lane +- (wq - 1)) of the torus's
ds_bpermute, the lanes whose inner_l / inner_r are 0 and the until kernel's per-field
ballot mask fmask.  The classes of wq within an lpf:
  full          wq = lpf          no padding lane
  most_padding  wq = lpf / 2 + 1  the most padding lanes
  one_padding   wq = lpf - 1      one (where that is neither of the above)

Columns.  The phase p = w - 64 (wq - 1) in 1 .. 64, the columns of the last word, with
cl = (w - 1) % 64 the last column's bit and cg = w % 64 the ghost column's:
  p   cl  send_hi  lshl  cg  ghost column
  1    0  no       31     1  gm[1], bit 0
  2    1  yes      31     2  gm[0], bit 1
  33  32  no       15    33  gm[1], bit 16
  62  61  yes       1    62  gm[0], bit 31
  63  62  no        0    63  gm[1], bit 31   (lshl = 0 with the even plane)
  64  63  yes       0     0  none: wfull, column 0 is the right carry

The lattice.  Part 1: every h of H x every wq of WQ, the phase rotated through the six
by (i + j) % 6 (i, j the indices in H and WQ): 224 cases, the ones the period-detecting
families run.  Part 2: every (wq, phase) pair at h = 2, 16, 31, 64.  544 distinct (h, w).

n.  2 fields_per_wave + 1, at most 33: the last wavefront is partly filled wherever a
wavefront holds more than one field.  One case per lpf (BIG, in part 1) has 4 fields_per_wave + a
part: five wavefronts, i.e. a second workgroup (kBatchWaves = 4) whose wavefronts 1 to 3
return at `wave >= a.waves`.
"""
from collections import namedtuple

import numpy as np

import batch_rules_ref
import rule_ref

ROWS_LIST = (8, 16, 32, 64)      # kBatchRowsList
LPF_LIST = (1, 2, 4, 8, 16, 32, 64)
PHASES = (1, 2, 33, 62, 63, 64)
PART2_H = (2, 16, 31, 64)
BATCH_WAVES = 4                  # kBatchWaves

Case = namedtuple("Case", "h w n part")


# ---- the classes, restated

def words(w):
    return -(-w // 64)


def rows_in_regs(h):
    return min(r for r in ROWS_LIST if r >= h)


def lanes_per_field(w):
    lpf = 1
    while lpf < words(w):
        lpf *= 2
    return lpf


def fields_per_wave(w):
    return 64 // lanes_per_field(w)


def waves(n, w):
    return -(-n // fields_per_wave(w))


def least_h(R):
    return 1 if R == ROWS_LIST[0] else R // 2 + 1


def row_classes(h):
    """The classes h belongs to (a set of names; 'inner' alone if none)."""
    R = rows_in_regs(h)
    c = set()
    if h == R:
        c.add("full")
    if h == R - 1:
        c.add("last_dead")
    if h == least_h(R):
        c.add("least")
    if h in (2, 3):
        c.add("torus_small")
    return c or {"inner"}


def lane_classes(wq):
    lpf = lanes_per_field(64 * wq)
    c = set()
    if wq == lpf:
        c.add("full")
    if wq == lpf // 2 + 1 and wq < lpf:
        c.add("most_padding")
    if wq == lpf - 1 and wq > lpf // 2:
        c.add("one_padding")
    return c or {"inner"}


def padding_lanes(w):
    return lanes_per_field(w) - words(w)


def phase(w):
    return w - 64 * (words(w) - 1)


def lane_setup(w):
    """What batch_run's setup derives from w alone: cl, cg, send_hi, lshl, wfull and the
    ghost column's (plane, bit) or None."""
    cl, cg = (w - 1) & 63, w & 63
    ghost = None if cg == 0 else (cg & 1, cg >> 1)
    return {"cl": cl, "cg": cg, "send_hi": bool(cl & 1), "lshl": 31 - (cl >> 1),
            "wfull": cg == 0, "ghost": ghost}


def last_mask(w):
    """Canonical valid bits of word wq - 1."""
    return np.uint64((1 << phase(w)) - 1)


# ---- the case list

H = sorted({h for R in ROWS_LIST for h in (R, R - 1, least_h(R))} | {2, 3})
WQ = sorted({wq for lpf in LPF_LIST for wq in (lpf, lpf // 2 + 1, lpf - 1) if lpf // 2 < wq <= lpf})
# the five-wavefront case of each lanes_per_field: (h, wq), rows_in_regs spread over them,
# wq the one with the most padding lanes
BIG = {1: (9, 1), 2: (33, 2), 4: (7, 3), 8: (17, 5), 16: (64, 9), 32: (15, 17), 64: (31, 33)}


def width(wq, p):
    return 64 * (wq - 1) + p


def fields(h, w, part):
    fpw = fields_per_wave(w)
    if part == 1 and BIG[lanes_per_field(w)] == (h, words(w)):
        return BATCH_WAVES * fpw + max(1, fpw // 2)
    return min(2 * fpw + 1, 33)


def build():
    cases, seen = [], set()
    for i, h in enumerate(H):
        for j, wq in enumerate(WQ):
            w = width(wq, PHASES[(i + j) % len(PHASES)])
            seen.add((h, w))
            cases.append(Case(h, w, fields(h, w, 1), 1))
    for wq in WQ:
        for p in PHASES:
            for h in PART2_H:
                w = width(wq, p)
                if (h, w) not in seen:
                    seen.add((h, w))
                    cases.append(Case(h, w, fields(h, w, 2), 2))
    return cases


CASES = build()
UNTIL_CASES = [c for c in CASES if c.part == 1]


def cases_of(lpf, until=False):
    return [c for c in (UNTIL_CASES if until else CASES) if lanes_per_field(c.w) == lpf]


# ---- the rule table of the RULE_LANE families

EMPTY = (0, 0)


def rule_table(case, k):
    """(birth, survive) uint32 [n]: batch_rules_ref.MIXED rotated by k and cycled over the
    fields, then FLOOD and the empty rule planted on two neighbouring fields of wavefront
    0 (in either order, by k): a lane that steps by its neighbour field's word of the
    table floods an empty field or empties a full one."""
    M = batch_rules_ref.MIXED
    rot = M[k % len(M):] + M[:k % len(M)]
    birth, survive = batch_rules_ref.cycled(case.n, rot)
    room = min(case.n, fields_per_wave(case.w))
    if room >= 2:
        i = k % (room - 1)
        pair = (rule_ref.FLOOD, EMPTY) if k % 2 else (EMPTY, rule_ref.FLOOD)
        for d in (0, 1):
            birth[i + d], survive[i + d] = pair[d]
    return birth, survive


def flood_beside_empty(birth, survive, fpw):
    """True if FLOOD and the empty rule sit on neighbouring fields of one wavefront."""
    r = list(zip(birth.tolist(), survive.tolist()))
    return any({r[i], r[i + 1]} == {rule_ref.FLOOD, EMPTY} and i // fpw == (i + 1) // fpw
               for i in range(len(r) - 1))


# ---- the codec kernels' results, vectorised (life_batch_aux.hip; gol.h defines both on
# the canonical word index r * wq + q of a field)

_U = np.uint64


def splitmix64_at(seed, idx):
    """uint64 arrays (or scalars), wrapping arithmetic."""
    with np.errstate(over="ignore"):
        z = np.asarray(seed, dtype=_U) + (np.asarray(idx, dtype=_U) + _U(1)) * _U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
        return z ^ (z >> _U(31))


def synthetic_fields(first, count, h, w, seed):
    """uint64 [count, h, wq]: field first + i of BatchEngine.init_random(seed), i.e.
    gol_init_random's field of seed + first + i."""
    wq = words(w)
    seeds = (np.arange(count, dtype=_U) + _U(first) + _U(seed))[:, None]
    idx = np.arange(h * wq, dtype=_U)[None, :]
    g = splitmix64_at(seeds, idx).reshape(count, h, wq)
    g[:, :, -1] &= last_mask(w)
    return g


def digests(fields_):
    """(live, hash) uint64 [n] of packed fields [n, h, wq] (bits at columns >= w are 0)."""
    a = np.ascontiguousarray(fields_, dtype=_U)
    n, h, wq = a.shape
    live = np.unpackbits(a.view(np.uint8).reshape(n, -1), axis=1).sum(axis=1, dtype=_U)
    salt = splitmix64_at(_U(0), np.arange(h * wq, dtype=_U))[None, :]
    with np.errstate(over="ignore"):
        hsh = splitmix64_at(a.reshape(n, h * wq) ^ salt, _U(0)).sum(axis=1, dtype=_U)
    return live, hsh


# ---- the per-field ballot cases: one blinker among blocks, at every field position

BALLOT_H = 17
BALLOT_CALL = (8, 2, 4)  # max_generations, lag, check_every
GLIDER = [(0, 1), (1, 2), (2, 0), (2, 1), (2, 2)]
# where the blinker lies: in word 0, wholly in word wq - 1, across the seam of the last two
BLINKERS = ("first", "last", "seam")


def ballot_shapes(lpf):
    """(h, w) per lanes_per_field 2 .. 32: one without padding lanes, and from 4 on one
    with the most.  The phases (62, 33) leave room for a blinker inside the last word."""
    assert 2 <= lpf <= 32
    out = [(BALLOT_H, width(lpf, 62))]
    if lpf >= 4:
        out.append((BALLOT_H, width(lpf // 2 + 1, 33)))
    return out


def ballot_kinds(h, w):
    """name -> uint8 [h, w]: what a field of a ballot case holds."""
    c = 64 * (words(w) - 1)  # first column of the last word
    k = {name: np.zeros((h, w), dtype=np.uint8) for name in ("block", "glider") + BLINKERS}
    k["block"][4:6, 4:6] = 1
    for r, col in GLIDER:
        k["glider"][r + 1, col + 1] = 1
    k["first"][8, 1:4] = 1
    k["last"][8, c + 1:c + 4] = 1
    k["seam"][8, c - 1:c + 2] = 1
    return k


def ballot_layout(w, j):
    """The kinds of the n = fields_per_wave + 2 fields of the case whose blinker is field
    j of wavefront 0 (None at j): blocks, and one glider, which is not found; it lies half
    a wavefront from j, or in wavefront 1 where a wavefront holds two fields, so that no
    neighbour of j is unfound for a reason of its own."""
    fpw = fields_per_wave(w)
    n = fpw + 2
    glider = (j + fpw // 2) % fpw if fpw >= 4 else fpw
    return [None if i == j else "glider" if i == glider else "block" for i in range(n)]
