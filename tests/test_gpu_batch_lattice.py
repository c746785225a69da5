"""GPU suite: the batch kernels over every lane and row geometry -- the 544 (h, w, n)
cases of tests/batch_lattice.py through the four kernel families (uniform step,
RULE_LANE step, step_until_periodic with one rule and with a rule per field), every
field word for word against the plain-numpy references batch_ref, batch_rules_ref and
batch_until_ref, and the until kernel's per-field ballot with a blinker at every field
position of a wavefront.

Why each case is there, and the floors the list keeps, are in tests/batch_lattice.py and
tests/test_batch_lattice_host.py (CPU).  One test per (lanes_per_field, boundary,
family); cells and references are computed once per case.
"""
import numpy as np
import pytest

import batch_lattice as bl
import batch_ref
import batch_rules_ref
import batch_until_ref
import rule_ref
from batch_rules_ref import B0, B36S23
from test_gpu_batch_until import check_result

pytestmark = pytest.mark.gpu

CONWAY, REF_RULE = rule_ref.CONWAY, rule_ref.REF_RULE
# one rule per kernel kind: RULE_REF (the only one without the column mask on a dead
# border), RULE_CONWAY, RULE_GENERIC, and RULE_GENERIC with B0, which lights every cell
# that is not masked: a wrong cm or ghost bit shows at once
UNIFORM = [REF_RULE, CONWAY, B36S23, B0]
OTHER = (0b101010101, 0b010101010)  # the create rule of the batches that get a table
UNTIL_CALL = (12, 4, 5)             # max_generations, lag, check_every: checks at 5 and 10
FAMILIES = ("uniform", "lanes", "until", "until_lanes")
INDEX = {c: k for k, c in enumerate(bl.CASES)}


def sem_of(pkg, torus):
    return pkg.SEM_TORUS if torus else pkg.SEM_GLOBAL


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


_cells, _until_cells, _refs = {}, {}, {}


def start_cells(case):
    """The case's random start (p = 0.5) and its packed words, computed once."""
    if case not in _cells:
        cells = batch_ref.random_batch(case.n, case.h, case.w, seed=100000 * case.h + case.w)
        _cells[case] = frozen(cells, batch_ref.pack(cells))
    return _cells[case]


def until_cells(case):
    """Fields for the period-detecting families, by i % 3: a soup (p = 0.4), a sparse one
    (p = 0.05), and three cells in a row that end at the last column (a blinker where the
    field has room for one): found and unfound fields side by side."""
    if case not in _until_cells:
        n, h, w = case.n, case.h, case.w
        rng = np.random.default_rng(100000 * h + w + 1)
        cells = np.zeros((n, h, w), dtype=np.uint8)
        for i in range(n):
            if i % 3 == 2:
                cells[i, h // 2, max(0, w - 3):] = 1
            else:
                cells[i] = rng.random((h, w)) < (0.4 if i % 3 == 0 else 0.05)
        _until_cells[case] = frozen(cells)
    return _until_cells[case]


def reference(key, make):
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


def bad_fields(got, want_cells):
    return np.argwhere((got != batch_ref.pack(want_cells)).any(axis=(1, 2))).ravel()[:8].tolist()


def with_junk(case, clean, rng):
    """The packed fields with junk at every bit a load must ignore: columns >= w of the
    last word, and a spare word per row."""
    n, h, wq = clean.shape
    out = rng.integers(0, 1 << 64, size=(n, h, wq + 1), dtype=np.uint64)
    out[:, :, :wq] = clean
    out[:, :, wq - 1] |= rng.integers(0, 1 << 64, size=(n, h), dtype=np.uint64) & ~bl.last_mask(case.w)
    return out


def codec_checks(pkg, oracle, b, case):
    """init_random, store_packed and digest (whole and sub-range) on the case's geometry,
    sampled fields against the oracle, all of them against its vectorised restatement."""
    n, h, w = case.n, case.h, case.w
    seed = 7 + INDEX[case]
    b.init_random(seed)
    got = b.store_packed()
    live, hsh = b.digest()
    assert (got == bl.synthetic_fields(0, n, h, w, seed)).all(), case
    rlive, rhsh = bl.digests(got)
    assert live.tolist() == rlive.tolist() and hsh.tolist() == rhsh.tolist(), case
    for i in sorted({0, n - 1, min(n - 1, b.fields_per_wave // 2)}):
        want = oracle.bp_random(h, w, seed + i)
        assert (got[i] == want).all(), (case, i)
        assert (int(live[i]), int(hsh[i])) == oracle.bp_digest(want, w), (case, i)
    first, count = n // 3, n - n // 3 - 1
    part_live, part_hsh = b.digest(first, count)
    assert part_live.tolist() == live[first:first + count].tolist(), case
    assert part_hsh.tolist() == hsh[first:first + count].tolist(), case
    assert (b.store_packed(first, count) == got[first:first + count]).all(), case


def run_uniform(pkg, oracle, case, torus):
    cells, clean = start_cells(case)
    junk = with_junk(case, clean, np.random.default_rng(INDEX[case]))
    for rule in UNIFORM:
        ref1 = batch_ref.run(cells, 1, rule, torus)
        ref3 = batch_ref.run(ref1, 2, rule, torus)
        with pkg.BatchEngine(case.n, case.h, case.w, rule=rule, device=0,
                             semantics=sem_of(pkg, torus)) as b:
            assert (b.lanes_per_field, b.rows_in_regs) == (bl.lanes_per_field(case.w),
                                                           bl.rows_in_regs(case.h))
            if rule is REF_RULE:
                codec_checks(pkg, oracle, b, case)
            b.load_packed(junk)
            assert (b.store_packed() == clean).all(), (case, "load ignores, store masks")
            b.step(1)
            assert not bad_fields(b.store_packed(), ref1), (case, rule_ref.rule_name(rule), 1)
            b.step(2)
            assert not bad_fields(b.store_packed(), ref3), (case, rule_ref.rule_name(rule), 3)


def table_of(case):
    birth, survive = bl.rule_table(case, INDEX[case])
    fpw = bl.fields_per_wave(case.w)
    if fpw >= 2:  # (on the table, not on the GPU)
        assert bl.flood_beside_empty(birth, survive, fpw), case
    return birth, survive


def run_lanes(pkg, case, torus):
    cells, clean = start_cells(case)
    birth, survive = table_of(case)
    ref1 = batch_rules_ref.run(cells, 1, birth, survive, torus)
    ref3 = batch_rules_ref.run(ref1, 2, birth, survive, torus)
    with pkg.BatchEngine(case.n, case.h, case.w, rule=OTHER, device=0,
                         semantics=sem_of(pkg, torus)) as b:
        b.set_rules(birth, survive)
        b.load_packed(clean)
        for gens, ref in ((1, ref1), (2, ref3)):
            b.step(gens)
            bad = bad_fields(b.store_packed(), ref)
            assert not bad, (case, [(i, rule_ref.rule_name((birth[i], survive[i]))) for i in bad])


def run_until(pkg, case, torus, per_field):
    max_g, lag, every = UNTIL_CALL
    cells = until_cells(case)
    if per_field:
        birth, survive = table_of(case)
        ref = reference((case, torus, "until_lanes"), lambda: batch_until_ref.until_ref_rules(
            cells, max_g, lag, every, birth, survive, torus))
    else:
        ref = reference((case, torus, "until"), lambda: batch_until_ref.until_ref(
            cells, max_g, lag, every, CONWAY, torus))
    with pkg.BatchEngine(case.n, case.h, case.w, rule=OTHER if per_field else CONWAY, device=0,
                         semantics=sem_of(pkg, torus)) as b:
        if per_field:
            b.set_rules(birth, survive)
        b.load_packed(batch_ref.pack(cells))
        got = b.step_until_periodic(max_g, lag, every)
        try:
            check_result(pkg, b, got, b.store_packed(), ref, max_g, lag, every, case.w)
        except AssertionError as e:
            raise AssertionError(f"{case} torus={torus}: {e}") from e
    return ref[0]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("torus", [False, True], ids=["dead", "torus"])
@pytest.mark.parametrize("lpf", bl.LPF_LIST)
def test_lattice(pkg, oracle, lpf, torus, family):
    if family == "uniform":
        for case in bl.cases_of(lpf):
            run_uniform(pkg, oracle, case, torus)
    elif family == "lanes":
        for case in bl.cases_of(lpf):
            run_lanes(pkg, case, torus)
    else:
        periods = [run_until(pkg, case, torus, family == "until_lanes")
                   for case in bl.cases_of(lpf, until=True)]
        found = np.concatenate(periods)
        # on the reference alone: the sweep holds found and unfound fields
        assert (found == 0).any() and (found != 0).any()


@pytest.mark.parametrize("torus", [False, True], ids=["dead", "torus"])
@pytest.mark.parametrize("lpf", [2, 4, 8, 16, 32])
def test_per_field_ballot(pkg, lpf, torus):
    """A blinker in field j of a wavefront of blocks, for every j, in the field's first
    word, wholly in its last word and across the seam before it: period[j] is 2 and every
    other found period 1.  A ballot mask one field off or one field too wide gives a
    neighbour period 2; one that misses the field's first or last lane gives field j
    period 1.  One field holds a glider and is not found."""
    max_g, lag, every = bl.BALLOT_CALL
    for h, w in bl.ballot_shapes(lpf):
        kinds = bl.ballot_kinds(h, w)
        names = sorted(kinds)
        alone = batch_until_ref.until_ref(np.stack([kinds[k] for k in names]), max_g, lag, every,
                                          CONWAY, torus)
        per_kind = {k: (alone[0][i], alone[1][i], alone[2][i]) for i, k in enumerate(names)}
        # on the reference alone: what each kind of field is here for
        assert per_kind["block"][:2] == (1, every) and per_kind["glider"][:2] == (0, max_g)
        assert all(per_kind[k][:2] == (2, every) for k in bl.BLINKERS)
        fpw = bl.fields_per_wave(w)
        with pkg.BatchEngine(fpw + 2, h, w, rule=CONWAY, device=0, semantics=sem_of(pkg, torus)) as b:
            assert (b.lanes_per_field, b.fields_per_wave) == (lpf, fpw) and fpw >= 2
            for where in bl.BLINKERS:
                for j in range(fpw):
                    layout = [k or where for k in bl.ballot_layout(w, j)]
                    cells = np.stack([kinds[k] for k in layout])
                    ref = tuple(np.array([per_kind[k][part] for k in layout],
                                         dtype=alone[part].dtype) for part in range(3))
                    assert ref[0][j] == 2 and sorted(np.delete(ref[0], j).tolist()) == [0] + [1] * fpw
                    b.load_packed(batch_ref.pack(cells))
                    got = b.step_until_periodic(max_g, lag, every)
                    assert got.period.tolist() == ref[0].tolist(), (h, w, where, j)
                    check_result(pkg, b, got, b.store_packed(), ref, max_g, lag, every, w)
