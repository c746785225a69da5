"""GPU suite: per-field rules of a batch (BatchEngine.set_rules, gol_batch_set_rules) --
every field of every case, word for word, against batch_rules_ref's plain numpy, which
test_batch_rules_host.py pins to batch_ref.run."""
import ctypes

import numpy as np
import pytest

import batch_ref
import batch_rules_ref
import batch_until_ref
import rule_ref
from batch_rules_ref import B0, B36S23, MIXED
from test_gpu_batch_until import check_result

pytestmark = pytest.mark.gpu

GENS = (1, 2, 3, 37)
SHAPES = [(64, 64, 130), (5, 7, 3), (8, 64, 65), (9, 65, 33), (17, 130, 17), (33, 200, 5),
          (64, 4096, 2), (16, 16, 300), (1, 1, 2), (2, 2, 2)]
OTHER = (0b101010101, 0b010101010)  # a create rule that none of the tests' tables holds


def sem_of(pkg, torus):
    return pkg.SEM_TORUS if torus else pkg.SEM_GLOBAL


def bad_fields(got, want_cells):
    return np.argwhere((got != batch_ref.pack(want_cells)).any(axis=(1, 2))).ravel()


def rule_draws(n, h, w):
    """The (birth, survive) tables of one shape: MIXED cycled, then seeded random pairs;
    four draws of each where n <= 5 (rotated through MIXED, so that every rule of the list
    meets the shape)."""
    draws = 4 if n <= 5 else 1
    out = []
    for d in range(draws):
        rot = MIXED[(6 * d) % len(MIXED):] + MIXED[:(6 * d) % len(MIXED)]
        out.append(batch_rules_ref.cycled(n, rot))
    for d in range(draws):
        out.append(batch_rules_ref.random_rules(n, seed=h * 1000 + w + 7919 * d))
    return out


@pytest.mark.parametrize("torus", [False, True], ids=["dead", "torus"])
@pytest.mark.parametrize("h,w,n", SHAPES)
def test_mixed_rules_match_reference(pkg, h, w, n, torus):
    with pkg.BatchEngine(n, h, w, rule=OTHER, device=0, semantics=sem_of(pkg, torus)) as b:
        for di, (birth, survive) in enumerate(rule_draws(n, h, w)):
            cells = batch_ref.random_batch(n, h, w, seed=100 * di + h + w)
            start = batch_ref.pack(cells)
            b.set_rules(birth, survive)
            ref, done = cells, 0
            for g in GENS:
                ref, done = batch_rules_ref.run(ref, g - done, birth, survive, torus), g
                b.load_packed(start)
                b.step(g)
                bad = bad_fields(b.store_packed(), ref)
                assert bad.size == 0, (di, g, [(int(i), rule_ref.rule_name((birth[i], survive[i])))
                                               for i in bad[:8]])


@pytest.mark.parametrize("torus", [False, True], ids=["dead", "torus"])
@pytest.mark.parametrize("h,w,n", [(64, 64, 130), (17, 130, 17)])
def test_rule_follows_the_field_not_the_lane(pkg, h, w, n, torus):
    """FLOOD in one field in the middle of a wavefront and the empty rule in all others,
    then the complement: a lane that reads a neighbour field's word of the table floods
    or empties the wrong field."""
    mid = pkg.batch_geometry(n, h, w)["fields_per_wave"] // 2
    cells = batch_ref.random_batch(n, h, w, seed=h + w + 1)
    start = batch_ref.pack(cells)
    for inside, outside in ((rule_ref.FLOOD, (0, 0)), ((0, 0), rule_ref.FLOOD)):
        birth = np.full(n, outside[0], dtype=np.uint32)
        survive = np.full(n, outside[1], dtype=np.uint32)
        birth[mid], survive[mid] = inside
        with pkg.BatchEngine(n, h, w, rule=OTHER, device=0, semantics=sem_of(pkg, torus)) as b:
            b.set_rules(birth, survive)
            b.load_packed(start)
            b.step(1)
            one = b.store_packed()
            b.step(39)
            got = b.store_packed()
        want = batch_rules_ref.run(cells, 40, birth, survive, torus)
        assert bad_fields(got, want).size == 0
        empty = np.delete(one, mid, axis=0) if inside == rule_ref.FLOOD else one[mid:mid + 1]
        assert not empty.any()  # the empty rule: nothing is left after generation 1
        assert (got[mid] == batch_ref.pack(batch_ref.run(cells[mid:mid + 1], 40, inside, torus))[0]).all()


@pytest.mark.parametrize("torus", [False, True], ids=["dead", "torus"])
def test_every_rule_pair_once(pkg, torus):
    n, h, w, gens = 262144, 8, 8, 4
    i = np.arange(n, dtype=np.uint32)
    birth, survive = i & 511, i >> 9
    soup = batch_ref.random_batch(1, h, w, seed=88)
    cells = np.broadcast_to(soup, (n, h, w))
    start = np.ascontiguousarray(np.broadcast_to(batch_ref.pack(soup), (n, h, 1)))
    with pkg.BatchEngine(n, h, w, rule=OTHER, device=0, semantics=sem_of(pkg, torus)) as b:
        b.set_rules(birth, survive)
        b.load_packed(start)
        b.step(gens)
        got = b.store_packed()
    want = batch_rules_ref.run(cells, gens, birth, survive, torus)
    bad = bad_fields(got, want)
    assert bad.size == 0, [rule_ref.rule_name((birth[k], survive[k])) for k in bad[:8]]


@pytest.mark.parametrize("h,w,n", [(17, 130, 17), (64, 64, 130)])
@pytest.mark.parametrize("rule", [rule_ref.REF_RULE, rule_ref.CONWAY, B36S23],
                         ids=["B/S2", "B3/S23", "B36/S23"])
def test_uniform_table_equals_uniform_batch(pkg, rule, h, w, n):
    start = batch_ref.pack(batch_ref.random_batch(n, h, w, seed=h * w))
    with pkg.BatchEngine(n, h, w, rule=rule, device=0) as a:
        a.load_packed(start)
        a.step(37)
        want = a.store_packed()
    with pkg.BatchEngine(n, h, w, rule=OTHER, device=0) as b:
        b.set_rules(np.full(n, rule[0]), np.full(n, rule[1]))
        b.load_packed(start)
        b.step(37)
        assert (b.store_packed() == want).all()
        b.drop_rules()
        assert not b.per_field_rules
        b.load_packed(start)
        b.step(37)
        got = b.store_packed()
    assert (got == batch_ref.pack(batch_ref.run(batch_ref.unpack(start, w), 37, OTHER))).all()


def test_table_calls(pkg):
    h, w, n = 9, 65, 70
    L = pkg.lib()
    cells = batch_ref.random_batch(n, h, w, seed=4)
    start = batch_ref.pack(cells)
    u32 = lambda v: np.ascontiguousarray(v, dtype=np.uint32)
    with pkg.BatchEngine(n, h, w, rule=rule_ref.CONWAY, device=0) as b:
        # before any set: the create rule, no table
        assert not b.per_field_rules
        birth, survive = b.rules()
        assert birth.dtype == np.uint32 and survive.dtype == np.uint32
        assert (birth == rule_ref.CONWAY[0]).all() and (survive == rule_ref.CONWAY[1]).all()
        assert b.rules(first=n, count=0)[0].shape == (0,)
        # count == 0 allocates nothing
        b.set_rules([], [], first=3)
        assert L.gol_batch_set_rules(b._h, n, 0, None, None) == pkg.GOL_OK
        assert not b.per_field_rules
        assert L.gol_batch_drop_rules(b._h) == pkg.GOL_OK  # GOL_OK when there is none

        # every GOL_EINVAL case, without a table: none is made
        ok = u32([1, 2])
        def einval_cases():
            big = u32([1, 0x200])
            return [(b._h, n - 1, 2, ok.ctypes.data, ok.ctypes.data),
                    (b._h, n + 1, 0, ok.ctypes.data, ok.ctypes.data),
                    (b._h, 0, 2, None, ok.ctypes.data), (b._h, 0, 2, ok.ctypes.data, None),
                    (b._h, 0, 2, big.ctypes.data, ok.ctypes.data),
                    (b._h, 0, 2, ok.ctypes.data, big.ctypes.data),
                    (None, 0, 2, ok.ctypes.data, ok.ctypes.data)], big
        cases, keep = einval_cases()
        for args in cases:
            assert L.gol_batch_set_rules(*args) == pkg.GOL_EINVAL, args[1:3]
            assert L.gol_last_error()
        assert not b.per_field_rules
        on = ctypes.c_uint32(7)
        assert L.gol_batch_has_rules(None, ctypes.byref(on)) == pkg.GOL_EINVAL
        assert L.gol_batch_has_rules(b._h, None) == pkg.GOL_EINVAL
        assert L.gol_batch_get_rules(None, 0, 1, None, None) == pkg.GOL_EINVAL
        assert L.gol_batch_get_rules(b._h, n, 1, None, None) == pkg.GOL_EINVAL
        assert L.gol_batch_drop_rules(None) == pkg.GOL_EINVAL
        for bad in (([1, 2], [1]), ([[1]], [[1]]), ([0x200], [0]), ([0], [-1])):
            with pytest.raises(pkg.GolError):
                b.set_rules(*bad)
        with pytest.raises(pkg.GolError):
            b.set_rules([1, 2], [1, 2], first=n - 1)
        assert not b.per_field_rules

        # a sub-range set changes only its range; the others keep the create rule
        b.set_rules([1 << 1, 1 << 2], [1 << 3, 1 << 4], first=5)
        assert b.per_field_rules
        want_b = np.full(n, rule_ref.CONWAY[0], dtype=np.uint32)
        want_s = np.full(n, rule_ref.CONWAY[1], dtype=np.uint32)
        want_b[5:7], want_s[5:7] = [2, 4], [8, 16]
        birth, survive = b.rules()
        assert birth.tolist() == want_b.tolist() and survive.tolist() == want_s.tolist()
        # a second set overwrites, again only its range; either out array may be NULL
        b.set_rules([0x1FF, 0, 3], [0, 0x1FF, 5], first=6)
        want_b[6:9], want_s[6:9] = [0x1FF, 0, 3], [0, 0x1FF, 5]
        birth, survive = b.rules()
        assert birth.tolist() == want_b.tolist() and survive.tolist() == want_s.tolist()
        pb, ps = b.rules(first=5, count=3)
        assert pb.tolist() == want_b[5:8].tolist() and ps.tolist() == want_s[5:8].tolist()
        only = np.zeros(3, dtype=np.uint32)
        assert L.gol_batch_get_rules(b._h, 5, 3, None, only.ctypes.data) == pkg.GOL_OK
        assert only.tolist() == want_s[5:8].tolist()
        assert L.gol_batch_get_rules(b._h, 5, 3, only.ctypes.data, None) == pkg.GOL_OK
        assert only.tolist() == want_b[5:8].tolist()

        # every GOL_EINVAL case again: the table and the fields stay as they are
        b.load_packed(start)
        cases, keep = einval_cases()
        for args in cases:
            assert L.gol_batch_set_rules(*args) == pkg.GOL_EINVAL, args[1:3]
        assert b.per_field_rules
        birth, survive = b.rules()
        assert birth.tolist() == want_b.tolist() and survive.tolist() == want_s.tolist()
        assert (b.store_packed() == start).all()

        # a set between two steps takes effect from the second
        b.step(3)
        mid = batch_rules_ref.run(cells, 3, want_b, want_s)
        nb, ns = batch_rules_ref.random_rules(n, seed=12)
        b.set_rules(nb, ns)
        b.step(4)
        assert bad_fields(b.store_packed(), batch_rules_ref.run(mid, 4, nb, ns)).size == 0

        # has_rules follows set and drop; after a drop rules() is the create rule again
        b.drop_rules()
        assert not b.per_field_rules
        assert (b.rules()[0] == rule_ref.CONWAY[0]).all() and (b.rules()[1] == rule_ref.CONWAY[1]).all()
        b.drop_rules()
        b.set_rules([7], [9], first=n - 1)
        assert b.per_field_rules
        birth, survive = b.rules()
        assert (birth[-1], survive[-1]) == (7, 9) and (birth[:-1] == rule_ref.CONWAY[0]).all()


@pytest.mark.parametrize("torus", [False, True], ids=["dead", "torus"])
def test_launch_split_with_rules(pkg, monkeypatch, torus):
    h, w, n = 17, 130, 17
    cells = batch_ref.random_batch(n, h, w, seed=78)
    start = batch_ref.pack(cells)
    birth, survive = batch_rules_ref.cycled(n, MIXED[13:] + MIXED[:13])
    want = batch_rules_ref.run(cells, 13, birth, survive, torus)
    monkeypatch.setenv("GOL_DEV_BATCH_LAUNCH_GENS", "5")
    with pkg.BatchEngine(n, h, w, rule=OTHER, device=0, semantics=sem_of(pkg, torus)) as b:
        assert b.launch_generations == 5
        b.set_rules(birth, survive)
        b.load_packed(start)
        b.step(13)
        assert bad_fields(b.store_packed(), want).size == 0
        b.load_packed(start)
        b.step(4)
        b.step(9)
        assert bad_fields(b.store_packed(), want).size == 0


_until_refs = {}


def until_ref_per_field(h, w, n, torus, max_g, lag, every):
    """(cells, birth, survive, (period, generation, final)): batch_until_ref.until_ref
    called on every field alone with its rule, computed once per case."""
    key = (h, w, n, torus, max_g, lag, every)
    if key not in _until_refs:
        cells = batch_ref.random_batch(n, h, w, seed=h * 1000 + w, p=.35)
        birth, survive = batch_rules_ref.cycled(n)
        period = np.zeros(n, dtype=np.uint32)
        generation = np.zeros(n, dtype=np.uint64)
        final = np.zeros_like(cells)
        for i in range(n):
            p, g, f = batch_until_ref.until_ref(cells[i:i + 1], max_g, lag, every,
                                                (int(birth[i]), int(survive[i])), torus)
            period[i], generation[i], final[i] = p[0], g[0], f[0]
        for a in (cells, birth, survive, period, generation, final):
            a.setflags(write=False)
        _until_refs[key] = (cells, birth, survive, (period, generation, final))
    return _until_refs[key]


@pytest.mark.parametrize("torus", [False, True], ids=["dead", "torus"])
@pytest.mark.parametrize("lag,every", [(6, 0), (4, 5)])
@pytest.mark.parametrize("h,w,n", [(16, 16, 130), (17, 130, 33)])
def test_period_detection_with_rules(pkg, h, w, n, lag, every, torus):
    max_g = 256
    cells, birth, survive, ref = until_ref_per_field(h, w, n, torus, max_g, lag, every)
    assert (ref[0] != 0).any() and (ref[0] == 0).any()  # found and unfound fields
    with pkg.BatchEngine(n, h, w, rule=OTHER, device=0, semantics=sem_of(pkg, torus)) as b:
        b.set_rules(birth, survive)
        b.load_packed(batch_ref.pack(cells))
        got = b.step_until_periodic(max_g, lag, every)
        check_result(pkg, b, got, b.store_packed(), ref, max_g, lag, every, w)
