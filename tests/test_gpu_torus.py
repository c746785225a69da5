"""GPU suite for the torus engines (GOL_SEM_TORUS): every case is exact, the stored
field against the torus reference of torus_ref.py (wrapped padding + the
dead-border oracle + crop, itself checked against np.roll in test_torus_host.py)
and the digest against the oracle's digest of that field."""
import numpy as np
import pytest

import torus_ref

pytestmark = pytest.mark.gpu

RULES = {"B/S2": (0, 1 << 2), "B3/S23": (1 << 3, (1 << 2) | (1 << 3)),
         "B36/S23": ((1 << 3) | (1 << 6), (1 << 2) | (1 << 3))}
SHAPES = [(1, 64), (3, 64), (64, 64), (100, 128), (130, 192), (257, 320), (37, 500), (1500, 500),
          (9, 65)]
# defaults (small fields: a resident inner engine is likely) and the streaming kernel
PLANS = {"default": {}, "streaming": {"tb_depth": 8, "resident": 1}}

_refs = {}


def reference(oracle, h, w, seed, gens, rule):
    """The torus reference of the oracle's synthetic h x w field, computed once per
    (field, generations, rule) and shared (read only)."""
    key = (h, w, seed, gens, rule)
    if key not in _refs:
        got = torus_ref.torus_run(oracle, oracle.bp_random(h, w, seed), w, gens, RULES[rule])
        got.setflags(write=False)
        _refs[key] = got
    return _refs[key]


def check(oracle, e, want, w):
    got = e.store_packed()
    assert (got == want).all(), f"{int((got != want).sum())} words differ"
    assert e.digest() == oracle.bp_digest(np.array(want), w)


def gens_list(G, K):
    return sorted({g for g in (1, G - 1, G, G + 1, 2 * G + K + 3) if g > 0})


def run_case(pkg, oracle, h, w, rule, seed=3, **kw):
    with pkg.Engine(h, w, rule=RULES[rule], semantics=pkg.SEM_TORUS, **kw) as e:
        assert (e.h, e.w, e.rows, e.row0) == (h, w, h, 0)
        G, K = e.halo_depth, e.tb_depth
        assert G >= 1 and K >= 1
        if "halo_depth" in kw:
            assert G == kw["halo_depth"]
        start = oracle.bp_random(h, w, seed)
        for gens in gens_list(G, K):
            e.load_packed(start)
            e.step(gens)
            check(oracle, e, reference(oracle, h, w, seed, gens, rule), w)


def glider_field():
    bits = np.zeros((64, 64), dtype=np.uint8)
    for y, x in ((0, 1), (1, 2), (2, 0), (2, 1), (2, 2)):  # heads down and right
        bits[60 + y, 59 + x] = 1
    return torus_ref.pack(bits)


def test_glider_crosses_every_edge(pkg, oracle):
    """B3/S23, 64 x 64, one glider starting near the bottom right corner: it moves
    one cell down and right every 4 generations, so in 256 generations it crosses
    the bottom edge, the right edge and the corner, comes in over the top and the
    left edge, and is back where it started."""
    start = glider_field()
    with pkg.Engine(64, 64, rule=RULES["B3/S23"], semantics=pkg.SEM_TORUS) as e:
        for gens in (30, 63, 64):
            e.load_packed(start)
            e.step(gens)
            want = torus_ref.roll_run(start, 64, gens, RULES["B3/S23"])
            assert int(torus_ref.unpack(want, 64).sum()) == 5  # still a glider
            check(oracle, e, want, 64)
        e.load_packed(start)
        e.step(256)
        check(oracle, e, start, 64)


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("h,w", SHAPES)
def test_random_fields(pkg, oracle, h, w, rule, plan):
    """p = 0.5 fields: 1, G-1, G, G+1 and 2G+K+3 generations from the same start,
    so one round, the round boundary and a remainder round each show."""
    run_case(pkg, oracle, h, w, rule, **PLANS[plan])


@pytest.mark.parametrize("G", [5, 200])
@pytest.mark.parametrize("rule", list(RULES))
def test_explicit_round_length(pkg, oracle, rule, G):
    """halo_depth sets G: below the fused depth, and above 64 columns per ghost
    word and close to h (ghost rows that wrap almost the whole field)."""
    run_case(pkg, oracle, 257, 320, rule, halo_depth=G)
    run_case(pkg, oracle, 257, 320, rule, halo_depth=G, **PLANS["streaming"])


@pytest.mark.parametrize("kw", [{}, {"resident": 1}], ids=["default", "streaming"])
def test_large(pkg, oracle, kw):
    """6200 x 4096, B3/S23, 2G + 5 generations: the default plan (on a 256-CU device
    the resident kernel still takes the padded field) and, with the resident kernel
    off, the K = 16 multi-block streaming plan under the wrap."""
    h, w, rule = 6200, 4096, "B3/S23"
    with pkg.Engine(h, w, rule=RULES[rule], semantics=pkg.SEM_TORUS, **kw) as e:
        if kw:
            assert e.resident is None and e.tb_depth == 16
        assert e.halo_depth == pkg.torus_geometry(h, w, rule=RULES[rule], **kw)["round_gens"]
        gens = 2 * e.halo_depth + 5
        e.init_random(3)
        e.step(gens)
        check(oracle, e, reference(oracle, h, w, 3, gens, rule), w)


@pytest.mark.parametrize("plan", list(PLANS))
def test_split_stepping(pkg, oracle, plan):
    """step(5); step(7); step(G) equals step(G + 12): every gol_step starts with a
    wrap of its own and nothing relies on the ghosts between calls."""
    h, w, rule = 130, 192, "B3/S23"
    with pkg.Engine(h, w, rule=RULES[rule], semantics=pkg.SEM_TORUS, **PLANS[plan]) as e:
        G = e.halo_depth
        e.init_random(3)
        for n in (5, 7, G):
            e.step(n)
        check(oracle, e, reference(oracle, h, w, 3, G + 12, rule), w)
        e.init_random(3)
        e.step(G + 12)
        check(oracle, e, reference(oracle, h, w, 3, G + 12, rule), w)


@pytest.mark.parametrize("plan", list(PLANS))
def test_load_mid_run_starts_clean(pkg, oracle, ref_data, plan):
    """A load between steps replaces the field, ghosts and skip history included."""
    h, w, rule = 1500, 500, "B/S2"
    with pkg.Engine(h, w, rule=RULES[rule], semantics=pkg.SEM_TORUS, **PLANS[plan]) as e:
        G = e.halo_depth
        e.load_ascii(ref_data)
        e.step(3 * G)
        e.load_packed(oracle.bp_random(h, w, 3))
        e.step(G + 1)
        check(oracle, e, reference(oracle, h, w, 3, G + 1, rule), w)


def test_settling_field_with_and_without_skip(pkg, oracle, ref_data, monkeypatch):
    """The reference input as a torus under B/S2 settles within a few dozen
    generations: the inner engine's activity skip and copy-through then leave units
    out, the wrap between rounds notwithstanding, and the field is the same as
    with the skip off and as the reference."""
    h, w = 1500, 500
    start = oracle.bp_pack(ref_data, h, w)
    fields = {}
    for skip in ("1", "0"):
        monkeypatch.setenv("GOL_DEV_ACTIVITY_SKIP", skip)
        # classic row blocks on the streaming kernel (where the skip lives), 8
        # launches per round
        with pkg.Engine(h, w, rule=RULES["B/S2"], semantics=pkg.SEM_TORUS, tb_depth=8,
                        resident=1, handoff=1, halo_depth=64) as e:
            G = e.halo_depth
            gens = 3 * G + 5  # four rounds
            e.load_ascii(ref_data)
            e.step(gens)
            fields[skip] = e.store_packed()
            digest = e.digest()
            computed, skipped = e.activity()
        want = torus_ref.torus_run(oracle, start, w, gens, RULES["B/S2"], chunk=64)
        assert (fields[skip] == want).all()
        assert digest == oracle.bp_digest(want, w)
        if skip == "1":
            assert computed > 0 and skipped > 0, (computed, skipped)
        else:
            assert skipped == 0
    assert (fields["1"] == fields["0"]).all()


@pytest.mark.parametrize("h,w", [(37, 500), (64, 64), (9, 65)])
def test_same_start_as_dead_border_engine(pkg, oracle, h, w):
    """init_random(seed) and its digest at generation 0: those of a dead-border
    engine of the same size and seed (the interior's own word index)."""
    with pkg.Engine(h, w, semantics=pkg.SEM_TORUS) as t, pkg.Engine(h, w) as d:
        t.init_random(11)
        d.init_random(11)
        a, b = t.store_packed(), d.store_packed()
        assert (a == b).all() and (a == oracle.bp_random(h, w, 11)).all()
        assert t.digest() == d.digest() == oracle.bp_digest(a, w)
        assert t.digest_rows(h // 2, h - h // 2) == d.digest_rows(h // 2, h - h // 2)
        # after a step the interior's last word holds ghost cells next to column
        # w - 1: the caller still sees columns >= w as 0
        t.step(3)
        got = t.store_packed()
        if w % 64:
            assert not (got[:, -1] >> np.uint64(w % 64)).any()
        lo, hi = t.digest_rows(0, h // 2), t.digest_rows(h // 2, h - h // 2)
        assert ((lo[0] + hi[0]), (lo[1] + hi[1]) & 0xFFFFFFFFFFFFFFFF) == t.digest()


def test_ascii_round_trip(pkg, oracle):
    """store_ascii of a w % 64 != 0 torus: only '0', '1' and '\\n', the stored
    field's cells, and load_ascii of it gives the same field back."""
    h, w, rule = 37, 500, "B3/S23"
    with pkg.Engine(h, w, rule=RULES[rule], semantics=pkg.SEM_TORUS) as e:
        e.init_random(3)
        e.step(9)
        text = e.store_ascii()
        want = reference(oracle, h, w, 3, 9, rule)
        assert set(text) <= set(b"01\n") and len(text) == h * (w + 1)
        assert text == oracle.bp_unpack(np.array(want), w)
        e.load_ascii(text)
        check(oracle, e, want, w)
        e.step(4)
        check(oracle, e, reference(oracle, h, w, 3, 13, rule), w)


def test_rejected_configs(pkg):
    for kw in ({"streams": 2}, {"word_planes": 4}, {"halo_depth": 1 << 17}):
        with pytest.raises(pkg.GolError) as ei:
            pkg.Engine(256, 256, semantics=pkg.SEM_TORUS, **kw)
        assert ei.value.status == pkg.GOL_EINVAL
    with pytest.raises(pkg.GolError) as ei:
        pkg.Group(1024, 256, 2, semantics=pkg.SEM_TORUS)
    assert ei.value.status == pkg.GOL_EINVAL
    with pytest.raises(pkg.GolError) as ei:
        pkg.Engine(1024, 256, semantics=pkg.SEM_TORUS, rank=0, nranks=2,
                   transport=lambda up, dn: (None, None))
    assert ei.value.status == pkg.GOL_EINVAL
    # streams = 1 and word_planes = 2 are the torus engine's own values
    with pkg.Engine(256, 256, semantics=pkg.SEM_TORUS, streams=1, word_planes=2) as e:
        assert e.halo_depth >= 1
