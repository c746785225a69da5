"""GPU: region I/O -- Engine.read_rect / write_rect / density (gol_read_rect,
gol_write_rect, gol_density) on every engine kind, exact against numpy on the
stored field and, after an edit between steps, against the CPU oracle.

An edit between steps meets the machinery that assumes nobody edits: the activity
skip and copy-through, replayed step graphs, stripe halos, torus ghosts and the
resident plan.  Every "edit, then step" case uses the same generation count before
and after the edit, at least 4 K and no multiple of K, so the step after the edit
replays a captured graph and ends with a remainder launch.
"""
import numpy as np
import pytest

import torus_ref

pytestmark = pytest.mark.gpu

SHAPES = [(9, 65), (37, 500), (130, 192), (257, 320), (1500, 500)]
BIG = (1500, 500)
CONWAY = (1 << 3, (1 << 2) | (1 << 3))
REF = (0, 1 << 2)
GLIDER = np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]], dtype=np.uint8)
RPENTO = np.array([[0, 1, 1], [1, 1, 0], [0, 1, 0]], dtype=np.uint8)


def step_gens(K):
    """At least 4 K generations and no multiple of K (K = 8: 37, four launches of 8
    and a remainder; a resident engine reports its epoch length as K)."""
    g = 4 * K + 5
    return g if g % K else g + 1


# name -> (constructor keywords, parts the field's rows are split into, torus)
KINDS = {
    "default": (dict(), 1, False),
    "streaming": (dict(tb_depth=8, resident=1), 1, False),
    "streams2": (dict(streams=2), 2, False),
    "streams3": (dict(streams=3), 3, False),
    "group3": (None, 3, False),
    "torus": (dict(semantics=2), 1, True),
    "torus_streaming": (dict(semantics=2, tb_depth=8, resident=1), 1, True),
}
SMALL_KINDS = ["default", "streaming", "torus", "torus_streaming"]
BIG_KINDS = ["streams2", "streams3", "group3"]
CASES = [(k, s) for k in SMALL_KINDS for s in SHAPES] + [(k, BIG) for k in BIG_KINDS]
CASE_IDS = [f"{k}-{h}x{w}" for k, (h, w) in CASES]


def make(pkg, kind, h, w, rule=REF):
    kw, _, _ = KINDS[kind]
    if kw is None:
        return pkg.Group(h, w, 3, rule=rule)
    return pkg.Engine(h, w, rule=rule, device=0, **kw)


def boundaries(pkg, kind, h):
    n = KINDS[kind][1]
    return [pkg.rank_rows(h, n, r)[0] for r in range(1, n)]


def crop(bits, y, x, rh, rw):
    """The window as packed words; indices wrap (a no-op inside the field)."""
    h, w = bits.shape
    return torus_ref.pack(bits[np.ix_((y + np.arange(rh)) % h, (x + np.arange(rw)) % w)])


def apply(bits, y, x, win, op):
    """bits with the window cells `win` combined at (y, x), wrapping."""
    h, w = bits.shape
    ix = np.ix_((y + np.arange(win.shape[0])) % h, (x + np.arange(win.shape[1])) % w)
    out = bits.copy()
    d = bits[ix]
    out[ix] = (win, d | win, d ^ win, d & (1 - win))[op]
    return out


def junk_window(rng, win):
    """Packed window whose bits beyond its width are random: they must be ignored."""
    rh, rw = win.shape
    words = torus_ref.pack(win)
    if rw % 64:
        words[:, -1] |= rng.integers(0, 1 << 63, rh, dtype=np.uint64) << np.uint64(rw % 64)
    return words


def row_spans(pkg, kind, h):
    spans = {(0, 1), (0, h), (h - 1, 1), (h // 2, min(3, h - h // 2))}
    for b in boundaries(pkg, kind, h):
        spans |= {(b - 1, 2), (b - 3, 7), (b, 1), (b - 1, 1)}
    return sorted(spans)


def col_spans(w):
    out = []
    for x in (0, 1, 31, 63, 64 + 31):
        for rw in (1, 63, 64, 65, 129, w - x):
            if rw >= 1 and x + rw <= w:
                out.append((x, rw))
    return sorted(set(out))


@pytest.mark.parametrize("kind,shape", CASES, ids=CASE_IDS)
def test_read(pkg, kind, shape):
    h, w = shape
    with make(pkg, kind, h, w) as e:
        e.init_random(5)
        stored = e.store_packed()
        bits = torus_ref.unpack(stored, w)
        assert (e.read_rect(0, 0, h, w) == torus_ref.pack(bits)).all()
        cols = col_spans(w)
        for n, (y, rh) in enumerate(row_spans(pkg, kind, h)):
            # every column case on the first spans, a rotating third on the others
            for x, rw in (cols if n < 2 else cols[n % 3::3]):
                got = e.read_rect(y, x, rh, rw)
                assert got.shape == (rh, (rw + 63) // 64)
                assert (got == crop(bits, y, x, rh, rw)).all(), (y, x, rh, rw)


def write_rects(pkg, kind, h, w):
    rects = [(0, 0, h, w), (h - 1, w - 1, 1, 1), (h // 3, max(0, w - 70), min(5, h - h // 3), min(70, w)),
             (1, 1, min(4, h - 1), min(63, w - 1))]
    if w > 129 + 31:
        rects.append((h // 2, 31, min(3, h - h // 2), 129))
    for b in boundaries(pkg, kind, h):
        rects.append((b - 2, 63, 5, 66))
    return rects


@pytest.mark.parametrize("kind,shape", CASES, ids=CASE_IDS)
def test_write(pkg, oracle, kind, shape):
    h, w = shape
    torus = KINDS[kind][2]
    rng = np.random.default_rng(h * 1000 + w)
    with make(pkg, kind, h, w, rule=CONWAY) as e:
        e.init_random(8)
        bits = torus_ref.unpack(e.store_packed(), w)
        for n, (y, x, rh, rw) in enumerate(write_rects(pkg, kind, h, w)):
            for op in ((0, 1, 2, 3) if n else (2, 0)):  # (whole field: XOR and SET)
                win = rng.integers(0, 2, (rh, rw), dtype=np.uint8)
                e.write_rect(y, x, junk_window(rng, win), rw, op)
                bits = apply(bits, y, x, win, op)
                # every word, so also every one outside the rectangle and the
                # columns >= w of a dead-border engine's last word
                want = torus_ref.pack(bits)
                assert (e.store_packed() == want).all(), (y, x, rh, rw, op)
            assert tuple(e.digest()) == tuple(oracle.bp_digest(want, w))
        # the cells at columns >= w stayed dead (torus: the ghosts are rewritten
        # from the edited interior): the field evolves as the oracle's
        e.step(9)
        if torus:
            want = torus_ref.torus_run(oracle, want, w, 9, CONWAY)
        else:
            want = oracle.bp_run(want, w, 9, CONWAY)
        assert (e.store_packed() == want).all()


@pytest.mark.parametrize("rule,pattern", [(CONWAY, GLIDER), (REF, RPENTO)], ids=["B3S23", "BS2"])
@pytest.mark.parametrize("kind,shape", CASES, ids=CASE_IDS)
def test_edit_then_step(pkg, oracle, kind, shape, rule, pattern):
    h, w = shape
    torus = KINDS[kind][2]

    def run(words, gens):
        if torus:
            return torus_ref.torus_run(oracle, words, w, gens, rule)
        return oracle.bp_run(words, w, gens, rule)

    with make(pkg, kind, h, w, rule=rule) as e:
        K = (e.members[0] if hasattr(e, "members") else e).tb_depth
        GENS = step_gens(K)
        assert GENS >= 4 * K and GENS % K
        start = oracle.bp_random(h, w, 21)
        e.load_packed(start)
        # twice: a step graph is keyed by (generations, starting buffer), and after
        # two steps the one for either buffer exists, so the step after the edit
        # replays a graph captured before it
        e.step(GENS)
        e.step(GENS)
        mid = run(start, 2 * GENS)
        # on a part boundary where there is one, else mid-field at an odd column
        bs = boundaries(pkg, kind, h)
        y, x = (bs[0] - 1 if bs else h // 2), min(w - 3, 62)
        e.write_rect(y, x, torus_ref.pack(pattern), 3, pkg.RECT_OR)
        edited = torus_ref.pack(apply(torus_ref.unpack(mid, w), y, x, pattern, 1))
        assert (e.store_packed() == edited).all() and not (edited == mid).all()
        e.step(GENS)
        want = run(edited, GENS)
        assert (e.store_packed() == want).all()


def test_edit_a_still_field(pkg, oracle, monkeypatch):
    """B/S2 from p = 0.5 is still after 5 generations (seed 3: checked with the
    oracle below), so the later launches of the first step skip.  An XOR of a 2 x 2
    block, whose cells have 3 neighbours each and die, into that field must be
    computed by the next step: no streak from before the edit may license a skip."""
    monkeypatch.delenv("GOL_DEV_ACTIVITY_SKIP", raising=False)
    h, w = BIG
    start = oracle.bp_random(h, w, 3)
    still = oracle.bp_run(start, w, 5)
    assert (oracle.bp_run(still, w, 1) == still).all()
    with pkg.Engine(h, w, device=0, tb_depth=8, resident=1, handoff=1, streams=1,
                    rows_per_wave=64) as e:
        e.load_packed(start)
        e.reset_timing()
        e.step(43)
        e.step(43)  # (the graphs of both starting buffers now exist)
        assert (e.store_packed() == still).all()
        computed, skipped = e.activity()
        assert skipped >= 1, "the first step never skipped: the case does not count"
        block = np.ones((2, 2), dtype=np.uint8)
        bits = torus_ref.unpack(still, w)
        assert not bits[699:703, 249:253].any()
        e.write_rect(700, 250, torus_ref.pack(block), 2, pkg.RECT_XOR)
        edited = torus_ref.pack(apply(bits, 700, 250, block, 2))
        want = oracle.bp_run(edited, w, 43)
        assert not (want == edited).all()
        e.step(43)
        assert (e.store_packed() == want).all()
        assert tuple(e.digest()) == tuple(oracle.bp_digest(want, w))
        # and the skip is back once the edit has died down
        assert e.activity()[1] > skipped


@pytest.mark.parametrize("shape", [(64, 64), (37, 500)])
@pytest.mark.parametrize("kind", ["torus", "torus_streaming"])
def test_torus_seams(pkg, kind, shape):
    h, w = shape
    rng = np.random.default_rng(h + w)
    with make(pkg, kind, h, w, rule=CONWAY) as e:
        e.init_random(2)
        bits = torus_ref.unpack(e.store_packed(), w)
        rects = [(h - 3, 5, 7, 40), (4, w - 9, 6, 30), (h - 2, w - 33, 5, 70 if w > 70 else 50),
                 (h - 1, w - 1, h, w), (0, w - 1, h, 2)]
        for y, x, rh, rw in rects:
            assert (e.read_rect(y, x, rh, rw) == crop(bits, y, x, rh, rw)).all(), (y, x, rh, rw)
        for y, x, rh, rw in rects:
            for op in range(4):
                win = rng.integers(0, 2, (rh, rw), dtype=np.uint8)
                e.write_rect(y, x, junk_window(rng, win), rw, op)
                bits = apply(bits, y, x, win, op)
                assert (e.store_packed() == torus_ref.pack(bits)).all(), (y, x, rh, rw, op)
                assert (e.read_rect(y, x, rh, rw) == crop(bits, y, x, rh, rw)).all()


@pytest.mark.parametrize("kind", ["torus", "torus_streaming"])
def test_torus_glider_across_the_corner(pkg, kind):
    with make(pkg, kind, 64, 64, rule=CONWAY) as e:
        e.load_packed(np.zeros((64, 1), dtype=np.uint64))
        e.write_rect(63, 62, torus_ref.pack(GLIDER), 3, pkg.RECT_SET)
        assert e.digest()[0] == 5
        first = e.read_rect(63, 62, 3, 3)
        assert (first == torus_ref.pack(GLIDER)).all()
        e.step(100)
        assert not (e.read_rect(63, 62, 3, 3) == first).all()
        e.step(156)
        assert (e.read_rect(63, 62, 3, 3) == first).all() and e.digest()[0] == 5


def block_sums(bits, by, bx):
    rows = np.add.reduceat(bits.astype(np.uint32), np.arange(0, bits.shape[0], by), axis=0)
    return np.add.reduceat(rows, np.arange(0, bits.shape[1], bx), axis=1)


DENSITY_CASES = [("default", (37, 500)), ("default", (257, 320)), ("streaming", BIG),
                 ("streams3", BIG), ("group3", BIG), ("torus", (37, 500)),
                 ("torus_streaming", (257, 320))]


@pytest.mark.parametrize("kind,shape", DENSITY_CASES, ids=[f"{k}-{h}x{w}" for k, (h, w) in DENSITY_CASES])
def test_density(pkg, kind, shape):
    h, w = shape
    torus = KINDS[kind][2]
    with make(pkg, kind, h, w) as e:
        e.init_random(4)
        bits = torus_ref.unpack(e.store_packed(), w)
        live = e.digest()[0]
        windows = [(0, 0, h, w), (3, 5, h - 4, w - 6), (h // 2 - 1, 63, min(h // 2, 70), min(w - 63, 131))]
        if torus:
            windows += [(h - 5, w - 37, 11, 100), (h - 1, w - 1, h, w)]
        for by, bx in ((1, 1), (1, 64), (8, 8), (16, 100), (64, 64), (h, w)):
            for y, x, rh, rw in windows:
                got = e.density(y, x, rh, rw, by, bx)
                want = block_sums(torus_ref.unpack(crop(bits, y, x, rh, rw), rw), by, bx)
                assert got.dtype == np.uint32 and got.shape == want.shape
                assert (got == want).all(), (by, bx, y, x, rh, rw)
            assert int(e.density(0, 0, h, w, by, bx).sum(dtype=np.uint64)) == live
        if hasattr(e, "members"):  # the members' counts add up, each its own rows
            parts = [m.density(0, 0, h, w, 64, 64) for m in e.members]
            assert (sum(p.astype(np.uint64) for p in parts) == block_sums(bits, 64, 64)).all()
            for m, p in zip(e.members, parts):
                assert int(p.sum()) == int(bits[m.row0:m.row0 + m.rows].sum())
            # and a member's read zero-fills the rows it does not own
            m = e.members[1]
            got = torus_ref.unpack(m.read_rect(0, 0, h, w), w)
            assert (got[m.row0:m.row0 + m.rows] == bits[m.row0:m.row0 + m.rows]).all()
            assert not got[:m.row0].any() and not got[m.row0 + m.rows:].any()


def test_errors(pkg):
    h, w = 37, 500
    win = np.zeros((4, 2), dtype=np.uint64)
    with pkg.Engine(h, w, device=0) as e, pkg.Engine(h, w, device=0, semantics=2) as t:
        e.init_random(1)
        before = e.store_packed()
        L = pkg.lib()
        # (the bounds are checked before the window is touched)
        for y, x, rh, rw in ((h - 3, 0, 4, 10), (0, w - 9, 4, 10), (h + 1, 0, 0, 0), (0, 0, h + 1, 1),
                             (2 ** 63, 0, 2 ** 63, 1), (0, 2 ** 64 - 1, 1, 2)):
            for st in (L.gol_read_rect(e._h, y, x, rh, rw, win.ctypes.data, 2),
                       L.gol_write_rect(e._h, y, x, rh, rw, win.ctypes.data, 2, 0)):
                assert st == pkg.GOL_EINVAL and b"outside" in L.gol_last_error()
        with pytest.raises(pkg.GolError) as ei:
            e.read_rect(h - 3, 0, 4, 10)
        assert ei.value.status == pkg.GOL_EINVAL and "outside" in str(ei.value)
        with pytest.raises(pkg.GolError) as ei:
            e.density(0, 0, h, w + 1, 8, 8)
        assert ei.value.status == pkg.GOL_EINVAL
        # torus: any start inside the field, at most one period
        for y, x, rh, rw in ((h, 0, 1, 1), (0, w, 1, 1), (0, 0, h + 1, 1), (0, 0, 1, w + 1)):
            with pytest.raises(pkg.GolError) as ei:
                t.read_rect(y, x, rh, rw)
            assert ei.value.status == pkg.GOL_EINVAL and "torus" in str(ei.value)
        # strides, ops, block sizes
        cnt = np.zeros((8, 8), dtype=np.uint32)
        assert L.gol_read_rect(e._h, 0, 0, 4, 129, win.ctypes.data, 2) == pkg.GOL_EINVAL
        assert L.gol_write_rect(e._h, 0, 0, 4, 129, win.ctypes.data, 2, 0) == pkg.GOL_EINVAL
        assert L.gol_write_rect(e._h, 0, 0, 4, 128, win.ctypes.data, 2, 4) == pkg.GOL_EINVAL
        assert L.gol_density(e._h, 0, 0, h, w, 8, 8, cnt.ctypes.data, 8) == pkg.GOL_EINVAL
        for by, bx, rh, rw in ((0, 8, 8, 8), (8, 0, 8, 8), (8, 8, 0, 8), (8, 8, 8, 0),
                               (1 << 16, 1 << 16, 8, 8)):
            assert L.gol_density(e._h, 0, 0, rh, rw, by, bx, cnt.ctypes.data, 8) == pkg.GOL_EINVAL
        assert L.gol_last_error()
        # zero-size rectangles do nothing
        e.write_rect(h, w, np.zeros((0, 1), dtype=np.uint64), 0)
        e.write_rect(3, 3, np.ones((2, 1), dtype=np.uint64), 0)
        assert e.read_rect(h, w, 0, 0).shape == (0, 0) and e.read_rect(1, 1, 3, 0).shape == (3, 0)
        assert (e.store_packed() == before).all()
    with pkg.Engine(h, w, device=0, semantics=pkg.SEM_REF_STRIPES, ref_ranks=3) as r:
        r.init_random(1)
        stored = r.store_packed()
        with pytest.raises(pkg.GolError) as ei:
            r.write_rect(0, 0, win, 128)
        assert ei.value.status == pkg.GOL_ESTATE
        bits = torus_ref.unpack(stored, w)
        assert (r.read_rect(5, 31, 30, 200) == crop(bits, 5, 31, 30, 200)).all()
        assert (r.density(0, 0, h, w, 8, 64) == block_sums(bits, 8, 64)).all()
        assert (r.store_packed() == stored).all()


def test_four_planes(pkg):
    """The NP = 4 kernels: only a library built with them (the dev build, through
    GOL_LIB) creates such an engine."""
    h, w = 130, 500
    try:
        e = pkg.Engine(h, w, device=0, word_planes=4, streams=1)
    except pkg.GolError as err:
        assert err.status == pkg.GOL_EINVAL
        pytest.skip("the loaded library has no 4-plane kernels")
    rng = np.random.default_rng(4)
    with e:
        e.init_random(6)
        bits = torus_ref.unpack(e.store_packed(), w)
        for y, x, rh, rw in ((0, 0, h, w), (3, 31, 100, 129), (7, 65, 5, 63), (9, 127, 3, 130),
                             (h - 1, w - 1, 1, 1)):
            assert (e.read_rect(y, x, rh, rw) == crop(bits, y, x, rh, rw)).all()
            for op in range(4):
                win = rng.integers(0, 2, (rh, rw), dtype=np.uint8)
                e.write_rect(y, x, junk_window(rng, win), rw, op)
                bits = apply(bits, y, x, win, op)
                assert (e.store_packed() == torus_ref.pack(bits)).all(), (y, x, rh, rw, op)
            for by, bx in ((1, 1), (8, 8), (16, 100), (64, 128), (h, w)):
                got = e.density(y, x, rh, rw, by, bx)
                assert (got == block_sums(bits[y:y + rh, x:x + rw], by, bx)).all()
