"""GPU: the auxiliary kernels past their grid caps and first tile column -- region
I/O, density, the ASCII codec, the torus wrap and the snapshot compare at the smallest
shapes at which their grid-stride loops take a second trip, density forms several
column chunks, and rect_stage goes to a transient buffer.

The shapes, the cells planted and the reason each is large enough are in
tests/aux_cases.py; tests/test_aux_caps.py checks them on the CPU against the caps in
the sources.  Every expectation comes from numpy on fields the test builds itself or
from the CPU oracle (bp_random, bp_run; torus_ref for tori), never from the engine.
"""
import numpy as np
import pytest

import aux_cases as ac
import torus_ref

pytestmark = pytest.mark.gpu

CONWAY = (1 << 3, (1 << 2) | (1 << 3))
ONE = np.ones((1, 1), dtype=np.uint64)


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words, dtype=np.uint64).view(np.uint8)).sum())


def random_window(rng, rh, rw):
    """(cells, packed window whose bits beyond rw are junk that must be ignored)."""
    words = rng.integers(0, 1 << 64, (rh, ac.cdiv(rw, 64)), dtype=np.uint64)
    return torus_ref.unpack(words, rw), words


def crop(bits, y, x, rh, rw):
    """The window's cells; indices wrap (a no-op inside the field)."""
    h, w = bits.shape
    if y + rh <= h and x + rw <= w:
        return bits[y:y + rh, x:x + rw]
    return bits[np.ix_((y + np.arange(rh)) % h, (x + np.arange(rw)) % w)]


def paste(bits, y, x, win, op):
    """bits with the cells `win` combined at (y, x) (RECT_SET or RECT_XOR), wrapping."""
    h, w = bits.shape
    out = bits.copy()
    for r0, r1, s0 in wrap_runs(y, win.shape[0], h):
        for c0, c1, t0 in wrap_runs(x, win.shape[1], w):
            blk = win[s0:s0 + r1 - r0, t0:t0 + c1 - c0]
            if op == 0:
                out[r0:r1, c0:c1] = blk
            else:
                out[r0:r1, c0:c1] ^= blk
    return out


def wrap_runs(start, n, period):
    """[start, start + n) modulo period, n <= period, as (lo, hi, offset into the
    window) runs: one, or two where the range crosses the seam."""
    first = min(n, period - start)
    return [(start, start + first, 0)] + ([(0, n - first, first)] if n > first else [])


def block_sums(bits, by, bx):
    """Live cells per by x bx block: columns first, so the row pass sees few columns."""
    cols = np.add.reduceat(bits, np.arange(0, bits.shape[1], bx), axis=1, dtype=np.uint32)
    return np.add.reduceat(cols, np.arange(0, bits.shape[0], by), axis=0, dtype=np.uint32)


def flip_each(pkg, e, cells):
    """One-cell flips, one at a time: each is seen by `same`, counted once by `diff`,
    and gone after the flip back."""
    for y, x in cells:
        e.write_rect(y, x, ONE, 1, pkg.RECT_XOR)
        assert e.snapshot_diff() == 1, (y, x)
        assert e.snapshot_same() is False, (y, x)
        e.write_rect(y, x, ONE, 1, pkg.RECT_XOR)
        assert e.snapshot_diff() == 0, (y, x)
        assert e.snapshot_same() is True, (y, x)


def test_snapshot_compare_second_trip(pkg, oracle):
    """Case 1: 12,302 tiles on one leaf, 8,192 per trip of life_snap_diff_kernel."""
    s = ac.SNAP
    h, w = s.h, s.w
    rng = np.random.default_rng(1)
    a = oracle.bp_random(h, w, 51)
    with pkg.Engine(h, w, rule=CONWAY, device=0, **s.kw) as e:
        assert e.timing()["streams"] == 1, \
            "two stripes stay under the diff kernel's cap: enlarge the case (aux_cases.py)"
        e.load_packed(a)
        e.snapshot()
        assert e.snapshot_same() is True and e.snapshot_diff() == 0
        flip_each(pkg, e, [cell for _, cell in s.flips])
        # all of them at once: a flip in either trip counts once
        for _, (y, x) in s.flips:
            e.write_rect(y, x, ONE, 1, pkg.RECT_XOR)
        assert e.snapshot_diff() == len(s.flips)
        for _, (y, x) in s.flips:
            e.write_rect(y, x, ONE, 1, pkg.RECT_XOR)
        assert e.snapshot_diff() == 0
        # a window of second-trip tiles only: the first trip's contribute nothing
        y, x, rh, rw = s.second_trip_window
        win, words = random_window(rng, rh, rw)
        e.write_rect(y, x, words, rw, pkg.RECT_XOR)
        assert e.snapshot_diff() == int(win.sum(dtype=np.uint64)) > 0
        assert e.snapshot_same() is False
        b = oracle.bp_random(h, w, 52)
        e.load_packed(b)
        assert e.snapshot_diff() == popcount(a ^ b)
        assert e.snapshot_same() is False
        e.snapshot_restore()
        assert (e.store_packed() == a).all()
        assert e.snapshot_diff() == 0 and e.snapshot_same() is True


@pytest.fixture(scope="module")
def rect_field(oracle):
    """Cases 2 and 3: (packed words, cells) of the start field; read only."""
    r = ac.RECT
    words = oracle.bp_random(r.h, r.w, 53)
    bits = torus_ref.unpack(words, r.w)
    words.setflags(write=False)
    bits.setflags(write=False)
    return words, bits


@pytest.mark.parametrize("kind", list(ac.RECT.kinds))
def test_rect_read_write_second_trip(pkg, oracle, rect_field, kind):
    """Case 2: windows of more than 2,097,152 words and lane groups."""
    r = ac.RECT
    h, w = r.h, r.w
    torus = kind == "torus"
    start, bits = rect_field
    rng = np.random.default_rng(2)
    y, x, rh, rw = r.torus_window if torus else r.window
    with pkg.Engine(h, w, rule=CONWAY, device=0, **r.kinds[kind]) as e:
        e.load_packed(start)
        got = e.read_rect(y, x, rh, rw)
        assert (got == torus_ref.pack(crop(bits, y, x, rh, rw))).all()
        if torus:  # and the window inside the field, as the dead-border engine's
            yy, xx, hh, ww = r.window
            assert (e.read_rect(yy, xx, hh, ww) == torus_ref.pack(crop(bits, yy, xx, hh, ww))).all()
        for op in (pkg.RECT_SET, pkg.RECT_XOR):
            win, words = random_window(rng, rh, rw)
            e.write_rect(y, x, words, rw, op)
            bits = paste(bits, y, x, win, op)
            want = torus_ref.pack(bits)
            # every word of the field: those outside the window too
            assert (e.store_packed() == want).all(), op
        # an edit made in the second trip is what the stencil sees
        e.step(1)
        if torus:
            want = torus_ref.torus_run(oracle, want, w, 1, CONWAY)
        else:
            want = oracle.bp_run(want, w, 1, CONWAY)
        assert (e.store_packed() == want).all()


@pytest.mark.parametrize("kind", list(ac.RECT.kinds))
def test_density_chunks_and_second_trip(pkg, rect_field, kind):
    """Case 3: more than 64 lane groups per row (several column chunks per block row),
    and with 1-row blocks more than 32,768 wavefront items."""
    r = ac.RECT
    h, w = r.h, r.w
    torus = kind == "torus"
    start, bits = rect_field
    live = int(bits.sum(dtype=np.uint64))
    with pkg.Engine(h, w, rule=CONWAY, device=0, **r.kinds[kind]) as e:
        e.load_packed(start)
        assert e.digest()[0] == live
        for y, x, rh, rw in ((0, 0, h, w), r.window):
            sub = crop(bits, y, x, rh, rw)
            for by, bx in r.blocks:
                got = e.density(y, x, rh, rw, by, bx)
                want = block_sums(sub, by, bx)
                assert got.dtype == np.uint32 and got.shape == want.shape
                assert (got == want).all(), (y, x, rh, rw, by, bx)
                if (rh, rw) == (h, w):
                    assert int(got.sum(dtype=np.uint64)) == e.digest()[0] == live
        if torus:
            y, x, rh, rw = r.torus_window
            by, bx = r.seam_block
            got = e.density(y, x, rh, rw, by, bx)
            assert (got == block_sums(crop(bits, y, x, rh, rw), by, bx)).all()


def test_transient_staging(pkg, oracle):
    """Case 4: a window and a count array above rect_stage's 64 MiB, each call twice,
    then a small read through the kept buffer.  References on packed words."""
    s = ac.STAGE
    h, w = s.h, s.w
    wq = ac.cdiv(w, 64)
    rng = np.random.default_rng(4)
    a = oracle.bp_random(h, w, 54)
    with pkg.Engine(h, w, rule=CONWAY, device=0) as e:
        e.load_packed(a)
        ys, xs, hs, ws = s.small
        small = ac.packed_window(a, ys, xs, hs, ws)
        assert (e.read_rect(ys, xs, hs, ws) == small).all()  # (the kept buffer exists)
        y, x, rh, rw = s.window
        want = ac.packed_window(a, y, x, rh, rw)
        for _ in range(2):
            assert (e.read_rect(y, x, rh, rw) == want).all()
        win = rng.integers(0, 1 << 64, (rh, ac.cdiv(rw, 64)), dtype=np.uint64)  # junk beyond rw
        edited = a.copy()
        edited[y:y + rh] ^= ac.placed_window(win, x, rw, wq)
        e.write_rect(y, x, win, rw, pkg.RECT_XOR)
        assert (e.store_packed() == edited).all()
        e.write_rect(y, x, win, rw, pkg.RECT_XOR)
        assert (e.store_packed() == a).all()
        y, x, rh, rw, by, bx = s.density
        corner = torus_ref.unpack(ac.packed_window(a, y, x, rh, rw), rw)
        for _ in range(2):
            got = e.density(y, x, rh, rw, by, bx)
            assert got.shape == (rh, rw) and (got == corner).all()
        assert (e.read_rect(ys, xs, hs, ws) == small).all()


def ascii_text(bits):
    """'0'/'1' per cell and a '\\n' per row."""
    h, w = bits.shape
    t = np.full((h, w + 1), ord("\n"), dtype=np.uint8)
    t[:, :w] = bits + ord("0")
    return t.tobytes()


def first_diff(got, want):
    """None if the two texts are equal, else the offset of the first difference (-1: the
    lengths differ).  The texts have megabytes: a failing `got == want` would leave
    pytest rendering their diff for minutes."""
    if got == want:
        return None
    if len(got) != len(want):
        return -1
    return int(np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))[0])


def test_ascii_codec_second_trip(pkg, oracle):
    """Case 5: 71,500 (row, lane group) items, 65,536 wavefronts per trip."""
    c = ac.ASCII
    h, w = c.h, c.w
    g = oracle.bp_random(h, w, 55)
    bits = torus_ref.unpack(g, w)
    data = ascii_text(bits)
    with pkg.Engine(h, w, rule=CONWAY, device=0, **c.kw) as e:
        e.load_ascii(data)
        assert (e.store_packed() == g).all()
        assert first_diff(e.store_ascii(), data) is None
        e.step(3)
        later = oracle.bp_run(g, w, 3, CONWAY)
        assert first_diff(e.store_ascii(), ascii_text(torus_ref.unpack(later, w))) is None
        # a line end that is not '\n', checked by a second-trip item
        bad = bytearray(data)
        bad[c.bad_row * (w + 1) + w] = ord("1")
        with pytest.raises(pkg.GolError) as ei:
            e.load_ascii(bytes(bad))
        assert ei.value.status == pkg.GOL_EINVAL
        # non-random content stored by the second trip: rows of ones to the last mask
        full = bits.copy()
        full[c.ones_from:] = 1
        e.load_ascii(ascii_text(full))
        got = e.store_packed()
        assert (got == torus_ref.pack(full)).all()
        assert (got[c.ones_from:, :-1] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
        assert (got[c.ones_from:, -1] == np.uint64((1 << (w % 64)) - 1)).all()
        assert first_diff(e.store_ascii(), ascii_text(full)) is None


def test_torus_wrap_second_trip(pkg, oracle):
    """Case 6: 2,101,824 ghost and side words, 2,097,152 threads per trip: the wrap at
    load, a full round of 256 generations, a second wrap and one more generation."""
    c = ac.WRAP
    h, w = c.h, c.w
    geo = pkg.torus_geometry(h, w, halo_depth=c.kw["halo_depth"])
    assert geo["ghost_rows"] == c.ghost_rows and geo["ghost_words"] == c.ghost_words
    start = oracle.bp_random(h, w, 56)
    with pkg.Engine(h, w, rule=CONWAY, device=0, **c.kw) as e:
        assert e.halo_depth == c.ghost_rows
        e.load_packed(start)
        e.step(1)
        assert (e.store_packed() == torus_ref.torus_run(oracle, start, w, 1, CONWAY)).all()
        e.load_packed(start)
        e.snapshot()
        e.step(c.ghost_rows + 1)
        want = torus_ref.torus_run(oracle, start, w, c.ghost_rows + 1, CONWAY)
        assert (e.store_packed() == want).all()
        # the torus view of the compare (8 x 64 tiles: one trip; aux_cases.py)
        assert e.snapshot_diff() == popcount(start ^ want) > 0
        assert e.snapshot_same() is False
        y, x, rh, rw = c.corner
        bits = torus_ref.unpack(want, w)
        assert (e.read_rect(y, x, rh, rw) == torus_ref.pack(crop(bits, y, x, rh, rw))).all()


def test_composite_snapshot_second_trip(pkg, oracle):
    """Case 7: two stripes of 12,302 tiles each: flips on both sides of the stripe
    boundary and in either leaf's second trip."""
    c = ac.COMPOSITE
    h, w = c.h, c.w
    n = c.kw["streams"]
    starts = [pkg.rank_rows(h, n, r)[0] for r in range(n)]
    cells = [cell for _, _, cell in ac.composite_flips(h, w, starts)]
    a = oracle.bp_random(h, w, 57)
    with pkg.Engine(h, w, rule=CONWAY, device=0, **c.kw) as e:
        assert e.timing()["streams"] == n
        e.load_packed(a)
        e.snapshot()
        assert e.snapshot_same() is True and e.snapshot_diff() == 0
        flip_each(pkg, e, cells)
        for k, (y, x) in enumerate(cells):
            e.write_rect(y, x, ONE, 1, pkg.RECT_XOR)
            assert e.snapshot_diff() == k + 1, (y, x)
        assert e.snapshot_same() is False
        e.snapshot_restore()
        assert (e.store_packed() == a).all()
        assert e.snapshot_diff() == 0 and e.snapshot_same() is True


def test_batch_codec_second_trip(pkg):
    """Case 8: a batch of 2,361,600 words, 2,097,152 per trip of batch_load_kernel,
    batch_store_kernel and batch_init_random_kernel; the trips' border lies in row 56 of
    field 3,640."""
    import batch_lattice as bl
    import batch_ref

    c = ac.BATCH_CODEC
    n, h, w = c.n, c.h, c.w
    wq = ac.cdiv(w, 64)
    rng = np.random.default_rng(8)
    with pkg.BatchEngine(n, h, w, rule=CONWAY, device=0) as b:
        assert b.lanes_per_field == 16 and b.fields_per_wave == 4
        # init_random: every field, against the synthetic field's numpy restatement
        # (test_batch_lattice_host.py pins it to the oracle)
        b.init_random(c.seed)
        start = bl.synthetic_fields(0, n, h, w, c.seed)
        got = b.store_packed()
        bad = np.argwhere((got != start).any(axis=(1, 2))).ravel()
        assert bad.size == 0, bad[:8].tolist()
        # sub-range stores: one trip across field 3,640, and one of two trips of its own
        for first, count in (c.sub, c.sub_trip):
            part = b.store_packed(first, count)
            bad = np.argwhere((part != start[first:first + count]).any(axis=(1, 2))).ravel()
            assert bad.size == 0, (first, count, bad[:8].tolist())
        # step: the sampled fields alone (the fields are independent)
        sample = sorted({0, n - 1, *c.boundary,
                         *rng.choice(n, c.sampled_others, replace=False).tolist()})
        want = batch_ref.pack(batch_ref.run(batch_ref.unpack(start[sample], w), c.gens, CONWAY))
        b.step(c.gens)
        after = b.store_packed()
        assert (after[sample] == want).all(), \
            [sample[i] for i in np.argwhere((after[sample] != want).any(axis=(1, 2))).ravel()[:8]]
        # load: all fields, junk at the columns >= w of every row's last word and in a
        # spare word per row
        words = rng.integers(0, 1 << 64, (n, h, wq + 1), dtype=np.uint64)
        clean = words[:, :, :wq].copy()
        clean[:, :, -1] &= bl.last_mask(w)
        b.load_packed(words)
        got = b.store_packed()
        bad = np.argwhere((got != clean).any(axis=(1, 2))).ravel()
        assert bad.size == 0, bad[:8].tolist()
        # a sub-range load of two trips of its own, into the middle of the batch
        first, count = c.sub_trip
        b.load_packed(start[first:first + count], first=first)
        clean[first:first + count] = start[first:first + count]
        assert (b.store_packed() == clean).all()


def test_batch_digest_second_trip(pkg):
    """Case 9: 33,000 fields, 32,768 wavefronts per trip of batch_digest_kernel."""
    import batch_lattice as bl

    c = ac.BATCH_DIGEST
    n, h, w = c.n, c.h, c.w
    with pkg.BatchEngine(n, h, w, rule=CONWAY, device=0) as b:
        b.init_random(c.seed)
        fields = bl.synthetic_fields(0, n, h, w, c.seed)
        assert (b.store_packed() == fields).all()
        want_live, want_hash = bl.digests(fields)
        live, hsh = b.digest()
        bad = np.flatnonzero((live != want_live) | (hsh != want_hash))
        assert bad.size == 0, bad[:8].tolist()
        first, count = c.sub
        live, hsh = b.digest(first, count)
        assert live.tolist() == want_live[first:first + count].tolist()
        assert hsh.tolist() == want_hash[first:first + count].tolist()
        # after a step the digests follow the fields
        import batch_ref
        b.step(1)
        live, hsh = b.digest()
        after = batch_ref.pack(batch_ref.run(batch_ref.unpack(fields, w), 1, CONWAY))
        assert (b.store_packed() == after).all()
        want_live, want_hash = bl.digests(after)
        assert live.tolist() == want_live.tolist() and hsh.tolist() == want_hash.tolist()
