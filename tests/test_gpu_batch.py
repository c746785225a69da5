"""GPU suite: gol_batch (BatchEngine) -- every field of every case, word for word,
against batch_ref's plain numpy, which test_batch_host.py pins to rule_ref.numpy_run
and torus_ref.roll_run."""
import numpy as np
import pytest

import batch_ref
import rule_ref

pytestmark = pytest.mark.gpu

B36S23 = (0b1001000, 0b1100)
B0 = (1, 0)  # a dead cell without neighbours is born: lights every unmasked row or column
# (rule, density of the random start)
RULE_CASES = [(rule_ref.REF_RULE, 0.5), (rule_ref.REF_RULE, 0.15), (rule_ref.CONWAY, 0.5),
              (B36S23, 0.5), (B0, 0.5), (rule_ref.FLOOD, 0.5)]
GENS = (1, 2, 3, 37)
SHAPES = [(64, 64, 130), (5, 7, 3), (8, 64, 65), (9, 65, 33), (17, 130, 17), (33, 200, 5),
          (64, 4096, 2), (16, 16, 300), (1, 1, 2), (1, 64, 2), (64, 1, 2), (2, 2, 2)]


def sem_of(pkg, torus):
    return pkg.SEM_TORUS if torus else pkg.SEM_GLOBAL


def stepped(pkg, words, h, w, gens, rule, torus):
    n = words.shape[0]
    with pkg.BatchEngine(n, h, w, rule=rule, device=0, semantics=sem_of(pkg, torus)) as b:
        b.load_packed(words)
        b.step(gens)
        return b.store_packed()


@pytest.mark.parametrize("torus", [False, True], ids=["dead", "torus"])
@pytest.mark.parametrize("h,w,n", SHAPES)
def test_batch_matches_reference(pkg, h, w, n, torus):
    for ci, (rule, p) in enumerate(RULE_CASES):
        cells = batch_ref.random_batch(n, h, w, seed=1000 * ci + h + w, p=p)
        start = batch_ref.pack(cells)
        with pkg.BatchEngine(n, h, w, rule=rule, device=0, semantics=sem_of(pkg, torus)) as b:
            ref, done = cells, 0
            for g in GENS:
                ref, done = batch_ref.run(ref, g - done, rule, torus), g
                b.load_packed(start)
                b.step(g)
                got = b.store_packed()
                want = batch_ref.pack(ref)
                bad = np.argwhere((got != want).any(axis=(1, 2))).ravel()
                assert bad.size == 0, (rule_ref.rule_name(rule), p, g, bad[:8].tolist())


@pytest.mark.parametrize("torus", [False, True], ids=["dead", "torus"])
@pytest.mark.parametrize("h,w,n", [(64, 64, 130), (17, 130, 17)])
def test_batch_fields_are_isolated(pkg, h, w, n, torus):
    """One full field in the middle of a wavefront, every other field empty, under
    FLOOD: a lane move that crosses a field's edge, or a row that leaks, lights a
    neighbour."""
    fpw = pkg.batch_geometry(n, h, w)["fields_per_wave"]
    mid = fpw // 2
    cells = np.zeros((n, h, w), dtype=np.uint8)
    cells[mid] = 1
    got = stepped(pkg, batch_ref.pack(cells), h, w, 40, rule_ref.FLOOD, torus)
    want = batch_ref.pack(batch_ref.run(cells, 40, rule_ref.FLOOD, torus))
    assert (got[mid] == want[mid]).all()
    others = np.delete(got, mid, axis=0)
    assert not others.any(), np.argwhere(others.any(axis=(1, 2))).ravel()[:8].tolist()


@pytest.mark.parametrize("torus", [False, True], ids=["dead", "torus"])
def test_batch_launch_split(pkg, monkeypatch, torus):
    h, w, n = 17, 130, 17
    cells = batch_ref.random_batch(n, h, w, seed=77)
    start = batch_ref.pack(cells)
    want = batch_ref.pack(batch_ref.run(cells, 13, rule_ref.CONWAY, torus))
    whole = stepped(pkg, start, h, w, 13, rule_ref.CONWAY, torus)
    monkeypatch.setenv("GOL_DEV_BATCH_LAUNCH_GENS", "5")
    with pkg.BatchEngine(n, h, w, rule=rule_ref.CONWAY, device=0, semantics=sem_of(pkg, torus)) as b:
        assert b.info["launch_generations"] == 5 and b.launch_generations == 5
        b.load_packed(start)
        b.step(13)
        split = b.store_packed()
        b.load_packed(start)
        b.step(4)
        b.step(9)
        two = b.store_packed()
    assert (whole == want).all() and (split == want).all() and (two == want).all()


def test_batch_default_launch_cap(pkg):
    with pkg.BatchEngine(3, 5, 7, device=0) as b:
        assert b.info == {"n": 3, "h": 5, "w": 7, "lanes_per_field": 1, "fields_per_wave": 64,
                          "rows_in_regs": 8, "launch_generations": 4096}


def test_batch_io_round_trip_padded_strides_and_subranges(pkg):
    h, w, n = 9, 65, 7
    wq = 2
    rng = np.random.default_rng(5)
    cells = batch_ref.random_batch(n, h, w, seed=6)
    clean = batch_ref.pack(cells)
    # padded strides: 3 words per row, 2 spare rows per field, junk in every spare word
    # and at the columns >= w of the last word
    padded = rng.integers(0, 2 ** 63, size=(n, h + 2, 3), dtype=np.uint64)
    padded[:, :h, :wq] = clean
    padded[:, :h, wq - 1] |= np.uint64(0xFFFFFFFFFFFFFFFE)  # columns 65..127
    L = pkg.lib()
    with pkg.BatchEngine(n, h, w, device=0) as b:
        assert L.gol_batch_load_packed(b._h, 0, n, padded.ctypes.data, (h + 2) * 3, 3) == pkg.GOL_OK
        assert (b.store_packed() == clean).all()  # junk ignored, stored as 0
        out = np.full((n, h + 2, 3), np.uint64(0xABCD), dtype=np.uint64)
        assert L.gol_batch_store_packed(b._h, 0, n, out.ctypes.data, (h + 2) * 3, 3) == pkg.GOL_OK
        assert (out[:, :h, :wq] == clean).all()
        assert (out[:, h:, :] == 0xABCD).all() and (out[:, :, wq:] == 0xABCD).all()
        # a sub-range: fields 3 and 4 replaced, the others unchanged
        new = batch_ref.pack(batch_ref.random_batch(2, h, w, seed=8))
        b.load_packed(new, first=3)
        want = clean.copy()
        want[3:5] = new
        assert (b.store_packed() == want).all()
        assert (b.store_packed(first=3, count=2) == new).all()
        assert b.store_packed(first=7, count=0).shape == (0, h, wq)
        # bad ranges and short strides
        buf = np.zeros((n, h, wq), dtype=np.uint64)
        for first, count, fs, rs in ((6, 2, h * wq, wq), (8, 0, h * wq, wq), (0, n, h * wq, wq - 1),
                                     (0, n, h * wq - 1, wq)):
            for fn in (L.gol_batch_load_packed, L.gol_batch_store_packed, L.gol_batch_load_device,
                       L.gol_batch_store_device):
                assert fn(b._h, first, count, buf.ctypes.data, fs, rs) == pkg.GOL_EINVAL
                assert L.gol_last_error()
        with pytest.raises(pkg.GolError):
            b.digest(first=6, count=2)
        assert (b.store_packed() == want).all()


def test_batch_tensor_path_equals_packed_path(pkg):
    torch = pytest.importorskip("torch")
    h, w, n = 33, 200, 5
    start = batch_ref.pack(batch_ref.random_batch(n, h, w, seed=9))
    want = stepped(pkg, start, h, w, 7, rule_ref.CONWAY, False)
    t = torch.from_numpy(start.view(np.int64)).to("cuda:0")
    with pkg.BatchEngine(n, h, w, rule=rule_ref.CONWAY, device=0) as b:
        b.load_tensor(t)
        b.step(7)
        out = b.store_tensor()
        part = b.store_tensor(first=1, count=2)
    assert out.is_cuda and out.dtype == torch.int64 and tuple(out.shape) == (n, h, 4)
    assert (out.cpu().numpy().view(np.uint64) == want).all()
    assert (part.cpu().numpy().view(np.uint64) == want[1:3]).all()


@pytest.mark.parametrize("torus", [False, True], ids=["dead", "torus"])
@pytest.mark.parametrize("h,w", [(64, 64), (33, 200), (17, 130)])
def test_batch_against_single_field_engines(pkg, oracle, h, w, torus):
    n, seed, gens = 3, 41, 37
    sem = sem_of(pkg, torus)
    with pkg.BatchEngine(n, h, w, rule=rule_ref.CONWAY, device=0, semantics=sem) as b:
        b.init_random(seed)
        start = b.store_packed()
        b.step(gens)
        live, hsh = b.digest()
        one_live, one_hsh = b.digest(first=1, count=1)
    ref = batch_ref.pack(batch_ref.run(batch_ref.unpack(start, w), gens, rule_ref.CONWAY, torus))
    for i in range(n):
        with pkg.Engine(h, w, rule=rule_ref.CONWAY, device=0, semantics=sem) as e:
            e.init_random(seed + i)
            assert (e.store_packed() == start[i]).all(), i
            e.step(gens)
            dig = e.digest()
        assert (int(live[i]), int(hsh[i])) == dig, i
        assert dig == oracle.bp_digest(ref[i], w), i
    assert (int(one_live[0]), int(one_hsh[0])) == (int(live[1]), int(hsh[1]))
