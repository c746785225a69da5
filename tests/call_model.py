"""The public calls of an engine as a numpy model, and seeded programs of such calls.

Host only: neither the package nor pytest is imported here.  test_call_model_host.py
checks the model against plain references and the generator against its floors;
test_gpu_call_sequences.py sends the programs through engines.

Model        the contract of include/gol.h on a uint8 [h, w] cell array: steps by the
             CPU oracle (torus_ref's recipe on a torus), loads, rectangle writes and
             reads, densities, digests, the snapshot slot and step-until-periodic as
             the header words it.  It knows nothing of the engines' remembered state
             (streaks, twin[], pending fixed steps, captured graphs): the field is the
             contract, and a stale flag shows as a wrong field.
draw_program one program: a list of ops, 4-6 phrases of "settle and look, quiet
             steps, one point call, a step".  Ops are tuples of names and numbers, so
             a failing program prints as it ran (format_ops).
run_op       one op on a Model: the model's answer and a record for program_facts.
program_facts what a program reached, from the model alone: steps that start on a
             fixed point the host has seen, runs of them, writers onto such a point.
"""
import numpy as np

import torus_ref

RECT_SET, RECT_OR, RECT_XOR, RECT_CLEAR = range(4)
OP_NAMES = ["SET", "OR", "XOR", "CLEAR"]
REF_RULE = (0, 1 << 2)
CONWAY = (1 << 3, (1 << 2) | (1 << 3))
HIGHLIFE = ((1 << 3) | (1 << 6), (1 << 2) | (1 << 3))
RULE_NAMES = {REF_RULE: "B/S2", CONWAY: "B3/S23", HIGHLIFE: "B36/S23"}

WINDOWS = {
    "block": np.ones((2, 2), dtype=np.uint8),
    "blinker": np.ones((1, 3), dtype=np.uint8),
    "glider": np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]], dtype=np.uint8),
    "eraser": np.ones((5, 5), dtype=np.uint8),
    "bar": np.ones((4, 70), dtype=np.uint8),  # B/S2 only: spans two words wherever it lies
}

WRITERS = ("write", "rewrite", "load", "load_ascii", "init_random", "restore", "until")
READERS = ("store", "digest", "digest_rows", "read", "density", "same", "diff", "until")


# ---- the model


def block_sums(bits, by, bx):
    rows = np.add.reduceat(bits.astype(np.uint32), np.arange(0, bits.shape[0], by), axis=0)
    return np.add.reduceat(rows, np.arange(0, bits.shape[1], bx), axis=1).astype(np.uint32)


class Model:
    def __init__(self, oracle, cells, rule, torus=False):
        self.oracle, self.rule, self.torus = oracle, rule, torus
        self.cells = np.array(cells, dtype=np.uint8)
        assert self.cells.ndim == 2
        self.h, self.w = self.cells.shape
        self.slot = None  # the snapshot slot: None = no snapshot
        self._fixed = None

    # the rule

    def run(self, cells, g):
        """`cells` after g generations; the model's field is left alone."""
        if g == 0:
            return cells.copy()
        words = torus_ref.pack(cells)
        if self.torus:
            out = torus_ref.torus_run(self.oracle, words, self.w, g, self.rule, chunk=64)
        else:
            out = self.oracle.bp_run(words, self.w, g, self.rule)
        return torus_ref.unpack(out, self.w)

    def _set(self, cells):
        self.cells = np.array(cells, dtype=np.uint8)
        assert self.cells.shape == (self.h, self.w)
        self._fixed = None

    def step(self, g):
        if g:
            self._set(self.run(self.cells, g))

    def is_fixed(self):
        if self._fixed is None:
            self._fixed = bool((self.run(self.cells, 1) == self.cells).all())
        return self._fixed

    # writers

    def load(self, cells):
        self._set(cells)

    def init_random(self, seed):
        self._set(torus_ref.unpack(self.oracle.bp_random(self.h, self.w, seed), self.w))

    def _index(self, y, x, rh, rw):
        if self.torus:
            assert y < self.h and x < self.w and rh <= self.h and rw <= self.w
            return np.ix_((y + np.arange(rh)) % self.h, (x + np.arange(rw)) % self.w)
        assert y + rh <= self.h and x + rw <= self.w
        return np.ix_(y + np.arange(rh), x + np.arange(rw))

    def write_rect(self, y, x, win, op):
        win = np.asarray(win, dtype=np.uint8)
        ix = self._index(y, x, win.shape[0], win.shape[1])
        d = self.cells[ix]
        out = self.cells.copy()
        out[ix] = (win, d | win, d ^ win, d & (1 - win))[op]
        self._set(out)

    # readers

    def window(self, y, x, rh, rw):
        return self.cells[self._index(y, x, rh, rw)]

    def read_rect(self, y, x, rh, rw):
        return torus_ref.pack(self.window(y, x, rh, rw))

    def density(self, y, x, rh, rw, by, bx):
        return block_sums(self.window(y, x, rh, rw), by, bx)

    def packed(self):
        return torus_ref.pack(self.cells)

    def digest(self):
        return tuple(self.oracle.bp_digest(self.packed(), self.w))

    def digest_rows(self, row0, rows):
        """The digest's terms of rows [row0, row0 + rows): a word's term depends on the
        word and its index alone, so two prefixes' digests differ by it."""
        g = self.packed()
        la, ha = self.oracle.bp_digest(g[:row0 + rows], self.w) if row0 + rows else (0, 0)
        lb, hb = self.oracle.bp_digest(g[:row0], self.w) if row0 else (0, 0)
        return la - lb, (ha - hb) & 0xFFFFFFFFFFFFFFFF

    # the snapshot slot

    def snapshot(self):
        self.slot = self.cells.copy()

    def same(self):
        return bool((self.cells == self.slot).all())

    def diff(self):
        return int((self.cells != self.slot).sum())

    def restore(self):
        self._set(self.slot)

    def until_periodic(self, max_generations, lag, check_every=0, finish=False):
        """include/gol.h, gol_step_until_periodic: checks at g = c * check_every; the
        field of generation g - lag is kept in the slot and compared with generation
        g's; at the first equal pair the minimal period is found by stepping on through
        lag's proper divisors in ascending order, and generation g's field is restored;
        a check that would lie beyond max_generations is not made, the rest is run and
        the period is 0.  The slot holds what the last check left in it (no check: the
        header does not say, and the model's slot is None)."""
        assert 1 <= lag <= 65536
        every = check_every or -(-lag // 64) * 64
        assert every >= lag
        g = checks = period = extra = 0
        cur = self.cells
        kept = None
        while g + every <= max_generations:
            kept = self.run(cur, every - lag)
            cur = self.run(kept, lag)
            g += every
            checks += 1
            if (kept == cur).all():
                period, walk, at = lag, cur, 0
                for d in (d for d in range(1, lag) if lag % d == 0):
                    walk = self.run(walk, d - at)
                    at = d
                    if (walk == cur).all():
                        period = d
                        break
                extra = at
                break
        else:
            cur = self.run(cur, max_generations - g)
            g = max_generations
        self.slot = kept
        if finish and period:
            cur = self.run(cur, (max_generations - g) % period)
        self._set(cur)
        return dict(period=period, advanced=g, checks=checks, extra_generations=extra, lag=lag,
                    check_every=every, field=self.cells.copy(),
                    slot=None if kept is None else kept.copy())


# ---- start fields and loads: small descriptions, made into cells by make_field


def lattice_cols(w):
    return sorted({min(100, w // 4), w // 2, w - 40})


def lattice_rows(h):
    return list(range(20, h - 2, 64))


def lattice(h, w, gliders=()):
    """2 x 2 blocks every 64 rows in three columns (test_gpu_twin.blocks' kind of
    field), still under B3/S23 and B36/S23, and gliders at the given cells."""
    g = np.zeros((h, w), dtype=np.uint8)
    for r in lattice_rows(h):
        for c in lattice_cols(w):
            g[r:r + 2, c:c + 2] = 1
    for r, c in gliders:
        g[r:r + 3, c:c + 3] |= WINDOWS["glider"]
    return g


def make_field(oracle, desc, h, w):
    if desc[0] == "soup":
        _, p, seed = desc
        return (np.random.default_rng(seed).random((h, w)) < p).astype(np.uint8)
    if desc[0] == "random":  # gol_init_random's field
        return torus_ref.unpack(oracle.bp_random(h, w, desc[1]), w)
    assert desc[0] == "lattice"
    return lattice(h, w, desc[1])


def draw_field(rnd, h, w, rule):
    if rule == REF_RULE:
        return ("soup", rnd.choice([0.02, 0.12, 0.5]), rnd.randint(1, 1 << 30))
    n = rnd.choice([0, 0, 1, 1, 2])
    gliders = []
    for _ in range(n):
        # between the lattice's columns, where it flies freely for a while; half of them
        # near the bottom, where the dead border turns them into a still life soon
        cols = lattice_cols(w)
        c = rnd.randint(cols[0] + 8, max(cols[0] + 9, cols[-1] - 12))
        r = rnd.randint(max(0, h - 40), h - 8) if rnd.random() < 0.5 else rnd.randint(0, h - 8)
        gliders.append((r, c))
    return ("lattice", tuple(gliders))


# ---- where windows go


def hot_coordinates(h, w, rects=None, tile_rows=8, stripes=()):
    """The coordinates at which the engines' bookkeeping has an edge: the field's first
    and last row and column, the copy and probe tiles' row edges, the plan's unit seams
    (rects: gol_plan_neighbours' rectangles, rows [r0, r1) x lane groups [q0, q1)), the
    word seam at 63/64, the ragged last word's first column, the stripes' first rows."""
    rows = {"edge": [0, h - 1], "tile": [r for r in range(tile_rows, h, tile_rows)]}
    cols = {"edge": [0, w - 1], "word": [c for c in (63, 64) if c < w]}
    if w % 64 and w > 64:
        cols["ragged"] = [64 * (w // 64)]
    if rects is not None and len(rects):
        rs, cs = set(), set()
        for u in range(rects.shape[0]):
            for r0, r1, q0, q1 in np.asarray(rects[u]).tolist():
                if r1 > r0 and q1 > q0:
                    rs |= {r for r in (r0, r1) if 0 < r < h}
                    cs |= {64 * q for q in (q0, q1) if 0 < 64 * q < w}
        if rs:
            rows["seam"] = sorted(rs)
        if cs:
            cols["seam"] = sorted(cs)
    if stripes:
        rows["stripe"] = [r for r in stripes if 0 < r < h]
    return {"rows": rows, "cols": cols}


def near_hot(coord, hot, tol=2):
    return any(abs(coord - v) <= tol for vs in hot.values() for v in vs)


def _axis(rnd, n, size, hot, use_hot):
    """A window's first coordinate on an axis of n cells: an edge of the window within
    2 cells of a hot coordinate, or uniform."""
    if use_hot and hot:
        v = rnd.choice(hot[rnd.choice(sorted(hot))])
        at = v + rnd.randint(-2, 2) - rnd.choice([0, size - 1, size // 2])
    else:
        at = rnd.randint(0, n - size)
    return min(max(at, 0), n - size)


def draw_position(rnd, h, w, wh, ww, hot, torus):
    wh, ww = min(wh, h), min(ww, w)
    if torus and rnd.random() < 1 / 3:
        # across the bottom edge, the right edge or the corner
        which = rnd.choice(["row", "col", "both"]) if wh > 1 else "col"
        y = h - rnd.randint(1, wh - 1) if which != "col" and wh > 1 else rnd.randint(0, h - wh)
        x = w - rnd.randint(1, ww - 1) if which != "row" and ww > 1 else rnd.randint(0, w - ww)
        return y, x
    if hot and rnd.random() < 0.6:
        both = rnd.random() < 0.5
        first = rnd.random() < 0.5
        return (_axis(rnd, h, wh, hot["rows"], both or first),
                _axis(rnd, w, ww, hot["cols"], both or not first))
    return rnd.randint(0, h - wh), rnd.randint(0, w - ww)


# ---- programs


def length_table(K):
    return [1, K - 4, K, K + 1, 2 * K, 3 * K + 5, 4 * K + 1, 5 * K + 3, 6 * K, 6 * K + 8,
            7 * K + 3, 8 * K + 15]


def ends_with_remainder(g, K):
    return g > K and g % K != 0


def draw_reader(rnd, h, w, hot, torus):
    what = rnd.choice(["store", "digest", "digest_rows", "read", "density"])
    if what == "digest_rows":
        r0 = rnd.randint(0, h - 1)
        return ("digest_rows", r0, rnd.randint(1, h - r0))
    if what in ("read", "density"):
        rh, rw = rnd.choice([(1, 1), (5, 70), (17, 130), (40, min(w, 300))])
        rh, rw = min(rh, h), min(rw, w)
        y, x = draw_position(rnd, h, w, rh, rw, hot, torus)
        if what == "read":
            return ("read", y, x, rh, rw)
        by, bx = rnd.choice([(1, 1), (8, 8), (3, 64), (16, 100)])
        return ("density", y, x, rh, rw, by, bx)
    return (what,)


def draw_write(rnd, h, w, rule, hot, torus):
    if rule != REF_RULE and rnd.random() < 0.15:
        # a block OR-ed onto a block of the lattice: the field stays what it was (where
        # an earlier call has not taken the block away)
        return ("write", rnd.choice(lattice_rows(h)), rnd.choice(lattice_cols(w)), "block", RECT_OR)
    if rnd.random() < 0.12:
        # the window as the model holds it, set again: the field stays what it was
        rh, rw = min(h, 6), min(w, 70)
        y, x = draw_position(rnd, h, w, rh, rw, hot, torus)
        return ("rewrite", y, x, rh, rw)
    names = ["block", "blinker", "glider", "eraser"] + (["bar"] if rule == REF_RULE and w >= 70 else [])
    name = rnd.choice(names)
    op = rnd.choice([RECT_SET, RECT_OR, RECT_XOR, RECT_CLEAR])
    wh, ww = WINDOWS[name].shape
    y, x = draw_position(rnd, h, w, wh, ww, hot, torus)
    return ("write", y, x, name, op)


def draw_program(rnd, K, h, w, rule, kind, hot=None, torus=False):
    """One program for an h x w engine of kernel depth K: (start field, ops).  `kind`
    names the engine kind (skip kinds also look at the activity state's words)."""
    table = length_table(K)
    rem = [g for g in table if ends_with_remainder(g, K)]
    rem_long = [g for g in rem if g >= 5 * K] or rem  # a short step's shape
    start = draw_field(rnd, h, w, rule)
    ops, has_snap = [], False
    still_start = start[0] == "lattice" and not start[1]

    def quiet_length():
        u = rnd.random()
        if u < 0.7:
            return rnd.choice(rem_long if rnd.random() < 0.6 else rem)
        # a short step's shape that ends with a depth-K launch: twin[] is 1 after it
        return 6 * K if u < 0.85 else rnd.choice(table)

    if not still_start and rnd.random() < 0.5:
        # a snapshot of the field in motion: what a later restore brings back
        ops.append(("snapshot",))
        has_snap = True

    phrases = rnd.randint(4, 6)
    # at most once per program, in the place of one phrase's point call
    big_at = rnd.randrange(phrases) if rnd.random() < 0.6 else -1
    big = rnd.choice(["init_random", "load_ascii", "until"])
    for ph in range(phrases):
        # 1. settle and let the host look
        if ph == 0 or rnd.random() < 0.7:
            ops += [("step", rnd.choice(rem)), ("sync",)]
            if rnd.random() < 0.5:
                ops += [("step", rnd.choice(rem)), ("sync",)]
        # 2. quiet steps, no call between them
        for _ in range(rnd.randint(0, 3)):
            ops.append(("step", quiet_length()))
        # 3. one point call
        timed = False
        u = rnd.random()
        if still_start and ph == phrases - 1:
            # a field that starts still moves at least once: a glider, and a step
            y, x = draw_position(rnd, h, w, 3, 3, hot, torus)
            ops.append(("write", y, x, "glider", RECT_OR))
        elif ph == big_at and big == "init_random":
            ops.append(("init_random", rnd.randint(1, 1 << 30)))
        elif ph == big_at and big == "load_ascii":
            ops.append(("load_ascii", draw_field(rnd, h, w, rule)))
        elif ph == big_at:
            lag = rnd.choice([1, 2, 4])
            # (at least one check is made: the slot then holds what the header says)
            ops.append(("until", rnd.choice([64, 100, 200]), lag, rnd.choice([0, lag, 64]),
                        rnd.random() < 0.5))
            has_snap = True
        elif u < 0.35:
            ops.append(draw_write(rnd, h, w, rule, hot, torus))
            if rnd.random() < 0.3:
                # two different writers in a row
                second = rnd.choice(["restore", "load", "write"])
                if second == "restore" and has_snap:
                    ops.append(("restore",))
                elif second == "load":
                    ops.append(("load", draw_field(rnd, h, w, rule)))
                else:
                    ops.append(draw_write(rnd, h, w, rule, hot, torus))
        elif u < 0.45:
            ops.append(("restore",) if has_snap else ("snapshot",))
            has_snap = True
        elif u < 0.55:
            # (a second snapshot would often replace one of motion by one of a still field)
            ops.append(("restore",) if has_snap and rnd.random() < 0.6 else ("snapshot",))
            has_snap = True
        elif u < 0.62:
            ops.append(("load", draw_field(rnd, h, w, rule)))
        elif u < 0.70:
            if has_snap:
                ops += [("same",), ("diff",)][::rnd.choice([1, -1])]
            else:
                ops.append(("snapshot",))
            has_snap = True
        elif u < 0.80:
            names = ["activity", "activity_copied", "activity_probed", "activity_elided",
                     "activity_pass_probed", "activity_pass_kept", "activity_pass_sure"]
            if kind.startswith("skip"):
                names.append("activity_state")
            ops.append(("act", rnd.choice(names)))
        elif u < 0.88:
            if rnd.random() < 0.5:
                ops.append(("reset_timing",))
            else:
                ops.append(("set_timing", 8))
                timed = True
        else:
            ops.append(draw_reader(rnd, h, w, hot, torus))
        # 4. a step of any length (after a writer, half of them of a short step's shape:
        # what a flag the writer left standing would license), a reader
        if timed or (still_start and ph == phrases - 1) or rnd.random() < 0.8:
            wrote = ops[-1][0] in WRITERS
            ops.append(("step", quiet_length() if wrote and rnd.random() < 0.5 else rnd.choice(table)))
        if timed:
            ops.append(("set_timing", 0))
        if rnd.random() < 0.3:
            ops.append(draw_reader(rnd, h, w, hot, torus))
    return start, ops


def format_op(op):
    if op[0] == "write":
        _, y, x, name, o = op
        return f"write_rect {OP_NAMES[o]} {name} at ({y}, {x})"
    if op[0] == "rewrite":
        return "write_rect SET of the window's own cells at (%d, %d) %d x %d" % op[1:]
    return " ".join(str(v) for v in op)


def format_ops(ops, upto=None):
    ops = ops if upto is None else ops[:upto + 1]
    return "\n".join(f"  {i:3d}  {format_op(op)}" for i, op in enumerate(ops))


# ---- running a program on the model


def run_op(model, op):
    """Applies one op to the model.  Returns (answer, record): the answer a reader's
    counterpart on an engine must give (None for ops that return nothing), and the
    record program_facts folds over."""
    name = op[0]
    rec = {"op": op, "fixed": None, "changed": None}
    if name in ("step",) or name in WRITERS:
        rec["fixed"] = model.is_fixed()
    before = model.cells if name in WRITERS else None
    ans = None
    if name == "step":
        model.step(op[1])
    elif name == "write":
        _, y, x, win, o = op
        model.write_rect(y, x, WINDOWS[win], o)
    elif name == "rewrite":
        _, y, x, rh, rw = op
        model.write_rect(y, x, model.window(y, x, rh, rw), RECT_SET)
    elif name in ("load", "load_ascii"):
        model.load(make_field(model.oracle, op[1], model.h, model.w))
    elif name == "init_random":
        model.init_random(op[1])
    elif name == "snapshot":
        model.snapshot()
    elif name == "restore":
        model.restore()
    elif name == "same":
        ans = model.same()
    elif name == "diff":
        ans = model.diff()
    elif name == "until":
        ans = model.until_periodic(*op[1:])
    elif name == "store":
        ans = model.packed()
    elif name == "digest":
        ans = model.digest()
    elif name == "digest_rows":
        ans = model.digest_rows(op[1], op[2])
    elif name == "read":
        ans = model.read_rect(*op[1:])
    elif name == "density":
        ans = model.density(*op[1:])
    else:
        assert name in ("sync", "act", "set_timing", "reset_timing"), op
    if before is not None:
        rec["changed"] = bool((before != model.cells).any())
    return ans, rec


def run_program(model, ops):
    return [run_op(model, op)[1] for op in ops]


def program_facts(model_run, K):
    """What a program reached, from the model's records alone.

    seen: a sync has come after a step that ended with a remainder launch, with no
    writer of the field between that step and now -- what lets the host know a fixed
    point (step.cpp sync_observing), if the field is one.  A timed step ends it, as a
    writer does.  A fixed candidate is a step that starts on a fixed point while seen."""
    seen = timed = False
    last_rem = False      # the last step ended with a remainder launch ...
    untouched = False     # ... and nobody has written the field since
    run = 0
    name = None
    facts = dict(steps=0, fixed_start=0, fixed_candidates=0, longest_run=0, seen_writes=0,
                 moving_steps=0, noop_writes=0, writers=0, writer_pairs=0, seen_restores=0,
                 lengths=set())
    for rec in model_run:
        op = rec["op"]
        before, name = name, op[0]  # (before: the op before this one)
        if name == "step":
            g = op[1]
            facts["steps"] += 1
            if rec["fixed"]:
                facts["fixed_start"] += 1
            else:
                facts["moving_steps"] += 1
            if g >= 4 * K and not timed:
                facts["lengths"].add(g)
            if seen and rec["fixed"] and not timed:
                facts["fixed_candidates"] += 1
                run += 1
                facts["longest_run"] = max(facts["longest_run"], run)
            else:
                run = 0
            if timed:
                seen = False
            last_rem, untouched = ends_with_remainder(g, K) and not timed, True
            continue
        run = 0
        if name == "sync":
            seen = seen or (last_rem and untouched)
        elif name == "set_timing":
            timed = op[1] != 0
        elif name in WRITERS:
            facts["writers"] += 1
            if before in WRITERS:
                facts["writer_pairs"] += 1
            if seen and rec["fixed"]:
                facts["seen_writes"] += 1
                if name == "restore" and rec["changed"]:
                    facts["seen_restores"] += 1
            if name in ("write", "rewrite") and not rec["changed"]:
                facts["noop_writes"] += 1
            seen = untouched = False
    facts["lengths"] = len(facts["lengths"])
    return facts


# ---- the sweep's cases: kind -> engine settings, shapes, rules and seeds

WIDTHS = [64 * 126, 64 * 127, 64 * 141 - 37, 64 * 156]  # test_gpu_probe_pass.WIDTHS
BASE = dict(resident=1, handoff=1, streams=1)            # test_gpu_probe_pass.BASE
SEM_TORUS = 2

# K: the kernel depth the lengths are drawn for; rules: (rule, seeds of the GPU sweep)
KINDS = {
    "skip16": dict(K=16, skip=True, rules=[(REF_RULE, 12), (CONWAY, 12)]),
    "skip8": dict(K=8, skip=True, rules=[(REF_RULE, 8)]),
    "skip12": dict(K=12, skip=True, rules=[(HIGHLIFE, 8)]),  # the generic-rule kernels
    "torus": dict(K=8, torus=True, rules=[(REF_RULE, 4), (CONWAY, 4)]),
    "torus_res": dict(K=16, torus=True, rules=[(REF_RULE, 2), (CONWAY, 2)]),
    "streams": dict(K=16, rules=[(REF_RULE, 3), (CONWAY, 3)]),
    "group": dict(K=16, rules=[(REF_RULE, 3), (CONWAY, 3)]),
    "hand": dict(K=12, rules=[(REF_RULE, 2), (CONWAY, 2)]),
    "resident": dict(K=16, rules=[(REF_RULE, 2), (CONWAY, 2)]),
    "default": dict(K=16, rules=[(REF_RULE, 2), (CONWAY, 2)]),
}


def draw_engine(rnd, kind):
    """(h, w, constructor keywords, stripes) of one case; stripes: the parts a composite
    engine or a group splits the rows into (1: none)."""
    if kind.startswith("skip"):
        h = 333 if rnd.random() < 0.5 else rnd.randint(130, 400)
        w = rnd.choice(WIDTHS) - rnd.randint(0, 63)
        rpw = rnd.choice([64, 15, 48, 90]) if kind == "skip16" else 64
        return h, w, dict(BASE, tb_depth=KINDS[kind]["K"], rows_per_wave=rpw), 1
    if kind == "torus":
        return 300, 500, dict(semantics=SEM_TORUS, tb_depth=8, resident=1, handoff=1,
                              halo_depth=rnd.choice([8, 64])), 1
    if kind == "torus_res":
        return 130, 192, dict(semantics=SEM_TORUS), 1
    if kind == "streams":
        n = rnd.choice([2, 3])
        return 1500, 500, dict(streams=n), n
    if kind == "group":
        return 1500, 500, dict(halo_depth=rnd.randint(1, 64), exchange_overlap=rnd.randint(0, 2)), 3
    if kind == "hand":
        return 333, WIDTHS[0], dict(resident=1, streams=1, tb_depth=12, handoff=2, rows_per_wave=30), 1
    if kind == "resident":
        return 257, 320, dict(resident=2), 1
    assert kind == "default"
    return 1500, 500, dict(), 1


def case_program(kind, rule, seed, hot_fn=None):
    """The case (kind, rule, seed): dict of h, w, cfg, stripes, start and ops.  hot_fn(h,
    w, cfg, stripes) -> hot_coordinates' dict, from the plan the engine would build."""
    import random
    rnd = random.Random(f"{kind} {RULE_NAMES[rule]} {seed}")
    h, w, cfg, stripes = draw_engine(rnd, kind)
    hot = hot_fn(h, w, dict(cfg, rule=rule), stripes) if hot_fn else hot_coordinates(h, w)
    spec = KINDS[kind]
    start, ops = draw_program(rnd, spec["K"], h, w, rule, kind, hot=hot,
                              torus=spec.get("torus", False))
    return dict(kind=kind, rule=rule, seed=seed, h=h, w=w, cfg=cfg, stripes=stripes, K=spec["K"],
                torus=spec.get("torus", False), hot=hot, start=start, ops=ops)


def plan_hot(pkg):
    """hot_fn from the package's host-only plan functions (no GPU): the unit seams of
    gol_plan_neighbours' rectangles, the probe tiles' rows, gol_rank_rows' stripes."""
    def hot_fn(h, w, cfg, stripes):
        rects, tile_rows = None, 8
        if cfg.get("streams") == 1 and cfg.get("resident") == 1:
            rects = pkg.plan_neighbours(h, w, **cfg)[0]
            tile_rows = pkg.plan_probe_tiles(h, w, **cfg)[0] or 8
        bounds = [pkg.rank_rows(h, stripes, r)[0] for r in range(1, stripes)]
        return hot_coordinates(h, w, rects, tile_rows, bounds)
    return hot_fn
