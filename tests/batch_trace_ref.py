"""What a batch's population trace is, for its tests (test_batch_trace_host.py,
test_gpu_batch_trace.py).

Built on batch_ref.run (one rule) or batch_rules_ref.run (a rule per field) one sample
interval at a time; a population is a plain sum over a field's cells.  The launch plan of
gol_batch_trace_plan_of is restated in Python.  CASES are the random cases of the GPU
tests; their conditions are checked on this reference alone in test_batch_trace_host.py.
"""
import numpy as np

import batch_ref
import batch_rules_ref
import rule_ref

B36S23 = batch_rules_ref.B36S23
STILL = (0, 0x1FF)  # nothing is born, nothing dies: every pattern is still


def trace_ref(cells, generations, every, rule_or_rules, torus=False):
    """(uint32 [generations // every, n] live cells after every `every` generations,
    uint8 [n, h, w] cells after `generations`).  rule_or_rules: (birth, survive) masks, or
    two arrays [n] of them for a rule per field."""
    birth, survive = rule_or_rules
    per_field = np.ndim(birth) > 0

    def run(c, g):
        if per_field:
            return batch_rules_ref.run(c, g, birth, survive, torus)
        return batch_ref.run(c, g, (int(birth), int(survive)), torus)

    cur = np.asarray(cells).astype(np.uint8)
    n = cur.shape[0]
    samples = generations // every
    live = np.zeros((samples, n), dtype=np.uint32)
    for s in range(samples):
        cur = run(cur, every)
        live[s] = cur.sum(axis=(1, 2))
    return live, run(cur, generations % every)


def plan(generations, every, launch_generations=4096):
    """gol_batch_trace_plan_of, restated."""
    samples = generations // every
    spl = max(1, launch_generations // every)
    launches = max(1, -(-samples // spl)) if generations > 0 else 0
    return {"samples": samples, "tail": generations % every, "samples_per_launch": spl,
            "launches": launches}


# (h, w, n, rule, torus, generations, every, p); seed h * 1000 + w
CASES = [
    (8, 8, 130, rule_ref.CONWAY, True, 40, 1, .35),
    (16, 16, 130, rule_ref.CONWAY, False, 50, 3, .5),
    (9, 65, 70, rule_ref.CONWAY, False, 45, 7, .4),
    (17, 130, 33, B36S23, True, 40, 5, .3),
    (33, 200, 20, rule_ref.REF_RULE, False, 12, 1, .15),
    (64, 4096, 2, rule_ref.CONWAY, True, 9, 2, .3),
    (31, 2050, 2, rule_ref.CONWAY, False, 6, 1, .3),
    (64, 64, 66, rule_ref.CONWAY, False, 48, 16, .3),
]
CASE_IDS = [f"{c[0]}x{c[1]}-n{c[2]}-every{c[6]}" for c in CASES]

_cache = {}


def case(i):
    """(cells, live, final) of CASES[i]; computed once, shared, read-only."""
    if i not in _cache:
        h, w, n, rule, torus, gens, every, p = CASES[i]
        cells = batch_ref.random_batch(n, h, w, h * 1000 + w, p)
        live, final = trace_ref(cells, gens, every, rule, torus)
        for a in (cells, live, final):
            a.setflags(write=False)
        _cache[i] = (cells, live, final)
    return _cache[i]


def lane_sum_cells(wq, n, h=8):
    """The lane-sum pattern: uint8 [n, h, 64 wq] cells in which word q of field f holds
    c = 1 + ((q + 3 f) % 8) live cells, in its column (5 q + f) % 64 of the last c rows, so
    that the counts of neighbouring lanes and of neighbouring fields differ; odd and even
    columns (the two planes of a word) both occur."""
    assert h >= 8
    cells = np.zeros((n, h, 64 * wq), dtype=np.uint8)
    for f in range(n):
        for q in range(wq):
            c = 1 + ((q + 3 * f) % 8)
            cells[f, h - c:, 64 * q + (5 * q + f) % 64] = 1
    return cells
