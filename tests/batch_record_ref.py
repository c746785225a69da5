"""What a batch's recorded rollout is, for its tests (test_batch_record_host.py,
test_gpu_batch_record.py).

Built on batch_ref.run (one rule) or batch_rules_ref.run (a rule per field) one sample
interval at a time; a frame is batch_ref.pack of the window's fields after the interval.
The launch plan is batch_trace_ref.plan (gol_batch_trace_plan_of restated: a record call
issues that plan's launches).  CASES are the random cases of the GPU tests; their
conditions are checked on this reference alone in test_batch_record_host.py.
"""
import numpy as np

import batch_ref
import batch_rules_ref
import rule_ref

B36S23 = batch_rules_ref.B36S23
STILL = (0, 0x1FF)  # nothing is born, nothing dies: every pattern is still


def record_ref(cells, generations, every, rule_or_rules, torus=False, first=0, count=None):
    """(uint64 [generations // every, count, h, ceil(w/64)] packed frames of fields
    [first, first + count) after every `every` generations, uint8 [n, h, w] cells of all
    fields after `generations`).  rule_or_rules: (birth, survive) masks, or two arrays [n]
    of them for a rule per field."""
    birth, survive = rule_or_rules
    per_field = np.ndim(birth) > 0

    def run(c, g):
        if per_field:
            return batch_rules_ref.run(c, g, birth, survive, torus)
        return batch_ref.run(c, g, (int(birth), int(survive)), torus)

    cur = np.asarray(cells).astype(np.uint8)
    n, h, w = cur.shape
    count = n - first if count is None else count
    samples = generations // every
    frames = np.zeros((samples, count, h, (w + 63) // 64), dtype=np.uint64)
    for s in range(samples):
        cur = run(cur, every)
        frames[s] = batch_ref.pack(cur[first:first + count])
    return frames, run(cur, generations % every)


# (h, w, n, rule, torus, generations, every, p, first, count); seed h * 1000 + w
CASES = [
    (8, 8, 130, rule_ref.CONWAY, True, 12, 1, .35, 0, 130),
    (16, 16, 130, rule_ref.CONWAY, False, 20, 3, .5, 3, 70),
    (9, 65, 70, rule_ref.CONWAY, False, 23, 7, .4, 31, 34),
    (17, 130, 33, B36S23, True, 22, 5, .3, 0, 33),
    (33, 200, 20, rule_ref.REF_RULE, False, 4, 1, .15, 5, 10),
    (64, 4096, 2, rule_ref.CONWAY, True, 5, 2, .3, 1, 1),
    (31, 2050, 2, rule_ref.CONWAY, False, 3, 1, .3, 0, 2),
    (64, 64, 66, rule_ref.CONWAY, False, 35, 16, .3, 60, 6),
]
CASE_IDS = [f"{c[0]}x{c[1]}-n{c[2]}-every{c[6]}-win{c[8]}+{c[9]}" for c in CASES]

_cache = {}


def case(i):
    """(cells, frames, final) of CASES[i]; computed once, shared, read-only."""
    if i not in _cache:
        h, w, n, rule, torus, gens, every, p, first, count = CASES[i]
        cells = batch_ref.random_batch(n, h, w, h * 1000 + w, p)
        frames, final = record_ref(cells, gens, every, rule, torus, first, count)
        for a in (cells, frames, final):
            a.setflags(write=False)
        _cache[i] = (cells, frames, final)
    return _cache[i]
