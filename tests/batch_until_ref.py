"""What BatchEngine.step_until_periodic does, for its tests (test_batch_until_host.py,
test_gpu_batch_until.py): gol_batch_step_until_periodic's contract (include/gol.h)
written over batch_ref.run, which test_batch_host.py pins to rule_ref and torus_ref.
Independent of the library: every generation up to max_g is kept, the checks are tested
in order and the least divisor is taken.
"""
import numpy as np

import batch_ref


def resolve(lag, check_every):
    """check_every as used: 0 means the least multiple of 64 that is >= lag."""
    return check_every if check_every else -(-lag // 64) * 64


def until_ref(cells, max_g, lag, check_every, rule, torus):
    """(period uint32 [n], generation uint64 [n], final uint8 [n, h, w] cells)."""
    return _until(cells, max_g, lag, check_every, lambda a: batch_ref.run(a, 1, rule, torus))


def until_ref_rules(cells, max_g, lag, check_every, birth, survive, torus):
    """until_ref with a rule per field, (birth[i], survive[i]), over batch_rules_ref.run
    (test_batch_lattice_host.py pins it to until_ref field by field)."""
    import batch_rules_ref
    return _until(cells, max_g, lag, check_every,
                  lambda a: batch_rules_ref.run(a, 1, birth, survive, torus))


def _until(cells, max_g, lag, check_every, step):
    C = resolve(lag, check_every)
    gens = [np.asarray(cells).astype(np.uint8)]
    for _ in range(max_g):
        gens.append(step(gens[-1]))
    n = gens[0].shape[0]
    period = np.zeros(n, dtype=np.uint32)
    generation = np.full(n, max_g, dtype=np.uint64)
    divisors = [d for d in range(1, lag + 1) if lag % d == 0]
    for g in range(C, max_g + 1, C):
        same = (gens[g] == gens[g - lag]).all(axis=(1, 2))
        for i in np.flatnonzero(same & (period == 0)):
            period[i] = next(p for p in divisors
                             if (gens[g - lag + p][i] == gens[g - lag][i]).all())
            generation[i] = g
    return period, generation, gens[max_g]


def wave_exits(period, generation, fields_per_wave):
    """Per wavefront the generation G at which its last field was found, None while one
    of its fields is unfound."""
    out = []
    for v in range(0, len(period), fields_per_wave):
        p, g = period[v:v + fields_per_wave], generation[v:v + fields_per_wave]
        out.append(int(g.max()) if (p != 0).all() else None)
    return out


def wave_generations(period, generation, max_g, lag, fields_per_wave):
    """Generations computed, summed over the wavefronts: a wavefront whose fields are all
    found at G runs (max_g - G) % lag more and leaves, any other runs all max_g."""
    return sum(max_g if G is None else G + (max_g - G) % lag
               for G in wave_exits(period, generation, fields_per_wave))


def plan(max_g, lag, check_every, launch_generations=4096):
    """gol_batch_until_plan_of, written out."""
    C = resolve(lag, check_every)
    checks, cpl = max_g // C, max(1, launch_generations // C)
    return {"check_every": C, "divisors": [d for d in range(1, lag) if lag % d == 0],
            "checks": checks, "tail": max_g % C, "checks_per_launch": cpl,
            "launches": max(-(-checks // cpl), 1 if max_g > 0 else 0)}


def launches(period, generation, max_g, lag, check_every, fields_per_wave,
             launch_generations=4096):
    """Launches issued: the plan's, or fewer where every wavefront has left by then."""
    p = plan(max_g, lag, check_every, launch_generations)
    exits = wave_exits(period, generation, fields_per_wave)
    if any(G is None for G in exits):
        return p["launches"]
    per_launch = p["checks_per_launch"] * p["check_every"]
    return min(p["launches"], -(-max(exits) // per_launch))
