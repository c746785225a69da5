"""batch_rules_ref.run (a rule per field) pinned to batch_ref.run (one rule per batch),
field by field.  No GPU."""
import numpy as np
import pytest

import batch_ref
import batch_rules_ref
import rule_ref


def mixed_rules(n, seed):
    """The named rules and B0 first, then seeded random pairs, n in all."""
    named = rule_ref.ONE_BIT + [rule_ref.REF_RULE, rule_ref.CONWAY, rule_ref.FLOOD,
                                batch_rules_ref.B0]
    rb, rs = batch_rules_ref.random_rules(n, seed)
    rules = named + list(zip(rb.tolist(), rs.tolist()))
    return rules[:n]


@pytest.mark.parametrize("torus", [False, True], ids=["dead", "torus"])
@pytest.mark.parametrize("h,w", [(5, 7), (9, 65), (17, 130)])
def test_per_field_runner_equals_uniform_runner(h, w, torus):
    n, gens = 40, 5
    rules = mixed_rules(n, seed=h * 100 + w)
    assert len(rules) == n and len(set(rules)) > 30
    cells = batch_ref.random_batch(n, h, w, seed=h + w)
    birth = np.array([r[0] for r in rules], dtype=np.uint32)
    survive = np.array([r[1] for r in rules], dtype=np.uint32)
    got = batch_rules_ref.run(cells, gens, birth, survive, torus)
    assert got.shape == cells.shape and got.dtype == np.uint8
    for i, rule in enumerate(rules):
        want = batch_ref.run(cells[i:i + 1], gens, rule, torus)[0]
        assert (got[i] == want).all(), (i, rule_ref.rule_name(rule))


def test_tables_and_rule_lists():
    t = batch_rules_ref.tables([0, 0x1FF, 1 << 3, 0b1100])
    assert t.tolist() == [[0] * 9, [1] * 9, [0, 0, 0, 1, 0, 0, 0, 0, 0], [0, 0, 1, 1, 0, 0, 0, 0, 0]]
    assert len(batch_rules_ref.MIXED) == 24
    b, s = batch_rules_ref.cycled(50)
    assert (b[24], s[24]) == batch_rules_ref.MIXED[0] and (b[23], s[23]) == (0, 0)
    rb, rs = batch_rules_ref.random_rules(1000, 3)
    assert rb.max() < 512 and rs.max() < 512 and len(set(zip(rb.tolist(), rs.tolist()))) > 990


def test_zero_generations_is_the_input():
    cells = batch_ref.random_batch(3, 5, 7, seed=1)
    b, s = batch_rules_ref.cycled(3)
    assert (batch_rules_ref.run(cells, 0, b, s) == cells).all()
