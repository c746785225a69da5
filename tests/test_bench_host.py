"""Host-side logic of bench.py (no GPU): the per-rank breakdown adds up, the
counters record lookup, and the JSON contract's timing passes.

rank_breakdown (r06) turns one rank's gol_timing into per-step spans:
kernel_span + exchange_exposed + other = ms_per_step, exchange_exposed +
exchange_hidden = exchange, none negative when the timing is self-consistent
(what the engine's disjoint compute-stream intervals guarantee).
"""
import importlib.util
import os
import types

import pytest

from conftest import ROOT


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fake_engine():
    return types.SimpleNamespace(rows=8192, row0=24576, halo_depth=128, tb_depth=16,
                                 rows_per_wave=58, handoff=True, age_skew=(82, 58, 1024),
                                 tuning=("models", 75.8, 75.8), w=65536)


def timing(round_ms, xch_ms, exposed_ms, steps=3, launches=24, issued=189):
    return {"launches": launches, "kernel_ms": launches * 0.0704, "cell_gens": 0.0,
            "cell_gens_computed": 0.0, "streams": 1, "launches_issued": issued,
            "launch_rows": launches * 8416.0, "exchanges": 8 * steps, "exchange_ms": xch_ms,
            "rounds": 8 * steps, "round_ms": round_ms, "exchange_exposed_ms": exposed_ms}


@pytest.mark.parametrize("mode", ["blocking", "overlapped"])
def test_rank_breakdown_adds_up(mode):
    bench = load_bench()
    steps = 3
    # per step: 4.30 ms of round spans, 0.16 ms of exchanges; blocking: all of it
    # exposed, overlapped: 0.02 ms past the round ends
    exposed = 0.16 * steps if mode == "blocking" else 0.02 * steps
    tm = timing(4.30 * steps, 0.16 * steps, exposed, steps)
    dt = 4.55e-3 * steps
    r = bench.rank_breakdown(fake_engine(), tm, dt, steps, 3)
    total = r["kernel_span_ms_per_step"] + r["exchange_exposed_ms_per_step"] + r["other_ms_per_step"]
    assert total == pytest.approx(r["ms_per_step"], abs=2e-3)
    assert r["exchange_exposed_ms_per_step"] + r["exchange_hidden_ms_per_step"] == \
        pytest.approx(r["exchange_ms_per_step"], abs=2e-3)
    for k in ("kernel_span_ms_per_step", "exchange_exposed_ms_per_step",
              "exchange_hidden_ms_per_step", "other_ms_per_step"):
        assert r[k] >= 0, (k, r)
    assert r["rounds_per_step"] == 8 and r["exchanges_per_step"] == 8
    # the mean launch is reported, not multiplied into a time share
    assert r["avg_launch_ms"] == pytest.approx(0.0704)
    assert "kernel_ms_per_step" not in r


def test_counters_lookup_prefers_newest_round():
    bench = load_bench()
    cfg = {"size": 65536, "rule": "ref", "tb_depth": 16, "streams": 1, "n_gpus": 1,
           "rows_per_wave": 440, "handoff": False}
    rec = bench.counters_for(cfg)
    assert rec is not None and rec["source_round"] == "r06", rec and rec.get("source")
    assert rec["insts_valu_per_launch"] > 0 and rec["hbm_bytes_per_launch"] > 0
    # a rows-per-wave more than 5% away matches nothing
    assert bench.counters_for(dict(cfg, rows_per_wave=600)) is None


def test_timed_steps_has_no_events_in_the_timed_pass():
    """timed_steps: the measured pass runs with timing off (set_timing(0)), the
    event pass after it with sampling on; the returned timing is the event pass's."""
    bench = load_bench()
    calls = []

    class Eng:
        def step(self, g):
            calls.append(("step", self.every))

        def sync(self):
            pass

        def set_timing(self, every):
            self.every = every
            calls.append(("timing", every))

        def reset_timing(self):
            calls.append(("reset", None))

        def timing(self):
            return {"pass": "events"}

    e = Eng()
    e.every = None
    torch = types.SimpleNamespace(cuda=types.SimpleNamespace(synchronize=lambda: None))
    dt, dt_ev, tm = bench.timed_steps(e, 1000, 3, 1, 1, None, torch, 8)
    steps = [c for c in calls if c[0] == "step"]
    assert len(steps) == 1 + 3 + 3
    assert all(every == 0 for _, every in steps[1:4]), steps  # the measured pass
    assert all(every == 8 for _, every in steps[4:]), steps    # the event pass
    assert tm == {"pass": "events"} and dt > 0 and dt_ev > 0
    assert calls[-1] == ("timing", 0)


def test_timed_steps_plain_run_stops_after_the_timed_pass():
    """events=False (a run without --full): W + K steps and no more, all with
    timing off, and after_timed sees the engine right after the K-th timed step."""
    bench = load_bench()
    calls = []

    class Eng:
        def step(self, g):
            calls.append("step")

        def sync(self):
            pass

        def set_timing(self, every):
            assert every == 0

        def reset_timing(self):
            raise AssertionError("no event pass in a plain run")

        timing = reset_timing

    torch = types.SimpleNamespace(cuda=types.SimpleNamespace(synchronize=lambda: None))
    dt, dt_ev, tm = bench.timed_steps(Eng(), 1000, 5, 2, 1, None, torch, 8, events=False,
                                      after_timed=lambda: calls.append("dump"))
    assert calls == ["step"] * 7 + ["dump"]
    assert dt > 0 and dt_ev is None and tm is None
    # with the event pass the dump still sits between the two passes
    calls.clear()

    class EvEng(Eng):
        def set_timing(self, every):
            pass

        def reset_timing(self):
            pass

        def timing(self):
            return {}

    bench.timed_steps(EvEng(), 1000, 3, 1, 1, None, torch, 8, after_timed=lambda: calls.append("dump"))
    assert calls == ["step"] * 4 + ["dump"] + ["step"] * 3


def test_dump_sample_rows_is_fixed_and_bounded():
    import numpy as np
    bench = load_bench()
    # a field that fits: every row
    assert (bench.dump_sample_rows(300, 777) == np.arange(300)).all()
    # the headline field: a seeded sample, the same every time, within the budget
    h = w = 65536
    idx = bench.dump_sample_rows(h, w)
    assert (idx == bench.dump_sample_rows(h, w)).all()
    assert idx[0] == 0 and idx[-1] == h - 1 and (np.diff(idx) > 0).all()
    assert len(idx) * w * 4 <= bench.DUMP_SAMPLE_BYTES
    assert len(idx) * w * 4 + 2 * h * 8 + 5 * 8 + 4 * 128 < 64 << 20  # all four files


@pytest.mark.parametrize("world", [1, 3])
def test_dump_outputs_files(tmp_path, oracle, monkeypatch, world):
    """dump_outputs on engines that hold an oracle-made field (one engine, or the
    stripes of 3 ranks gathered in row order): the sampled rows' cells, every
    row's population and the digest, with a sample budget smaller than the field."""
    import numpy as np
    bench = load_bench()
    h, w = 301, 777
    monkeypatch.setattr(bench, "DUMP_SAMPLE_BYTES", 40 * 4 * w)
    field = oracle.bp_run(oracle.bp_random(h, w, 11), w, 2, oracle.CONWAY)
    cells = np.unpackbits(field.view(np.uint8), axis=1, bitorder="little")[:, :w]
    bounds = np.linspace(0, h, world + 1).astype(int)

    def engine(r):
        r0, r1 = bounds[r], bounds[r + 1]
        # a rank engine hashes its rows at their place in the field (gol_digest)
        (l0, h0), (l1, h1) = oracle.bp_digest(field[:r0], w), oracle.bp_digest(field[:r1], w)
        return types.SimpleNamespace(row0=r0, rows=r1 - r0, store_packed=lambda: field[r0:r1],
                                     digest=lambda: (l1 - l0, (h1 - h0) & ((1 << 64) - 1)))

    parts = []

    class Dist:  # ranks 1.. run first and leave their part; rank 0 gathers them
        @staticmethod
        def all_gather_object(out, obj):
            parts.append(obj)
            if len(parts) == world:
                out[:] = parts[-1:] + parts[:-1]

    for r in list(range(1, world)) + [0]:
        bench.dump_outputs(str(tmp_path), engine(r), h, w, world, r, Dist)
    idx = bench.dump_sample_rows(h, w)
    assert len(idx) == 40 and idx[0] == 0 and idx[-1] == h - 1
    got = np.load(tmp_path / "cells_sample.npy")
    assert got.dtype == np.float32 and got.shape == (40, w) and (got == cells[idx]).all()
    assert (np.load(tmp_path / "sample_rows.npy") == idx).all()
    assert (np.load(tmp_path / "row_population.npy") == cells.sum(axis=1)).all()
    live, hsh = oracle.bp_digest(field, w)
    assert np.load(tmp_path / "digest.npy").tolist() == \
        [live] + [(hsh >> (16 * i)) & 0xFFFF for i in range(4)]
