"""Python binding of libgol.so (include/gol.h) -- the MI355X Game of Life engine.

Thin ctypes layer used by bench.py, the tests and __graft_entry__: no compute
happens here.  Every call goes to the C ABI, whose kernels run on the GPU; there
is no CPU fallback.  Loading fails loudly (GolError) if libgol.so is missing.

The directory name is not a Python identifier, so load it with `load_package()`
from __graft_entry__.py, or importlib with an explicit path.
"""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
# GOL_LIB: dev-only override (A/B of kernel builds in tools/); the product loads libgol.so
LIB_PATH = os.environ.get("GOL_LIB") or os.path.join(HERE, "libgol.so")
CLI_PATH = os.path.join(HERE, "gol")

GOL_OK, GOL_EINVAL, GOL_ENOMEM, GOL_EHIP, GOL_ERCCL, GOL_EIO, GOL_ESTATE, GOL_EXFER = range(8)
# gol_sched_kind (include/gol.h)
OP_EXCHANGE, OP_WAIT_EXCHANGE, OP_LAUNCH, OP_BAND, OP_INTERIOR, OP_EXCHANGE_ASYNC = range(6)
OP_NAMES = ["EXCHANGE", "WAIT_EXCHANGE", "LAUNCH", "BAND", "INTERIOR", "EXCHANGE_ASYNC"]
SEM_GLOBAL, SEM_REF_STRIPES, SEM_TORUS = 0, 1, 2
# gol_rect_op: how write_rect / rect_blit combine the window with the field
RECT_SET, RECT_OR, RECT_XOR, RECT_CLEAR = range(4)

# (birth, survive) masks; bit n <=> n live neighbours
REF_RULE = (0, 1 << 2)  # effective rule of Parallel_Life_MPI.cpp:44-50 ("B/S2")
CONWAY = (1 << 3, (1 << 2) | (1 << 3))  # B3/S23

# Every symbol include/gol.h declares (checked by tests/test_abi.py).
EXPORTS = [
    "gol_config_init", "gol_create", "gol_load_ascii", "gol_store_ascii",
    "gol_load_packed", "gol_store_packed", "gol_init_random", "gol_step", "gol_sync",
    "gol_digest", "gol_destroy", "gol_last_error", "gol_set_timing", "gol_get_timing",
    "gol_reset_timing", "gol_info", "gol_rank_rows", "gol_comm_unique_id",
    "gol_create_rank", "gol_create_group", "gol_group_step", "gol_plan_info",
    "gol_create_rank_transport", "gol_round_schedule", "gol_plan_handoff",
    "gol_plan_resident", "gol_plan_skew", "gol_plan_columns", "gol_plan_tuning",
    "gol_digest_rows", "gol_comm_info", "gol_plan_model", "gol_plan_passes",
    "gol_plan_resident_rows", "gol_plan_exchange", "gol_activity", "gol_plan_neighbours",
    "gol_activity_copied", "gol_activity_probed", "gol_activity_elided", "gol_torus_geometry", "gol_torus_pad",
    "gol_activity_pass_probed", "gol_plan_probe_tiles", "gol_activity_pass_kept",
    "gol_activity_pass_sure", "gol_activity_short_steps",
    "gol_plan_still_step", "gol_activity_fixed_steps", "gol_activity_fixed_launches",
    "gol_activity_state",
    "gol_read_rect", "gol_write_rect", "gol_density", "gol_rect_blit",
    "gol_snapshot", "gol_snapshot_same", "gol_snapshot_diff", "gol_snapshot_restore",
    "gol_snapshot_drop", "gol_step_until_periodic",
    "gol_batch_geometry", "gol_batch_create", "gol_batch_destroy", "gol_batch_info",
    "gol_batch_load_packed", "gol_batch_store_packed", "gol_batch_load_device",
    "gol_batch_store_device", "gol_batch_init_random", "gol_batch_step", "gol_batch_sync",
    "gol_batch_digest", "gol_batch_step_until_periodic", "gol_batch_until_plan_of",
    "gol_batch_set_rules", "gol_batch_get_rules", "gol_batch_drop_rules", "gol_batch_has_rules",
    "gol_batch_step_trace", "gol_batch_step_trace_device", "gol_batch_trace_plan_of",
    "gol_batch_step_record", "gol_batch_step_record_device",
]

# gol_step_until_periodic flag: run on to max_generations once a period is known
UNTIL_FINISH = 1

# gol_plan_tuning's variants (plan.cpp kTuneVariantNames): 0 = the models' plan
TUNE_VARIANTS = ["models", "no_half_strip", "skew_0.95", "skew_1.05", "other_block_kind"]


class GolError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"gol status {status}: {msg}")
        self.status = status


class Config(ctypes.Structure):
    _fields_ = [
        ("birth_mask", ctypes.c_uint32),
        ("survive_mask", ctypes.c_uint32),
        ("device", ctypes.c_int32),
        ("semantics", ctypes.c_uint32),
        ("ref_ranks", ctypes.c_uint32),
        ("tb_depth", ctypes.c_uint32),
        ("halo_depth", ctypes.c_uint32),
        ("rows_per_wave", ctypes.c_uint32),
        ("handoff", ctypes.c_uint32),
        ("streams", ctypes.c_uint32),
        ("strip_lanes", ctypes.c_uint32),
        ("word_planes", ctypes.c_uint32),
        ("resident", ctypes.c_uint32),
        ("exchange_overlap", ctypes.c_uint32),
    ]


class Timing(ctypes.Structure):
    _fields_ = [
        ("launches", ctypes.c_uint64),
        ("kernel_ms", ctypes.c_double),
        ("cell_gens", ctypes.c_double),
        ("cell_gens_computed", ctypes.c_double),
        ("streams", ctypes.c_uint32),
        ("struct_size", ctypes.c_uint32),  # in: sizeof(gol_timing) (gol.h)
        ("launches_issued", ctypes.c_uint64),
        ("launch_rows", ctypes.c_double),
        ("exchanges", ctypes.c_uint64),
        ("exchange_ms", ctypes.c_double),
        ("rounds", ctypes.c_uint64),
        ("round_ms", ctypes.c_double),
        ("exchange_exposed_ms", ctypes.c_double),
    ]


class PlanSummary(ctypes.Structure):
    _fields_ = [
        ("tb_depth", ctypes.c_uint32), ("halo_depth", ctypes.c_uint32),
        ("plans", ctypes.c_uint32), ("distinct_plans", ctypes.c_uint32),
        ("rows_lo", ctypes.c_int64), ("rows_hi", ctypes.c_int64),
        ("rows_per_wave", ctypes.c_int64),
        ("rows_old", ctypes.c_int32), ("units_old", ctypes.c_int32),
        ("strips", ctypes.c_int32), ("lane_shift", ctypes.c_int32),
        ("total_units", ctypes.c_int64), ("half_units", ctypes.c_int64),
        ("blocks", ctypes.c_int64),
        ("handoff", ctypes.c_int32), ("tail_off", ctypes.c_int32),
        ("candidates", ctypes.c_uint32), ("passes", ctypes.c_uint32),
    ]


class StillEffect(ctypes.Structure):
    """gol_still_effect: what a step on a proven fixed point does to the activity state."""
    _fields_ = [("launches", ctypes.c_uint64)] + [(k, ctypes.c_uint32) for k in (
        "computed", "skipped", "copied", "probed", "pass_probed", "elided", "busy0_add",
        "busy1", "streak0", "streak1", "need", "held", "moved", "twin", "twin_ok",
        "kept_passes", "sure_passes")]


class Until(ctypes.Structure):
    """gol_until: what gol_step_until_periodic found."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32),  # in: sizeof(gol_until) (gol.h)
        ("period", ctypes.c_uint32),
        ("advanced", ctypes.c_uint64),
        ("lag", ctypes.c_uint32),
        ("check_every", ctypes.c_uint32),
        ("checks", ctypes.c_uint32),
        ("extra_generations", ctypes.c_uint32),
    ]

    def __repr__(self):
        return "Until(" + ", ".join(f"{k}={getattr(self, k)}" for k, _ in self._fields_[1:]) + ")"


class BatchUntil(ctypes.Structure):
    """gol_batch_until: the counters of gol_batch_step_until_periodic."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32),  # in: sizeof(gol_batch_until) (gol.h)
        ("lag", ctypes.c_uint32),
        ("check_every", ctypes.c_uint32),
        ("launches", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("found", ctypes.c_uint64),
        ("wave_generations", ctypes.c_uint64),
    ]


class BatchUntilPlan(ctypes.Structure):
    """gol_batch_until_plan: how gol_batch_step_until_periodic splits its work."""
    _fields_ = [
        ("check_every", ctypes.c_uint32),
        ("ndivisors", ctypes.c_uint32),
        ("divisors", ctypes.c_uint32 * 32),
        ("checks", ctypes.c_uint64),
        ("tail", ctypes.c_uint32),
        ("checks_per_launch", ctypes.c_uint32),
        ("launches", ctypes.c_uint64),
    ]


class BatchPeriods:
    """What BatchEngine.step_until_periodic found: period (uint32 [n], 0 = none) and
    generation (uint64 [n]) per field, and the call's lag, check_every, launches, found
    and wave_generations (gol_batch_until)."""

    def __init__(self, period, generation, r):
        self.period, self.generation = period, generation
        self.lag, self.check_every, self.launches = r.lag, r.check_every, r.launches
        self.found, self.wave_generations = r.found, r.wave_generations

    def __repr__(self):
        return (f"BatchPeriods(found={self.found}/{len(self.period)}, lag={self.lag}, "
                f"check_every={self.check_every}, launches={self.launches}, "
                f"wave_generations={self.wave_generations})")


class BatchTrace(ctypes.Structure):
    """gol_batch_trace: the counters of gol_batch_step_trace."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32),  # in: sizeof(gol_batch_trace) (gol.h)
        ("every", ctypes.c_uint32),
        ("samples", ctypes.c_uint64),
        ("launches", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]

    def __repr__(self):
        return f"BatchTrace(every={self.every}, samples={self.samples}, launches={self.launches})"


class BatchTracePlan(ctypes.Structure):
    """gol_batch_trace_plan: how gol_batch_step_trace splits its work."""
    _fields_ = [
        ("samples", ctypes.c_uint64),
        ("tail", ctypes.c_uint32),
        ("samples_per_launch", ctypes.c_uint32),
        ("launches", ctypes.c_uint64),
    ]


class BatchRecord(ctypes.Structure):
    """gol_batch_record: the counters of gol_batch_step_record."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32),  # in: sizeof(gol_batch_record) (gol.h)
        ("every", ctypes.c_uint32),
        ("samples", ctypes.c_uint64),
        ("launches", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]

    def __repr__(self):
        return f"BatchRecord(every={self.every}, samples={self.samples}, launches={self.launches})"


class SchedOp(ctypes.Structure):
    _fields_ = [
        ("kind", ctypes.c_uint32),
        ("depth", ctypes.c_uint32),
        ("shrink", ctypes.c_uint32),
        ("nseg", ctypes.c_uint32),
        ("out_lo", ctypes.c_int64 * 2),
        ("out_hi", ctypes.c_int64 * 2),
    ]


# gol_halo_exchange_fn(ctx, send_up, recv_up, send_down, recv_down, bytes) -> int
HALO_EXCHANGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_uint64)


class Transport(ctypes.Structure):
    _fields_ = [("exchange", HALO_EXCHANGE_FN), ("ctx", ctypes.c_void_p)]


def build(force=False):
    """Compile libgol.so and the CLI in-tree (hipcc --offload-arch=gfx950)."""
    args = ["make", "-s", "-C", HERE, "-j8"]
    if force:
        subprocess.run(["make", "-s", "-C", HERE, "clean"], check=True)
    subprocess.run(args, check=True)


_lib = None


def lib():
    """Load libgol.so (torch first, so one HIP runtime serves the process)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GolError(-1, f"{LIB_PATH} not built; run __graft_entry__.build()")
    try:  # share torch's HIP runtime when torch is present (same SONAME)
        import torch  # noqa: F401
    except Exception:
        pass
    L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    pu64 = ctypes.POINTER(ctypes.c_uint64)
    L.gol_config_init.argtypes = [ctypes.POINTER(Config)]
    L.gol_config_init.restype = None
    L.gol_create.argtypes = [u64, u64, ctypes.POINTER(Config), ctypes.POINTER(vp)]
    L.gol_create_rank.argtypes = [u64, u64, ctypes.POINTER(Config), i32, i32, ctypes.c_char_p,
                                  ctypes.POINTER(vp)]
    L.gol_load_ascii.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t]
    L.gol_store_ascii.argtypes = [vp, vp, ctypes.c_size_t]
    L.gol_load_packed.argtypes = [vp, vp, u64]
    L.gol_store_packed.argtypes = [vp, vp, u64]
    L.gol_init_random.argtypes = [vp, u64]
    L.gol_step.argtypes = [vp, u64]
    L.gol_sync.argtypes = [vp]
    L.gol_digest.argtypes = [vp, pu64, pu64]
    L.gol_destroy.argtypes = [vp]
    L.gol_destroy.restype = None
    L.gol_last_error.argtypes = []
    L.gol_last_error.restype = ctypes.c_char_p
    L.gol_set_timing.argtypes = [vp, i32]
    L.gol_get_timing.argtypes = [vp, ctypes.POINTER(Timing)]
    L.gol_reset_timing.argtypes = [vp]
    L.gol_info.argtypes = [vp, pu64, pu64, pu64, pu64, ctypes.POINTER(u32), ctypes.POINTER(u32),
                           ctypes.POINTER(u32)]
    L.gol_rank_rows.argtypes = [u64, i32, i32, pu64, pu64]
    L.gol_comm_unique_id.argtypes = [ctypes.c_char_p]
    L.gol_create_group.argtypes = [u64, u64, ctypes.POINTER(Config), i32,
                                   ctypes.POINTER(ctypes.c_int), ctypes.POINTER(vp)]
    L.gol_group_step.argtypes = [ctypes.POINTER(vp), i32, u64]
    L.gol_plan_info.argtypes = [vp, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.gol_plan_handoff.argtypes = [vp, ctypes.POINTER(u32)]
    L.gol_plan_resident.argtypes = [vp, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.gol_plan_skew.argtypes = [vp, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.gol_plan_columns.argtypes = [vp, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.gol_create_rank_transport.argtypes = [u64, u64, ctypes.POINTER(Config), i32, i32,
                                            ctypes.POINTER(Transport), ctypes.POINTER(vp)]
    pf32 = ctypes.POINTER(ctypes.c_float)
    L.gol_plan_tuning.argtypes = [vp, ctypes.POINTER(u32), pf32, pf32]
    L.gol_plan_passes.argtypes = [vp, ctypes.POINTER(u32)]
    L.gol_plan_exchange.argtypes = [vp, ctypes.POINTER(u32), pf32, pf32]
    L.gol_plan_resident_rows.argtypes = [vp] + [ctypes.POINTER(u32)] * 4
    L.gol_digest_rows.argtypes = [vp, u64, u64, pu64, pu64]
    pi32 = ctypes.POINTER(ctypes.c_int)
    L.gol_comm_info.argtypes = [vp, pi32, pi32, pi32, pi32, pi32]
    L.gol_round_schedule.argtypes = [u64, u64, ctypes.POINTER(Config), i32, i32, u64, i32,
                                     ctypes.POINTER(SchedOp), u64, pu64, ctypes.POINTER(u32),
                                     ctypes.POINTER(u32)]
    L.gol_plan_model.argtypes = [u64, u64, ctypes.POINTER(Config), i32, i32, i32, i32, i32,
                                 ctypes.POINTER(PlanSummary)]
    L.gol_activity.argtypes = [vp, pu64, pu64]
    L.gol_activity_copied.argtypes = [vp, pu64]
    L.gol_activity_probed.argtypes = [vp, pu64]
    L.gol_activity_elided.argtypes = [vp, pu64]
    L.gol_activity_pass_probed.argtypes = [vp, pu64]
    L.gol_activity_pass_kept.argtypes = [vp, pu64]
    L.gol_activity_pass_sure.argtypes = [vp, pu64]
    L.gol_activity_short_steps.argtypes = [vp, pu64]
    L.gol_activity_fixed_steps.argtypes = [vp, pu64]
    L.gol_activity_fixed_launches.argtypes = [vp, pu64]
    L.gol_activity_state.argtypes = [vp, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    L.gol_plan_still_step.argtypes = [u32, u64, ctypes.POINTER(StillEffect)]
    L.gol_plan_probe_tiles.argtypes = [u64, u64, ctypes.POINTER(Config), i32, i32, i32, vp, u64,
                                       ctypes.POINTER(u32), ctypes.POINTER(u32),
                                       ctypes.POINTER(u32), pu64, pu64]
    L.gol_plan_neighbours.argtypes = [u64, u64, ctypes.POINTER(Config), i32, i32, i32, vp, vp, u64,
                                      vp, u64, pu64, pu64]
    L.gol_torus_geometry.argtypes = [u64, u64, ctypes.POINTER(Config), ctypes.POINTER(u32),
                                     ctypes.POINTER(u32), ctypes.POINTER(u32), pu64, pu64]
    L.gol_torus_pad.argtypes = [vp, u64, u64, u64, u32, u32, vp, u64]
    L.gol_read_rect.argtypes = [vp, u64, u64, u64, u64, vp, u64]
    L.gol_write_rect.argtypes = [vp, u64, u64, u64, u64, vp, u64, u32]
    L.gol_density.argtypes = [vp, u64, u64, u64, u64, u64, u64, vp, u64]
    L.gol_rect_blit.argtypes = [vp, u64, u64, vp, u64, u64, u64, u64, u32]
    L.gol_snapshot.argtypes = [vp]
    L.gol_snapshot_same.argtypes = [vp, ctypes.POINTER(u32)]
    L.gol_snapshot_diff.argtypes = [vp, pu64]
    L.gol_snapshot_restore.argtypes = [vp]
    L.gol_snapshot_drop.argtypes = [vp]
    L.gol_step_until_periodic.argtypes = [vp, u64, u32, u32, u32, ctypes.POINTER(Until)]
    pu32 = ctypes.POINTER(u32)
    L.gol_batch_geometry.argtypes = [u64, u64, u64, ctypes.POINTER(Config), pu32, pu32, pu32, pu64]
    L.gol_batch_create.argtypes = [u64, u64, u64, ctypes.POINTER(Config), ctypes.POINTER(vp)]
    L.gol_batch_destroy.argtypes = [vp]
    L.gol_batch_destroy.restype = None
    L.gol_batch_info.argtypes = [vp, pu64, pu64, pu64, pu32, pu32, pu32, pu32]
    for name in ["gol_batch_load_packed", "gol_batch_store_packed", "gol_batch_load_device",
                 "gol_batch_store_device"]:
        getattr(L, name).argtypes = [vp, u64, u64, vp, u64, u64]
    L.gol_batch_init_random.argtypes = [vp, u64]
    L.gol_batch_step.argtypes = [vp, u64]
    L.gol_batch_sync.argtypes = [vp]
    L.gol_batch_digest.argtypes = [vp, u64, u64, vp, vp]
    L.gol_batch_step_until_periodic.argtypes = [vp, u64, u32, u32, vp, vp,
                                                ctypes.POINTER(BatchUntil)]
    L.gol_batch_until_plan_of.argtypes = [u64, u32, u32, u32, ctypes.POINTER(BatchUntilPlan)]
    L.gol_batch_set_rules.argtypes = [vp, u64, u64, vp, vp]
    L.gol_batch_get_rules.argtypes = [vp, u64, u64, vp, vp]
    L.gol_batch_drop_rules.argtypes = [vp]
    L.gol_batch_has_rules.argtypes = [vp, pu32]
    L.gol_batch_step_trace.argtypes = [vp, u64, u32, vp, u64, ctypes.POINTER(BatchTrace)]
    L.gol_batch_step_trace_device.argtypes = [vp, u64, u32, vp, u64, ctypes.POINTER(BatchTrace)]
    L.gol_batch_trace_plan_of.argtypes = [u64, u32, u32, ctypes.POINTER(BatchTracePlan)]
    for name in ["gol_batch_step_record", "gol_batch_step_record_device"]:
        getattr(L, name).argtypes = [vp, u64, u32, u64, u64, vp, u64, u64, u64,
                                     ctypes.POINTER(BatchRecord)]
    for name in ["gol_batch_geometry", "gol_batch_create", "gol_batch_info",
                 "gol_batch_load_packed", "gol_batch_store_packed", "gol_batch_load_device",
                 "gol_batch_store_device", "gol_batch_init_random", "gol_batch_step",
                 "gol_batch_sync", "gol_batch_digest", "gol_batch_step_until_periodic",
                 "gol_batch_until_plan_of", "gol_batch_set_rules", "gol_batch_get_rules",
                 "gol_batch_drop_rules", "gol_batch_has_rules", "gol_batch_step_trace",
                 "gol_batch_step_trace_device", "gol_batch_trace_plan_of",
                 "gol_batch_step_record", "gol_batch_step_record_device"]:
        getattr(L, name).restype = ctypes.c_int
    for name in ["gol_read_rect", "gol_write_rect", "gol_density", "gol_rect_blit", "gol_snapshot",
                 "gol_snapshot_same", "gol_snapshot_diff", "gol_snapshot_restore",
                 "gol_snapshot_drop", "gol_step_until_periodic"]:
        getattr(L, name).restype = ctypes.c_int
    for name in ["gol_torus_geometry", "gol_torus_pad", "gol_create", "gol_create_rank", "gol_load_ascii", "gol_store_ascii",
                 "gol_load_packed", "gol_store_packed", "gol_init_random", "gol_step",
                 "gol_sync", "gol_digest", "gol_set_timing", "gol_get_timing",
                 "gol_reset_timing", "gol_info", "gol_rank_rows", "gol_comm_unique_id",
                 "gol_create_group", "gol_group_step", "gol_plan_info", "gol_plan_handoff",
                 "gol_plan_resident", "gol_plan_skew", "gol_plan_columns",
                 "gol_create_rank_transport", "gol_round_schedule", "gol_plan_tuning",
                 "gol_digest_rows", "gol_comm_info", "gol_plan_model", "gol_plan_passes",
                 "gol_plan_resident_rows", "gol_plan_exchange", "gol_activity",
                 "gol_plan_neighbours", "gol_activity_copied", "gol_activity_probed",
                 "gol_activity_elided", "gol_activity_pass_probed", "gol_plan_probe_tiles",
                 "gol_activity_pass_kept", "gol_activity_pass_sure",
                 "gol_activity_short_steps", "gol_plan_still_step",
                 "gol_activity_fixed_steps", "gol_activity_fixed_launches",
                 "gol_activity_state"]:
        getattr(L, name).restype = ctypes.c_int
    _lib = L
    return L


def _check(st):
    if st != GOL_OK:
        raise GolError(st, lib().gol_last_error().decode(errors="replace"))


def make_config(rule=REF_RULE, device=-1, semantics=SEM_GLOBAL, ref_ranks=1, tb_depth=0,
                halo_depth=0, rows_per_wave=0, handoff=0, streams=0, strip_lanes=0,
                word_planes=0, resident=0, exchange_overlap=0):
    c = Config()
    lib().gol_config_init(ctypes.byref(c))
    c.birth_mask, c.survive_mask = rule
    c.device = device
    c.semantics = semantics
    c.ref_ranks = ref_ranks
    c.tb_depth = tb_depth
    c.halo_depth = halo_depth
    c.rows_per_wave = rows_per_wave
    c.handoff = handoff
    c.streams = streams
    c.strip_lanes = strip_lanes
    c.word_planes = word_planes
    c.resident = resident
    c.exchange_overlap = exchange_overlap
    return c


def rank_rows(h, nranks, rank):
    r0, n = ctypes.c_uint64(), ctypes.c_uint64()
    _check(lib().gol_rank_rows(h, nranks, rank, ctypes.byref(r0), ctypes.byref(n)))
    return r0.value, n.value


def round_schedule(h, w, rank, nranks, gens, halo_fresh=False, **cfg_kw):
    """The launch/exchange schedule gol_step runs on stripe `rank` of `nranks`
    (gol_round_schedule; host-only).  Returns (ops, K, Hx), ops as dicts with
    kind (OP_*), depth, shrink and segs [(out_lo, out_hi), ...] in local rows."""
    cfg = make_config(**cfg_kw)
    n, K, Hx = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
    _check(lib().gol_round_schedule(h, w, ctypes.byref(cfg), rank, nranks, gens,
                                    1 if halo_fresh else 0, None, 0, ctypes.byref(n),
                                    ctypes.byref(K), ctypes.byref(Hx)))
    arr = (SchedOp * max(1, n.value))()
    _check(lib().gol_round_schedule(h, w, ctypes.byref(cfg), rank, nranks, gens,
                                    1 if halo_fresh else 0, arr, n.value, ctypes.byref(n),
                                    ctypes.byref(K), ctypes.byref(Hx)))
    ops = [{"kind": o.kind, "depth": o.depth, "shrink": o.shrink,
            "segs": [(o.out_lo[i], o.out_hi[i]) for i in range(o.nseg)]}
           for o in arr[:n.value]]
    return ops, K.value, Hx.value


def plan_model(h, w, rank=0, nranks=1, cus=256, occ_classic=2, occ_hand=2, **cfg_kw):
    """gol_plan_model (host only, no GPU): the first full-depth launch plan the
    engine would build on a device of `cus` CUs with those occupancies (256-thread
    workgroups per CU), before the autotuner.  Returns a dict of PlanSummary."""
    cfg = make_config(**cfg_kw)
    out = PlanSummary()
    _check(lib().gol_plan_model(h, w, ctypes.byref(cfg), rank, nranks, cus, occ_classic,
                                occ_hand, ctypes.byref(out)))
    return {k: getattr(out, k) for k, _ in PlanSummary._fields_ if k != "reserved"}


def plan_still_step(tb_depth, generations):
    """gol_plan_still_step (host only, no GPU): what a gol_step of `generations`
    generations at depth `tb_depth` does to the activity state of a field that is a
    proven fixed point (DESIGN §4 "Fixed step").  Returns a dict of StillEffect."""
    out = StillEffect()
    _check(lib().gol_plan_still_step(tb_depth, generations, ctypes.byref(out)))
    return {k: getattr(out, k) for k, _ in StillEffect._fields_}


def plan_neighbours(h, w, cus=256, occ_classic=2, occ_hand=2, **cfg_kw):
    """gol_plan_neighbours (host only, no GPU): the activity skip's view of the launch
    plan gol_create would build.  Returns (rects, offsets, ids): rects an int64
    array [units, 2, 4] of (r0, r1, q0, q1) -- rows [r0, r1) x 64-column lane groups
    [q0, q1), r1 <= r0: none -- and the units' neighbour lists in CSR form
    (ids[offsets[u]:offsets[u + 1]]); ids is empty for a plan that never skips."""
    import numpy as np
    cfg = make_config(**cfg_kw)
    nu, ni = ctypes.c_uint64(), ctypes.c_uint64()
    _check(lib().gol_plan_neighbours(h, w, ctypes.byref(cfg), cus, occ_classic, occ_hand, None,
                                     None, 0, None, 0, ctypes.byref(nu), ctypes.byref(ni)))
    rects = np.zeros((nu.value, 2, 4), dtype=np.int64)
    offs = np.zeros(nu.value + 1, dtype=np.uint32)
    ids = np.zeros(max(1, ni.value), dtype=np.uint32)
    _check(lib().gol_plan_neighbours(h, w, ctypes.byref(cfg), cus, occ_classic, occ_hand,
                                     rects.ctypes.data, offs.ctypes.data, nu.value,
                                     ids.ctypes.data, ni.value, ctypes.byref(nu),
                                     ctypes.byref(ni)))
    return rects, offs, ids[:ni.value]


def plan_probe_tiles(h, w, cus=256, occ_classic=2, occ_hand=2, **cfg_kw):
    """gol_plan_probe_tiles (host only, no GPU): the probe pass's table of the launch
    plan gol_create would build.  Returns (tile_rows, tile_words, ncol, table): the
    plan's output rows in tiles of tile_rows rows x tile_words 64-column words, ncol
    column segments per row chunk fastest; table a uint32 array [tiles, slots] of
    unit indices (unused slots 0xFFFFFFFF), or None for a plan without the pass."""
    import numpy as np
    cfg = make_config(**cfg_kw)
    tr, tw, sl = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    nt, nc = ctypes.c_uint64(), ctypes.c_uint64()
    args = (h, w, ctypes.byref(cfg), cus, occ_classic, occ_hand)
    outs = (ctypes.byref(tr), ctypes.byref(tw), ctypes.byref(sl), ctypes.byref(nt), ctypes.byref(nc))
    _check(lib().gol_plan_probe_tiles(*args, None, 0, *outs))
    if nt.value == 0:
        return tr.value, tw.value, 0, None
    table = np.zeros((nt.value, sl.value), dtype=np.uint32)
    _check(lib().gol_plan_probe_tiles(*args, table.ctypes.data, table.size, *outs))
    return tr.value, tw.value, nc.value, table


def torus_geometry(h, w, **cfg_kw):
    """gol_torus_geometry (host only, no GPU): the geometry Engine(h, w,
    semantics=SEM_TORUS, **cfg_kw) would use.  Returns a dict: round_gens (G,
    generations per wrap round), ghost_rows, ghost_words, padded_h, padded_w."""
    cfg_kw.setdefault("semantics", SEM_TORUS)
    cfg = make_config(**cfg_kw)
    g, gr, gw = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    ph, pw = ctypes.c_uint64(), ctypes.c_uint64()
    _check(lib().gol_torus_geometry(h, w, ctypes.byref(cfg), ctypes.byref(g), ctypes.byref(gr),
                                    ctypes.byref(gw), ctypes.byref(ph), ctypes.byref(pw)))
    return {"round_gens": g.value, "ghost_rows": gr.value, "ghost_words": gw.value,
            "padded_h": ph.value, "padded_w": pw.value}


def torus_pad(arr, w, ghost_rows, ghost_words):
    """gol_torus_pad (host only, no GPU): the packed h x w field `arr` (uint64
    [h, >= ceil(w/64)]) wrapped into its padded field, uint64 [h + 2 ghost_rows,
    ceil(w/64) + 2 ghost_words], by the wrap kernel's own word gather."""
    import numpy as np
    a = np.ascontiguousarray(arr, dtype=np.uint64)
    h = a.shape[0]
    out = np.zeros((h + 2 * ghost_rows, (w + 63) // 64 + 2 * ghost_words), dtype=np.uint64)
    _check(lib().gol_torus_pad(a.ctypes.data, a.shape[1], h, w, ghost_rows, ghost_words,
                               out.ctypes.data, out.shape[1]))
    return out


def rect_blit(src, sx, dst, dx, rows, cols, op=RECT_SET):
    """gol_rect_blit (host only, no GPU): combines bits [sx, sx + cols) of the first
    `rows` rows of the packed uint64 array `src` onto bits [dx, dx + cols) of `dst`
    (a C-contiguous uint64 array, changed in place) with `op`, through the word
    gather and merge the rectangle kernels use."""
    import numpy as np
    a = np.ascontiguousarray(src, dtype=np.uint64)
    if not (isinstance(dst, np.ndarray) and dst.dtype == np.uint64 and dst.ndim == 2
            and dst.flags.c_contiguous and dst.flags.writeable):
        raise GolError(GOL_EINVAL, "dst must be a writeable C-contiguous 2-D uint64 array")
    if a.ndim != 2 or rows > a.shape[0] or rows > dst.shape[0]:
        raise GolError(GOL_EINVAL, "src and dst must be 2-D with at least `rows` rows")
    _check(lib().gol_rect_blit(a.ctypes.data, a.shape[1], sx, dst.ctypes.data, dst.shape[1], dx,
                               rows, cols, op))
    return dst


def batch_geometry(n, h, w, **cfg_kw):
    """gol_batch_geometry (host only, no GPU): the geometry BatchEngine(n, h, w, ...)
    would use.  Returns a dict: lanes_per_field, fields_per_wave, rows_in_regs, waves."""
    cfg = make_config(**cfg_kw)
    lpf, fpw, rows = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    waves = ctypes.c_uint64()
    _check(lib().gol_batch_geometry(n, h, w, ctypes.byref(cfg), ctypes.byref(lpf),
                                    ctypes.byref(fpw), ctypes.byref(rows), ctypes.byref(waves)))
    return {"lanes_per_field": lpf.value, "fields_per_wave": fpw.value,
            "rows_in_regs": rows.value, "waves": waves.value}


def batch_until_plan(max_generations, lag, check_every=0, launch_generations=4096):
    """gol_batch_until_plan_of (host only, no GPU): how BatchEngine.step_until_periodic
    splits its work on a batch whose launch cap is launch_generations.  Returns a dict:
    check_every (resolved), divisors (lag's proper divisors, ascending), checks, tail,
    checks_per_launch, launches."""
    p = BatchUntilPlan()
    _check(lib().gol_batch_until_plan_of(max_generations, lag, check_every, launch_generations,
                                         ctypes.byref(p)))
    return {"check_every": p.check_every, "divisors": list(p.divisors[:p.ndivisors]),
            "checks": p.checks, "tail": p.tail, "checks_per_launch": p.checks_per_launch,
            "launches": p.launches}


def batch_trace_plan(generations, every, launch_generations=4096):
    """gol_batch_trace_plan_of (host only, no GPU): how BatchEngine.step_trace splits its
    work on a batch whose launch cap is launch_generations.  Returns a dict: samples, tail,
    samples_per_launch, launches."""
    p = BatchTracePlan()
    _check(lib().gol_batch_trace_plan_of(generations, every, launch_generations, ctypes.byref(p)))
    return {"samples": p.samples, "tail": p.tail, "samples_per_launch": p.samples_per_launch,
            "launches": p.launches}


def unpack_cells(words, w):
    """Packed frames to cells: uint64 [..., h, >= ceil(w/64)] canonical words (what
    BatchEngine.step_record and store_packed return) -> uint8 [..., h, w]."""
    import numpy as np
    a = np.ascontiguousarray(words, dtype=np.uint64)
    if a.ndim < 2 or w < 1 or a.shape[-1] * 64 < w:
        raise GolError(GOL_EINVAL, "words must be a uint64 array [..., h, >= ceil(w/64)]")
    bits = np.unpackbits(a.view(np.uint8).reshape(a.shape[:-1] + (-1,)), axis=-1,
                         bitorder="little")
    return np.ascontiguousarray(bits[..., :w])


def pack_cells(cells):
    """The inverse of unpack_cells: [..., h, w] cells (nonzero = live) -> uint64
    [..., h, ceil(w/64)] canonical words, zero-padded to whole words."""
    import numpy as np
    c = np.asarray(cells)
    if c.ndim < 2 or c.shape[-1] < 1:
        raise GolError(GOL_EINVAL, "cells must be an array [..., h, w] with w >= 1")
    w = c.shape[-1]
    wq = (w + 63) // 64
    b = np.zeros(c.shape[:-1] + (wq * 64,), dtype=np.uint8)
    b[..., :w] = c != 0
    packed = np.packbits(b, axis=-1, bitorder="little")
    return np.ascontiguousarray(packed).view(np.uint64).reshape(c.shape[:-1] + (wq,))


def unique_id() -> bytes:
    buf = ctypes.create_string_buffer(128)
    _check(lib().gol_comm_unique_id(buf))
    return buf.raw


class Engine:
    """One field (or one rank's stripe of it) resident on one GPU.
    semantics=SEM_TORUS joins the field's opposite edges (one GPU, one stream;
    halo_depth = generations per wrap round, reported back as self.halo_depth)."""

    def __init__(self, h, w, rule=REF_RULE, device=-1, semantics=SEM_GLOBAL, ref_ranks=1,
                 tb_depth=0, halo_depth=0, rows_per_wave=0, rank=None, nranks=1, uid=None,
                 handoff=0, streams=0, strip_lanes=0, word_planes=0, transport=None,
                 resident=0, exchange_overlap=0, _handle=None):
        """transport: for a rank engine, a callable (send_up, send_down) -> (recv_up,
        recv_down) of bytes objects (None where there is no neighbour) used instead
        of RCCL (gol_create_rank_transport)."""
        self.h, self.w = h, w
        self.wq = (w + 63) // 64
        self._tp = None
        cfg = make_config(rule, device, semantics, ref_ranks, tb_depth, halo_depth,
                          rows_per_wave, handoff, streams, strip_lanes, word_planes, resident,
                          exchange_overlap)
        handle = ctypes.c_void_p()
        if _handle is not None:
            handle = _handle
        elif rank is None:
            _check(lib().gol_create(h, w, ctypes.byref(cfg), ctypes.byref(handle)))
        elif transport is not None:
            self._tp = _make_transport(transport)
            _check(lib().gol_create_rank_transport(h, w, ctypes.byref(cfg), rank, nranks,
                                                   ctypes.byref(self._tp[0]),
                                                   ctypes.byref(handle)))
        else:
            if uid is None or len(uid) != 128:
                raise GolError(GOL_EINVAL, "rank engines need a 128-byte RCCL unique id")
            _check(lib().gol_create_rank(h, w, ctypes.byref(cfg), rank, nranks, uid,
                                         ctypes.byref(handle)))
        self._h = handle
        h_, w_, r0, rows = (ctypes.c_uint64() for _ in range(4))
        k, hx, rpw = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        _check(lib().gol_info(self._h, ctypes.byref(h_), ctypes.byref(w_), ctypes.byref(r0),
                              ctypes.byref(rows), ctypes.byref(k), ctypes.byref(hx),
                              ctypes.byref(rpw)))
        self.row0, self.rows, self.tb_depth, self.halo_depth = r0.value, rows.value, k.value, hx.value
        self.rows_per_wave = rpw.value
        sl, rp, wp = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        _check(lib().gol_plan_info(self._h, ctypes.byref(sl), ctypes.byref(rp), ctypes.byref(wp)))
        self.strip_lanes = sl.value
        self.word_planes = wp.value
        ho = ctypes.c_uint32()
        _check(lib().gol_plan_handoff(self._h, ctypes.byref(ho)))
        self.handoff = bool(ho.value)
        on, nb, ns = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        _check(lib().gol_plan_resident(self._h, ctypes.byref(on), ctypes.byref(nb), ctypes.byref(ns)))
        # resident kernel: (bands, strips) of its tiles, or None
        self.resident = (nb.value, ns.value) if on.value else None
        rr = [ctypes.c_uint32() for _ in range(4)]
        _check(lib().gol_plan_resident_rows(self._h, *(ctypes.byref(v) for v in rr)))
        # resident kernel: rows per wavefront, band rows, epoch K, generations
        # between the wavefronts' LDS row swaps (1: every one), or None
        self.resident_rows = tuple(v.value for v in rr) if on.value else None
        ro, ry, uo = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        _check(lib().gol_plan_skew(self._h, ctypes.byref(ro), ctypes.byref(ry), ctypes.byref(uo)))
        # age-skewed row blocks: (rows_old, rows_young, units_old), or None
        self.age_skew = (ro.value, ry.value, uo.value) if ro.value else None
        st, hu, hg = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        _check(lib().gol_plan_columns(self._h, ctypes.byref(st), ctypes.byref(hu), ctypes.byref(hg)))
        # (strips per row block, half-strip units, half-strip lane groups)
        self.columns = (st.value, hu.value, hg.value)
        tv, tu, mu = ctypes.c_uint32(), ctypes.c_float(), ctypes.c_float()
        _check(lib().gol_plan_tuning(self._h, ctypes.byref(tv), ctypes.byref(tu), ctypes.byref(mu)))
        # autotuner outcome of the first full-depth plan: (variant name, best launch us
        # of the plan that runs, of the models' plan); us 0 = not timed
        self.tuning = (TUNE_VARIANTS[tv.value] if tv.value < len(TUNE_VARIANTS) else str(tv.value),
                       round(tu.value, 2), round(mu.value, 2))
        np_ = ctypes.c_uint32()
        _check(lib().gol_plan_passes(self._h, ctypes.byref(np_)))
        self.passes = np_.value  # passes per full-depth launch (multi-pass launches)
        xm, xb, xo = ctypes.c_uint32(), ctypes.c_float(), ctypes.c_float()
        _check(lib().gol_plan_exchange(self._h, ctypes.byref(xm), ctypes.byref(xb), ctypes.byref(xo)))
        # exchange mode of a stripe engine ("blocking" / "overlapped", None without
        # exchanges) and, when it was chosen by timing at create (exchange_overlap =
        # 0 over RCCL), the max over ranks of each mode's best ms per round
        self.exchange = ({1: "blocking", 2: "overlapped"}.get(xm.value),
                         round(xb.value, 4), round(xo.value, 4))

    def close(self):
        if self._h:
            lib().gol_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def load_ascii(self, data: bytes):
        _check(lib().gol_load_ascii(self._h, data, len(data)))

    def store_ascii(self, nbytes=None) -> bytes:
        n = nbytes if nbytes is not None else self.rows * (self.w + 1)
        buf = ctypes.create_string_buffer(n)
        _check(lib().gol_store_ascii(self._h, buf, n))
        return buf.raw

    def load_packed(self, arr):
        import numpy as np
        a = np.ascontiguousarray(arr, dtype=np.uint64)
        _check(lib().gol_load_packed(self._h, a.ctypes.data, a.shape[1]))

    def store_packed(self, rows=None):
        import numpy as np
        rows = rows if rows is not None else self.rows
        a = np.zeros((rows, self.wq), dtype=np.uint64)
        _check(lib().gol_store_packed(self._h, a.ctypes.data, self.wq))
        return a

    def init_random(self, seed=1):
        _check(lib().gol_init_random(self._h, seed))

    def read_rect(self, y, x, rh, rw):
        """The rh x rw window at field cell (y, x) as packed uint64 [rh, ceil(rw/64)]
        (gol_read_rect: only the window leaves the GPU).  A torus window may cross
        the seams; a rank engine or group member fills its own rows, 0 elsewhere."""
        import numpy as np
        a = np.zeros((rh, (rw + 63) // 64), dtype=np.uint64)
        _check(lib().gol_read_rect(self._h, y, x, rh, rw, a.ctypes.data, a.shape[1]))
        return a

    def write_rect(self, y, x, arr, rw, op=RECT_SET):
        """Combines the packed window `arr` (uint64 [rh, >= ceil(rw/64)], rw columns)
        into the field at cell (y, x) with `op` (RECT_SET / OR / XOR / CLEAR), between
        steps (gol_write_rect).  Rank engines: every rank calls it, like a load."""
        import numpy as np
        a = np.ascontiguousarray(arr, dtype=np.uint64)
        if a.ndim != 2:
            raise GolError(GOL_EINVAL, "the window must be a 2-D uint64 array")
        _check(lib().gol_write_rect(self._h, y, x, a.shape[0], rw, a.ctypes.data, a.shape[1], op))

    def density(self, y, x, rh, rw, by, bx):
        """Live cells per by x bx block of the rh x rw window at (y, x): uint32
        [ceil(rh/by), ceil(rw/bx)] (gol_density; a rank engine counts its own rows)."""
        import numpy as np
        c = np.zeros((-(-rh // by) if by else 0, -(-rw // bx) if bx else 0), dtype=np.uint32)
        _check(lib().gol_density(self._h, y, x, rh, rw, by, bx, c.ctypes.data, c.shape[1]))
        return c

    def step(self, gens):
        _check(lib().gol_step(self._h, gens))

    def sync(self):
        _check(lib().gol_sync(self._h))

    def snapshot(self):
        """Keeps a device copy of the field as it is now in the engine's one snapshot
        slot (gol_snapshot; enqueued, replaces an earlier snapshot)."""
        _check(lib().gol_snapshot(self._h))

    def snapshot_same(self) -> bool:
        """Whether every cell of the field equals the snapshot's (gol_snapshot_same;
        waits for the engine's work, stops reading at the first difference)."""
        v = ctypes.c_uint32()
        _check(lib().gol_snapshot_same(self._h, ctypes.byref(v)))
        return bool(v.value)

    def snapshot_diff(self) -> int:
        """The exact number of cells that differ from the snapshot's (gol_snapshot_diff)."""
        v = ctypes.c_uint64()
        _check(lib().gol_snapshot_diff(self._h, ctypes.byref(v)))
        return v.value

    def snapshot_restore(self):
        """Makes the field the snapshot's field again; the snapshot stays
        (gol_snapshot_restore)."""
        _check(lib().gol_snapshot_restore(self._h))

    def snapshot_drop(self):
        """Frees the snapshot slot (gol_snapshot_drop)."""
        _check(lib().gol_snapshot_drop(self._h))

    def step_until_periodic(self, max_generations, lag, check_every=0, finish=False):
        """Steps until the field repeats with a period that divides `lag`, checking every
        `check_every` generations (0: the least multiple of 64 >= lag), or for
        max_generations (gol_step_until_periodic; uses the snapshot slot).  Returns an
        Until: period (0 = none found), advanced (the generation the engine holds, before
        the rest that finish=True runs to reach max_generations' field), lag,
        check_every, checks, extra_generations."""
        r = Until(struct_size=ctypes.sizeof(Until))
        _check(lib().gol_step_until_periodic(self._h, max_generations, lag, check_every,
                                             UNTIL_FINISH if finish else 0, ctypes.byref(r)))
        return r

    def digest(self):
        live, hsh = ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().gol_digest(self._h, ctypes.byref(live), ctypes.byref(hsh)))
        return live.value, hsh.value

    def digest_rows(self, row0, rows):
        """gol_digest over field rows [row0, row0 + rows) only."""
        live, hsh = ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().gol_digest_rows(self._h, row0, rows, ctypes.byref(live), ctypes.byref(hsh)))
        return live.value, hsh.value

    def comm_info(self):
        """RCCL communicator of a rank engine: dict(count, rank, peer_up, peer_down,
        device) as RCCL reports them (gol_comm_info)."""
        v = [ctypes.c_int() for _ in range(5)]
        _check(lib().gol_comm_info(self._h, *(ctypes.byref(x) for x in v)))
        return dict(zip(("count", "rank", "peer_up", "peer_down", "device"), (x.value for x in v)))

    def set_timing(self, every=1):
        """Time every `every`-th stencil launch with HIP events (0/False = off)."""
        _check(lib().gol_set_timing(self._h, int(every)))

    def reset_timing(self):
        _check(lib().gol_reset_timing(self._h))

    def activity(self):
        """(computed, skipped): units (wavefronts) that computed / skipped a stencil
        launch of step() since create or reset_timing() (gol_activity; waits for
        the engine's stream)."""
        c, k = ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().gol_activity(self._h, ctypes.byref(c), ctypes.byref(k)))
        return c.value, k.value

    def activity_copied(self):
        """Units counted as computed by activity() that stored their rows without
        stage logic (copy-through; gol_activity_copied)."""
        c = ctypes.c_uint64()
        _check(lib().gol_activity_copied(self._h, ctypes.byref(c)))
        return c.value

    def activity_probed(self):
        """Units counted as computed by activity() that a step's first launch found
        still after one generation and stored as they were (the still probe;
        gol_activity_probed).  Not counted in activity_copied()."""
        c = ctypes.c_uint64()
        _check(lib().gol_activity_probed(self._h, ctypes.byref(c)))
        return c.value

    def activity_pass_probed(self):
        """Units counted by activity_probed() that went through on the probe pass's
        word, without a field load in the launch (gol_activity_pass_probed)."""
        c = ctypes.c_uint64()
        _check(lib().gol_activity_pass_probed(self._h, ctypes.byref(c)))
        return c.value

    def activity_pass_kept(self):
        """Tile passes of the probe pass that stored no row because the other buffer
        already held the tile's rows (gol_activity_pass_kept)."""
        c = ctypes.c_uint64()
        _check(lib().gol_activity_pass_kept(self._h, ctypes.byref(c)))
        return c.value

    def activity_pass_sure(self):
        """Of the tile passes activity_pass_kept() counts, those that left before any
        field load: every owner was calm in the remainder launch that ended the step
        before (gol_activity_pass_sure)."""
        c = ctypes.c_uint64()
        _check(lib().gol_activity_pass_sure(self._h, ctypes.byref(c)))
        return c.value

    def activity_short_steps(self):
        """Steps that replayed the short graph: sync() had seen the field at a fixed
        point and nothing wrote it since (gol_activity_short_steps; a host count)."""
        c = ctypes.c_uint64()
        _check(lib().gol_activity_short_steps(self._h, ctypes.byref(c)))
        return c.value

    def activity_fixed_steps(self):
        """Of the steps activity_short_steps() counts, those that ran as one kernel: the
        host also knew that the step before had ended with a remainder launch that found
        every unit calm (gol_activity_fixed_steps; a host count)."""
        c = ctypes.c_uint64()
        _check(lib().gol_activity_fixed_steps(self._h, ctypes.byref(c)))
        return c.value

    def activity_fixed_launches(self):
        """Launches of the fixed step's kernel: one for every run of fixed steps with no
        look at the activity state between them, one per step with GOL_DEV_FIXED_DEFER=0
        (gol_activity_fixed_launches; a host count)."""
        c = ctypes.c_uint64()
        _check(lib().gol_activity_fixed_launches(self._h, ctypes.byref(c)))
        return c.value

    def activity_state(self):
        """The activity state's words as they lie on the device, after everything
        enqueued has run (gol_activity_state): a uint32 array of 12 * units + 3."""
        import numpy as np
        n = ctypes.c_size_t()
        _check(lib().gol_activity_state(self._h, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=np.uint32)
        _check(lib().gol_activity_state(self._h, out.ctypes.data, out.size, ctypes.byref(n)))
        return out

    def activity_elided(self):
        """Calm units whose rows the copy pass left alone because its destination
        already held them (gol_activity_elided).  They stay counted in activity()
        and activity_copied() by the launch that follows the pass."""
        c = ctypes.c_uint64()
        _check(lib().gol_activity_elided(self._h, ctypes.byref(c)))
        return c.value

    def timing(self):
        t = Timing(struct_size=ctypes.sizeof(Timing))
        _check(lib().gol_get_timing(self._h, ctypes.byref(t)))
        if t.struct_size != ctypes.sizeof(Timing):
            raise GolError(GOL_ESTATE, f"libgol.so's gol_timing is {t.struct_size} bytes, "
                                       f"this binding's {ctypes.sizeof(Timing)}")
        return {k: getattr(t, k) for k, _ in Timing._fields_ if k != "struct_size"}


class BatchEngine:
    """n independent h x w fields of one rule (or, after set_rules, one per field) and
    one boundary (SEM_GLOBAL: a dead border per field, SEM_TORUS: a torus per field) on
    one GPU, advanced together by
    one launch per step (gol_batch).  Fields are packed uint64 arrays of shape
    [count, h, ceil(w/64)], or contiguous torch.int64 CUDA tensors of that shape."""

    def __init__(self, n, h, w, rule=REF_RULE, device=-1, semantics=SEM_GLOBAL):
        self.n, self.h, self.w, self.device = n, h, w, device
        self.wq = (w + 63) // 64
        self._h = None
        self.last_trace = None
        self.last_record = None
        cfg = make_config(rule, device, semantics)
        handle = ctypes.c_void_p()
        _check(lib().gol_batch_create(n, h, w, ctypes.byref(cfg), ctypes.byref(handle)))
        self._h = handle
        lpf, fpw, rows, lg = (ctypes.c_uint32() for _ in range(4))
        _check(lib().gol_batch_info(self._h, None, None, None, ctypes.byref(lpf),
                                    ctypes.byref(fpw), ctypes.byref(rows), ctypes.byref(lg)))
        self._info = {"n": n, "h": h, "w": w, "lanes_per_field": lpf.value,
                      "fields_per_wave": fpw.value, "rows_in_regs": rows.value,
                      "launch_generations": lg.value}

    @property
    def info(self):
        """n, h, w, lanes_per_field, fields_per_wave, rows_in_regs and
        launch_generations (the launch cap) of the batch as created."""
        return dict(self._info)

    lanes_per_field = property(lambda self: self._info["lanes_per_field"])
    fields_per_wave = property(lambda self: self._info["fields_per_wave"])
    rows_in_regs = property(lambda self: self._info["rows_in_regs"])
    launch_generations = property(lambda self: self._info["launch_generations"])

    def close(self):
        if self._h:
            lib().gol_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _count(self, first, count):
        return self.n - first if count is None else count

    def load_packed(self, arr, first=0):
        """Fields [first, first + len(arr)) from a uint64 array [count, h, >= ceil(w/64)]
        (bits at columns >= w are ignored)."""
        import numpy as np
        a = np.ascontiguousarray(arr, dtype=np.uint64)
        if a.ndim != 3 or a.shape[1] != self.h:
            raise GolError(GOL_EINVAL, "fields must be a uint64 array [count, h, words]")
        _check(lib().gol_batch_load_packed(self._h, first, a.shape[0], a.ctypes.data,
                                           a.shape[1] * a.shape[2], a.shape[2]))

    def store_packed(self, first=0, count=None):
        """Fields [first, first + count) as a uint64 array [count, h, ceil(w/64)]."""
        import numpy as np
        count = self._count(first, count)
        a = np.zeros((max(count, 0), self.h, self.wq), dtype=np.uint64)
        _check(lib().gol_batch_store_packed(self._h, first, count, a.ctypes.data,
                                            self.h * self.wq, self.wq))
        return a

    def load_tensor(self, t, first=0):
        """load_packed from a contiguous torch.int64 CUDA tensor [count, h, ceil(w/64)]
        on the batch's device (gol_batch_load_device: nothing crosses to the host).
        Waits for torch's current stream first."""
        import torch
        if (t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous() or t.dim() != 3
                or t.shape[1] != self.h or t.shape[2] != self.wq):
            raise GolError(GOL_EINVAL, "fields must be a contiguous torch.int64 CUDA tensor "
                                       "[count, h, ceil(w/64)]")
        torch.cuda.current_stream(t.device).synchronize()
        _check(lib().gol_batch_load_device(self._h, first, t.shape[0], t.data_ptr(),
                                           self.h * self.wq, self.wq))

    def store_tensor(self, first=0, count=None):
        """store_packed into a new contiguous torch.int64 CUDA tensor [count, h,
        ceil(w/64)] on the batch's device (gol_batch_store_device; with device=-1 at
        create that is taken to be torch's current device)."""
        import torch
        count = self._count(first, count)
        dev = torch.device("cuda", self.device if self.device >= 0 else torch.cuda.current_device())
        t = torch.zeros((max(count, 0), self.h, self.wq), dtype=torch.int64, device=dev)
        torch.cuda.current_stream(t.device).synchronize()
        _check(lib().gol_batch_store_device(self._h, first, count, t.data_ptr(),
                                            self.h * self.wq, self.wq))
        return t

    def init_random(self, seed=1):
        """Field i = Engine(h, w).init_random(seed + i)'s field."""
        _check(lib().gol_batch_init_random(self._h, seed))

    def step(self, gens):
        _check(lib().gol_batch_step(self._h, gens))

    def sync(self):
        _check(lib().gol_batch_sync(self._h))

    def step_until_periodic(self, max_generations, lag, check_every=0):
        """Steps every field until it repeats with a period that divides `lag`, checking
        every check_every generations (0: the least multiple of 64 >= lag), or for
        max_generations (gol_batch_step_until_periodic).  On return every field holds
        what step(max_generations) would have left.  Returns a BatchPeriods: period
        (0 = none found) and generation per field, and the call's counters."""
        import numpy as np
        period = np.zeros(self.n, dtype=np.uint32)
        generation = np.zeros(self.n, dtype=np.uint64)
        r = BatchUntil(struct_size=ctypes.sizeof(BatchUntil))
        _check(lib().gol_batch_step_until_periodic(self._h, max_generations, lag, check_every,
                                                   period.ctypes.data, generation.ctypes.data,
                                                   ctypes.byref(r)))
        return BatchPeriods(period, generation, r)

    def _trace_samples(self, generations, every):
        # (the shape of the result; the call itself rejects a bad `every`)
        import operator
        try:
            every = operator.index(every)
        except TypeError:
            every = 0
        if every < 1 or every > 65536:
            raise GolError(GOL_EINVAL, "a batch trace's `every` must be 1..65536")
        return generations // every

    def step_trace(self, generations, every=1):
        """Steps every field `generations` generations and samples its live cells every
        `every` of them, in the kernel (gol_batch_step_trace).  Returns a uint32 array
        [generations // every, n]: row s holds the counts (s + 1) * every generations after
        the call, what digest()[0] would return there.  On return every field holds what
        step(generations) would have left.  The call's counters (every, samples, launches)
        are in last_trace, a BatchTrace."""
        import numpy as np
        live = np.zeros((self._trace_samples(generations, every), self.n), dtype=np.uint32)
        r = BatchTrace(struct_size=ctypes.sizeof(BatchTrace))
        _check(lib().gol_batch_step_trace(self._h, generations, every, live.ctypes.data, self.n,
                                          ctypes.byref(r)))
        self.last_trace = r
        return live

    def step_trace_tensor(self, generations, every=1):
        """step_trace into a new contiguous torch.int32 CUDA tensor [generations // every, n]
        on the batch's device (gol_batch_step_trace_device: no sample crosses to the host;
        with device=-1 at create that is taken to be torch's current device)."""
        import torch
        dev = torch.device("cuda", self.device if self.device >= 0 else torch.cuda.current_device())
        t = torch.zeros((self._trace_samples(generations, every), self.n), dtype=torch.int32,
                        device=dev)
        torch.cuda.current_stream(t.device).synchronize()
        r = BatchTrace(struct_size=ctypes.sizeof(BatchTrace))
        _check(lib().gol_batch_step_trace_device(self._h, generations, every, t.data_ptr(),
                                                 self.n, ctypes.byref(r)))
        self.last_trace = r
        return t

    def _record_shape(self, generations, every, first, count):
        # (the shape of the result; the call itself rejects a bad `every` or window)
        import operator
        try:
            every, first = operator.index(every), operator.index(first)
            count = self.n - first if count is None else operator.index(count)
        except TypeError:
            raise GolError(GOL_EINVAL, "a batch record's every, first and count are integers")
        if every < 1 or every > 65536:
            raise GolError(GOL_EINVAL, "a batch record's `every` must be 1..65536")
        if first < 0 or count < 0 or first + count > self.n:
            raise GolError(GOL_EINVAL, "first + count exceeds the batch's fields")
        return (generations // every, count, self.h, self.wq), first, count

    def step_record(self, generations, every=1, first=0, count=None):
        """Steps every field `generations` generations and records the states of fields
        [first, first + count) every `every` of them, written by the kernel
        (gol_batch_step_record).  Returns a uint64 array [generations // every, count, h,
        ceil(w/64)]: frame s holds what store_packed(first, count) would return (s + 1) *
        every generations after the call (unpack_cells turns frames into cells).  On return
        every field, in the window or not, holds what step(generations) would have left.
        The call's counters (every, samples, launches) are in last_record, a BatchRecord."""
        import numpy as np
        shape, first, count = self._record_shape(generations, every, first, count)
        frames = np.zeros(shape, dtype=np.uint64)
        fs = self.h * self.wq
        r = BatchRecord(struct_size=ctypes.sizeof(BatchRecord))
        _check(lib().gol_batch_step_record(self._h, generations, every, first, count,
                                           frames.ctypes.data, count * fs, fs, self.wq,
                                           ctypes.byref(r)))
        self.last_record = r
        return frames

    def step_record_tensor(self, generations, every=1, first=0, count=None):
        """step_record into a new contiguous torch.int64 CUDA tensor [generations // every,
        count, h, ceil(w/64)] on the batch's device (gol_batch_step_record_device: no frame
        crosses to the host; with device=-1 at create that is taken to be torch's current
        device)."""
        import torch
        shape, first, count = self._record_shape(generations, every, first, count)
        dev = torch.device("cuda", self.device if self.device >= 0 else torch.cuda.current_device())
        t = torch.zeros(shape, dtype=torch.int64, device=dev)
        torch.cuda.current_stream(t.device).synchronize()
        fs = self.h * self.wq
        r = BatchRecord(struct_size=ctypes.sizeof(BatchRecord))
        _check(lib().gol_batch_step_record_device(self._h, generations, every, first, count,
                                                  t.data_ptr(), count * fs, fs, self.wq,
                                                  ctypes.byref(r)))
        self.last_record = r
        return t

    def set_rules(self, birth, survive, first=0):
        """Fields [first, first + len(birth)) get the rules (birth[i], survive[i]), 9-bit
        masks (gol_batch_set_rules).  From the first call on every field steps by the rule
        table, in which a field not set yet holds the create rule."""
        import numpy as np
        try:
            bm = np.asarray(birth, dtype=np.int64)
            sm = np.asarray(survive, dtype=np.int64)
        except (TypeError, ValueError, OverflowError):
            raise GolError(GOL_EINVAL, "birth and survive must be arrays of 9-bit masks")
        if bm.ndim != 1 or bm.shape != sm.shape:
            raise GolError(GOL_EINVAL, "birth and survive must be 1-d arrays of equal length")
        if ((bm < 0) | (bm > 0x1FF) | (sm < 0) | (sm > 0x1FF)).any():
            raise GolError(GOL_EINVAL, "rule masks are 9-bit")
        b = np.ascontiguousarray(bm, dtype=np.uint32)
        s = np.ascontiguousarray(sm, dtype=np.uint32)
        _check(lib().gol_batch_set_rules(self._h, first, b.shape[0], b.ctypes.data, s.ctypes.data))

    def rules(self, first=0, count=None):
        """(birth, survive): two uint32 arrays [count], the rule each field runs (the create
        rule where none was set; gol_batch_get_rules)."""
        import numpy as np
        count = self._count(first, count)
        b = np.zeros(max(count, 0), dtype=np.uint32)
        s = np.zeros(max(count, 0), dtype=np.uint32)
        _check(lib().gol_batch_get_rules(self._h, first, count, b.ctypes.data, s.ctypes.data))
        return b, s

    def drop_rules(self):
        """Back to the one rule given at create (gol_batch_drop_rules)."""
        _check(lib().gol_batch_drop_rules(self._h))

    @property
    def per_field_rules(self):
        """True while the batch steps with a rule table (gol_batch_has_rules)."""
        on = ctypes.c_uint32()
        _check(lib().gol_batch_has_rules(self._h, ctypes.byref(on)))
        return bool(on.value)

    def digest(self, first=0, count=None):
        """(live, hash): two uint64 arrays [count], per field what Engine.digest()
        returns for an h x w engine holding it."""
        import numpy as np
        count = self._count(first, count)
        live = np.zeros(max(count, 0), dtype=np.uint64)
        hsh = np.zeros(max(count, 0), dtype=np.uint64)
        _check(lib().gol_batch_digest(self._h, first, count, live.ctypes.data, hsh.ctypes.data))
        return live, hsh


def _make_transport(fn):
    """Wrap a Python halo exchange `fn(send_up, send_down) -> (recv_up, recv_down)`
    (bytes or None) as a gol_transport; keep the result alive with the engine."""
    def cb(ctx, send_up, recv_up, send_dn, recv_dn, nbytes):
        try:
            su = ctypes.string_at(send_up, nbytes) if send_up else None
            sd = ctypes.string_at(send_dn, nbytes) if send_dn else None
            ru, rd = fn(su, sd)
            for ptr, data in ((recv_up, ru), (recv_dn, rd)):
                if ptr:
                    if data is None or len(data) != nbytes:
                        return 2
                    ctypes.memmove(ptr, data, nbytes)
            return 0
        except Exception:  # a Python error must not unwind through C
            import traceback
            traceback.print_exc()
            return 1
    cfn = HALO_EXCHANGE_FN(cb)
    return Transport(cfn, None), cfn


class Group:
    """`nranks` stripe engines of one field in this process (gol_create_group):
    the multi-GPU partition/halo logic with device-copy transport; stripes may
    share a GPU."""

    def __init__(self, h, w, nranks, devices=None, rule=REF_RULE, tb_depth=0, halo_depth=0,
                 rows_per_wave=0, handoff=0, strip_lanes=0, word_planes=0, exchange_overlap=0,
                 semantics=SEM_GLOBAL):
        self.h, self.w, self.n = h, w, nranks
        cfg = make_config(rule, -1 if devices else 0, semantics, 1, tb_depth, halo_depth,
                          rows_per_wave, handoff, strip_lanes=strip_lanes,
                          word_planes=word_planes, exchange_overlap=exchange_overlap)
        hs = (ctypes.c_void_p * nranks)()
        devs = (ctypes.c_int * nranks)(*(devices or [0] * nranks))
        _check(lib().gol_create_group(h, w, ctypes.byref(cfg), nranks, devs, hs))
        self._hs = hs
        self.members = [Engine(h, w, _handle=ctypes.c_void_p(hs[r])) for r in range(nranks)]

    def close(self):
        for m in self.members:
            m.close()
        self.members = []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def step(self, gens):
        _check(lib().gol_group_step(self._hs, self.n, gens))

    def sync(self):
        for m in self.members:
            m.sync()

    def init_random(self, seed=1):
        for m in self.members:
            m.init_random(seed)

    def load_packed(self, arr):
        for m in self.members:
            m.load_packed(arr[m.row0:m.row0 + m.rows])

    def load_ascii(self, data: bytes):
        for m in self.members:
            m.load_ascii(data[m.row0 * (self.w + 1):(m.row0 + m.rows) * (self.w + 1)])

    def store_packed(self):
        import numpy as np
        return np.concatenate([m.store_packed() for m in self.members])

    def store_ascii(self) -> bytes:
        return b"".join(m.store_ascii() for m in self.members)

    def read_rect(self, y, x, rh, rw):
        """Engine.read_rect of the whole field: the members' windows OR-ed."""
        out = self.members[0].read_rect(y, x, rh, rw)
        for m in self.members[1:]:
            out |= m.read_rect(y, x, rh, rw)
        return out

    def write_rect(self, y, x, arr, rw, op=RECT_SET):
        """Engine.write_rect on every member (each applies its own rows)."""
        for m in self.members:
            m.write_rect(y, x, arr, rw, op)

    def density(self, y, x, rh, rw, by, bx):
        """Engine.density of the whole field: the members' counts added."""
        out = self.members[0].density(y, x, rh, rw, by, bx)
        for m in self.members[1:]:
            out += m.density(y, x, rh, rw, by, bx)
        return out

    def digest(self):
        live = hsh = 0
        for m in self.members:
            a, b = m.digest()
            live += a
            hsh = (hsh + b) & 0xFFFFFFFFFFFFFFFF
        return live, hsh
