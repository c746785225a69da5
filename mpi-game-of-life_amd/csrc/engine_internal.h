// engine_internal.h -- what the host side of libgol.so shares between its
// translation units: the engine struct, the stripe geometry, the error macros and
// the internal functions each unit exports to the others.
//   engine.cpp   C ABI lifecycle, load/store, the resident step, launches and
//                timing, digests, region I/O, plan queries
//   step.cpp     the single-stream step: its launches from the schedule of
//                step_plan.h, run or captured; the short and the fixed step and what
//                gol_sync observes for them; the activity counters' getters
//   plan.cpp     launch planning: column layout, rows per wavefront, age-skewed
//                blocks, hand-off vs classic, the plan autotuner
//   stripes.cpp  multi-GPU stripes: rank geometry and halo rounds, the exchange
//                (RCCL, host transport, device copies) and its mode, rank and
//                group engines
//   torus.cpp    torus engines: ghost-zone geometry, wrap rounds around an inner
//                dead-border engine, I/O and digests of the interior
//   snapshot.cpp the snapshot slot: keep / compare / restore a generation on the
//                device, and gol_step_until_periodic on top of the public calls
// Mirrors main()'s flow in Parallel_Life_MPI.cpp:190-240: create
// (readGridFromFile's allocation :88-89) -> load (:91-99) -> step (the epoch loop
// :215-221 with the halo exchange :104-145) -> store (:157-164).
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/gol.h"
#include "bitlayout.h"
#include "life_internal.h"
#include "rect_blit.h"
#include "step_plan.h"
#include "still_pending.h"

namespace golh __attribute__((visibility("hidden"))) {

using gol::SegDesc;
using gol::StepArgs;

extern thread_local std::string g_last_error;

#if GOL_WAVE_LOG
// device buffer the kernels log per-wavefront stamps into (life_internal.h); set by
// gol_dev_set_wave_log
extern uint64_t* g_dev_wave_log;
#endif

// The activity state (gol_engine::d_streak; StepArgs in life_internal.h says how
// the kernel uses each region): words of a buffer of `units` units, on the device
// or a host copy of it.
struct ActState {
    uint32_t* base;
    size_t units;
    // per unit: quiet launches so far, as the launches of one parity wrote them
    uint32_t* streak(int parity) const { return base + (size_t)parity * units; }
    // per unit: launches computed, launches skipped
    uint32_t* act() const { return base + 2 * units; }
    // per unit: launches copied through
    uint32_t* copied() const { return base + 4 * units; }
    // [0] launches that skipped as a whole, [1] index + 1 of the step's last launch
    // in which a unit stored rows
    uint32_t* busy() const { return base + 5 * units; }
    // per unit: first launches of a step that found it still after one generation
    uint32_t* probed() const { return base + 5 * units + 2; }
    // per unit: the copy pass's flags (life_copy.hip: calm and its rows to be moved),
    // rewritten by every pass
    uint32_t* need() const { return base + 6 * units + 2; }
    // per unit: 1 = took the still probe's quiet exit in the step's first launch,
    // rewritten by every launch that probes
    uint32_t* held() const { return base + 7 * units + 2; }
    // per unit: passes that found it calm with its rows already in the destination
    uint32_t* elided() const { return base + 8 * units + 2; }
    // per unit: the probe pass's word (life_probe.hip), zeroed before every pass: 1 =
    // a tile that meets the unit's dilated rectangles changes in one generation
    uint32_t* moved() const { return base + 9 * units + 2; }
    // per unit: first launches that took it through on the probe pass's word
    uint32_t* pass_probed() const { return base + 10 * units + 2; }
    // per unit: 1 or 2 = both field buffers hold the unit's rows, word for word, as the
    // step's last launch left them (life_copy.hip writes it, life_probe.hip reads it in
    // the next step); it says so only while *twin_ok is 1, which every other writer
    // of the field clears (DESIGN §4 "Probe pass: rows both buffers hold"); 2 = written
    // before a remainder launch: the unit's rows also keep their state for one more
    // generation (DESIGN §4 "Sure tiles")
    uint32_t* twin() const { return base + 11 * units + 2; }
    uint32_t* twin_ok() const { return base + 12 * units + 2; }
    size_t words() const { return 12 * units + 3; }
};

// gol_create splits GLOBAL fields of at least this many rows into 2 same-device
// stripes on 2 streams (measured +11% at 65536^2; no gain at <= 16384 rows,
// profiles/r01/group_bench_*.jsonl)
constexpr uint64_t kCompositeMinRows = 32768;
// captured step graphs kept per engine (least recently used evicted)
constexpr size_t kGraphCache = 8;

// Auto launch layout: fused depth K and planes per lane group (bitlayout.h).
//  * K = 16 with 2 planes (one word per lane; ~230 VGPRs, 2 waves/SIMD, enough
//    for full VALU issue) for stripes of more than 6144 rows: 124.5 TCUPS at
//    65536^2 vs 122.4 (K = 8) and 106.0 (K = 12); K >= 20 drops to 1 wave/SIMD
//    and loses 30-35% (profiles/r01/sweep_total_sum_depth.jsonl).
//  * Short fields are launch-latency bound and keep K = 8 (4096^2: 11.0-11.6
//    TCUPS vs 8.7 at K = 16).
//  * Rules other than B/S2 and B3/S23 evaluate a 10-term mask sum whose K = 16
//    state spills: K = 12.
//  * 4 planes (two words per lane) only on request (dev build), with K = 8.
struct Layout {
    uint32_t K;
    int planes;
};

inline Layout auto_layout(uint64_t rows, const gol_config* cfg)
{
    const bool fixed = (cfg->birth_mask == GOL_REF_BIRTH && cfg->survive_mask == GOL_REF_SURVIVE) ||
                       (cfg->birth_mask == GOL_CONWAY_BIRTH &&
                        cfg->survive_mask == GOL_CONWAY_SURVIVE);
    Layout l;
    l.planes = cfg->word_planes ? (int)cfg->word_planes : 2;
    // resident = 2 takes any epoch length; the streaming launches of an engine
    // that cannot run the resident kernel (rank engines, composite parts, fields
    // it does not fit) then use the auto depth when that length has no stencil
    // kernel, instead of failing
    const bool res_only = cfg->resident == 2 && cfg->tb_depth &&
                          !gol::life_has_kernel((int)cfg->tb_depth, l.planes);
    if (cfg->tb_depth && !res_only)
        l.K = cfg->tb_depth;
    else if (cfg->word_planes == 4 || rows <= 6144)
        l.K = 8;
    else
        l.K = fixed ? 16 : 12;
    return l;
}

inline gol_status fail(gol_status st, const std::string& msg)
{
    g_last_error = msg;
    return st;
}

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess)                                                               \
            return fail(_e == hipErrorOutOfMemory ? GOL_ENOMEM : GOL_EHIP,                  \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                 \
    } while (0)

#define NCCL_TRY(expr)                                                                      \
    do {                                                                                    \
        ncclResult_t _r = (expr);                                                           \
        if (_r != ncclSuccess)                                                              \
            return fail(GOL_ERCCL, std::string(#expr) + ": " + ncclGetErrorString(_r));     \
    } while (0)

#define GOL_TRY(expr)                                                                       \
    do {                                                                                    \
        gol_status _s = (expr);                                                             \
        if (_s != GOL_OK) return _s;                                                        \
    } while (0)

inline uint64_t last_mask(uint64_t w)
{
    const unsigned rem = (unsigned)(w & 63);
    return rem ? ((1ull << rem) - 1ull) : ~0ull;
}

// Parallel_Life_MPI.cpp:70-81 -- rank r's extended stripe [start, start+rows).
inline bool ref_stripe(uint64_t h, uint64_t P, uint64_t r, uint64_t* start, uint64_t* rows)
{
    if (P == 0 || r >= P || h / P == 0) return false;
    uint64_t chunk = h / P, s = r * chunk;
    if (r != 0) {
        s--;
        chunk++;
    }
    chunk += (r == P - 1) ? h % P : 1;
    *start = s;
    *rows = chunk;
    return true;
}

// Scoped device allocation (staging for the ASCII codec).
struct DeviceBytes {
    char* p = nullptr;
    ~DeviceBytes()
    {
        if (p) (void)hipFree(p);
    }
};

// A host-visible region of the field: buffer rows [buf_row, buf_row+rows) are field
// rows [glob_row, glob_row+rows); it corresponds to the caller's ASCII/packed rows
// [user_row, user_row+rows).
struct Region {
    uint64_t buf_row, glob_row, user_row, rows;
};

// Geometry of stripe `rank` of `nranks` (GLOBAL field), host-only: its rows, the
// halo depth, the fused depth, and the segment tables of its launch plans --
// plans[c-1] computes the local rows still valid after a cumulative shrink c of a
// round (c = 1..Hx); with overlap, plans[Hx] (band: the rows the neighbours need)
// and plans[Hx+1] (interior) split the round's last launch.  Shared by the rank
// engines and gol_round_schedule, so the exported schedule is the one run.
// `overlap`: the mode the schedule starts in; `band`: the band and interior plans
// exist (overlap, or an exchange mode to be chosen by timing: `tune`).
struct RankGeom {
    uint64_t row0 = 0, R = 0, Hx = 0, buf_rows = 0;
    uint32_t K = 8;
    bool overlap = false, band = false, tune = false;
    std::vector<std::vector<SegDesc>> raw;
};

gol_status rank_geometry(uint64_t h, const gol_config* cfg, int rank, int nranks, RankGeom* g,
                         bool group = false, bool tune_ok = false);

}  // namespace golh

using namespace golh;  // (internal header: the library's own units only)

// The kinds of exchange a stripe engine does (gol_create_rank /
// gol_create_rank_transport / gol_create_group).
enum XferKind { XFER_NONE = 0, XFER_RCCL = 1, XFER_HOST = 2, XFER_GROUP = 3 };

struct gol_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    uint64_t H = 0, W = 0, wq = 0, stride = 0, lastmask = 0;
    int planes = 2;                      // planes per lane group (bitlayout.h)
    uint64_t ng = 0;                     // lane groups per row
    uint64_t lastmask_split[2] = {0, 0};  // stored form of the last group's valid bits
    uint32_t birth = 0, survive = 0;
    gol::RuleKind rule = gol::RULE_REF;
    uint32_t K = 8;
    uint32_t rows_per_wave = 0;
    int lane_shift = -1;  // strip width 64 >> lane_shift; -1 = chosen per plan
    uint32_t handoff = 0; // gol_config.handoff
    uint32_t sem = GOL_SEM_GLOBAL;
    uint32_t P = 1;

    // rank geometry (single-GPU: rank 0 of 1, Hx = 0)
    int rank = 0, nranks = 1;
    uint64_t row0 = 0, R = 0, Hx = 0;
    XferKind xfer = XFER_NONE;
    ncclComm_t comm = nullptr;
    // RCCL peers of the up/down halo (rank -+ 1; both 0 for the self-loop test
    // communicator of GOL_DEV_RCCL_SELF, gol_create_rank)
    int peer_up = -1, peer_dn = -1;
    gol_transport tp{nullptr, nullptr};
    uint64_t* host_xfer = nullptr;  // pinned: send_up | recv_up | send_dn | recv_dn

    // in-process group (gol_create_group): halo exchange by device copies
    gol_engine* up = nullptr;
    gol_engine* down = nullptr;
    bool grouped = false;
    // other engines launch on this device concurrently (composite parts, group
    // members sharing a GPU): the age skew's dispatch-order premise does not hold
    bool shared_device = false;
    // registered in the device's waiting-kernel registry (wait_registry) as the
    // hand-off engine / as a resident engine
    bool reg_hand = false, reg_res = false;
    hipEvent_t ev_ready = nullptr, ev_copied = nullptr;

    // exchange/compute overlap (multi-rank): the last launch of a full round is
    // split into a band launch (the rows the neighbours need) and an interior
    // launch; the exchange runs on `comm_stream` between them.  halo_fresh: the
    // current buffer's halo rows were already exchanged (completion signalled by
    // ev_xdone on comm_stream).  The band launch runs on its own stream,
    // concurrently with the interior launch: it is a few hundred rows, far too
    // few wavefronts to fill the GPU.
    hipStream_t comm_stream = nullptr, band_stream = nullptr;
    hipEvent_t ev_band = nullptr, ev_xdone = nullptr, ev_in = nullptr, ev_join = nullptr;
    bool overlap = false;     // the mode gol_step runs (RankGeom::overlap at create)
    bool band_plans = false;  // the band and interior plans exist (RankGeom::band)
    bool halo_fresh = false;
    // (late r06) exchange_overlap = 0 on a rank engine over RCCL: both modes timed at
    // create (tune_exchange), the max over ranks of each mode's best sample (ms);
    // 0 = not timed
    bool xchg_tune = false;
    float xchg_ms[2] = {0.f, 0.f};  // blocking, overlapped

    // composite engine (gol_create, large GLOBAL fields): the field is S row
    // stripes on S streams of this device (a gol_create_group), so one stripe's
    // launch tail overlaps the others' work; every call is routed to the parts
    std::vector<gol_engine*> parts;

    // torus engine (gol_create, GOL_SEM_TORUS; torus.cpp): the h x w interior lives
    // inside `inner`, a single-stream GLOBAL engine of the padded field, at row tG,
    // word tGx; gol_step wraps the ghosts every tG generations.  H, W, wq, lastmask
    // describe the interior; every call is routed to torus.cpp or to `inner`
    gol_engine* inner = nullptr;
    uint64_t tG = 0, tGx = 0;

    uint64_t buf_rows = 0;
    // state buffers: 2, or 4 with multi-pass launches (a launch of P <= 3 passes
    // reads buf[cur] and writes buf[cur + 1 .. cur + P], mod nbuf); those also hold
    // a shadow half (shadow_off bytes after each row) for the strips' halo lanes
    uint64_t* alloc[4] = {nullptr, nullptr, nullptr, nullptr};
    uint64_t* buf[4] = {nullptr, nullptr, nullptr, nullptr};
    int cur = 0;
    int nbuf = 2;
    uint32_t npass = 1;       // passes per full-depth launch the engine may run
    uint32_t xcd_shift = 0;   // (r06 dev A/B) StepArgs::xcd_shift, GOL_DEV_XCD_SHIFT
    uint32_t shadow_off = 0;  // bytes from a buffer word to its shadow
    uint32_t* mpflags = nullptr;  // multi-pass head/done flags: 4 x max units

    // plans: plan p = a device table of nseg SegDesc (+ host copy)
    struct Plan {
        std::vector<SegDesc> segs;
        int32_t groups = 0;      // strip groups per row block (StepArgs::strips)
        int32_t lane_shift = 0;  // strips of 64 >> lane_shift lanes
        double own_rows = 0;  // output rows of this plan that are the caller's rows
        int64_t rpw = 0;      // rows per wavefront
        int64_t total_units = 0;
        bool multi_blk = false;  // some segment has more than one row block
        bool hand = false;       // the planner chose hand-off row blocks
        // age-skewed row blocks (age_skew; 0 = off): the same blocks per strip, the
        // first-dispatched units rows_old rows, the others rows_young (both = rpw
        // mod the prefetch block, so the hand-off tail offset is rpw's)
        int32_t rows_old = 0, rows_young = 0, units_old = 0;
        // 64-lane strips: edge-aligned columns (col_layout) and the packed half
        // strip's units after the full strips' (pairs: 3 words per unit)
        int32_t edge = 0;
        int64_t right_q0 = -1, half_q0 = 0, half_hi = -1;
        int64_t pair_units = 0, half_rows = 0;
        std::vector<int64_t> pairs;
        int64_t* dpairs = nullptr;
        SegDesc* dev = nullptr;
        // activity skip (build_neighbours): the units' neighbour lists, CSR; on the
        // device the offsets followed by the ids.  Empty: the plan never skips
        std::vector<uint32_t> nb_off, nb_ids;
        uint32_t* d_nb = nullptr;
        // copy pass (life_copy.hip): the owners of its tiles, kCopyOwners slots per
        // tile, uploaded next to d_nb.  Empty: the plan takes no pass
        std::vector<uint32_t> owners;
        uint32_t* d_own = nullptr;
        int32_t copy_ncol = 0;
        // probe pass (life_probe.hip): per tile of the copy pass the units one of whose
        // rectangles, dilated by K - 1 cells, meets it; kProbeSlots slots per tile.
        // Empty: the plan takes no probe pass (its first launch probes in the kernel)
        std::vector<uint32_t> probe_tiles;
        uint32_t* d_ptab = nullptr;
        // a copy of an earlier plan of the same rows (rank engines: the full-depth
        // launches of a round share one plan); its device tables are the owner's
        bool alias = false;
        // passes per full-depth launch of this plan (multi-pass launches, life_stencil.h:
        // one-segment plans of one round without the half strip; 1 = single pass)
        int32_t npass = 1;
        // autotuner: the candidate that runs (0 = the models' plan, else 1 + the
        // index in kTuneVariantNames) and its best create-time launch vs the
        // models' plan (ms; 0 = not tuned)
        int32_t tuned = 0;
        float tune_ms = 0.f, tune_ms_model = 0.f;
    };
    std::vector<Plan> plans;  // GLOBAL/REF: plans[0]; rank: see RankGeom
    std::vector<int> plan_alias;  // plans[i] copies plans[plan_alias[i]] (-1: own plan)
    std::vector<std::vector<Plan>> plan_alts;  // autotuner candidates per plan (build_plans)
    // host-only planning (gol_plan_model): build_plans takes the device's CU count
    // and occupancies from here and makes no device call or allocation
    struct DevModel {
        bool on = false;
        int cus = 0, occ_c = 0, occ_h = 0;
    } model;

    // row-block hand-off buffers (life_stencil.h): region 0 serves launches on
    // `stream`, region 1 those on `band_stream` (the two may run concurrently)
    uint64_t* side[2] = {nullptr, nullptr};
    uint32_t* flags[2] = {nullptr, nullptr};
    int* d_err = nullptr;

    // Activity skip (life_stencil.h).  d_streak: the device state of
    // act_units units, laid out as ActState says (single-GPU engines with a plan).
    // What each launch of a gol_step does with it is the schedule's to say
    // (step_plan.h); the engine keeps no state of a step: history never outlives one,
    // so nothing that touches the field between steps can leave a stale streak.
    uint32_t* d_streak = nullptr;
    int64_t act_units = 0;
    // what the schedule reads of this engine (engine.cpp step_traits, made on first
    // use; gol_set_timing keeps its interval, the one part that changes, in step)
    golh::StepTraits traits;
    bool traits_ok = false;
    // what the engine may do, decided at create:
    bool act_on = false;    // skip units at all
    int through_on = 0;     // copy-through: 0 = off, 1 = launches at depth K, 2 = the
                            // remainder launches too (GOL_DEV_COPY_THROUGH, default 2)
    bool pass_on = false;   // the copy pass before a step's second launch and its
                            // remainder launches (GOL_DEV_COPY_PASS=0 turns it off)
    bool still_on = false;  // the one-load exit (GOL_DEV_STILL_EXIT=0 turns it off)
    bool probe_on = false;  // the still probe (GOL_DEV_STILL_PROBE=0 turns it off)
    bool elide_on = false;  // the copy pass leaves rows its destination already holds
                            // (GOL_DEV_COPY_ELIDE=0 turns it off)
    bool ppass_on = false;  // the probe pass before a step's first launch
                            // (GOL_DEV_PROBE_PASS=0 turns it off)
    bool twin_on = false;   // the probe pass leaves rows that both buffers hold
                            // (GOL_DEV_TWIN=0 turns it off)
    // per tile of plan 0's probe pass: passes that left the tile's rows unstored
    uint32_t* d_kept = nullptr;
    int64_t kept_tiles = 0;
    // sure tiles: a remainder launch that ends a step writes twin = 2, and a tile of
    // the next probe pass whose owners all have it leaves before its field loads
    // (GOL_DEV_TWIN_SURE=0 turns it off; only with twin_on).  d_sure: per tile, the
    // passes in which it left so (kept_tiles words).
    bool sure_on = false;
    uint32_t* d_sure = nullptr;
    // Short step: gol_sync found twin_ok set and every unit's twin 2, so
    // the field is a fixed point, and nobody has written it since (twin_clear withdraws
    // the flag, on whatever stream it is called).  A captured step of 5 or more depth-K
    // launches then replays a graph without the stencil kernels of launches 4 .. n.
    // short_on: GOL_DEV_SHORT_STEP, 0 = off, 1 = on (needs sure_on, the only writer of
    // 2), 2 = take the short graph wherever the shape allows (the error-code test).
    // twin_fresh: a step ran since gol_sync last read twin[] (into sync_host);
    // short_steps: steps that replayed a short graph (gol_activity_short_steps).
    int short_on = 0;
    bool still_seen = false;
    bool twin_fresh = false;
    uint64_t short_steps = 0;
    uint32_t* sync_host = nullptr;  // pinned, act_units + 2 words: d_err, twin[], twin_ok
    // Fixed step: on a fixed point whose twin[] words the host knows to be 2,
    // a step is life_still_step_kernel alone, launched directly.
    // fixed_on: GOL_DEV_FIXED_STEP, 0 = off, 1 = on, 2 = after every step that ended with
    // a remainder launch, seen or not (the error-status test); 0 wherever the plan or
    // the switches leave one of the kernels the path stands for out (create).
    // twin_two: gol_sync saw a 2 in every unit's word, and every step since ended with a
    // remainder launch on the still field (twin_clear and a step that ends with a
    // depth-K launch, which writes 1, withdraw it).  rem_ended: the engine's last step
    // ended with a remainder launch, whatever happened since (fixed_on == 2 only).
    // fixed_steps: steps that took the path; fixed_passes: their probe passes, each of
    // which counts every one of plan 0's owned_tiles in kept[] and sure[] (added on the
    // host, gol_activity_pass_kept / _sure, so that no step touches those arrays).
    int fixed_on = 0;
    bool twin_two = false;
    bool rem_ended = false;
    uint64_t fixed_steps = 0;
    uint64_t fixed_passes = 0;
    int64_t owned_tiles = 0;
    // Pending fixed steps (still_pending.h): with defer_on (GOL_DEV_FIXED_DEFER, default
    // on; 0 = one kernel per step) a fixed step does its host part at once and folds
    // its effect on the device state into `pending`; flush_still launches the one kernel
    // that stands for all of them before anybody reads or writes the activity state or
    // the error word.  fixed_launches: launches of life_still_step_kernel
    // (gol_activity_fixed_launches).  still_memo: still_effect() of the last length a
    // fixed step had (still_memo_gens, 0 = none), so that a repeat walks no schedule.
    bool defer_on = false;
    golh::StillPending pending;
    uint64_t fixed_launches = 0;
    uint64_t still_memo_gens = 0;
    gol_still_effect still_memo{};

    // resident kernel (life_resident.hip): small GLOBAL fields, one launch per
    // gol_step; flags count the epochs published, from flag_base on
    struct Resident {
        bool on = false;
        int rows = 0;  // rows per wavefront
        int32_t strips = 0, bands = 0, band_rows = 0, K = 0;
        uint32_t* flags = nullptr;
        uint32_t flag_base = 0;
        // hipLaunchCooperativeKernel (GOL_DEV_RES_COOP=1): the device re-checks that
        // every tile fits at once, but the launch costs ~30 us more (C2: 640 vs
        // 609-614 us per 1000 generations, profiles/r03/ab_resident_coop.jsonl);
        // the planner's occupancy check and the bounded waits cover it by default
        bool coop = false;
        // wave-level temporal blocking (life_resident_mb.hip): wavefronts swap rows
        // through LDS every `mb` generations; 1 = every generation (life_res_kernel)
        int mb = 1;
        hipEvent_t ev_in = nullptr, ev_out = nullptr;  // ordering with the shared stream
    } res;

    std::vector<Region> user_regions;  // load/store mapping (own output rows)
    std::vector<Region> load_regions;  // rows loaded (REF_STRIPES loads overlaps too)

    unsigned long long* d_acc = nullptr;
    int* d_flag = nullptr;  // ASCII codec error flag
    // snapshot slot (snapshot.cpp, DESIGN §4 "Snapshots"): a copy of one whole field
    // buffer, guard, halo and ghost rows included, allocated by the first gol_snapshot;
    // snap_set: it holds a field.  A composite engine's stripes and a torus engine's
    // inner engine hold the slots; the engine the caller sees holds none
    uint64_t* snap = nullptr;
    unsigned long long* snap_host = nullptr;  // pinned: where a comparison's answer lands
    bool snap_set = false;
    // region I/O: device staging kept between calls (engine.cpp rect_stage)
    char* rect_stage = nullptr;
    size_t rect_stage_bytes = 0;

    // single-stream engines replay a captured hipGraph of the launch sequence of a
    // gol_step(gens) call (keyed by gens and the starting buffer), so a step of
    // many short launches costs one graph launch of host work
    struct GraphEntry {
        hipGraphExec_t exec;
        int cur_after;
        uint64_t used;
    };
    std::map<std::pair<uint64_t, int>, GraphEntry> graphs;
    uint64_t graph_clock = 0;

    // timing: HIP events around every `timing_every`-th stencil launch (0 = off)
    uint32_t timing_every = 0;
    uint64_t launch_count = 0;
    std::vector<hipEvent_t> ev_free;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pending;
    std::vector<double> pending_cells, pending_cells_comp, pending_rows;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_xpending;  // exchanges
    std::vector<char> xpending_blocking;  // ... on the compute stream (1) or comm (0)
    // rank engines, per round: the compute stream's span from before the round's
    // first launch to after its last (band launch joined), and the end of the
    // overlapped exchange issued in that round (null when it blocks)
    struct RoundEv {
        hipEvent_t start, end, xend;
    };
    std::vector<RoundEv> ev_rpending;
    gol_timing tm{};
};

namespace golh __attribute__((visibility("hidden"))) {

// One operation of a stripe engine's step (gol_sched_op without the rows).
struct SchedOp {
    uint32_t kind, depth;
    int plan;  // launch ops: index into the plans (RankGeom)
};

// ---- engine.cpp
gol_status check_cfg(const gol_config* cfg);
gol_status host_layout(gol_engine* e, uint64_t h, uint64_t w, const gol_config* cfg);
gol_status init_common(gol_engine* e, uint64_t h, uint64_t w, const gol_config* cfg,
                       const RankGeom* geom);
gol_status plan_resident(gol_engine* e, const gol_config* cfg);
// One stencil launch of `plan` and the kernels that go with it.  rec: the launch's
// record in the schedule of a single-stream step (step.cpp), which says all that the
// launch does with the activity state; every other caller passes none, and the launch
// leaves that state alone but for twin_ok, which a launch of plan 0 clears.
// skip_stencil: everything but the stencil kernel itself (the short graph).
gol_status launch(gol_engine* e, int plan, uint32_t depth, bool swap = true,
                  hipStream_t stream = nullptr, int passes = 1, const StepLaunch* rec = nullptr,
                  bool skip_stencil = false);
const StepTraits& step_traits(gol_engine* e);
gol_status step_resident(gol_engine* e, uint64_t generations);
gol_status get_event(gol_engine* e, hipEvent_t* ev);
gol_status join_side_streams(gol_engine* e);
gol_status quiesce(gol_engine* e);
gol_status check_err(gol_engine* e);
// Every writer of a field buffer other than an activity step's own launches calls
// this: ActState::twin says nothing about the buffers from here on (a 4-byte memset
// on the engine's stream, a memset node inside a captured step).
gol_status twin_clear(gol_engine* e, hipStream_t s = nullptr);

// Region I/O (gol_read_rect / gol_write_rect / gol_density).  A piece is a
// non-wrapping rectangle in a leaf engine's field coordinates -- rows [frow, frow +
// rows) x columns [fcol, fcol + cols) -- whose first cell is cell (wrow, wcol) of the
// caller's window.  The leaf_ functions apply pieces to the rows of `regs` (field row
// -> buffer row, as user_regions) of the view that starts word_off words into each
// buffer row (0, or a torus interior's ghost words).  leaf_read fills only the
// pieces' bits of `words`; leaf_density adds to `counts`.
struct RectPiece {
    uint64_t frow, fcol, rows, cols, wrow, wcol;
};
gol_status leaf_read(gol_engine* e, const std::vector<Region>& regs, uint64_t word_off,
                     const RectPiece* pcs, size_t npc, uint64_t* words, uint64_t rs);
gol_status leaf_write(gol_engine* e, const std::vector<Region>& regs, uint64_t word_off,
                      const RectPiece* pcs, size_t npc, const uint64_t* words, uint64_t rs,
                      uint32_t op);
gol_status leaf_density(gol_engine* e, const std::vector<Region>& regs, uint64_t word_off,
                        const RectPiece* pcs, size_t npc, uint64_t by, uint64_t bx, uint64_t nby,
                        uint64_t nbx, uint32_t* counts, uint64_t cs);

// ---- plan.cpp
struct URect {
    int64_t r0, r1, q0, q1;  // rows [r0, r1) x lane groups [q0, q1)
};
void unit_rects(const gol_engine::Plan& p, int64_t ng, std::vector<URect>& out);
void build_neighbours(gol_engine::Plan& p, int64_t ng, int K);
bool handoff_fits(int64_t R, int d, int planes);
bool single_stream_skews(uint64_t h, uint64_t w, const gol_config* cfg);
void free_plan(gol_engine::Plan& q);
gol_status build_plans(gol_engine* e, const std::vector<std::vector<SegDesc>>& raw);
void decide_passes(gol_engine* e, size_t words);
gol_status autotune_plans(gol_engine* e);
void resolve_aliases(gol_engine* e);

// ---- torus.cpp
// Geometry of a torus engine: inner depth K (streaming launches), generations per
// wrap round = ghost rows G, ghost words Gx per side, padded field ph x pw.
struct TorusGeom {
    uint32_t K = 0, G = 0;
    uint64_t Gx = 0, ph = 0, pw = 0;
};
gol_status torus_geometry(uint64_t h, uint64_t w, const gol_config* cfg, TorusGeom* g);
gol_status torus_create(uint64_t h, uint64_t w, const gol_config* cfg, gol_engine** out);
gol_status torus_step(gol_engine* e, uint64_t generations);
gol_status torus_load_packed(gol_engine* e, const uint64_t* words, uint64_t rs);
gol_status torus_store_packed(gol_engine* e, uint64_t* words, uint64_t rs);
gol_status torus_load_ascii(gol_engine* e, const char* buf, size_t len);
gol_status torus_store_ascii(gol_engine* e, char* buf, size_t len);
gol_status torus_init_random(gol_engine* e, uint64_t seed);
gol_status torus_digest_rows(gol_engine* e, uint64_t row0, uint64_t rows, uint64_t* live,
                             uint64_t* hash);
gol_status torus_read_rect(gol_engine* e, uint64_t y, uint64_t x, uint64_t rh, uint64_t rw,
                           uint64_t* words, uint64_t rs);
gol_status torus_write_rect(gol_engine* e, uint64_t y, uint64_t x, uint64_t rh, uint64_t rw,
                            const uint64_t* words, uint64_t rs, uint32_t op);
gol_status torus_density(gol_engine* e, uint64_t y, uint64_t x, uint64_t rh, uint64_t rw,
                         uint64_t by, uint64_t bx, uint64_t nby, uint64_t nbx, uint32_t* counts,
                         uint64_t cs);

// ---- snapshot.cpp
void snapshot_free(gol_engine* e);

// ---- step.cpp
gol_status step_single(gol_engine* e, uint64_t generations);
gol_status sync_observing(gol_engine* e);
// Pending fixed steps (still_pending.h) reach the device: one life_still_step_kernel on
// the engine's stream for all of them.  Whoever enqueues work on that stream that reads
// or writes the activity state or the error word, or reads them on the host, calls this
// first (DESIGN §4 "Fixed step" lists the callers); with nothing pending it tests one
// word.  Every caller has made the engine's device the current one.
gol_status flush_still_launch(gol_engine* e);
inline gol_status flush_still(gol_engine* e)
{
    return e->pending.steps ? flush_still_launch(e) : GOL_OK;
}

// ---- stripes.cpp
inline uint32_t pick_depth(uint32_t K, uint64_t remaining)
{
    return pick_depth(gol::kDepthList, (int)std::size(gol::kDepthList), K, remaining);
}
void step_schedule(uint32_t K, uint64_t Hx, bool overlap, bool halo_fresh, uint64_t gens,
                   std::vector<SchedOp>& ops);
gol_status step_stripe(gol_engine* e, uint64_t generations);

}  // namespace golh
