// Internal interface between the host engine (engine.cpp) and the HIP kernels
// (life_stencil.h, life_tb_d*.hip, life_aux.hip).  Not part of the public C ABI
// (include/gol.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef GOL_DEV_KERNELS
#define GOL_DEV_KERNELS 0
#endif
// Dev timing build only (tools/variant_build.sh wavelog "-DGOL_WAVE_LOG=1"): every
// wavefront of the stencil and resident kernels logs its start/end stamps and its
// hardware id (the stencil kernel its phase stamps too) into the buffer given to
// gol_dev_set_wave_log (tools/wave_log.py, tools/res_log.py).  The field stays valid.
#ifndef GOL_WAVE_LOG
#define GOL_WAVE_LOG 0
#endif

namespace gol {

// Rule specialisations of the stencil kernel.
enum RuleKind : int {
    RULE_REF = 0,     // birth = {}, survive = {2}: the reference's effective rule
    RULE_CONWAY = 1,  // birth = {3}, survive = {2,3}
    RULE_GENERIC = 2,  // any 9-bit mask pair, full 0..8 neighbour count
    RULE_LANE = 3      // a mask pair per lane (batches with per-field rules, life_rule_lane.h)
};

// One independent field region streamed by the stencil kernel.
//   Buffer row (base_row + i) holds segment-local row i.  Local row i is field row
//   (glob0 + i); field rows outside [0, field_h) are dead (never loaded, forced 0).
//   The kernel reads local rows [out_lo - K, out_hi + K) (only those inside
//   [0, in_rows) and inside the field; others read as dead) and writes local rows
//   [out_lo, out_hi) of the output buffer.
struct SegDesc {
    int64_t base_row;
    int64_t in_rows;
    int64_t glob0;
    int64_t field_h;
    int64_t out_lo, out_hi;
    int64_t nblk;   // row blocks of rows_per_wave rows
    int64_t unit0;  // index of this segment's first wavefront in the launch
};

// Strips: a strip is L consecutive lanes (L = 64 >> lane_shift: 64, 32 or 16),
// each holding one lane group of a row (NP 32-bit planes = NP/2 words,
// bitlayout.h); its first and last lane are the horizontal halo (exact for up to
// 63 fused generations), so a strip outputs L - 2 groups.  A wavefront runs 64 / L
// strips side by side over the same rows: narrow strips trade 2 halo lanes per
// strip for more wavefronts per row block, which lets short stripes use longer row
// blocks (less vertical halo recompute).
constexpr int kStripOut = 62;  // output lane groups of a full 64-lane strip
constexpr int kWavesPerBlock = 4;
// Zeroed guard rows allocated before/after every state buffer so that the
// streaming loads (K rows of halo + prefetch distance) never leave the allocation.
constexpr int kGuardRows = 64;
constexpr int kMaxDepth = 32;

struct StepArgs {
    // state buffers, row 0 (guard rows precede it): pass p of the launch reads
    // pbuf[p] and writes pbuf[p + 1]
    uint64_t* pbuf[4];
    // multi-pass launches (life_stencil.h): passes (1 = single), the byte offset of
    // the halo lanes' shadow half of each buffer, and the head/done flags (4 x
    // total_units words, all 0 between launches)
    int32_t npass;
    uint32_t shadow_off;
    uint32_t* mpflags;
    const SegDesc* segs;  // device table
    int32_t nseg;
    int32_t strips;       // strip groups per row: ceil(ceil(wq / (L-2)) / (64/L))
    int32_t lane_shift;   // L = 64 >> lane_shift lanes per strip (0, 1 or 2)
    int32_t tail_off;     // hand-off kernels: (R + 2 - warm-up) mod prefetch block
    int64_t stride;       // words per buffer row
    int64_t ng;           // lane groups per field row = ceil(ceil(w / 64) / (NP/2))
    uint64_t lastmask[2]; // stored-form valid bits of the last group's words
    int64_t rows_per_wave;
    int64_t total_units;  // wavefronts in the launch
    // Age-skewed row blocks (one-segment launches of one round, engine.cpp
    // age_skew): units below units_old start first on their SIMD, win its VALU
    // arbitration and get rows_old rows; the others rows_per_wave.  0 = off.
    int32_t rows_old;
    int32_t units_old;
    uint32_t birth, survive;
    // Row-block hand-off (kernels instantiated with HAND = true; see
    // life_stencil.h): each wavefront's slot of side rows, its ready flag, and a
    // flag the kernel sets when a wait for a neighbour's rows timed out.
    uint64_t* side;       // total_units slots of side_slot words (per pass parity)
    uint32_t* flags;      // total_units words (per pass parity), all 0 between launches
    int* err;
    int64_t side_slot;    // words per slot: 2 (K-1) rows x 64 lanes x NP/2 words
    uint64_t* wlog;       // GOL_WAVE_LOG builds only: 8 words per wavefront
    // Edge-aligned strips and the packed half strip (plan.cpp col_layout;
    // one-segment launches of 64-lane strips).  A lane whose neighbour lane is the
    // DPP shift's zero (lane 0 / 63) or outside the field is exact, so strip 0 starts
    // at group 0 (63 output groups), strip s at group 62 s (lane 0 its halo), and
    // the last strip ends at group ng - 1 in lane 63 (right_q0 = ng - 64; -1: 62 s).
    // The gap of <= 30 groups left between the last two strips is the half strip
    // [half_q0 + 1, half_hi]: 32 lanes.  Units [pair0, pair0 + pair_units) run it,
    // two row blocks per wavefront (lanes 32-63 offset by the second block's rows),
    // with classic block closure (the device segment table carries one more
    // segment for them: a copy of segment 0 with nblk = 1 and unit0 = pair0, so
    // that no unit of theirs is a hand-off producer or consumer); pairs holds
    // (first row A, first row B or -1 for lanes 32-63 idle, rows) per unit.
    int32_t edge;
    // (r05) the launch's one segment (nseg is 1, or 2 with the half strip's
    // copy): the kernel takes it from here instead of the device table
    int32_t seg0_only;
    SegDesc seg0;
    int64_t right_q0;
    int64_t half_q0, half_hi;
    int64_t pair0, pair_units;
    const int64_t* pairs;
    // (r06 dev A/B) per-XCD row shift between paired blocks (life_stencil.h):
    // bits 2x..2x+1 = speed class of blockIdx mod 8 == x, bits 16-23 = strip
    // modulus m; 0 = off
    uint32_t xcd_shift;
    // Activity skip (classic single-pass launches of one segment at the plan's depth;
    // life_stencil.h): a unit that stored no word different from the
    // generation before writes min(streak_in + 1, kStreakCap) to streak_out[unit],
    // else 0; a unit whose neighbour list nb_ids[nb_off[unit] .. nb_off[unit + 1])
    // (plan.cpp build_neighbours; it holds the unit itself) has streak_in >= 2
    // throughout stores no row.  streak_out null = off; no_hist: the first launch
    // of a step, which ignores streak_in.  act (may be set alone): 2 counters per
    // unit, launches computed (stored its rows) / skipped.
    // Copy-through (`through`): a unit whose list has streak_in >= 1 throughout
    // copies its rows from pbuf[0] to pbuf[1] without stage logic; it counts in
    // act as computed and in copied[unit].  A launch with streak_in and no
    // streak_out (the remainder of a step with history) reads the streaks for
    // this only: it never skips and writes no streak.
    // One-load exit (`busy`, 2 words): every unit that stores rows writes
    // launch_idx + 1 (the launch's index within its step) to busy[1]; a launch
    // that finds busy[1] < launch_idx skips as a whole, and its unit 0 counts it in
    // busy[0].
    // Still probe (`probe`, set with no_hist): a unit of a launch without history
    // runs one generation over its stream first and, where that equals the input
    // on its rectangles dilated by depth - 1, stores its input rows and ends quiet;
    // it counts in act as computed and in probed[unit], not in copied.
    // Copy pass (`through` = 2; life_copy.hip): life_copy_kernel, enqueued
    // directly before this launch on the same stream, has already stored the rows of
    // every unit whose list has streak_in >= 1 throughout; such a unit writes its
    // streak, busy[1] and its counters as under `through` = 1 and stores no row.
    // Copy elision (`held`, set with probe or null): every unit of a probing launch
    // writes held[unit], 1 where it took the probe's quiet exit, else 0; the pass
    // before the step's second launch reads it (CopyArgs::held).
    const uint32_t* streak_in;
    uint32_t* streak_out;
    const uint32_t* nb_off;
    const uint32_t* nb_ids;
    uint32_t* act;
    uint32_t* copied;
    uint32_t* busy;
    uint32_t* probed;
    int32_t no_hist;
    int32_t probe;
    int32_t through;
    int32_t launch_idx;
    uint32_t* held;
    // Probe pass (life_probe.hip; set with probe, or both null):
    // life_probe_kernel, enqueued directly before this launch on the same stream, left
    // moved[unit] = 0 exactly where no tile that meets the unit's rectangles dilated by
    // depth - 1 differs after one generation, and stored those tiles' rows.  Such a
    // unit takes the probe's quiet exit without a field load and counts in
    // pass_probed[unit] as well; every other unit probes as without the pass.
    const uint32_t* moved;
    uint32_t* pass_probed;
};
constexpr uint32_t kStreakCap = 255;

// Fused depths with an instantiated kernel, largest first.  The shipped library
// builds the depths auto_layout and the remainder launches use; the dev build
// (make dev, GOL_DEV_KERNELS) adds 20/24/32 and the 4-plane lane groups.
#if GOL_DEV_KERNELS
constexpr int kDepthList[] = {32, 24, 20, 16, 12, 8, 7, 6, 4, 2, 1};
#else
constexpr int kDepthList[] = {16, 12, 8, 7, 6, 4, 2, 1};
#endif
constexpr bool kDevKernels = GOL_DEV_KERNELS != 0;

// Row blocks hand their first rows of every fused generation to the block above
// (life_stencil.h) from this depth on.
constexpr int kHandoffMinDepth = 4;
// ... except for the generic-mask rule above depth 12, whose 10-term mask sum
// already spills without the hand-off's extra state (auto_layout gives it K = 12)
constexpr bool handoff_kernel_exists(int K, RuleKind rule)
{
    return K >= kHandoffMinDepth && (rule != RULE_GENERIC || K <= 12);
}

// Multi-pass stencil kernels (StepArgs::npass > 1, life_stencil.h): 2-plane lane
// groups at depths 12 and 16 (the generic-mask rule at 12 only, as its hand-off
// kernels).  Measured slower than single-pass launches (r05): the dev
// build only (make dev), so the shipped library carries no multi-pass kernel.
constexpr bool multipass_kernel_exists(int K, RuleKind rule, int planes)
{
    return kDevKernels && planes == 2 && (K == 12 || (K == 16 && rule != RULE_GENERIC));
}

// Steps per block of the stencil kernel's register prefetch ring (host copy of
// life_stencil.h kPfOf): 8 for 2-plane kernels of depth >= 16, 4 elsewhere.
constexpr int prefetch_of(int K, int planes) { return (planes == 2 && K >= 16) ? 8 : 4; }
// Unrolled warm-up steps (a multiple of the prefetch block covering 2K steps).
constexpr int warm_steps_of(int K, int planes)
{
    return (2 * K + prefetch_of(K, planes) - 1) / prefetch_of(K, planes) * prefetch_of(K, planes);
}
// Tail offsets with a hand-off kernel: 0 and prefetch/2, and 2 and 6 with the
// 8-step prefetch block (offset 2 there would take 258 VGPRs, one wave per SIMD:
// it is built capped at 256, GOL_TOFF2_CAP).
constexpr bool handoff_toff_exists(int off, int pf)
{
    return off == 0 || off == pf / 2 || (pf == 8 && (off == 6 || off == 2));
}
// A consumer block of R rows streams R + 2 input steps after the warm-up, i.e.
// (R + 2 - warm) mod prefetch must be an offset with a kernel, and at least two
// whole steady blocks must precede the tail (the flag wait sits at the end of the
// first of them).  Returns the offset, or -1 if R does not fit.  Every offset with
// a kernel, the warm-up and the prefetch are even, so R is even: the B/S2 pair sum
// (life_stencil.h) relies on the tail starting at an even step t_side = R + 2.
constexpr int handoff_toff(int64_t R, int K, int planes)
{
    const int pf = prefetch_of(K, planes), warm = warm_steps_of(K, planes);
    if (K < kHandoffMinDepth || R + 2 < warm + 2 * pf) return -1;
    const int off = (int)((R + 2 - warm) % pf);
    if (!handoff_toff_exists(off, pf)) return -1;
    return R + 2 - off >= warm + 2 * pf ? off : -1;
}

// Launch `depth` fused generations (depth in kDepthList) on lane groups of
// `planes` (2, or 4 in the dev build).  hand: the row-block hand-off kernel
// (a.side/flags/err set); else every row block recomputes its vertical halo.
hipError_t launch_life(const StepArgs& a, int depth, RuleKind rule, int planes, bool hand,
                       hipStream_t s);
bool life_has_kernel(int depth, int planes);

// The copy pass (life_copy.hip, DESIGN §4 "Copy pass"): two low-register kernels
// that store the rows of the calm units (neighbour list all streak_in >= 1) of a
// one-segment plan of 2-plane groups from `src` to `dst`, for the stencil launch
// that follows them with StepArgs::through = 2.  The first writes calm[unit] for
// every unit.  The second works on line-aligned tiles of the segment's output rows,
// kCopyTileRows rows x kCopyTileWords words (512 bytes: every 128-byte line of a row
// is written by one wavefront), tile t = row chunk t / ncol, column segment
// t % ncol, and takes from a device table the units with a rectangle (plan.cpp
// unit_rects) that meets each tile: its owners, kCopyOwners slots per tile, the
// unused ones ~0.
// Copy elision (DESIGN §4 "Copy pass"): the first kernel also finds the calm units
// whose rows `dst` already holds -- probed through in the step's first launch
// (`held`, non-null only before the step's second launch after a first launch that
// probed), every streak_in of the list >= 2, or all of them in the second and later
// launches of one remainder (`all_held`, which run the first kernel alone) -- counts
// them in elided[unit] and writes need[unit] = calm and not held; the second copies
// a tile when one of its owners has `need`.
constexpr int kCopyTileRows = 8;
constexpr int kCopyTileWords = 64;
constexpr int kCopyOwners = 8;
struct CopyArgs {
    const uint64_t* src;  // row 0 of the launch's pbuf[0] and pbuf[1]
    uint64_t* dst;
    const uint32_t* owners;     // ntile x kCopyOwners unit indices
    uint32_t* need;             // total_units words, written by the pass's first kernel
    const uint32_t* held;       // StepArgs::held of the step's first launch, or null
    uint32_t* elided;           // per-unit counter, or null: no elision (every calm unit copies)
    int32_t all_held;           // every calm unit's rows are in dst: no tile kernel
    const uint32_t* streak_in;  // as the launch that follows reads them
    const uint32_t* nb_off;
    const uint32_t* nb_ids;
    int64_t stride;    // words per buffer row
    int64_t base_row;  // buffer row of the segment's local row 0
    uint64_t lastmask; // stored-form valid bits of group ng - 1
    int32_t ntile, ncol;
    int32_t total_units;
    int32_t out_lo, out_hi;  // the segment's output rows (local)
    int32_t ng;
    int32_t vlo, vhi;  // local rows inside the buffer and the field; others store 0
    // Rows both buffers hold (both set before a step's last launch, or both
    // null): the first kernel also writes twin[unit] = calm, and *twin_ok = 1.  With
    // `need` null it writes nothing else (launch_twin_flags).
    uint32_t* twin;
    uint32_t* twin_ok;
    // Sure tiles: the value a calm unit's twin word gets.  2 only before a
    // remainder launch (fewer than K generations run since the streaks were written);
    // anything else writes 1.
    uint32_t twin_val;
};
hipError_t launch_copy_pass(const CopyArgs& a, hipStream_t s);
// The pass's first kernel alone, for twin[] only (need and elided null): before a
// step's last launch where that is a depth-K launch that takes no copy pass.
hipError_t launch_twin_flags(const CopyArgs& a, hipStream_t s);
// twin[] = held[] (StepArgs::held) and *twin_ok = 1: after a step's only launch, where
// that launch probed and wrote held[] for every unit.
hipError_t launch_twin_held(const uint32_t* held, uint32_t* twin, uint32_t* twin_ok, int32_t units,
                            hipStream_t s);
// The short step (DESIGN §4 "Short step"): one wavefront in place of `count` depth-K
// launches of a step, the first of them with StepArgs::launch_idx = first_idx, that
// would all take the one-load exit: busy[1] < first_idx adds count to busy[0], anything
// else stores kErrShortStep to *err (the engine's error word; the kernels' wait
// timeouts store 1).
constexpr int kErrShortStep = 2;
hipError_t launch_still_span(uint32_t* busy, int* err, uint32_t first_idx, uint32_t count,
                             hipStream_t s);

// The fixed step (DESIGN §4 "Fixed step"): one workgroup in place of every kernel of a
// step on a proven fixed point.  The proof is *twin_ok != 0 and twin[u] == 2 for every
// unit; where it holds the kernel adds the step's increments to the counters and
// stores its final values to the state words (step.cpp still_effect computes both),
// else it stores kErrShortStep to *err and nothing else.  The regions are ActState's
// (engine_internal.h), each of act_units words (act: 2 per unit), of which the first
// total_units are touched.
struct StillArgs {
    uint32_t *streak0, *streak1, *act, *copied, *busy, *probed, *need, *held, *elided, *moved,
        *pass_probed, *twin, *twin_ok;
    int* err;
    uint32_t total_units, act_units;
    // increments per unit, and of busy[0]
    uint32_t computed, skipped, n_copied, n_probed, n_pass_probed, n_elided, busy0_add;
    // final values
    uint32_t busy1, v_streak0, v_streak1, v_need, v_held, v_moved, v_twin, v_twin_ok;
};
hipError_t launch_still_step(const StillArgs& a, hipStream_t s);

// The probe pass (life_probe.hip, DESIGN §4 "Probe pass"): one generation over the
// copy pass's tiles before a step's first launch, in the copy pass's shape.  A device
// table gives per tile the units one of whose rectangles, dilated by depth - 1
// cells, meets it (kProbeSlots slots, unused ones ~0).  A tile whose cells all keep
// their state stores its rows to `dst` as the copy pass would; any other tile stores
// moved[unit] = 1 for its listed units and no row.  moved[] is zeroed on the stream
// directly before the kernel.
constexpr int kProbeSlots = 8;
struct ProbeArgs {
    const uint64_t* src;  // row 0 of the launch's pbuf[0] and pbuf[1]
    uint64_t* dst;
    const uint32_t* tiles;  // ntile x kProbeSlots unit indices
    uint32_t* moved;        // total_units words
    int64_t stride;    // words per buffer row
    int64_t base_row;  // buffer row of the segment's local row 0
    uint64_t lastmask; // stored-form valid bits of group ng - 1
    int32_t ntile, ncol;
    int32_t total_units;
    int32_t out_lo, out_hi;  // the segment's output rows (local)
    int32_t ng;
    int32_t vlo, vhi;  // local rows inside the buffer and the field; others are dead
    uint32_t birth, survive;
    // Rows both buffers hold (all four set, or all null): a tile without a
    // difference stores no row and counts in kept[tile] where *twin_ok is set, the
    // tile has an owner (the copy pass's table, kCopyOwners slots per tile of the same
    // grid) and twin[] is set for every owner: dst holds those rows already.
    const uint32_t* owners;
    const uint32_t* twin;
    const uint32_t* twin_ok;
    uint32_t* kept;  // ntile words
    // Sure tiles (set with the four above, or null): a tile that would be
    // kept and whose owners' twin words are all 2 is proven to keep its state for one
    // generation, so it counts in kept[tile] and in sure[tile] before any field load.
    uint32_t* sure;  // ntile words
};
hipError_t launch_probe_pass(const ProbeArgs& a, RuleKind rule, hipStream_t s);

// The snapshot compare (life_snap.hip, DESIGN §4 "Snapshots"): `rows` buffer rows from
// row_base on, `nwords` stored words per row from word0 on, of the engine's current
// buffer against the same words of its snapshot, over the copy pass's tiles
// (kCopyTileRows x kCopyTileWords, column segments fastest).  A leaf's own rows: word0
// = 0 and the field's words; a torus interior: row tG, word tGx of the inner engine.
// mask: the stored-form valid bits of words nwords - 2 and nwords - 1 (the last lane
// group: all ones and lastmask_split[0] with 2 planes, both lastmask_split words with
// 4).  count = false: *flag (zeroed by the caller on the stream) is set to 1 when any
// word differs (one store per workgroup at most), and wavefronts that find it set
// leave out their field loads; count
// = true: the differing cells are added to *count, one atomic per workgroup at most.
struct SnapArgs {
    const uint64_t* cur;   // row 0 of the current buffer and of the snapshot
    const uint64_t* snap;
    int64_t stride;        // words per buffer row
    int64_t row_base, word0, nwords, rows;
    uint64_t mask[2];
    uint32_t* flag;
    unsigned long long* count;
    int32_t ntile, ncol;   // set by launch_snap_compare
};
hipError_t launch_snap_compare(const SnapArgs& a, bool count, hipStream_t s);

// Resident 256-thread blocks per CU of the stencil kernel (occupancy query).
// mp: of the multi-pass kernels (0 where none exists)
int life_blocks_per_cu(int depth, RuleKind rule, int planes, bool hand, bool mp = false);

// Per-depth entry points (explicitly instantiated in life_tb_d<K>.hip).
template <int K>
hipError_t launch_depth(const StepArgs& a, RuleKind rule, int planes, bool hand, hipStream_t s);
template <int K>
int occupancy_depth(RuleKind rule, int planes, bool hand, bool mp);

// The resident kernel (life_resident.hip): one launch runs a whole gol_step on a
// small field held in registers by one 1024-thread workgroup per (band, strip)
// tile; neighbouring tiles swap their band rows every K generations through
// the two field buffers (epoch e's result in buf0 if e is even, else buf1;
// buf0 holds the input).
constexpr int kResWaves = 16;                     // wavefronts per workgroup
constexpr int kResRowsList[] = {2, 3, 4, 6, 8};   // rows per wavefront (instantiated)
struct ResArgs {
    uint64_t* buf0;       // row 0 of the input buffer (also the even epochs' output)
    uint64_t* buf1;
    uint32_t* flags;      // one per tile: epochs published, counting from flag_base
    int* err;             // set when a neighbour wait timed out
    int64_t stride;       // words per buffer row
    int64_t h;            // field rows
    int64_t ng;           // lane groups (= words) per row
    uint64_t lastmask;    // stored-form valid bits of group ng - 1
    int32_t strips;       // 1: lane l = group l (ng <= 64); else 62 groups + 2 halo lanes
    int32_t bands;
    int32_t band_rows;    // B; tiles hold B + 2K <= kResWaves * M rows
    int32_t K;            // generations per epoch (<= 63 when strips > 1)
    int32_t span;         // ceil(K / band_rows): bands a halo reaches; (2 span + 1) x
                          // (strips > 1 ? 3 : 1) - 1 <= 64 neighbour tiles
    int32_t gens;         // generations of this launch
    uint32_t flag_base;
    uint32_t birth, survive;
    uint64_t* wlog;       // GOL_WAVE_LOG builds only: 8 words per wavefront, 6 used
};
// coop: hipLaunchCooperativeKernel, else a plain launch (engine.cpp Resident::coop)
hipError_t launch_resident(const ResArgs& a, int rows, RuleKind rule, int grid, hipStream_t s,
                           bool coop = false);
int resident_blocks_per_cu(int rows, RuleKind rule);
// The resident kernel with wave-level temporal blocking (life_resident_mb.hip, r06,
// dev build only: slower than life_res_kernel at every MB): wavefronts
// swap MB rows through LDS every MB generations.  (rows, mb) pairs:
// (the generic-mask rule at rows = mb = 4 spills: not offered)
constexpr bool resident_mb_exists(int rows, int mb, RuleKind rule)
{
    return mb >= 2 && mb <= rows && rows <= 4 && !(rule == RULE_GENERIC && mb == 4);
}
hipError_t launch_resident_mb(const ResArgs& a, int rows, int mb, RuleKind rule, int grid,
                              hipStream_t s);
int resident_mb_blocks_per_cu(int rows, int mb, RuleKind rule);

// Device-side synthetic init: buffer rows [row_base, row_base+nrows) get field
// rows [glob_row0, glob_row0+nrows).  row_words: the words written per row (the
// field's, then zeros), 0 = the whole stride; a torus interior (torus.cpp), whose
// rows sit inside longer buffer rows, passes its own width.
hipError_t launch_init_random(uint64_t* buf, int64_t stride, int64_t wq, uint64_t lastmask,
                              int64_t row_base, int64_t glob_row0, int64_t nrows,
                              uint64_t seed, int planes, hipStream_t s, int64_t row_words = 0);

// ASCII codec: `rows` lines of w cell bytes + '\n' (device memory) <-> stored
// lane groups (ng per row) at dst/src with `stride` words per row.  *bad is set
// if a line does not end in '\n' at byte w.
hipError_t launch_ascii_pack(const char* src, int64_t rows, int64_t w, int64_t ng, uint64_t* dst,
                             int64_t stride, int* bad, int planes, hipStream_t s);
hipError_t launch_ascii_unpack(const uint64_t* src, int64_t stride, int64_t rows, int64_t w,
                               int64_t ng, char* dst, int planes, hipStream_t s);

// Adds popcount and hash of buffer rows [row_base, row_base+nrows) (field rows
// glob_row0..) into acc[0], acc[1].  lastmask: the field's bits of word wq - 1
// (all ones where the buffer keeps columns >= w at 0; a torus interior has ghost
// cells there).
hipError_t launch_digest(const uint64_t* buf, int64_t stride, int64_t wq, int64_t ng,
                         int64_t row_base, int64_t glob_row0, int64_t nrows,
                         unsigned long long* acc, int planes, hipStream_t s,
                         uint64_t lastmask = ~0ull);

// Torus wrap (GOL_SEM_TORUS, torus.cpp): rewrites every ghost cell of a padded
// 2-plane field from its h x w interior by the rule of torus_wrap.h.  `buf` is the
// padded field's row 0, `stride` its words per row; the interior starts at row G,
// word Gx; wq_pad = ceil((w + 128 Gx) / 64) words per row are the field's.
hipError_t launch_torus_wrap(uint64_t* buf, int64_t stride, int64_t h, int64_t w, int64_t G,
                             int64_t Gx, hipStream_t s);

// Region I/O (gol_read_rect / gol_write_rect / gol_density), one non-wrapping piece
// per launch: buffer rows [row_base, row_base + rows) x field columns [x, x + cols)
// of the view `buf` (word 0 = field column 0).  Read fills a compact staging window
// (bit 0 of a row = column x, 0 from cols on); write merges one under op
// (gol_rect_op); density adds the piece's live cells per by x bx block of the
// window whose cell (wrow0, wcol0) is the piece's first, into counts[bi * cstride +
// bj] (zeroed by the caller).
hipError_t launch_rect_read(const uint64_t* buf, int64_t stride, int64_t row_base, int64_t x,
                            int64_t rows, int64_t cols, uint64_t* dst, int64_t dst_stride,
                            int planes, hipStream_t s);
hipError_t launch_rect_write(uint64_t* buf, int64_t stride, int64_t row_base, int64_t x,
                             int64_t rows, int64_t cols, const uint64_t* src, int64_t src_stride,
                             uint32_t op, int planes, hipStream_t s);
hipError_t launch_density(const uint64_t* buf, int64_t stride, int64_t row_base, int64_t x,
                          int64_t rows, int64_t cols, int64_t wrow0, int64_t wcol0, int64_t by,
                          int64_t bx, uint32_t* counts, int64_t cstride, int planes,
                          hipStream_t s);

}  // namespace gol
