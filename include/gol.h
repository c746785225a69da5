/*
 * gol.h -- C ABI of the MI355X Game of Life engine (libgol.so).
 *
 * Drop-in boundary for the hot path of krutovsky-danya/mpi-game-of-life,
 * Parallel_Life_MPI.cpp.  The reference has no plugin API: its hot path is
 * `void updateGrid()` (:37-54, with countNeighbours :16-35) mutating the
 * process globals `grid`/`nextGrid` (:13), driven by the loop in main
 * (:215-221) together with `exchangeGridData` (:104-145), and fed/drained by
 * readGridFromFile (:56-102) and writeDataToFile (:147-188).  This header
 * replaces main's lines :211-231 (read -> epochs x {update, exchange, barrier}
 * -> write) with an engine handle; each entry point names the reference code
 * it stands in for.
 *
 * Conventions
 *  - Cells: bit-packed, 64 per uint64, row-major; bit j of word q is column 64q+j.
 *    Columns >= w are kept 0.  Outside the field every cell is dead
 *    (Parallel_Life_MPI.cpp:21-27), except on a torus (GOL_SEM_TORUS), which has no
 *    outside.
 *  - Rule: a (birth, survive) pair of 9-bit masks, bit n <=> n live neighbours.
 *    The reference's *effective* rule is birth=0, survive=1<<2 ("B/S2"): the
 *    `count == 3` store at :44-46 is always overwritten by :47-50.
 *  - Ownership: the caller owns every host buffer; the engine owns all device
 *    memory, its HIP stream and its RCCL communicator.
 *  - Errors: every call returns gol_status; it never aborts.  gol_last_error()
 *    gives a thread-local message for the last failure.
 *  - Threading: a handle is not thread-safe; use it from one host thread.
 */
#ifndef GOL_H
#define GOL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gol_status {
    GOL_OK = 0,
    GOL_EINVAL = 1, /* bad argument (sizes, masks, lengths, malformed ASCII) */
    GOL_ENOMEM = 2, /* device or host allocation failed */
    GOL_EHIP = 3,   /* HIP runtime error */
    GOL_ERCCL = 4,  /* RCCL error */
    GOL_EIO = 5,    /* file I/O error (CLI helpers) */
    GOL_ESTATE = 6, /* call not valid in the engine's current state */
    GOL_EXFER = 7   /* halo transport callback failed (gol_create_rank_transport) */
} gol_status;

typedef enum gol_semantics {
    /* The reference's intended semantics == its `mpirun -np 1` output: one field
     * evolving with a dead border. */
    GOL_SEM_GLOBAL = 0,
    /* The reference's actual `mpirun -np P` output: its halo exchange receives
     * into copies (:110-111, :126-127) and has no effect, so each rank's
     * extended stripe (:70-81) evolves alone and the output keeps each rank's
     * own rows (:149-175).  P = gol_config.ref_ranks. */
    GOL_SEM_REF_STRIPES = 1,
    /* One h x w field whose opposite edges are joined (periodic boundary): column
     * w - 1 is the left neighbour of column 0 and row h - 1 the upper neighbour of
     * row 0, for any h, w >= 1.  gol_create only, on one stream (streams 0 or 1,
     * word_planes 0 or 2).  The engine owns an "inner" dead-border engine of the
     * field padded with ghost cells -- G ghost rows above and below, ceil(G/64)
     * ghost words (64 columns each) left and right: (h + 2G) x (w + 128 ceil(G/64))
     * cells -- and gol_step runs rounds of at most G generations, each one wrap
     * kernel, which rewrites every ghost cell from the interior, and then the inner
     * engine's launches (gol_torus_geometry; gol_config.halo_depth sets G).  Load,
     * store, init and digest see the h x w interior only: the same bytes, the same
     * gol_init_random field and the same digest as a dead-border engine of h x w.
     * Queries: gol_info reports the interior's h, w, the inner engine's tb_depth and
     * G as halo_depth; gol_plan_*, gol_activity* and gol_*_timing report the inner
     * engine's values (its launches cover the padded field; the wrap kernel is not
     * timed), as a composite engine reports its first stripe. */
    GOL_SEM_TORUS = 2
} gol_semantics;

/* Reference-effective rule and Conway's rule as (birth, survive) masks. */
#define GOL_REF_BIRTH 0u
#define GOL_REF_SURVIVE (1u << 2)
#define GOL_CONWAY_BIRTH (1u << 3)
#define GOL_CONWAY_SURVIVE ((1u << 2) | (1u << 3))

typedef struct gol_config {
    uint32_t birth_mask;   /* 9-bit */
    uint32_t survive_mask; /* 9-bit */
    int32_t device;        /* HIP device ordinal; -1 = current device */
    uint32_t semantics;    /* gol_semantics */
    uint32_t ref_ranks;    /* P for GOL_SEM_REF_STRIPES (must satisfy h >= P) */
    uint32_t tb_depth;     /* generations fused per kernel launch (temporal
                              blocking); 0 = auto; allowed 1,2,4,6,7,8,12,16
                              (the dev build, make dev, adds 20,24,32); with
                              resident = 2, the resident kernel's epoch length,
                              any of 1..63 */
    uint32_t halo_depth;   /* multi-rank: halo rows exchanged per round
                              (= generations between exchanges); 0 = auto.
                              GOL_SEM_TORUS: G, the generations per wrap round
                              (= ghost rows), 1..65536; 0 = auto: the largest
                              multiple of the inner engine's streaming depth K
                              that is <= max(K, min(h, w) / 4) and <= 256 for
                              fields of at most 2^25 cells, <= 128 for larger */
    uint32_t rows_per_wave;/* rows each wavefront streams per launch; 0 = auto */
    uint32_t handoff;      /* row blocks of a launch: 0 = auto (= on), 1 = off
                              (every block recomputes the K(K-1) stage-steps of
                              its vertical halo), 2 = on (each block takes the
                              rows it needs beyond its own from the block below,
                              which computed them first; tb_depth >= 4) */
    uint32_t streams;      /* (GOL_SEM_TORUS: 0 or 1)
                              gol_create, GLOBAL only: split the field into this
                              many row stripes advanced on their own streams of
                              the device (k-deep halos, device copies), so one
                              stripe's launch tail overlaps the others' work;
                              0 = auto (2 when h >= 32768), 1 = one stream */
    uint32_t strip_lanes;  /* lanes per column strip of the stencil kernel: 64, 32
                              or 16 (2 of them halo, 64/L strips per wavefront);
                              0 = auto (narrow strips for short stripes) */
    uint32_t word_planes;  /* cell planes per lane: 0 = auto (= 2: one word = 64
                              columns per lane); 4 (two words per lane) exists
                              only in the dev build (make dev) */
    uint32_t resident;     /* gol_create, GLOBAL only: small fields held in
                              registers across the chip and advanced by ONE
                              launch per gol_step (tiles swap halo rows every K
                              generations inside the launch); 0 = auto (when the
                              field fits and no streaming-kernel knob --
                              tb_depth, rows_per_wave, handoff, strip_lanes,
                              word_planes -- is set), 1 = off, 2 = on if the
                              field fits (then tb_depth sets K and rows_per_wave
                              the rows each wavefront holds: 2,3,4,6,8) */
    uint32_t exchange_overlap; /* rank engines and groups: 0 = auto (rank engines
                              over RCCL time both modes at create on their
                              communicator and keep the faster, the same on
                              every rank: gol_plan_exchange; rank engines over a
                              host transport block; in-process groups overlap),
                              1 = blocking, 2 =
                              overlapped (the round's last launch splits into a
                              band launch of the rows the neighbours need and an
                              interior launch, and the exchange of the band rows
                              runs on a side stream beside the interior launch;
                              needs stripes of >= 2 halo_depth rows, else
                              blocking) */
} gol_config;

typedef struct gol_engine gol_engine;

typedef struct gol_timing {
    uint64_t launches;     /* stencil kernel launches timed (sampled) */
    double kernel_ms;      /* sum of their HIP-event durations */
    double cell_gens;      /* cell-generations those launches produced (own rows) */
    double cell_gens_computed; /* what the lanes process: including the vertical
                                  halo stage-rows of classic blocks and the
                                  strips' halo lanes */
    uint32_t streams;      /* stripe streams whose launches run concurrently */
    /* (r06; `reserved` before) in: the caller's sizeof(gol_timing).  The layout
     * grew in r05 and r06; gol_get_timing writes the whole struct only when this
     * equals the library's sizeof(gol_timing), else only the r04 fields above
     * (40 bytes), so a caller built against an older header is never overrun.
     * out: the bytes written. */
    uint32_t struct_size;
    /* (r05) while timing is on: every stencil launch issued (sampled or not) and
     * the buffer rows the sampled launches computed; rank engines also time
     * every halo exchange with HIP events on its stream (RCCL: the stream time
     * of ncclGroupStart..End, which includes waiting for the peers; host
     * transport: staging + callback) */
    uint64_t launches_issued;
    double launch_rows;
    uint64_t exchanges;
    double exchange_ms;
    /* (r06) rank engines while timing is on: `rounds` halo rounds, round_ms = the
     * sum of their compute-stream spans (HIP events before the round's first
     * launch and after its last, the band stream joined), exchange_exposed_ms =
     * the part of the exchanges outside those spans (a blocking exchange: all of
     * it; an overlapped one: what runs past the end of its round's span).  Per
     * step: round_ms + exchange_exposed_ms <= the wall time; the rest is host
     * work and launch gaps between rounds. */
    uint64_t rounds;
    double round_ms;
    double exchange_exposed_ms;
} gol_timing;
#define GOL_TIMING_R04_BYTES 40u

/* Defaults: reference-effective rule, GLOBAL semantics, auto tuning. */
void gol_config_init(gol_config* cfg);

/* Replaces the allocation in readGridFromFile (:88-89).  h rows x w columns.
 * An engine alone on its device times a few equally exact launch plans on its
 * own buffers before returning (tens of ms) and keeps the fastest. */
gol_status gol_create(uint64_t h, uint64_t w, const gol_config* cfg, gol_engine** out);

/* Replaces readGridFromFile's parse (:91-99): buf holds the data.txt bytes,
 * h lines of exactly w cell bytes followed by '\n' (len == h*(w+1)); a cell is
 * alive iff its byte is '1'.  A rank engine (gol_create_rank) takes only its
 * own rows: len == rows*(w+1). */
gol_status gol_load_ascii(gol_engine* e, const char* buf, size_t len);

/* Replaces writeDataToFile's serialisation (:157-164): writes '0'/'1' bytes and
 * '\n' per row, len == h*(w+1) (own rows for a rank engine). */
gol_status gol_store_ascii(gol_engine* e, char* buf, size_t len);

/* Packed transfer; row_stride_words >= ceil(w/64).  Rank engines: own rows. */
gol_status gol_load_packed(gol_engine* e, const uint64_t* words, uint64_t row_stride_words);
gol_status gol_store_packed(gol_engine* e, uint64_t* words, uint64_t row_stride_words);

/* Synthetic p = 0.5 field generated on the device: word (r, q) =
 * splitmix64(seed, r*ceil(w/64)+q) masked to w (identical on the CPU oracle). */
gol_status gol_init_random(gol_engine* e, uint64_t seed);

/* Replaces the epoch loop (:215-221): advances `generations` generations
 * (including the halo exchange of a rank engine).  Returns after the work is
 * enqueued; gol_sync() waits for it.
 * A fixed step (below, gol_activity_fixed_steps) may enqueue nothing: its one kernel is
 * launched by the next call that looks at the activity state or the error word or
 * enqueues work that does, gol_sync among them, and stands for every fixed step since
 * the last such call.  If that kernel does not launch, the status (GOL_EHIP) is that
 * call's, not gol_step's. */
gol_status gol_step(gol_engine* e, uint64_t generations);
gol_status gol_sync(gol_engine* e);

/* Live-cell count and an order-independent 64-bit hash of the field
 * (sum over words of splitmix64(word ^ splitmix64(0, r*ceil(w/64)+q))).
 * Rank engines return the partial sums of their own rows (add them up). */
gol_status gol_digest(gol_engine* e, uint64_t* live, uint64_t* hash);

void gol_destroy(gol_engine* e);
const char* gol_last_error(void);

/* HIP-event timing of the stencil kernel on the engine's stream: events bracket
 * every `every`-th launch (1 = all; 0 = off).  An event pair costs a few
 * microseconds of stream time, so sample short launches (bench.py uses 8).
 * gol_timing then covers the sampled launches only. */
gol_status gol_set_timing(gol_engine* e, int every);
gol_status gol_get_timing(gol_engine* e, gol_timing* out);
gol_status gol_reset_timing(gol_engine* e);

/* Activity skip.  A single-stream engine's classic launches leave out the units
 * (wavefronts) whose neighbourhood stored nothing new in the two launches before,
 * within one gol_step: the field is the same, a still region costs almost nothing.
 * Off on hand-off plans, composite / multi-stream engines, groups, rank engines,
 * the resident kernel, while gol_set_timing(n > 0) is on, and with
 * GOL_DEV_ACTIVITY_SKIP=0 in the environment at create.  gol_activity returns how
 * many units computed and how many skipped a launch, summed over the stencil
 * launches of gol_step since create or gol_reset_timing (it waits for the
 * engine's stream).  "Computed" = the unit stored its rows; gol_activity_copied
 * returns how many of those did so without stage logic: a unit whose neighbourhood
 * ended the launch before quiet copies its rows into the output buffer
 * (copy-through, on wherever the skip is; GOL_DEV_COPY_THROUGH=0 at create turns it
 * off and leaves the skip alone).  Before a step's second launch and its remainder
 * launches a copy kernel of its own stores those rows and the launch only counts
 * the units (the copy pass; the counters are the same with GOL_DEV_COPY_PASS=0 at
 * create, which leaves the copying to the launch).  gol_activity_probed returns how
 * many computed units were found still by the first launch of a gol_step, which has no history:
 * such a unit runs one generation over the rows it streams and, where that changes
 * nothing within depth - 1 cells of its rows, stores its input rows without the
 * other generations' stage logic (the still probe, on wherever the skip is;
 * GOL_DEV_STILL_PROBE=0 at create turns it off); these units are not counted as
 * copied.  gol_activity_elided returns how many calm units the copy pass left
 * alone because the buffer it writes already held their rows: units that probed
 * through in the step's first launch (before the second launch), units still for
 * two launches (before a remainder launch), and every calm unit of the second and
 * later launches of one remainder.  The launch after the pass counts them as
 * computed and copied all the same; GOL_DEV_COPY_ELIDE=0 at create makes the pass
 * copy them as before (the count stays 0).  Any out pointer may be NULL.  Composite engines, group members and rank
 * engines of more than one rank keep no counters: all 0. */
gol_status gol_activity(gol_engine* e, uint64_t* computed_units, uint64_t* skipped_units);
gol_status gol_activity_copied(gol_engine* e, uint64_t* copied_units);
gol_status gol_activity_probed(gol_engine* e, uint64_t* probed_units);
gol_status gol_activity_elided(gol_engine* e, uint64_t* elided_units);
/* The probe pass: before a step's first launch a kernel of its own runs that one
 * generation over line-aligned tiles of the field (the copy pass's tiles), stores the
 * tiles that keep their state and marks the units near a tile that does not.  A unit
 * it leaves unmarked is found still by the launch on that word alone;
 * gol_activity_pass_probed returns how many of the units gol_activity_probed counts
 * went through that way.  The pass changes no other counter and no field word; it
 * runs wherever the copy pass does, and GOL_DEV_PROBE_PASS=0 at create turns it off
 * (the count stays 0). */
gol_status gol_activity_pass_probed(gol_engine* e, uint64_t* pass_probed_units);
/* Rows both buffers hold: a tile of the probe pass that keeps its state stores no row
 * where the buffer it would write holds those rows already, word for word.  The last
 * launch of the step before records that per unit (a unit that did not compute in it),
 * and every other writer of the field -- a load, gol_init_random, gol_write_rect, a
 * torus round's wrap, a timed or hand-off launch -- withdraws the record.
 * gol_activity_pass_kept returns how many tile passes left their rows that way since
 * create or gol_reset_timing.  No field word and no other counter depends on it;
 * GOL_DEV_TWIN=0 at create turns it off (every such tile stores; the count stays 0).
 * Torus engines wrap before every round: their count stays 0. */
gol_status gol_activity_pass_kept(gol_engine* e, uint64_t* kept_tiles);

/* Sure tiles (DESIGN.md section 4 "Sure tiles").  Where the step before ended with a
 * remainder launch (fewer than tb_depth generations), a unit that launch found calm
 * also keeps its state for one more generation, so a tile of the next step's probe
 * pass all of whose owners were calm there is known to keep its state: it counts as
 * kept and leaves before it loads a field word.  gol_activity_pass_sure returns how
 * many of the tile passes gol_activity_pass_kept counts left that way since create or
 * gol_reset_timing.  No field word and no other counter depends on it;
 * GOL_DEV_TWIN_SURE=0 at create turns it off (every kept tile loads its rows and
 * compares, as before; the count stays 0), and so does whatever turns
 * gol_activity_pass_kept off. */
gol_status gol_activity_pass_sure(gol_engine* e, uint64_t* sure_tiles);

/* Short step (DESIGN.md section 4 "Short step").  When gol_sync finds that every unit was
 * calm in the remainder launch that ended the last step, the field is a fixed point,
 * and it stays one until somebody writes it (a load, gol_init_random, gol_write_rect,
 * gol_snapshot_restore, a timed step, a step of fewer than tb_depth generations, a
 * failed step: whatever withdraws gol_activity_pass_kept's record).  Until then a
 * gol_step of at least 5 tb_depth generations replays a graph that leaves out the
 * stencil launches from the fourth full-depth one on, which would each exit on one
 * load, and runs one small kernel in their place; that kernel repeats their test, and
 * if it fails the next gol_sync returns GOL_ESTATE ("short step on a field that was
 * not still").  gol_step still returns once the work is enqueued.
 * gol_activity_short_steps returns how many steps ran that way since create or
 * gol_reset_timing (a host count; 0 on torus, composite, rank, group and resident
 * engines, which never do).  The field and every other counter are what the full step
 * leaves.  GOL_DEV_SHORT_STEP=0 at create turns it off, and so do GOL_DEV_TWIN_SURE=0
 * and GOL_DEV_STILL_EXIT=0; GOL_DEV_SHORT_STEP=2 takes the short graph wherever the
 * step's shape allows, seen or not (tests of the error status only). */
gol_status gol_activity_short_steps(gol_engine* e, uint64_t* steps);

/* Fixed step (DESIGN.md section 4 "Fixed step").  Where the short step's conditions
 * hold and the host also knows that the last step ended with a remainder launch that
 * found every unit calm (gol_sync saw a 2 in every unit's word, and every step since
 * kept it), a gol_step is one small kernel, launched directly: it repeats that test on
 * the device and then leaves the activity state and the counters word for word as the
 * step's kernels would.  Where the test fails it writes nothing, and the next gol_sync
 * returns GOL_ESTATE as for the short step.
 * gol_plan_still_step (host only, no GPU) returns what such a step of `generations`
 * generations at depth tb_depth does to the activity state: increments of the
 * counters, final values of the state words (none of which depends on what the word
 * held before), and how many probe passes count every owned tile.  GOL_EINVAL where
 * the step has fewer than 5 full-depth launches or tb_depth is no kernel depth.
 * gol_activity_fixed_steps: steps that ran so since create or gol_reset_timing (a host
 * count; they count in gol_activity_short_steps as well).  GOL_DEV_FIXED_STEP=0 at
 * create turns the path off (the short graph runs instead), as does whatever turns
 * the short step off; GOL_DEV_FIXED_STEP=2 takes it after every step that ended with
 * a remainder launch, seen or not (tests of the error status only).
 * Pending fixed steps: consecutive fixed steps do not interact on the device (the
 * increments add up modulo 2^32, the final values are the last step's), so gol_step
 * only books them on the host, and one kernel with the sums runs when a call needs
 * the state: gol_sync, every gol_activity_* getter that reads the device,
 * gol_activity_state, gol_reset_timing, a step that is not fixed, every writer of the
 * field, a snapshot comparison, and whatever checks the error word after its own work
 * (digests, stores, rectangle reads).  gol_activity_fixed_launches: launches of that
 * kernel since create or gol_reset_timing (a host count): with n fixed steps between
 * two such calls it grows by 1, by n with GOL_DEV_FIXED_DEFER=0 at create, which
 * launches one kernel per fixed step. */
typedef struct gol_still_effect {
    uint64_t launches;    /* stencil launches the step stands for (the buffers swap per launch) */
    /* added to every unit's counter */
    uint32_t computed, skipped, copied, probed, pass_probed, elided;
    uint32_t busy0_add;   /* added to the count of launches that every unit skipped */
    /* final values */
    uint32_t busy1;       /* index + 1 of the last launch in which a unit stored rows */
    uint32_t streak0, streak1, need, held, moved, twin; /* per unit */
    uint32_t twin_ok;
    uint32_t kept_passes, sure_passes; /* probe passes that count every owned tile */
} gol_still_effect;
gol_status gol_plan_still_step(uint32_t tb_depth, uint64_t generations, gol_still_effect* out);
gol_status gol_activity_fixed_steps(gol_engine* e, uint64_t* steps);
gol_status gol_activity_fixed_launches(gol_engine* e, uint64_t* launches);

/* The activity state as it lies on the device, after everything enqueued has run:
 * 12 * units + 3 words (engine_internal.h ActState names the regions), for tests that
 * compare two engines word for word.  *words receives the count; the words are copied
 * where cap holds them all, else GOL_EINVAL.  GOL_ESTATE: the engine keeps no activity
 * state (torus, composite, rank, group and resident engines). */
gol_status gol_activity_state(gol_engine* e, uint32_t* out, size_t cap, size_t* words);

/* Engine geometry as chosen (for tools / tests); any out pointer may be NULL.
 * rows_per_wave: the rows each wavefront streams in a full-depth launch. */
gol_status gol_info(gol_engine* e, uint64_t* h, uint64_t* w, uint64_t* row0,
                    uint64_t* rows, uint32_t* tb_depth, uint32_t* halo_depth,
                    uint32_t* rows_per_wave);

/* Launch plan of a full-depth launch as chosen (strip width in lanes, rows per
 * wavefront, planes per lane); with age-skewed blocks the rows per wavefront are
 * the shorter (young) length, gol_plan_skew gives both.  A composite engine
 * reports its first stripe's plan.  Any out pointer may be NULL. */
gol_status gol_plan_info(gol_engine* e, uint32_t* strip_lanes, uint32_t* rows_per_wave,
                         uint32_t* word_planes);

/* (r06) Resident plan details: rows per wavefront, band rows per tile, epoch
 * length K (generations between the tiles' swaps through memory), and
 * *swap_every: the generations between the wavefronts' row swaps through LDS
 * inside a tile (1 = every generation, life_res_kernel; >= 2 = the wave-level
 * temporal blocking of life_resident_mb.hip).  All 0 when the engine does not run
 * the resident kernel.  Out pointers may be NULL. */
gol_status gol_plan_resident_rows(gol_engine* e, uint32_t* rows, uint32_t* band_rows,
                                  uint32_t* epoch, uint32_t* swap_every);

/* Whether full-depth launches use hand-off row blocks (gol_config.handoff, as
 * the planner resolved it): 1 = yes, 0 = every block recomputes its halo. */
gol_status gol_plan_handoff(gol_engine* e, uint32_t* handoff);

/* Age-skewed row blocks of full-depth launches (a one-round launch at 2
 * wavefronts per SIMD: the units dispatched first win their SIMD's VALU
 * arbitration and get longer blocks): *rows_old rows for the first *units_old
 * units' blocks, *rows_young for the others; all 0 when the launches use equal
 * blocks.  A composite engine reports its first stripe (which never skews: its
 * stripes share the device).  Out pointers may be NULL. */
gol_status gol_plan_skew(gol_engine* e, uint32_t* rows_old, uint32_t* rows_young,
                         uint32_t* units_old);

/* Column layout of full-depth launches: *strips wavefront strips per row block
 * and the packed half strip's units (64-lane strips of a one-segment launch: the
 * last strip ends at the field's right edge and the gap of <= 30 lane groups
 * before it runs 32 lanes wide, two row blocks per wavefront): *half_units
 * wavefronts over *half_groups lane groups (both 0 without one).  A resident or
 * composite engine reports its first stripe / 0.  Out pointers may be NULL. */
gol_status gol_plan_columns(gol_engine* e, uint32_t* strips, uint32_t* half_units,
                            uint32_t* half_groups);

/* Resident plan (gol_config.resident): *on = 1 if gol_step runs the resident
 * kernel; then *bands x *strips tiles, one workgroup each (bands, strips may be
 * NULL).  A composite engine reports 0. */
gol_status gol_plan_resident(gol_engine* e, uint32_t* on, uint32_t* bands, uint32_t* strips);

/* The plan autotuner's outcome for the first full-depth launch plan (an engine
 * alone on its device times a few variants of the cost models' plan at create
 * and keeps one only if it is >= 3% faster): *variant 0 = the models' plan, else
 * 1 + the index in {no_half_strip, skew_0.95, skew_1.05, other_block_kind};
 * *tuned_us / *model_us = the best create-time launch of the plan that runs / of
 * the models' plan (0 when nothing was timed).  Out pointers may be NULL. */
gol_status gol_plan_tuning(gol_engine* e, uint32_t* variant, float* tuned_us, float* model_us);

/* (late r06) Exchange mode of a stripe engine: *mode = 1 blocking (the exchange after
 * the round's last launch), 2 overlapped (band launch, then the exchange beside
 * the interior launch), 0 for an engine without halo exchanges.  With
 * exchange_overlap = 0 a rank engine over RCCL chooses it at create by timing
 * rounds of both modes on its communicator (a collective: every rank of the job
 * runs the same rounds); *blocking_ms / *overlapped_ms are then the max over ranks
 * of each mode's best time per round, else 0.  gol_round_schedule called with
 * exchange_overlap set to *mode lists what gol_step runs.  Out pointers may be
 * NULL. */
gol_status gol_plan_exchange(gol_engine* e, uint32_t* mode, float* blocking_ms,
                             float* overlapped_ms);

/* Passes per full-depth launch of the first full-depth plan: 1, or 2-3 for
 * multi-pass launches (each launch runs that many depth-K passes over its row
 * blocks, alternating direction; dev switch GOL_DEV_PASSES at create, read only by
 * the dev build, libgol_dev.so: the shipped library has no multi-pass kernel
 * since r06 and always reports 1). */
gol_status gol_plan_passes(gol_engine* e, uint32_t* passes);

/* gol_digest restricted to field rows [row0, row0 + rows) (for a rank engine:
 * the part of its own rows inside that range).  Lets one engine of the whole
 * field check each rank's stripe separately. */
gol_status gol_digest_rows(gol_engine* e, uint64_t row0, uint64_t rows, uint64_t* live,
                           uint64_t* hash);

/* ---- Region I/O: rectangles of a field that stays on the GPU ----
 * A window is canonical and packed like gol_load_packed's words: bit j of word q of
 * window row i is field cell (y + i, x + 64q + j); row_stride_words >= ceil(rw/64).
 * Only the window moves between host and device, never the field, and every call
 * returns after the host buffer has been filled or consumed.
 * Bounds (else GOL_EINVAL): y + rh <= h and x + rw <= w.  On a torus
 * (GOL_SEM_TORUS) y < h, x < w, rh <= h, rw <= w, and the rectangle may cross either
 * seam or both: window cell (i, j) is field cell ((y + i) mod h, (x + j) mod w).
 * rh == 0 or rw == 0: GOL_OK, nothing done.
 * Rank engines and group members take the coordinates of the global field and
 * apply the part of the rectangle that lies in their own rows. */

/* Reads the rectangle; bits at or beyond rw in a row's last word are written 0.
 * Waits for the engine's work first, like gol_store_packed.  A rank engine
 * zero-fills the window rows it does not own (OR the ranks' windows together). */
gol_status gol_read_rect(gol_engine* e, uint64_t y, uint64_t x, uint64_t rh, uint64_t rw,
                         uint64_t* words, uint64_t row_stride_words);

/* Combines the window into the field between steps: SET copies it, OR / XOR
 * combine, CLEAR is field AND NOT window; an unknown op is GOL_EINVAL.  Window bits
 * at or beyond rw are ignored, and no cell outside the rectangle changes.  Like a
 * load it finishes the engine's streams first, and the next gol_step of a stripe
 * engine starts with a halo exchange; so for rank engines it is collective like a
 * load: every rank calls it with the same rectangle before the next gol_step.
 * GOL_SEM_REF_STRIPES engines return GOL_ESTATE (their overlap rows exist twice
 * and evolve apart: "the cell" is ambiguous); reads and densities work there. */
typedef enum gol_rect_op {
    GOL_RECT_SET = 0,
    GOL_RECT_OR = 1,
    GOL_RECT_XOR = 2,
    GOL_RECT_CLEAR = 3
} gol_rect_op;
gol_status gol_write_rect(gol_engine* e, uint64_t y, uint64_t x, uint64_t rh, uint64_t rw,
                          const uint64_t* words, uint64_t row_stride_words, uint32_t op);

/* Live cells per block: the window is tiled with by x bx blocks from its corner
 * (edge blocks partial), counts[bi * row_stride + bj] = live cells of block (bi,
 * bj), row_stride >= ceil(rw/bx).  GOL_EINVAL if by, bx, rh or rw is 0 or by * bx
 * > UINT32_MAX.  Only the counts move to the host.  A rank engine counts its own
 * rows only (add the ranks' counts, as with gol_digest). */
gol_status gol_density(gol_engine* e, uint64_t y, uint64_t x, uint64_t rh, uint64_t rw,
                       uint64_t by, uint64_t bx, uint32_t* counts, uint64_t row_stride);

/* Host-only, no GPU: the blit the kernels run, on canonical packed words.  Bits
 * [sx, sx + cols) of each of `rows` rows of src are combined with op (gol_rect_op)
 * onto bits [dx, dx + cols) of dst; no other bit of dst changes.  Strides in words,
 * src_stride_words >= ceil((sx + cols)/64), dst_stride_words >= ceil((dx + cols)/64). */
gol_status gol_rect_blit(const uint64_t* src, uint64_t src_stride_words, uint64_t sx,
                         uint64_t* dst, uint64_t dst_stride_words, uint64_t dx, uint64_t rows,
                         uint64_t cols, uint32_t op);

/* ---- Snapshots: one earlier generation kept on the device ----
 * One snapshot slot per engine: keep the field as it is now, ask later whether the
 * field equals it or in how many cells it differs, go back to it, and step until the
 * field repeats.  Nothing but one word or one count moves to the host.  An engine that
 * never calls gol_snapshot allocates nothing for the slot.
 * Engines: gol_create with GOL_SEM_GLOBAL (a composite engine keeps one slot per
 * stripe and adds the stripes' answers up) or GOL_SEM_TORUS (the h x w interior is what
 * is compared; the ghost cells are not).  GOL_SEM_REF_STRIPES engines, rank engines
 * and group members return GOL_ESTATE from every call of this section: a partitioned
 * field's answer is a collective one. */

/* Keeps a device copy of the field as it is now, enqueued behind the engine's work; it
 * does not wait on the host.  The first call allocates the slot (as much device memory
 * as one of the engine's two field buffers; GOL_ENOMEM if that fails), a later call
 * replaces the snapshot.  Loads, steps and edits after the call do not touch it. */
gol_status gol_snapshot(gol_engine* e);
/* *same = 1 if every cell of the h x w field equals the snapshot's, else 0.  Waits for
 * the engine's work and reads both fields at most once: it may stop as soon as one
 * difference is known.  GOL_ESTATE without a snapshot. */
gol_status gol_snapshot_same(gol_engine* e, uint32_t* same);
/* *cells = the exact number of field cells that differ from the snapshot's.  Waits for
 * the engine's work.  GOL_ESTATE without a snapshot. */
gol_status gol_snapshot_diff(gol_engine* e, uint64_t* cells);
/* Makes the field the snapshot's field again; the snapshot stays.  A writer of the
 * field like gol_write_rect: it finishes the engine's streams first.  GOL_ESTATE
 * without a snapshot. */
gol_status gol_snapshot_restore(gol_engine* e);
/* Frees the slot (GOL_OK when there is none); gol_destroy does the same. */
gol_status gol_snapshot_drop(gol_engine* e);

/* Steps until the field repeats with a period that divides `lag`, or for
 * max_generations.  This call uses the snapshot slot: it replaces whatever the slot
 * held, and on return the slot holds what the last check left in it.
 * 1 <= lag <= 65536; check_every = 0 means the least multiple of 64 that is >= lag,
 * else check_every >= lag (GOL_EINVAL otherwise).  Checks happen at the generations
 * g = c * check_every, c = 1, 2, ..., counted from the call: the field of generation
 * g - lag is kept as the snapshot and compared with generation g's.  The first g at
 * which they are equal ends the run: then the minimal period p (a divisor of lag) is
 * found by stepping on through lag's proper divisors in ascending order, comparing
 * each time, and the field of generation g is restored.  If the next check would lie
 * beyond max_generations, the generations that remain are run and period = 0.
 * On return the engine holds generation `advanced`'s field; with GOL_UNTIL_FINISH and a
 * period found it then runs (max_generations - g) mod p generations more, after which
 * it holds the field gol_step(e, max_generations) would have left.
 * out->struct_size must be sizeof(gol_until) and flags 0 or GOL_UNTIL_FINISH
 * (GOL_EINVAL otherwise, before anything is stepped).
 * Why a lag and no cycle search: comparing with one kept generation costs one pass
 * over the field per check and one slot, and finds every period that divides lag (16
 * covers still lifes, blinkers and the period 2, 4, 8 and 16 oscillators; 30 the
 * common 2, 3, 5, 6, 15); a search for an unknown period would have to keep, or
 * recompute, every generation back to the cycle's start. */
#define GOL_UNTIL_FINISH 1u
typedef struct gol_until {
    uint32_t struct_size;   /* in: sizeof(gol_until) of the caller, as gol_timing does */
    uint32_t period;        /* out: minimal period found, 0 = none within max_generations */
    uint64_t advanced;      /* out: g, the generation (counted from the call) whose field the
                               engine holds, before any GOL_UNTIL_FINISH residue */
    uint32_t lag, check_every; /* out: as used (check_every resolved from 0) */
    uint32_t checks;        /* out: lag comparisons made */
    uint32_t extra_generations; /* out: generations run beyond g to find the minimal period */
} gol_until;
gol_status gol_step_until_periodic(gol_engine* e, uint64_t max_generations, uint32_t lag,
                                   uint32_t check_every, uint32_t flags, gol_until* out);

/* ---- Batches: many small independent fields stepped in one launch ----
 * A gol_batch holds n fields of the same h x w, the same rule (or, after
 * gol_batch_set_rules, a rule per field) and the same boundary on
 * one device and advances all of them with one kernel launch per step: a lane holds a
 * 64-column word of a field and all its rows in registers, so a 64 x 64 field is one
 * lane, a wavefront 64 fields, and between a launch's loads and stores nothing touches
 * memory.  Every field evolves exactly as an h x w gol_create engine would.
 * Create: cfg supplies birth_mask, survive_mask, device and semantics.  GOL_SEM_GLOBAL
 * gives every field a dead border; GOL_SEM_TORUS joins every field's opposite edges, for
 * any h, w >= 1, by the torus engine's definition (a field so small that a cell is its
 * own neighbour included); GOL_SEM_REF_STRIPES is GOL_EINVAL.  Every other gol_config
 * field must be 0 (ref_ranks: 0 or gol_config_init's 1), else GOL_EINVAL: a batch has no
 * plan knobs.
 * Limits: 1 <= h <= 64, 1 <= w <= 4096, n >= 1 and n * lanes_per_field <= 2^31; beyond
 * them GOL_EINVAL with a message that names gol_create, the engine for larger fields.
 * Like gol_create, bad arguments are rejected before the GPU is touched.
 * Geometry (fixed): lanes_per_field = the least power of two >= ceil(w/64),
 * fields_per_wave = 64 / lanes_per_field, rows_in_regs = the least of {8, 16, 32, 64}
 * that is >= h, waves = ceil(n / fields_per_wave).
 * I/O: fields [first, first + count), canonical packed words as gol_load_packed's: word
 * q of row r of field first + i at words[i * field_stride_words + r * row_stride_words
 * + q]; row_stride_words >= ceil(w/64), field_stride_words >= h * row_stride_words and
 * first + count <= n, else GOL_EINVAL; count == 0 is GOL_OK with nothing done.  Bits of
 * the input at columns >= w are ignored, and a store writes 0 there.  Every I/O call and
 * gol_batch_digest returns after the caller's buffer has been consumed or filled, as
 * gol_read_rect does.  The _device forms take a device pointer on the batch's device and
 * move nothing to the host; the caller makes sure its own work on that buffer has
 * finished before the call.  The host forms are the device forms behind a staging
 * buffer.
 * Errors go through gol_status and gol_last_error; a handle is not thread-safe; the
 * batch owns its stream and its memory. */
typedef struct gol_batch gol_batch;

/* Host-only, no GPU: the geometry gol_batch_create would use (the same GOL_EINVALs).
 * Out pointers may be NULL. */
gol_status gol_batch_geometry(uint64_t n, uint64_t h, uint64_t w, const gol_config* cfg,
                              uint32_t* lanes_per_field, uint32_t* fields_per_wave,
                              uint32_t* rows_in_regs, uint64_t* waves);
/* All fields start dead.  GOL_DEV_BATCH_LAUNCH_GENS=<k> in the environment sets the
 * launch cap (gol_batch_step) of the batch being created. */
gol_status gol_batch_create(uint64_t n, uint64_t h, uint64_t w, const gol_config* cfg,
                            gol_batch** out);
void gol_batch_destroy(gol_batch* b);
/* The batch as created; *launch_generations is the launch cap.  Out pointers may be NULL. */
gol_status gol_batch_info(gol_batch* b, uint64_t* n, uint64_t* h, uint64_t* w,
                          uint32_t* lanes_per_field, uint32_t* fields_per_wave,
                          uint32_t* rows_in_regs, uint32_t* launch_generations);

gol_status gol_batch_load_packed(gol_batch* b, uint64_t first, uint64_t count,
                                 const uint64_t* words, uint64_t field_stride_words,
                                 uint64_t row_stride_words);
gol_status gol_batch_store_packed(gol_batch* b, uint64_t first, uint64_t count, uint64_t* words,
                                  uint64_t field_stride_words, uint64_t row_stride_words);
gol_status gol_batch_load_device(gol_batch* b, uint64_t first, uint64_t count,
                                 const uint64_t* words, uint64_t field_stride_words,
                                 uint64_t row_stride_words);
gol_status gol_batch_store_device(gol_batch* b, uint64_t first, uint64_t count, uint64_t* words,
                                  uint64_t field_stride_words, uint64_t row_stride_words);

/* Field i becomes exactly what gol_init_random(e, seed + i) gives an h x w engine.
 * Enqueued like a step. */
gol_status gol_batch_init_random(gol_batch* b, uint64_t seed);

/* Advances every field `generations` generations in ceil(generations /
 * launch_generations) launches (default cap 4096, so that no single launch holds a
 * shared GPU for long).  Returns after the work is enqueued; gol_batch_sync waits. */
gol_status gol_batch_step(gol_batch* b, uint64_t generations);
gol_status gol_batch_sync(gol_batch* b);

/* Steps every field until it repeats with a period that divides `lag`, or for
 * max_generations: gol_step_until_periodic for all n fields at once, in the batch
 * kernel.  With F_i(g) field i's state g generations after the call, L = lag and
 * C = check_every (0 means the least multiple of 64 that is >= L, as
 * gol_step_until_periodic): checks happen at g = C, 2 C, ... <= max_generations, and the
 * first such g with F_i(g) == F_i(g - L), cell for cell, ends field i's search:
 * generation[i] = g and period[i] = the least divisor p of L with F_i(g - L + p) ==
 * F_i(g - L), which is the cycle's minimal period (the orbit from g - L on is purely
 * periodic, so its minimal period divides L).  No repeat found: period[i] = 0 and
 * generation[i] = max_generations.  On return every field holds F_i(max_generations),
 * word for word what gol_batch_step(b, max_generations) would have left: a field in a
 * known cycle need not be computed to know that state, so a wavefront whose fields have
 * all been found stops computing, and once every wavefront has, nothing more is
 * launched.  The call is synchronous like gol_batch_digest; only n periods, n
 * generations and a few counters cross to the host.  A later call counts from 0 again
 * and forgets earlier results.  `period` and `generation` ([n] each) may be NULL.
 * GOL_EINVAL, before anything is stepped: null batch or out, out->struct_size not
 * sizeof(gol_batch_until), lag outside 1..1024 (no such lag has more than 32 divisors,
 * which travel in the kernel's arguments), 0 < check_every < lag, check_every > 65536.
 * max_generations == 0: GOL_OK with nothing run, every period and generation 0.
 * The first call allocates a snapshot buffer as large as the batch (GOL_ENOMEM if that
 * fails), freed by gol_batch_destroy. */
typedef struct gol_batch_until {
    uint32_t struct_size;      /* in: sizeof(gol_batch_until), as gol_until */
    uint32_t lag, check_every; /* out: as used (check_every resolved from 0) */
    uint32_t launches;         /* out: kernel launches issued by this call */
    uint32_t reserved;
    uint64_t found;            /* out: fields with period != 0 */
    uint64_t wave_generations; /* out: generations computed, summed over wavefronts */
} gol_batch_until;
gol_status gol_batch_step_until_periodic(gol_batch* b, uint64_t max_generations, uint32_t lag,
                                         uint32_t check_every, uint32_t* period,
                                         uint64_t* generation, gol_batch_until* out);

/* Host-only, no GPU: how gol_batch_step_until_periodic splits its work for a batch whose
 * launch cap is launch_generations (the same GOL_EINVALs for lag and check_every; null
 * out is GOL_EINVAL).  Every launch covers whole check intervals, each starting at a
 * multiple of check_every; the last one also runs the tail. */
typedef struct gol_batch_until_plan {
    uint32_t check_every;        /* resolved */
    uint32_t ndivisors;          /* proper divisors of lag, ascending, in divisors[] */
    uint32_t divisors[32];
    uint64_t checks;             /* max_generations / check_every */
    uint32_t tail;               /* max_generations % check_every */
    uint32_t checks_per_launch;  /* max(1, launch_generations / check_every) */
    uint64_t launches;           /* ceil(checks / checks_per_launch), at least 1 if max_generations > 0 */
} gol_batch_until_plan;
gol_status gol_batch_until_plan_of(uint64_t max_generations, uint32_t lag, uint32_t check_every,
                                   uint32_t launch_generations, gol_batch_until_plan* out);

/* Population traces: every field's live cells sampled in the kernel while it steps.
 * With F_i(g) field i's state g generations after the call: live[s * sample_stride + i] =
 * the live cells of F_i((s + 1) * every), for 0 <= s < samples = generations / every and
 * 0 <= i < n; exactly the `live` gol_batch_digest would return at that generation.
 * Elements at columns i >= n of a row of `live` are not touched.  On return every field
 * holds F_i(generations), word for word what gol_batch_step(b, generations) leaves: the
 * tail of generations % every generations is run and not sampled.  Each call counts from
 * 0.  A count fits 32 bits (a field has at most 64 x 4096 cells).  While a rule table
 * exists (gol_batch_set_rules) the call runs the rule-per-lane kernels, like
 * gol_batch_step.  A sample costs one popcount per row and plane in the registers that
 * hold the field between two generations, a sum over the field's lanes and one 4-byte
 * store; the fields are loaded and stored once per launch, not once per sample.
 * Both forms are synchronous like gol_batch_digest: they return after the caller's buffer
 * is filled.  The _device form takes a device pointer on the batch's device; the host form
 * is the device form behind a buffer of samples * n words that the batch owns, allocated
 * at the first call, grown on demand (GOL_ENOMEM if that fails) and freed by
 * gol_batch_destroy.
 * Each launch covers whole sample intervals and the last one also runs the tail, as
 * gol_batch_trace_plan_of tells; the call issues exactly that plan's launches.
 * generations == 0: GOL_OK with nothing run.  generations < every: no samples, the fields
 * stepped, one launch.
 * GOL_EINVAL, before anything is stepped: null batch or out, out->struct_size not
 * sizeof(gol_batch_trace), every == 0 or every > 65536 (gol_batch_step_until_periodic's
 * bound on an interval, so that no launch outruns the launch cap by more than it does
 * there), and while samples > 0: sample_stride < n, null live, samples * sample_stride
 * not representable. */
typedef struct gol_batch_trace {
    uint32_t struct_size;   /* in: sizeof(gol_batch_trace), as gol_batch_until */
    uint32_t every;         /* out: as used */
    uint64_t samples;       /* out: generations / every */
    uint32_t launches;      /* out: kernel launches issued by this call */
    uint32_t reserved;
} gol_batch_trace;
gol_status gol_batch_step_trace(gol_batch* b, uint64_t generations, uint32_t every,
                                uint32_t* live, uint64_t sample_stride, gol_batch_trace* out);
gol_status gol_batch_step_trace_device(gol_batch* b, uint64_t generations, uint32_t every,
                                       uint32_t* live, uint64_t sample_stride,
                                       gol_batch_trace* out);

/* Host-only, no GPU: how gol_batch_step_trace splits its work for a batch whose launch cap
 * is launch_generations.  GOL_EINVAL: null out, every == 0, every > 65536. */
typedef struct gol_batch_trace_plan {
    uint64_t samples;             /* generations / every */
    uint32_t tail;                /* generations % every */
    uint32_t samples_per_launch;  /* max(1, launch_generations / every) */
    uint64_t launches;            /* max(1, ceil(samples / samples_per_launch)) if generations > 0, else 0 */
} gol_batch_trace_plan;
gol_status gol_batch_trace_plan_of(uint64_t generations, uint32_t every,
                                   uint32_t launch_generations, gol_batch_trace_plan* out);

/* Rollouts: the states of a window of fields, written by the kernel while it steps.
 * With F_i(g) field i's state g generations after the call, for 0 <= s < samples =
 * generations / every, 0 <= j < count, r < h and q < ceil(w/64):
 *   frames[s * sample_stride_words + j * field_stride_words + r * row_stride_words + q]
 *       = canonical word q of row r of F_{first+j}((s + 1) * every),
 * exactly the words gol_batch_store_packed(b, first, count, ...) would write at that
 * generation; bits at columns >= w are 0.  No other word of `frames` is touched: gaps left
 * by wider strides keep what they held.  On return every one of the n fields, inside the
 * window or not, holds F_i(generations), word for word what gol_batch_step(b, generations)
 * leaves: the tail of generations % every generations is run and not recorded.  Each call
 * counts from 0.  While a rule table exists (gol_batch_set_rules) the call runs the
 * rule-per-lane kernels, like gol_batch_step.  A sample costs one 8-byte store per row by
 * every lane that holds a word of a field of the window, from the registers that hold the
 * field between two generations; wavefronts with no field in the window store nothing, and
 * the fields are loaded and stored once per launch, not once per sample.
 * Both forms are synchronous like gol_batch_step_trace: they return after the caller's
 * buffer is filled.  The _device form takes a device pointer on the batch's device; the
 * host form is the device form behind a compact buffer of samples * count * h * ceil(w/64)
 * words that the batch owns, allocated at the first call, grown on demand (GOL_ENOMEM if
 * that fails, and the fields are not stepped) and freed by gol_batch_destroy, which is then
 * copied to the caller with the caller's strides.
 * The call issues exactly the launches of gol_batch_trace_plan_of(generations, every,
 * launch_generations): whole sample intervals per launch, the tail in the last one.
 * generations == 0: GOL_OK with nothing run.  generations < every: no samples, the fields
 * stepped, one launch.  count == 0: the fields are stepped and nothing is recorded.
 * GOL_EINVAL, before anything is stepped and with nothing changed, in this order: null
 * batch; null out; out->struct_size not sizeof(gol_batch_record); every == 0 or
 * every > 65536; first + count > n; and while samples > 0 and count > 0:
 * row_stride_words < ceil(w/64), field_stride_words < h * row_stride_words,
 * sample_stride_words < count * field_stride_words, null frames,
 * samples * sample_stride_words * 8 not representable. */
typedef struct gol_batch_record {
    uint32_t struct_size;   /* in: sizeof(gol_batch_record), as gol_batch_trace */
    uint32_t every;         /* out: as used */
    uint64_t samples;       /* out: generations / every */
    uint32_t launches;      /* out: kernel launches issued by this call */
    uint32_t reserved;
} gol_batch_record;
gol_status gol_batch_step_record(gol_batch* b, uint64_t generations, uint32_t every,
                                 uint64_t first, uint64_t count, uint64_t* frames,
                                 uint64_t sample_stride_words, uint64_t field_stride_words,
                                 uint64_t row_stride_words, gol_batch_record* out);
gol_status gol_batch_step_record_device(gol_batch* b, uint64_t generations, uint32_t every,
                                        uint64_t first, uint64_t count, uint64_t* frames,
                                        uint64_t sample_stride_words,
                                        uint64_t field_stride_words, uint64_t row_stride_words,
                                        gol_batch_record* out);

/* Per-field rules: one launch sweeps many rules.
 * gol_batch_set_rules gives field first + i the rule (birth[i], survive[i]), 9-bit masks
 * as gol_config's.  The first call with count > 0 allocates a device table of n words
 * (birth | survive << 16) in which every field starts with the create rule; a call writes
 * its range into the table and leaves every other field's rule as it is, so later calls
 * overwrite only their own range.  While the table exists, gol_batch_step and
 * gol_batch_step_until_periodic run the kernels that hold a rule per lane for every
 * field, fields that happen to share one rule included, and each field evolves exactly
 * as a batch created with that field's rule would.  Loads, stores, gol_batch_init_random,
 * gol_batch_digest and the geometry are untouched.  The table copy is enqueued on the
 * batch's stream, behind the steps already enqueued, which therefore still run by the
 * rules they were enqueued under; like gol_batch_load_packed the call returns once the
 * caller's arrays have been consumed.  The table is a call of its own and not a create
 * argument because a rule table is data like the fields: set per range and replaceable
 * between steps.
 * GOL_EINVAL: null batch, first + count > n, null birth or survive with count > 0, any
 * mask above 0x1FF; in each of these cases nothing changes: no table is made and an
 * existing one is not altered.  count == 0 is GOL_OK with nothing done and nothing
 * allocated.  GOL_ENOMEM if the table cannot be allocated.  gol_batch_destroy frees it. */
gol_status gol_batch_set_rules(gol_batch* b, uint64_t first, uint64_t count,
                               const uint32_t* birth, const uint32_t* survive);
/* The rule each of the fields [first, first + count) runs: the table's, or the create rule
 * where none was set.  Either array may be NULL.  GOL_EINVAL: null batch, first + count >
 * n.  Synchronous like gol_batch_digest. */
gol_status gol_batch_get_rules(gol_batch* b, uint64_t first, uint64_t count, uint32_t* birth,
                               uint32_t* survive);
/* Back to the one rule given at create: waits for the steps enqueued and frees the table.
 * GOL_OK when there is none. */
gol_status gol_batch_drop_rules(gol_batch* b);
/* *on = 1 while the batch steps with per-field rules, else 0.  Host only. */
gol_status gol_batch_has_rules(gol_batch* b, uint32_t* on);

/* live[i], hash[i] = exactly what gol_digest returns for an h x w engine that holds
 * field first + i (either array may be NULL).  Only 2 * count words cross to the host. */
gol_status gol_batch_digest(gol_batch* b, uint64_t first, uint64_t count, uint64_t* live,
                            uint64_t* hash);

/* ---- Multi-GPU, one process per GPU (replaces the MPI stripes :70-81 and the
 * halo exchange :104-145 with RCCL send/recv over xGMI) ---- */

/* Rows of global stripe `rank` of `nranks`: contiguous, ceil-balanced.
 * Host-only; needs no GPU. */
gol_status gol_rank_rows(uint64_t h, int nranks, int rank, uint64_t* row0, uint64_t* rows);

/* Generate an RCCL unique id on one rank; broadcast its 128 bytes to the
 * others by any means (torch.distributed, a file, MPI). */
gol_status gol_comm_unique_id(uint8_t id[128]);

/* Engine for stripe `rank` of `nranks` of an h x w GLOBAL field; all ranks call
 * it collectively with the same id.  cfg->semantics must be GLOBAL (rank engines,
 * groups and gol_round_schedule reject GOL_SEM_TORUS: a torus is one engine on
 * one GPU). */
gol_status gol_create_rank(uint64_t h, uint64_t w, const gol_config* cfg, int rank,
                           int nranks, const uint8_t id[128], gol_engine** out);

/* The RCCL communicator of a gol_create_rank engine as RCCL reports it
 * (ncclCommCount, ncclCommUserRank, ncclCommCuDevice) and the engine's up/down
 * peers (-1: no such neighbour).  Out pointers may be NULL.  GOL_ESTATE for an
 * engine without a communicator. */
gol_status gol_comm_info(gol_engine* e, int* count, int* rank, int* peer_up, int* peer_down,
                         int* device);

/* Halo transport supplied by the caller (host memory): the same rank engine,
 * partition and rounds as gol_create_rank, but each exchange stages the Hx
 * boundary rows through host buffers and calls `exchange`, which must send
 * send_up to rank-1 and send_down to rank+1 and receive recv_up from rank-1 and
 * recv_down from rank+1, `bytes` each (NULL pointers where there is no such
 * neighbour), and return 0 on success.  This is the reference's own transport
 * shape (MPI_Sendrecv of boundary rows, Parallel_Life_MPI.cpp:104-145, here with
 * the receive landing in the halo); gol-mpi --transport mpi uses it, and it lets
 * several ranks share one GPU, which RCCL refuses. */
typedef int (*gol_halo_exchange_fn)(void* ctx, const void* send_up, void* recv_up,
                                    const void* send_down, void* recv_down, uint64_t bytes);
typedef struct gol_transport {
    gol_halo_exchange_fn exchange;
    void* ctx;
} gol_transport;
gol_status gol_create_rank_transport(uint64_t h, uint64_t w, const gol_config* cfg, int rank,
                                     int nranks, const gol_transport* transport,
                                     gol_engine** out);

/* The launch/exchange schedule a rank engine (or group member) runs for one
 * gol_step(generations) call -- host-only, no GPU needed; gol_step executes
 * exactly this list.  halo_fresh: the previous call ended with an overlapped
 * exchange still to be waited for (0 after create/load).  Launch ops name the
 * local buffer rows they write (local row i = field row row0 - Hx + i).
 * Computed is not valid: since r04 every full-depth launch of a round writes
 * the first launch's region, so after a launch only the rows inside
 * [shrink, buf_rows - shrink) (buf_rows = own rows + 2 Hx, shrink = this op's
 * field) hold that generation; rows of [out_lo, out_hi) outside that range were
 * computed from rows that were no longer valid and must not be read (an external
 * transport moves only [Hx, 2 Hx) and [R, R + Hx) after a round's last launch,
 * which are always valid). */
typedef enum gol_sched_kind {
    GOL_OP_EXCHANGE = 0,       /* blocking halo exchange on the compute stream */
    GOL_OP_WAIT_EXCHANGE = 1,  /* compute waits for the overlapped exchange */
    GOL_OP_LAUNCH = 2,         /* stencil launch over the valid region */
    GOL_OP_BAND = 3,           /* last launch of a round, boundary rows only */
    GOL_OP_INTERIOR = 4,       /* ... and the rest of the own rows, concurrently */
    GOL_OP_EXCHANGE_ASYNC = 5  /* exchange of the band rows, overlapping INTERIOR */
} gol_sched_kind;
typedef struct gol_sched_op {
    uint32_t kind;      /* gol_sched_kind */
    uint32_t depth;     /* fused generations of a launch (0 otherwise) */
    uint32_t shrink;    /* halo rows consumed per side once this launch is done */
    uint32_t nseg;      /* row ranges a launch writes: [out_lo[i], out_hi[i]); valid
                           only inside [shrink, buf_rows - shrink), see above */
    int64_t out_lo[2];
    int64_t out_hi[2];
} gol_sched_op;
gol_status gol_round_schedule(uint64_t h, uint64_t w, const gol_config* cfg, int rank,
                              int nranks, uint64_t generations, int halo_fresh,
                              gol_sched_op* ops, uint64_t cap, uint64_t* nops,
                              uint32_t* tb_depth, uint32_t* halo_depth);

/* Host-only planning model (no GPU needed): the launch plans gol_create
 * (nranks = 1: a single-stream engine) or gol_create_rank (rank of nranks)
 * would build on a device of `cus` compute units whose stencil kernels fit
 * occ_classic (classic blocks) / occ_hand (hand-off blocks) 256-thread
 * workgroups per CU, as the occupancy query reports them, before the autotuner
 * times its candidates.  Summarises the first full-depth launch plan: what the
 * planner's tests check (tests/test_planner.py, also run under the host
 * sanitizers) and what tools print. */
typedef struct gol_plan_summary {
    uint32_t tb_depth, halo_depth;
    uint32_t plans, distinct_plans; /* launch plans built; aliases share one */
    int64_t rows_lo, rows_hi;       /* buffer rows the plan computes */
    int64_t rows_per_wave;          /* the block length (the young one when skewed) */
    int32_t rows_old, units_old;    /* age-skewed blocks: old length and units (0: none) */
    int32_t strips, lane_shift;     /* strips per row block, strip width 64 >> lane_shift */
    int64_t total_units;            /* wavefronts of the launch */
    int64_t half_units;             /* of which run the packed half strip */
    int64_t blocks;                 /* row blocks per strip (summed over segments) */
    int32_t handoff, tail_off;      /* hand-off blocks, their kernel's tail offset (-1) */
    uint32_t candidates;            /* autotuner variants built for this plan */
    uint32_t passes;                /* passes per full-depth launch (gol_plan_passes);
                                       always 1 with the shipped library (multi-pass
                                       kernels: dev build).  The model assumes the
                                       multi-pass kernels fit the same occupancies
                                       as the single-pass ones (their real occupancy
                                       may be lower, where the engine would then
                                       fall back to single-pass launches). */
} gol_plan_summary;
gol_status gol_plan_model(uint64_t h, uint64_t w, const gol_config* cfg, int rank, int nranks,
                          int cus, int occ_classic, int occ_hand, gol_plan_summary* out);

/* Host-only, same model: the activity skip's view of the single-stream engine's
 * launch plan.  Per unit two output rectangles of 4 words each in `rects` (rows
 * [r0, r1) x 64-column lane groups [q0, q1); r1 <= r0: none; 8 words per unit) and
 * its neighbour list in CSR form (offsets[units + 1], ids): the units whose
 * streaks the unit reads before it may skip a launch.  *units and *nids return
 * the sizes; the arrays are filled only when unit_cap / id_cap hold them (pass 0
 * and NULLs to ask).  A plan that never skips (hand-off blocks, several segments)
 * has *nids == 0. */
gol_status gol_plan_neighbours(uint64_t h, uint64_t w, const gol_config* cfg, int cus,
                               int occ_classic, int occ_hand, int64_t* rects,
                               uint32_t* offsets, uint64_t unit_cap, uint32_t* ids,
                               uint64_t id_cap, uint64_t* units, uint64_t* nids);

/* Host-only, same model: the probe pass's table of that plan.  The plan's output
 * rows are cut into tiles of *tile_rows rows x *tile_words 64-column words, row
 * chunks from the first output row, *ncol column segments per chunk fastest; per
 * tile *slots unit indices in `table` (unused slots ~0): every unit one of whose
 * rectangles (gol_plan_neighbours), dilated by depth - 1 cells and clipped to the
 * field, meets the tile.  *ntile returns the tile count, 0 for a plan without the
 * pass (no copy pass, or a tile with more units than slots); `table` is filled only
 * when cap >= *ntile x *slots words (pass NULL and 0 to ask).  tile_rows, tile_words
 * and slots may be NULL. */
gol_status gol_plan_probe_tiles(uint64_t h, uint64_t w, const gol_config* cfg, int cus,
                                int occ_classic, int occ_hand, uint32_t* table, uint64_t cap,
                                uint32_t* tile_rows, uint32_t* tile_words, uint32_t* slots,
                                uint64_t* ntile, uint64_t* ncol);

/* ---- Torus geometry and wrap rule, host-only (no GPU needed) ---- */

/* The geometry gol_create would use for an h x w engine with this config
 * (cfg->semantics must be GOL_SEM_TORUS; the same GOL_EINVALs as gol_create):
 * *round_gens = G generations per wrap round, *ghost_rows = G rows above and below,
 * *ghost_words = ceil(G/64) words of 64 ghost columns left and right, and the
 * inner engine's field *padded_h x *padded_w = (h + 2G) x (w + 128 ghost_words).
 * Out pointers may be NULL. */
gol_status gol_torus_geometry(uint64_t h, uint64_t w, const gol_config* cfg,
                              uint32_t* round_gens, uint32_t* ghost_rows,
                              uint32_t* ghost_words, uint64_t* padded_h, uint64_t* padded_w);

/* The wrap on canonical packed words, through the same word gather as the wrap
 * kernel: fills the whole padded field `out` ((h + 2 ghost_rows) rows of
 * out_stride_words >= ceil(w/64) + 2 ghost_words words), interior included, from
 * the h x w `field`: padded cell (y, x) = field cell ((y - ghost_rows) mod h,
 * (x - 64 ghost_words) mod w); columns >= w + 128 ghost_words are 0.  Bits of
 * `field` at columns >= w are ignored. */
gol_status gol_torus_pad(const uint64_t* field, uint64_t row_stride_words, uint64_t h,
                         uint64_t w, uint32_t ghost_rows, uint32_t ghost_words, uint64_t* out,
                         uint64_t out_stride_words);

/* ---- Multi-GPU (or multi-stripe) inside ONE process, no RCCL ----
 * `nranks` stripe engines of one GLOBAL field (the same partition and halo
 * rounds as gol_create_rank), stripe r on devices[r] (NULL = cfg->device for
 * all; repeats allowed, so several stripes can share one GPU).  Halos move by
 * device-to-device / xGMI peer copies ordered with HIP events.  Members are
 * loaded, stored and digested one by one like rank engines, advanced together
 * by gol_group_step, and destroyed with gol_destroy. */
gol_status gol_create_group(uint64_t h, uint64_t w, const gol_config* cfg, int nranks,
                            const int* devices, gol_engine** engines);
gol_status gol_group_step(gol_engine** engines, int nranks, uint64_t generations);

#ifdef __cplusplus
}
#endif

#endif /* GOL_H */
