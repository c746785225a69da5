// life_batch.h -- the batch kernel: many small independent fields, one launch per
// step (gol_batch, batch.cpp; DESIGN §4 "life_batch_kernel").
//
// The first part is the interface between batch.cpp and the kernels (host code
// includes it as it stands).  The second part, behind GOL_BATCH_DEVICE, is the kernel
// itself: included by one translation unit per register-row count
// (life_batch_r<R>.hip), each of which instantiates life_batch_kernel<R, RULE> for
// the three rule kinds.
//
// Kernel shape (one wavefront = 64 / lanes_per_field fields, no LDS, no barriers):
//   * A lane holds one 64-column word of one field, column-split into two 32-bit
//     planes (bitlayout.h), for all R = rows_in_regs rows: 2 R VGPRs of state.  The
//     lanes_per_field (a power of two) lanes of a field are adjacent; words beyond
//     ceil(w/64) and lanes beyond field n - 1 hold zeros and store nothing.
//   * One generation is one fully unrolled pass down the rows with a single rolling
//     stage of life_stencil.h (StageT: the H3 sums of the two rows above and the cells
//     of the row above): step t ingests row t and emits row t - 1, which goes back
//     into the registers of the row it replaces.  The generation loop is a runtime
//     loop around the pass: between a launch's loads and its stores nothing touches
//     memory.
//   * Horizontal ends: inside a word the v_alignbit form of life_stencil.h; across
//     the lanes of a field a DPP wave shift that is replaced at the field's first and
//     last lane by the boundary's value (0, or on a torus the wrapped column by one
//     ds_bpermute), so nothing crosses between two fields.  One lane per field: no
//     lane move at all.
//   * Dead border: rows >= h are never written and stay 0 (row h is the dead row
//     below the field; for h = R a constant 0), columns >= w are masked after the
//     rule for every rule that can give birth.  Torus: row h - 1 (kept in `last`) is
//     the row above row 0, the old row 0 (`top`) the row below row h - 1, column
//     w - 1 arrives as the carry left of column 0, and column 0 is copied to the
//     ghost column w of the ingested row (w % 64 != 0) or arrives as the carry right
//     of column w - 1 (w % 64 == 0).  h is uniform, so every row test is a scalar one.
//   * The four forms of the pass (boundary x one lane or several per field) are
//     chosen by a uniform branch at the kernel's top: one kernel per (R, rule kind).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "life_internal.h"

namespace gol {

// Wavefronts per workgroup of the batch kernel.
constexpr int kBatchWaves = 4;
// rows_in_regs with an instantiated kernel
constexpr int kBatchRowsList[] = {8, 16, 32, 64};

// The batch buffer's internal order: the word of (wavefront v, row r, lane l) at
// (v * h + r) * 64 + l, column-split; field f = v * fields_per_wave + l / lanes_per_field,
// word q = l % lanes_per_field of its row.  A wavefront's loads and stores of one row
// are 512 contiguous bytes.
struct BatchArgs {
    uint64_t* buf;
    int64_t waves;       // wavefronts of the launch = ceil(n / fields_per_wave)
    int64_t n;           // fields
    int32_t h, w;
    int32_t wq;          // words per field row = ceil(w / 64)
    int32_t lpf_shift;   // lanes_per_field = 1 << lpf_shift
    int32_t gens;        // generations of this launch
    int32_t torus;
    uint32_t birth, survive;
    uint64_t lastmask;   // stored-form valid bits of word wq - 1
};

__host__ __device__ inline int64_t batch_word_index(int64_t f, int32_t r, int32_t q, int32_t h,
                                                    int32_t lpf_shift)
{
    const int64_t v = f >> (6 - lpf_shift);
    const int64_t l = ((f & ((64 >> lpf_shift) - 1)) << lpf_shift) + q;
    return (v * h + r) * 64 + l;
}

// `rows` in kBatchRowsList, >= a.h.
hipError_t launch_batch(const BatchArgs& a, int rows, RuleKind rule, hipStream_t s);
// Per-R entry point (explicitly instantiated in life_batch_r<R>.hip).
template <int R>
hipError_t launch_batch_rows(const BatchArgs& a, RuleKind rule, hipStream_t s);

// Codec kernels (life_batch_aux.hip) between the internal order and the canonical
// [n][h][words] order of gol_batch_load_packed: fields [first, first + count), word q
// of row r of field first + i at words[i * fs + r * rs + q] (device memory).  Bits at
// columns >= w are ignored on load and written 0 on store; `lastmask` here is the
// canonical mask of word wq - 1.
struct BatchGeom {
    uint64_t* buf;
    int64_t n;
    int32_t h, wq, lpf_shift;
    uint64_t lastmask;
};
hipError_t launch_batch_load(const BatchGeom& g, int64_t first, int64_t count,
                             const uint64_t* words, int64_t fs, int64_t rs, hipStream_t s);
hipError_t launch_batch_store(const BatchGeom& g, int64_t first, int64_t count, uint64_t* words,
                              int64_t fs, int64_t rs, hipStream_t s);
// field i = gol_init_random's field of seed + i
hipError_t launch_batch_init_random(const BatchGeom& g, uint64_t seed, hipStream_t s);
// out[2 i], out[2 i + 1] = gol_digest's live count and hash of field first + i
hipError_t launch_batch_digest(const BatchGeom& g, int64_t first, int64_t count, uint64_t* out,
                               hipStream_t s);

}  // namespace gol

#ifdef GOL_BATCH_DEVICE
#include "life_rule_lane.h"
#include "life_stencil.h"

namespace gol {

namespace {

// What a lane knows about its place in its field (set once per launch).  The per-lane
// choices are bit masks, not conditions: a lane move under a condition would be
// compiled into a branch on EXEC, and a DPP move reads 0 from a lane that EXEC has
// switched off.
struct BatchLane {
    uint32_t cm[2];      // valid columns of the lane's word, per plane; 0 in a lane without one
    uint32_t inner_l;    // all ones unless the lane holds the field's word 0
    uint32_t inner_r;    // all ones unless the lane holds the field's word wq - 1
    int partner;         // torus, several lanes: byte address of the lane at the other end
    // torus: column w - 1 is a bit of plane 0 or 1 (send_hi: all ones in the last lane if
    // plane 1) of word wq - 1 and goes to bit 31 of the carry by << lshl (uniform); the
    // ghost column w is the bit gm[k] of plane k in the last lane (0 elsewhere, and
    // where w % 64 == 0: then column 0 is the right carry, wfull all ones)
    uint32_t send_hi, lshl;
    uint32_t gm[2];
    uint32_t wfull;
};

constexpr uint32_t kSelect = 0xCA;  // a ? b : c, bit by bit

// The horizontal end columns of row x (life_stencil.h `ends`) for a field of the
// batch; on a torus also sets the ghost column of x.
template <bool TORUS, bool MULTI>
__device__ __forceinline__ Ends batch_ends(Pl<2>& x, const BatchLane& b)
{
    uint32_t hp, ln;  // bit 31: the column left of the word; bit 0: the column right of it
    if constexpr (!TORUS) {
        if constexpr (MULTI) {
            hp = lane_from_left(x.v[1]) & b.inner_l;
            ln = lane_from_right(x.v[0]) & b.inner_r;
        } else {
            hp = ln = 0u;
        }
    } else {
        // from_last: the plane with column w - 1, as the first lane sees it;
        // from_first: plane 0 of word 0 (bit 0 = column 0), as the last lane sees it
        const uint32_t send = lop3<kSelect>(b.send_hi, x.v[1], x.v[0]);
        uint32_t from_last, from_first;
        if constexpr (MULTI) {
            from_last = from_first = (uint32_t)__builtin_amdgcn_ds_bpermute(b.partner, (int)send);
        } else {
            from_last = send;
            from_first = x.v[0];
        }
        const uint32_t wl = from_last << b.lshl;
        const uint32_t wr = from_first & b.wfull;
        if constexpr (MULTI) {
            hp = lop3<kSelect>(b.inner_l, lane_from_left(x.v[1]), wl);
            ln = lop3<kSelect>(b.inner_r, lane_from_right(x.v[0]), wr);
        } else {
            hp = wl;
            ln = wr;
        }
        const uint32_t c0 = 0u - (from_first & 1u);  // column 0 on every bit
        x.v[0] |= c0 & b.gm[0];
        x.v[1] |= c0 & b.gm[1];
    }
    Ends e;
    e.l0 = __builtin_amdgcn_alignbit(x.v[1], hp, 31);
    e.rn = __builtin_amdgcn_alignbit(ln, x.v[0], 1);
    return e;
}

// One generation of the R rows in x.  `last`: row h - 1 (torus only; kept up to date).
// Every step sits under a scalar test of its own, t <= h.  Where a step taken and a
// step left out join, the stage's registers have to agree, which costs 8 v_mov per
// step; what was tried against that, each compiled for 64 rows:
//   * tests that leave the pass at the first step beyond h (nested tests; a break
//     out of the unrolled loop): 256 VGPRs and scratch;
//   * a straight-line pass for h = R beside this one: 256 VGPRs and more, 1 wave per
//     SIMD, with or without a scheduling fence between the steps;
//   * groups of 8 steps under one test: 205 VGPRs and scratch.
// birth, survive: the launch's masks (uniform), under RULE_LANE the lane's own.
template <int R, int RULE, bool TORUS, bool MULTI>
__device__ __forceinline__ void batch_pass(Pl<2> (&x)[R], Pl<2>& last, int32_t h,
                                           const BatchLane& b, uint32_t birth, uint32_t survive)
{
    // columns >= w: nothing is born there under B/S2 on a dead border; the torus's
    // ghost column is a live cell like any other
    constexpr bool kMask = RULE != RULE_REF || TORUS;
    // (h opaque per pass: else every row test is hoisted out of the generation loop
    // into an SGPR pair of its own, 2 R of them, which spill into VGPR lanes)
    asm volatile("" : "+s"(h));
    StageT<2> st = {};
    // prime the stage: H3 of row -1 (dead, or row h - 1) and of row 0
    if constexpr (TORUS) {
        Pl<2> up = last;
        const Ends e = batch_ends<TORUS, MULTI>(up, b);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint32_t L = left_of(up, e, k), Rn = right_of(up, e, k);
            st.cs.v[k] = lop3<kXor3>(L, up.v[k], Rn);
            st.cc.v[k] = lop3<kMaj>(L, up.v[k], Rn);
        }
    }
    const Pl<2> top = x[0];
    {
        Pl<2> r0 = x[0];
        const Ends e = batch_ends<TORUS, MULTI>(r0, b);
        st.ps = st.cs;
        st.pc = st.cc;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint32_t L = left_of(r0, e, k), Rn = right_of(r0, e, k);
            st.cs.v[k] = lop3<kXor3>(L, r0.v[k], Rn);
            st.cc.v[k] = lop3<kMaj>(L, r0.v[k], Rn);
        }
        st.al = r0;
    }
    // step t ingests row t (row h: the dead row, or the old row 0) and emits row t - 1;
    // odd steps reduce the pair (H3(t - 1), H3(t)), even ones reuse it
#pragma unroll
    for (int t = 1; t <= R; ++t) {
        if (t <= h) {
            Pl<2> in;
            if (t < R) {
                in = x[t];  // (dead border: row h is 0, it is never written)
            } else {
                in.v[0] = in.v[1] = 0u;
            }
            if constexpr (TORUS) {
                if (t == h) in = top;
            }
            const Ends e = batch_ends<TORUS, MULTI>(in, b);
            Pl<2> y;
            if constexpr (RULE == RULE_LANE)
                y = stage_step_lane<2>(st, in, e, birth, survive);
            else
                y = stage_step_ends<RULE, 2>(st, in, e, birth, survive, (t & 1) == 1);
            if constexpr (kMask) {
                y.v[0] &= b.cm[0];
                y.v[1] &= b.cm[1];
            }
            x[t - 1] = y;
            if constexpr (TORUS) {
                if (t == h) last = y;
            }
        }
    }
}

// RULE_LANE: the masks a lane steps by, from the word of its field in the table
// (birth | survive << 16), read once per launch.  All lanes of a field read the same
// word; lanes without a word of a field < n (padding lanes, fields >= n) read nothing
// and take the empty rule.
struct LaneRule {
    uint32_t birth, survive;
};
__device__ __forceinline__ LaneRule batch_lane_rule(const uint32_t* rules, int64_t f, bool live)
{
    uint32_t word = 0u;
    if (live) word = rules[f];
    return LaneRule{word & 0x1FFu, (word >> 16) & 0x1FFu};
}

// (life_batch_until.h's batch_until_run, life_batch_trace.h's batch_trace_run and
// life_batch_record.h's batch_record_run repeat the lane setup and the row load below line
// for line, so that this kernel compiles as it did: change all four together)
// `rules`: RULE_LANE's table (life_batch_rules.h), unused by every other rule kind.
template <int R, int RULE, bool TORUS, bool MULTI>
__device__ __forceinline__ void batch_run(const BatchArgs& a, int64_t wave, int lane,
                                          const uint32_t* rules = nullptr)
{
    const int32_t h = a.h;
    const int lpf = 1 << a.lpf_shift;
    const int q = lane & (lpf - 1);
    const int64_t f = (wave << (6 - a.lpf_shift)) + (lane >> a.lpf_shift);
    const bool live = q < a.wq && f < a.n;
    LaneRule rule = {};
    if constexpr (RULE == RULE_LANE) rule = batch_lane_rule(rules, f, live);
    BatchLane b;
    const bool first = q == 0, last_lane = q == a.wq - 1;
    b.inner_l = first ? 0u : ~0u;
    b.inner_r = last_lane ? 0u : ~0u;
    const uint64_t m = live ? (last_lane ? a.lastmask : ~0ull) : 0ull;
    b.cm[0] = (uint32_t)m;
    b.cm[1] = (uint32_t)(m >> 32);
    b.partner = 4 * (first ? lane + a.wq - 1 : last_lane ? lane - (a.wq - 1) : lane);
    const uint32_t cl = (uint32_t)(a.w - 1) & 63u, cg = (uint32_t)a.w & 63u;
    b.send_hi = (last_lane && (cl & 1u)) ? ~0u : 0u;
    b.lshl = 31u - (cl >> 1);
    b.wfull = cg == 0u ? ~0u : 0u;
    b.gm[0] = (last_lane && cg != 0u && !(cg & 1u)) ? 1u << (cg >> 1) : 0u;
    b.gm[1] = (last_lane && (cg & 1u)) ? 1u << (cg >> 1) : 0u;
    // (opaque from here on, so that no mask is turned back into the condition it came from)
    asm volatile("" : "+v"(b.inner_l), "+v"(b.inner_r), "+v"(b.send_hi));

    uint64_t* base = a.buf + wave * (int64_t)h * 64 + lane;
    Pl<2> x[R];
    Pl<2> last = {};
#pragma unroll
    for (int r = 0; r < R; ++r) {
        x[r].v[0] = x[r].v[1] = 0u;
        if (r < h) {
            const uint64_t g = base[(int64_t)r * 64];
            x[r].v[0] = (uint32_t)g & b.cm[0];
            x[r].v[1] = (uint32_t)(g >> 32) & b.cm[1];
        }
    }
    if constexpr (TORUS) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r == h - 1) last = x[r];
    }
    // (the uniform kinds name a.birth and a.survive here and nowhere earlier: read into a
    // local at the top, the 8- and 16-row kernels no longer compiled as they did)
#pragma nounroll
    for (int32_t g = 0; g < a.gens; ++g)
        batch_pass<R, RULE, TORUS, MULTI>(x, last, h, b,
                                          RULE == RULE_LANE ? rule.birth : a.birth,
                                          RULE == RULE_LANE ? rule.survive : a.survive);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r < h) {
            if (live) base[(int64_t)r * 64] = ((uint64_t)x[r].v[1] << 32) | x[r].v[0];
        }
    }
}

}  // namespace

template <int R, int RULE>
__global__ __launch_bounds__(64 * kBatchWaves) void life_batch_kernel(BatchArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave =
        (int64_t)blockIdx.x * kBatchWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave >= a.waves) return;
    if (a.lpf_shift == 0) {
        if (a.torus)
            batch_run<R, RULE, true, false>(a, wave, lane);
        else
            batch_run<R, RULE, false, false>(a, wave, lane);
    } else {
        if (a.torus)
            batch_run<R, RULE, true, true>(a, wave, lane);
        else
            batch_run<R, RULE, false, true>(a, wave, lane);
    }
}

template <int R>
hipError_t launch_batch_rows(const BatchArgs& a, RuleKind rule, hipStream_t s)
{
    if (a.waves <= 0 || a.gens <= 0) return hipSuccess;
    if (a.h < 1 || a.h > R) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.waves + kBatchWaves - 1) / kBatchWaves)), block(64 * kBatchWaves);
    switch (rule) {
    case RULE_REF: hipLaunchKernelGGL((life_batch_kernel<R, RULE_REF>), grid, block, 0, s, a); break;
    case RULE_CONWAY:
        hipLaunchKernelGGL((life_batch_kernel<R, RULE_CONWAY>), grid, block, 0, s, a);
        break;
    default: hipLaunchKernelGGL((life_batch_kernel<R, RULE_GENERIC>), grid, block, 0, s, a); break;
    }
    return hipGetLastError();
}

#define GOL_INSTANTIATE_BATCH(R) \
    template hipError_t launch_batch_rows<R>(const BatchArgs&, RuleKind, hipStream_t);

}  // namespace gol
#endif  // GOL_BATCH_DEVICE
