// life_batch_record.h -- the batch kernel that writes sampled field states while it steps
// (gol_batch_step_record, batch.cpp; DESIGN §4 "life_batch_record_kernel").
//
// The first part is the interface between batch.cpp and the kernels.  The second part,
// behind GOL_BATCH_DEVICE, is the kernel: life_batch.h's pass (batch_pass) inside its lane
// setup and row load / store, with the generation loop cut into intervals of `every`
// passes exactly as life_batch_trace.h cuts it, included by one translation unit per
// register-row count (life_batch_record_r<R>.hip), all four rule kinds in each.  The other
// batch kernels are not touched and share no code path with this kernel beyond batch_pass
// and batch_lane_rule.
//
// One launch covers `intervals` whole sample intervals and then `tail` generations (the
// last launch only).  After interval k the fields of the window [first, first + count) go
// to frames[(s0 + k) * ss + (f - first) * fs + r * rs + q] in the canonical layout of
// gol_batch_store_packed: between two generations a lane holds its word of the field for
// all rows in registers, so a sample is one gol_join64 and one 8-byte store per row by every
// lane that holds a word of a field of the window.  The fields themselves touch memory at
// the launch's loads and stores only; no codec pass and no reload.
// The generation loop has one call site of the pass, as life_batch_trace.h's has and for
// its reason.
#pragma once
#include "life_batch.h"

namespace gol {

// an interval is at most this long (life_batch_trace.h's kBatchTraceMaxEvery)
constexpr uint32_t kBatchRecordMaxEvery = 65536;

struct BatchRecordArgs {
    BatchArgs a;         // (gens unused)
    uint64_t* frames;    // device memory; see above
    uint64_t ss, fs, rs; // sample, field and row stride in words
    uint64_t s0;         // the launch's first sample
    int64_t first;       // the window: fields [first, first + count), inside [0, a.n)
    int64_t count;
    uint32_t every;      // generations per interval
    uint32_t intervals;  // whole intervals of this launch, a sample after each
    uint32_t tail;       // generations after them, not recorded (the last launch only)
    uint32_t pad;
};
// RULE_LANE: rules[f] = birth | survive << 16 of field f, as life_batch_rules.h's table
struct BatchRecordRuleArgs {
    BatchRecordArgs t;  // (a.birth, a.survive unused)
    const uint32_t* rules;
};

// `rows` in kBatchRowsList, >= t.a.h.
hipError_t launch_batch_record(const BatchRecordArgs& t, int rows, RuleKind rule, hipStream_t s);
hipError_t launch_batch_record_rules(const BatchRecordRuleArgs& rt, int rows, hipStream_t s);
template <int R>
hipError_t launch_batch_record_rows(const BatchRecordArgs& t, RuleKind rule, hipStream_t s);
template <int R>
hipError_t launch_batch_record_rules_rows(const BatchRecordRuleArgs& rt, hipStream_t s);

}  // namespace gol

#ifdef GOL_BATCH_DEVICE
#include "bitlayout.h"

namespace gol {

namespace {

// One sample: every lane that holds word q < wq of a field f of the window stores the
// canonical form of its word of each row r < h.  No mask: x holds valid columns only
// (life_batch_trace.h's batch_trace_count tells why), so bits at columns >= w are 0 as
// gol_batch_store_packed writes them.  A wavefront none of whose fields lies in the window
// leaves under a scalar test.  The lane's place, its field and the address are worked out
// anew from the opaque lane number, as batch_trace_sample does, so that none of it stays in
// registers across the passes; h is opaque per sample for batch_trace_count's reason.  The
// stores are plain vector stores: with one lane per field a row's store instruction writes
// 64 pieces of 8 bytes, fs words apart, and a lane fills its own h rows one after another.
template <int R>
__device__ __forceinline__ void batch_record_sample(const BatchRecordArgs& t, const Pl<2> (&x)[R],
                                                    int64_t wave, int lane, uint32_t k)
{
    const BatchArgs& a = t.a;
    const int64_t f0 = wave << (6 - a.lpf_shift), end = t.first + t.count;
    if (f0 >= end || f0 + (64 >> a.lpf_shift) <= t.first) return;
    asm volatile("" : "+v"(lane));
    int32_t h = a.h;
    asm volatile("" : "+s"(h));
    const int q = lane & ((1 << a.lpf_shift) - 1);
    const int64_t f = f0 + (lane >> a.lpf_shift);
    if (q < a.wq && f >= t.first && f < end) {
        uint64_t* p = t.frames + (t.s0 + k) * t.ss + (uint64_t)(f - t.first) * t.fs + (uint64_t)q;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (r < h) p[(uint64_t)r * t.rs] = gol_join64(((uint64_t)x[r].v[1] << 32) | x[r].v[0]);
        }
    }
}

// (lane setup, row load, interval loop and row store: batch_trace_run's, line for line, which
// are batch_run's; change all four together)
template <int R, int RULE, bool TORUS, bool MULTI>
__device__ __forceinline__ void batch_record_run(const BatchRecordArgs& t, int64_t wave, int lane,
                                                 const uint32_t* rules = nullptr)
{
    const BatchArgs& a = t.a;
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

    // intervals of `every` passes with a sample after each, then the tail.  (togo comes from
    // the counter at the loop's top, as in batch_trace_run, so that it stays scalar)
    for (uint32_t k = 0;; ++k) {
        const uint32_t togo = k < t.intervals ? t.every : t.tail;
#pragma nounroll
        for (uint32_t i = 0; i < togo; ++i)
            batch_pass<R, RULE, TORUS, MULTI>(x, last, h, b,
                                              RULE == RULE_LANE ? rule.birth : a.birth,
                                              RULE == RULE_LANE ? rule.survive : a.survive);
        if (k >= t.intervals) break;
        batch_record_sample<R>(t, x, wave, lane, k);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r < h) {
            if (live) base[(int64_t)r * 64] = ((uint64_t)x[r].v[1] << 32) | x[r].v[0];
        }
    }
}

}  // namespace

template <int R, int RULE>
__global__ __launch_bounds__(64 * kBatchWaves) void life_batch_record_kernel(BatchRecordArgs t)
{
    static_assert(RULE != RULE_LANE, "the rule table travels in BatchRecordRuleArgs");
    const int lane = threadIdx.x & 63;
    const int64_t wave =
        (int64_t)blockIdx.x * kBatchWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave >= t.a.waves) return;
    if (t.a.lpf_shift == 0) {
        if (t.a.torus)
            batch_record_run<R, RULE, true, false>(t, wave, lane);
        else
            batch_record_run<R, RULE, false, false>(t, wave, lane);
    } else {
        if (t.a.torus)
            batch_record_run<R, RULE, true, true>(t, wave, lane);
        else
            batch_record_run<R, RULE, false, true>(t, wave, lane);
    }
}

// life_batch_record_kernel<R, RULE_LANE>: the overload that takes the rule table.
template <int R, int RULE>
__global__ __launch_bounds__(64 * kBatchWaves) void life_batch_record_kernel(BatchRecordRuleArgs rt)
{
    static_assert(RULE == RULE_LANE, "the rule table is RULE_LANE's");
    const int lane = threadIdx.x & 63;
    const int64_t wave =
        (int64_t)blockIdx.x * kBatchWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave >= rt.t.a.waves) return;
    if (rt.t.a.lpf_shift == 0) {
        if (rt.t.a.torus)
            batch_record_run<R, RULE, true, false>(rt.t, wave, lane, rt.rules);
        else
            batch_record_run<R, RULE, false, false>(rt.t, wave, lane, rt.rules);
    } else {
        if (rt.t.a.torus)
            batch_record_run<R, RULE, true, true>(rt.t, wave, lane, rt.rules);
        else
            batch_record_run<R, RULE, false, true>(rt.t, wave, lane, rt.rules);
    }
}

// What both launchers check: the window lies inside the batch, and a sample's words stay
// inside [s0, s0 + intervals) x ss (batch.cpp's record_check bounds the whole buffer).
template <int R>
inline bool batch_record_args_ok(const BatchRecordArgs& t)
{
    if (t.a.h < 1 || t.a.h > R) return false;
    if (t.every < 1 || t.every > kBatchRecordMaxEvery || t.tail >= t.every) return false;
    if (t.first < 0 || t.count < 0 || t.first > t.a.n || t.count > t.a.n - t.first) return false;
    if (t.intervals && t.count) {
        if (!t.frames || t.rs < (uint64_t)t.a.wq) return false;
        if (t.fs / (uint64_t)t.a.h < t.rs || t.ss / (uint64_t)t.count < t.fs) return false;
    }
    return true;
}

template <int R>
hipError_t launch_batch_record_rows(const BatchRecordArgs& t, RuleKind rule, hipStream_t s)
{
    if (t.a.waves <= 0 || (t.intervals == 0 && t.tail == 0)) return hipSuccess;
    if (!batch_record_args_ok<R>(t)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((t.a.waves + kBatchWaves - 1) / kBatchWaves)), block(64 * kBatchWaves);
    switch (rule) {
    case RULE_REF:
        hipLaunchKernelGGL((life_batch_record_kernel<R, RULE_REF>), grid, block, 0, s, t);
        break;
    case RULE_CONWAY:
        hipLaunchKernelGGL((life_batch_record_kernel<R, RULE_CONWAY>), grid, block, 0, s, t);
        break;
    default:
        hipLaunchKernelGGL((life_batch_record_kernel<R, RULE_GENERIC>), grid, block, 0, s, t);
        break;
    }
    return hipGetLastError();
}

template <int R>
hipError_t launch_batch_record_rules_rows(const BatchRecordRuleArgs& rt, hipStream_t s)
{
    const BatchRecordArgs& t = rt.t;
    if (t.a.waves <= 0 || (t.intervals == 0 && t.tail == 0)) return hipSuccess;
    if (!batch_record_args_ok<R>(t) || !rt.rules) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((t.a.waves + kBatchWaves - 1) / kBatchWaves)), block(64 * kBatchWaves);
    life_batch_record_kernel<R, RULE_LANE><<<grid, block, 0, s>>>(rt);
    return hipGetLastError();
}

#define GOL_INSTANTIATE_BATCH_RECORD(R)                                                           \
    template hipError_t launch_batch_record_rows<R>(const BatchRecordArgs&, RuleKind, hipStream_t); \
    template hipError_t launch_batch_record_rules_rows<R>(const BatchRecordRuleArgs&, hipStream_t);

}  // namespace gol
#endif  // GOL_BATCH_DEVICE
