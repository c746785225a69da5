// life_batch_trace.h -- the batch kernel that samples every field's population while it
// steps (gol_batch_step_trace, batch.cpp; DESIGN §4 "life_batch_trace_kernel").
//
// The first part is the interface between batch.cpp and the kernels.  The second part,
// behind GOL_BATCH_DEVICE, is the kernel: life_batch.h's pass (batch_pass) inside its lane
// setup and row load / store, with the generation loop cut into intervals of `every`
// passes, included by one translation unit per register-row count
// (life_batch_trace_r<R>.hip), all four rule kinds in each.  life_batch_kernel and
// life_batch_until_kernel are not touched and share no code path with this kernel beyond
// batch_pass and batch_lane_rule.
//
// One launch covers `intervals` whole sample intervals and then `tail` generations (the
// last launch only).  After interval k every field's live cells go to
// trace[(s0 + k) * stride + f]: between two generations a lane holds its word of the
// field for all rows in registers, so a sample is one popcount per row and plane, a sum
// over the field's adjacent lanes and one 4-byte store by the field's first lane.  The
// fields themselves touch memory at the launch's loads and stores only.
// The generation loop has one call site of the pass, as life_batch_until.h's has and for
// its reason: a second inlined 64-row pass would not share the instruction cache.
#pragma once
#include "life_batch.h"

namespace gol {

// an interval is at most this long (gol_batch_step_until_periodic's bound on check_every)
constexpr uint32_t kBatchTraceMaxEvery = 65536;

struct BatchTraceArgs {
    BatchArgs a;         // (gens unused)
    uint32_t* trace;     // sample s of field f at trace[s * stride + f] (device memory)
    uint64_t stride;     // >= a.n
    uint64_t s0;         // the launch's first sample
    uint32_t every;      // generations per interval
    uint32_t intervals;  // whole intervals of this launch, a sample after each
    uint32_t tail;       // generations after them, not sampled (the last launch only)
    uint32_t pad;
};
// RULE_LANE: rules[f] = birth | survive << 16 of field f, as life_batch_rules.h's table
struct BatchTraceRuleArgs {
    BatchTraceArgs t;  // (a.birth, a.survive unused)
    const uint32_t* rules;
};

// `rows` in kBatchRowsList, >= t.a.h.
hipError_t launch_batch_trace(const BatchTraceArgs& t, int rows, RuleKind rule, hipStream_t s);
hipError_t launch_batch_trace_rules(const BatchTraceRuleArgs& rt, int rows, hipStream_t s);
template <int R>
hipError_t launch_batch_trace_rows(const BatchTraceArgs& t, RuleKind rule, hipStream_t s);
template <int R>
hipError_t launch_batch_trace_rules_rows(const BatchTraceRuleArgs& rt, hipStream_t s);

}  // namespace gol

#ifdef GOL_BATCH_DEVICE

namespace gol {

namespace {

// The live cells of the lane's word over all rows.  No mask: x holds valid columns only.
// Rows are masked by cm at the load, every row a pass writes is masked by cm after the
// rule (kMask; B/S2 on a dead border gives no birth at columns >= w), and the torus's
// ghost column w is set in the copy of a row that the stage ingests, never in x.  Lanes
// without a word of a field < n hold zeros (cm = 0) and add nothing.
template <int R>
__device__ __forceinline__ uint32_t batch_trace_count(const Pl<2> (&x)[R], int32_t h)
{
    // (h opaque per sample, as batch_pass makes it per pass, so that no row test is hoisted
    // out of the interval loop into an SGPR pair of its own)
    asm volatile("" : "+s"(h));
    uint32_t c = 0u;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r < h) {
            c += (uint32_t)__builtin_popcount(x[r].v[0]);
            c += (uint32_t)__builtin_popcount(x[r].v[1]);
        }
    }
    return c;
}

// One sample: the field's count, summed over its lanes_per_field adjacent lanes by a
// butterfly of lpf_shift ds_bpermute steps (every lane of the field ends with the total;
// all 64 lanes are active, and each step sits under a uniform test, never a per-lane
// one), stored by the field's first lane.  The lane's place is worked out anew from the
// opaque lane number, as batch_until_place does, so that none of it stays in registers
// across the passes.
template <int R, bool MULTI>
__device__ __forceinline__ void batch_trace_sample(const BatchTraceArgs& t, const Pl<2> (&x)[R],
                                                   int64_t wave, int lane, uint32_t k)
{
    const BatchArgs& a = t.a;
    asm volatile("" : "+v"(lane));
    uint32_t c = batch_trace_count<R>(x, a.h);
    if constexpr (MULTI) {
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            if (j < a.lpf_shift)
                c += (uint32_t)__builtin_amdgcn_ds_bpermute(4 * (lane ^ (1 << j)), (int)c);
        }
    }
    const int q = lane & ((1 << a.lpf_shift) - 1);
    const int64_t f = (wave << (6 - a.lpf_shift)) + (lane >> a.lpf_shift);
    if (q == 0 && f < a.n) t.trace[(t.s0 + k) * t.stride + (uint64_t)f] = c;
}

template <int R, int RULE, bool TORUS, bool MULTI>
__device__ __forceinline__ void batch_trace_run(const BatchTraceArgs& t, int64_t wave, int lane,
                                                const uint32_t* rules = nullptr)
{
    const BatchArgs& a = t.a;
    // (lane setup and row load: batch_run's, line for line; life_batch_record.h's
    // batch_record_run repeats them and the interval loop below: change all four together)
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
    // the counter at the loop's top: selected after the sample instead, `every` and `tail`
    // were kept in VGPRs across the passes and the 64-row kernels spilled)
    for (uint32_t k = 0;; ++k) {
        const uint32_t togo = k < t.intervals ? t.every : t.tail;
#pragma nounroll
        for (uint32_t i = 0; i < togo; ++i)
            batch_pass<R, RULE, TORUS, MULTI>(x, last, h, b,
                                              RULE == RULE_LANE ? rule.birth : a.birth,
                                              RULE == RULE_LANE ? rule.survive : a.survive);
        if (k >= t.intervals) break;
        batch_trace_sample<R, MULTI>(t, x, wave, lane, k);
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
__global__ __launch_bounds__(64 * kBatchWaves) void life_batch_trace_kernel(BatchTraceArgs t)
{
    static_assert(RULE != RULE_LANE, "the rule table travels in BatchTraceRuleArgs");
    const int lane = threadIdx.x & 63;
    const int64_t wave =
        (int64_t)blockIdx.x * kBatchWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave >= t.a.waves) return;
    if (t.a.lpf_shift == 0) {
        if (t.a.torus)
            batch_trace_run<R, RULE, true, false>(t, wave, lane);
        else
            batch_trace_run<R, RULE, false, false>(t, wave, lane);
    } else {
        if (t.a.torus)
            batch_trace_run<R, RULE, true, true>(t, wave, lane);
        else
            batch_trace_run<R, RULE, false, true>(t, wave, lane);
    }
}

// life_batch_trace_kernel<R, RULE_LANE>: the overload that takes the rule table.
template <int R, int RULE>
__global__ __launch_bounds__(64 * kBatchWaves) void life_batch_trace_kernel(BatchTraceRuleArgs rt)
{
    static_assert(RULE == RULE_LANE, "the rule table is RULE_LANE's");
    const int lane = threadIdx.x & 63;
    const int64_t wave =
        (int64_t)blockIdx.x * kBatchWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave >= rt.t.a.waves) return;
    if (rt.t.a.lpf_shift == 0) {
        if (rt.t.a.torus)
            batch_trace_run<R, RULE, true, false>(rt.t, wave, lane, rt.rules);
        else
            batch_trace_run<R, RULE, false, false>(rt.t, wave, lane, rt.rules);
    } else {
        if (rt.t.a.torus)
            batch_trace_run<R, RULE, true, true>(rt.t, wave, lane, rt.rules);
        else
            batch_trace_run<R, RULE, false, true>(rt.t, wave, lane, rt.rules);
    }
}

// What both launchers check: a sample's address stays inside [s0, s0 + intervals) x stride.
template <int R>
inline bool batch_trace_args_ok(const BatchTraceArgs& t)
{
    if (t.a.h < 1 || t.a.h > R) return false;
    if (t.every < 1 || t.every > kBatchTraceMaxEvery || t.tail >= t.every) return false;
    if (t.intervals && (!t.trace || t.stride < (uint64_t)t.a.n)) return false;
    return true;
}

template <int R>
hipError_t launch_batch_trace_rows(const BatchTraceArgs& t, RuleKind rule, hipStream_t s)
{
    if (t.a.waves <= 0 || (t.intervals == 0 && t.tail == 0)) return hipSuccess;
    if (!batch_trace_args_ok<R>(t)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((t.a.waves + kBatchWaves - 1) / kBatchWaves)), block(64 * kBatchWaves);
    switch (rule) {
    case RULE_REF:
        hipLaunchKernelGGL((life_batch_trace_kernel<R, RULE_REF>), grid, block, 0, s, t);
        break;
    case RULE_CONWAY:
        hipLaunchKernelGGL((life_batch_trace_kernel<R, RULE_CONWAY>), grid, block, 0, s, t);
        break;
    default:
        hipLaunchKernelGGL((life_batch_trace_kernel<R, RULE_GENERIC>), grid, block, 0, s, t);
        break;
    }
    return hipGetLastError();
}

template <int R>
hipError_t launch_batch_trace_rules_rows(const BatchTraceRuleArgs& rt, hipStream_t s)
{
    const BatchTraceArgs& t = rt.t;
    if (t.a.waves <= 0 || (t.intervals == 0 && t.tail == 0)) return hipSuccess;
    if (!batch_trace_args_ok<R>(t) || !rt.rules) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((t.a.waves + kBatchWaves - 1) / kBatchWaves)), block(64 * kBatchWaves);
    life_batch_trace_kernel<R, RULE_LANE><<<grid, block, 0, s>>>(rt);
    return hipGetLastError();
}

#define GOL_INSTANTIATE_BATCH_TRACE(R)                                                          \
    template hipError_t launch_batch_trace_rows<R>(const BatchTraceArgs&, RuleKind, hipStream_t); \
    template hipError_t launch_batch_trace_rules_rows<R>(const BatchTraceRuleArgs&, hipStream_t);

}  // namespace gol
#endif  // GOL_BATCH_DEVICE
