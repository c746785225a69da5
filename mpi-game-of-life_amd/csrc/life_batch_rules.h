// life_batch_rules.h -- the batch kernels with a rule per field (gol_batch_set_rules,
// batch.cpp; DESIGN §4 "Per-field rules").
//
// The first part is the interface between batch.cpp and the kernels.  The second part,
// behind GOL_BATCH_DEVICE, is the RULE_LANE instantiation of life_batch.h's batch_run and
// of life_batch_until.h's batch_until_run, included by one translation unit per
// register-row count (life_batch_rules_r<R>.hip).  Lane setup, pass and check schedule are
// those two functions; what differs is where a lane's masks come from (batch_lane_rule:
// the field's word of the rule table) and the rule network of the pass
// (life_rule_lane.h).  The table pointer travels in argument structs that only these
// kernels take, so BatchArgs, BatchUntilArgs and the kernels of the uniform rules stay
// exactly as they are.
#pragma once
#include "life_batch.h"
#include "life_batch_until.h"

namespace gol {

// rules[f] = birth | survive << 16 of field f, [a.n] words
struct BatchRuleArgs {
    BatchArgs a;  // (birth, survive unused)
    const uint32_t* rules;
};
struct BatchUntilRuleArgs {
    BatchUntilArgs u;
    const uint32_t* rules;
};

// `rows` in kBatchRowsList, >= a.h.
hipError_t launch_batch_rules(const BatchRuleArgs& ra, int rows, hipStream_t s);
hipError_t launch_batch_until_rules(const BatchUntilRuleArgs& ru, int rows, hipStream_t s);
template <int R>
hipError_t launch_batch_rules_rows(const BatchRuleArgs& ra, hipStream_t s);
template <int R>
hipError_t launch_batch_until_rules_rows(const BatchUntilRuleArgs& ru, hipStream_t s);

}  // namespace gol

#ifdef GOL_BATCH_DEVICE

namespace gol {

// life_batch_kernel<R, RULE_LANE>: the overload that takes the rule table.
template <int R, int RULE>
__global__ __launch_bounds__(64 * kBatchWaves) void life_batch_kernel(BatchRuleArgs ra)
{
    static_assert(RULE == RULE_LANE, "the rule table is RULE_LANE's");
    const int lane = threadIdx.x & 63;
    const int64_t wave =
        (int64_t)blockIdx.x * kBatchWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave >= ra.a.waves) return;
    if (ra.a.lpf_shift == 0) {
        if (ra.a.torus)
            batch_run<R, RULE, true, false>(ra.a, wave, lane, ra.rules);
        else
            batch_run<R, RULE, false, false>(ra.a, wave, lane, ra.rules);
    } else {
        if (ra.a.torus)
            batch_run<R, RULE, true, true>(ra.a, wave, lane, ra.rules);
        else
            batch_run<R, RULE, false, true>(ra.a, wave, lane, ra.rules);
    }
}

// life_batch_until_kernel<R, RULE_LANE>, likewise.
template <int R, int RULE>
__global__ __launch_bounds__(64 * kBatchWaves) void life_batch_until_kernel(BatchUntilRuleArgs ru)
{
    static_assert(RULE == RULE_LANE, "the rule table is RULE_LANE's");
    const int lane = threadIdx.x & 63;
    const int64_t wave =
        (int64_t)blockIdx.x * kBatchWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave >= ru.u.a.waves) return;
    if (__builtin_amdgcn_readfirstlane(ru.u.done[wave])) return;
    if (ru.u.a.lpf_shift == 0) {
        if (ru.u.a.torus)
            batch_until_run<R, RULE, true, false>(ru.u, wave, lane, ru.rules);
        else
            batch_until_run<R, RULE, false, false>(ru.u, wave, lane, ru.rules);
    } else {
        if (ru.u.a.torus)
            batch_until_run<R, RULE, true, true>(ru.u, wave, lane, ru.rules);
        else
            batch_until_run<R, RULE, false, true>(ru.u, wave, lane, ru.rules);
    }
}

template <int R>
hipError_t launch_batch_rules_rows(const BatchRuleArgs& ra, hipStream_t s)
{
    if (ra.a.waves <= 0 || ra.a.gens <= 0) return hipSuccess;
    if (ra.a.h < 1 || ra.a.h > R || !ra.rules) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((ra.a.waves + kBatchWaves - 1) / kBatchWaves)),
        block(64 * kBatchWaves);
    life_batch_kernel<R, RULE_LANE><<<grid, block, 0, s>>>(ra);
    return hipGetLastError();
}

template <int R>
hipError_t launch_batch_until_rules_rows(const BatchUntilRuleArgs& ru, hipStream_t s)
{
    const BatchUntilArgs& u = ru.u;
    if (u.a.waves <= 0) return hipSuccess;
    if (u.a.h < 1 || u.a.h > R || !ru.rules) return hipErrorInvalidValue;
    if (u.lag < 1 || u.lag > kBatchUntilMaxLag || u.check_every < u.lag ||
        u.ndiv > (uint32_t)kBatchUntilDivisors)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((u.a.waves + kBatchWaves - 1) / kBatchWaves)), block(64 * kBatchWaves);
    life_batch_until_kernel<R, RULE_LANE><<<grid, block, 0, s>>>(ru);
    return hipGetLastError();
}

#define GOL_INSTANTIATE_BATCH_RULES(R)                                                        \
    template hipError_t launch_batch_rules_rows<R>(const BatchRuleArgs&, hipStream_t);        \
    template hipError_t launch_batch_until_rules_rows<R>(const BatchUntilRuleArgs&, hipStream_t);

}  // namespace gol
#endif  // GOL_BATCH_DEVICE
