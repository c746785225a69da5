// life_batch_until.h -- the batch kernel with per-field period detection
// (gol_batch_step_until_periodic, batch.cpp; DESIGN §4 "life_batch_until_kernel").
//
// The first part is the interface between batch.cpp and the kernels.  The second part,
// behind GOL_BATCH_DEVICE, is the kernel: life_batch.h's pass (batch_pass) and lane
// setup around a schedule of snapshots and compares, included by one translation unit
// per register-row count (life_batch_until_r<R>.hip).  life_batch_kernel itself is not
// touched and shares no code path with this kernel beyond batch_pass.
//
// One launch covers `intervals` whole check intervals of C = check_every generations,
// each starting at a multiple of C (counted from the call), for lag L <= C:
//   run C - L generations; store the rows to the snapshot buffer; for each proper
//   divisor d of L, ascending: run on to snapshot + d and compare (the first d that is
//   equal is the lane's candidate); run on to snapshot + L and compare: the check.  A
//   field that is equal there and not yet found gets period = the candidate (or L) and
//   generation = the check's generation.
// A wavefront whose fields are all found runs (max_generations - g) mod L generations
// more, which is generation max_generations for every one of them (all their periods
// divide L), stores, sets its done word and leaves for good.  The snapshot and the
// candidates never cross a launch boundary.
// The generation loop has one call site of the pass, one of the compare and one of the
// snapshot store, around a uniform phase variable: five inlined copies of a 64-row pass
// would not share the instruction cache with anything.
#pragma once
#include "life_batch.h"

namespace gol {

// at most this many proper divisors for a lag <= kBatchUntilMaxLag (840 has 31)
constexpr int kBatchUntilDivisors = 32;
constexpr uint32_t kBatchUntilMaxLag = 1024;

// Device counters of one gol_batch_step_until_periodic call.
struct BatchUntilCounters {
    unsigned long long wave_generations;  // generations computed, summed over wavefronts
    uint32_t pending;                     // wavefronts that have not left for good
    uint32_t pad;
};

struct BatchUntilArgs {
    BatchArgs a;             // (gens unused)
    uint64_t* snap;          // as large as a.buf, the same order
    uint32_t* period;        // [n], 0 = not found yet
    uint64_t* generation;    // [n]
    uint32_t* done;          // [waves]
    BatchUntilCounters* ctr;
    uint64_t g0;             // generation at the launch's start, a multiple of check_every
    uint64_t max_g;
    uint32_t lag, check_every;
    uint32_t intervals;      // whole check intervals of this launch
    uint32_t tail;           // generations after them (the last launch only)
    uint32_t ndiv;
    uint32_t div[kBatchUntilDivisors];  // proper divisors of lag, ascending
};

// `rows` in kBatchRowsList, >= u.a.h.
hipError_t launch_batch_until(const BatchUntilArgs& u, int rows, RuleKind rule, hipStream_t s);
template <int R>
hipError_t launch_batch_until_rows(const BatchUntilArgs& u, RuleKind rule, hipStream_t s);

}  // namespace gol

#ifdef GOL_BATCH_DEVICE

namespace gol {

namespace {

// OR of x ^ snapshot over the lane's rows.  sbase comes from batch_until_place, opaque
// per event: else every row's address is hoisted out of the generation loop into a VGPR
// pair of its own, 2 R of them.
template <int R>
__device__ __forceinline__ uint32_t batch_until_diff(const Pl<2> (&x)[R], const uint64_t* sbase,
                                                     int32_t h, bool live)
{
    uint32_t d = 0u;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r < h) {
            if (live) {
                const uint64_t s = sbase[(int64_t)r * 64];
                d |= (x[r].v[0] ^ (uint32_t)s) | (x[r].v[1] ^ (uint32_t)(s >> 32));
            }
        }
    }
    return d;
}

// A lane's place for the schedule's events, worked out anew from the lane number at
// each of them (opaque, so that none of it stays in registers across the passes).
struct BatchUntilPlace {
    int64_t f;       // the lane's field
    bool head;       // the field's first lane, of a field < n
    bool live;       // as batch_run's
    uint64_t fmask;  // the ballot bits of the lane's field
    int64_t off;     // the lane's word of row 0 in buf and snap
};

__device__ __forceinline__ BatchUntilPlace batch_until_place(const BatchArgs& a, int64_t wave,
                                                             int lane)
{
    asm volatile("" : "+v"(lane));
    const int lpf = 1 << a.lpf_shift;
    const int q = lane & (lpf - 1);
    BatchUntilPlace p;
    p.f = (wave << (6 - a.lpf_shift)) + (lane >> a.lpf_shift);
    p.head = q == 0 && p.f < a.n;
    p.live = q < a.wq && p.f < a.n;
    p.fmask = (lpf == 64 ? ~0ull : (1ull << lpf) - 1ull) << (lane & ~(lpf - 1));
    p.off = wave * (int64_t)a.h * 64 + lane;
    return p;
}

template <int R, int RULE, bool TORUS, bool MULTI>
__device__ __forceinline__ void batch_until_run(const BatchUntilArgs& u, int64_t wave, int lane,
                                                const uint32_t* rules = nullptr)
{
    const BatchArgs& a = u.a;
    // (lane setup: batch_run's, line for line, as in life_batch_trace.h and
    // life_batch_record.h: change all four together)
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

    const uint64_t* base = a.buf + wave * (int64_t)h * 64 + lane;
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

    // found: the lane's field has its result (a lane of a field >= n counts as found)
    bool found = true;
    if (f < a.n) found = u.period[f] != 0u;
    uint32_t cand = 0u;

    enum { kSnap, kDiv, kCheck, kEnd };
    const uint32_t L = u.lag, C = u.check_every;
    uint64_t g = u.g0;
    unsigned long long computed = 0;
    uint32_t iv = 0, k = 0, prev = 0;
    bool left = false;
    int phase = kSnap;
    uint32_t togo = C - L;
    if (u.intervals == 0) {
        phase = kEnd;
        togo = u.tail;
    }
    for (;;) {
#pragma nounroll
        for (uint32_t i = 0; i < togo; ++i)
            batch_pass<R, RULE, TORUS, MULTI>(x, last, h, b,
                                              RULE == RULE_LANE ? rule.birth : a.birth,
                                              RULE == RULE_LANE ? rule.survive : a.survive);
        computed += togo;
        if (phase == kEnd) break;
        const BatchUntilPlace p = batch_until_place(a, wave, lane);
        if (phase == kSnap) {
            uint64_t* sp = u.snap + p.off;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (r < h) {
                    if (p.live) sp[(int64_t)r * 64] = ((uint64_t)x[r].v[1] << 32) | x[r].v[0];
                }
            }
            cand = 0u;
            k = 0;
            prev = 0;
        } else {
            const uint32_t d = batch_until_diff<R>(x, u.snap + p.off, h, p.live);
            const bool eq = (__ballot(d != 0u) & p.fmask) == 0ull;
            if (phase == kDiv) {
                if (eq && cand == 0u) cand = prev;
            } else {
                g += C;
                if (eq && !found) {
                    if (p.head) {
                        u.period[p.f] = cand ? cand : L;
                        u.generation[p.f] = g;
                    }
                    found = true;
                }
                ++iv;
                if (__ballot(!found) == 0ull) {
                    left = true;
                    phase = kEnd;
                    togo = (uint32_t)((u.max_g - g) % L);
                } else if (iv == u.intervals) {
                    phase = kEnd;
                    togo = u.tail;
                } else {
                    phase = kSnap;
                    togo = C - L;
                }
                continue;
            }
        }
        if (k < u.ndiv) {
            const uint32_t d = u.div[k++];
            togo = d - prev;
            prev = d;
            phase = kDiv;
        } else {
            togo = L - prev;
            prev = L;
            phase = kCheck;
        }
    }
    const BatchUntilPlace p = batch_until_place(a, wave, lane);
    uint64_t* out = a.buf + p.off;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r < h) {
            if (p.live) out[(int64_t)r * 64] = ((uint64_t)x[r].v[1] << 32) | x[r].v[0];
        }
    }
    if (lane == 0) {
        if (left) {
            u.done[wave] = 1u;
            atomicSub(&u.ctr->pending, 1u);
        }
        atomicAdd(&u.ctr->wave_generations, computed);
    }
}

}  // namespace

template <int R, int RULE>
__global__ __launch_bounds__(64 * kBatchWaves) void life_batch_until_kernel(BatchUntilArgs u)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave =
        (int64_t)blockIdx.x * kBatchWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave >= u.a.waves) return;
    if (__builtin_amdgcn_readfirstlane(u.done[wave])) return;
    if (u.a.lpf_shift == 0) {
        if (u.a.torus)
            batch_until_run<R, RULE, true, false>(u, wave, lane);
        else
            batch_until_run<R, RULE, false, false>(u, wave, lane);
    } else {
        if (u.a.torus)
            batch_until_run<R, RULE, true, true>(u, wave, lane);
        else
            batch_until_run<R, RULE, false, true>(u, wave, lane);
    }
}

template <int R>
hipError_t launch_batch_until_rows(const BatchUntilArgs& u, RuleKind rule, hipStream_t s)
{
    if (u.a.waves <= 0) return hipSuccess;
    if (u.a.h < 1 || u.a.h > R) return hipErrorInvalidValue;
    if (u.lag < 1 || u.lag > kBatchUntilMaxLag || u.check_every < u.lag ||
        u.ndiv > (uint32_t)kBatchUntilDivisors)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((u.a.waves + kBatchWaves - 1) / kBatchWaves)), block(64 * kBatchWaves);
    switch (rule) {
    case RULE_REF:
        hipLaunchKernelGGL((life_batch_until_kernel<R, RULE_REF>), grid, block, 0, s, u);
        break;
    case RULE_CONWAY:
        hipLaunchKernelGGL((life_batch_until_kernel<R, RULE_CONWAY>), grid, block, 0, s, u);
        break;
    default:
        hipLaunchKernelGGL((life_batch_until_kernel<R, RULE_GENERIC>), grid, block, 0, s, u);
        break;
    }
    return hipGetLastError();
}

#define GOL_INSTANTIATE_BATCH_UNTIL(R) \
    template hipError_t launch_batch_until_rows<R>(const BatchUntilArgs&, RuleKind, hipStream_t);

}  // namespace gol
#endif  // GOL_BATCH_DEVICE
