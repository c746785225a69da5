// life_batch_aux.hip -- the batch kernels' dispatch over rows_in_regs and the
// memory-bound codec kernels between the batch buffer's internal order and the
// canonical [n][h][words] order (load, store, random init, digest); see life_batch.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bitlayout.h"
#include "life_batch.h"
#include "life_batch_until.h"
#include "life_batch_rules.h"
#include "life_batch_trace.h"
#include "life_batch_record.h"

namespace gol {

extern template hipError_t launch_batch_rows<8>(const BatchArgs&, RuleKind, hipStream_t);
extern template hipError_t launch_batch_rows<16>(const BatchArgs&, RuleKind, hipStream_t);
extern template hipError_t launch_batch_rows<32>(const BatchArgs&, RuleKind, hipStream_t);
extern template hipError_t launch_batch_rows<64>(const BatchArgs&, RuleKind, hipStream_t);

hipError_t launch_batch(const BatchArgs& a, int rows, RuleKind rule, hipStream_t s)
{
    switch (rows) {
    case 8: return launch_batch_rows<8>(a, rule, s);
    case 16: return launch_batch_rows<16>(a, rule, s);
    case 32: return launch_batch_rows<32>(a, rule, s);
    case 64: return launch_batch_rows<64>(a, rule, s);
    default: return hipErrorInvalidValue;
    }
}

extern template hipError_t launch_batch_until_rows<8>(const BatchUntilArgs&, RuleKind, hipStream_t);
extern template hipError_t launch_batch_until_rows<16>(const BatchUntilArgs&, RuleKind, hipStream_t);
extern template hipError_t launch_batch_until_rows<32>(const BatchUntilArgs&, RuleKind, hipStream_t);
extern template hipError_t launch_batch_until_rows<64>(const BatchUntilArgs&, RuleKind, hipStream_t);

hipError_t launch_batch_until(const BatchUntilArgs& u, int rows, RuleKind rule, hipStream_t s)
{
    switch (rows) {
    case 8: return launch_batch_until_rows<8>(u, rule, s);
    case 16: return launch_batch_until_rows<16>(u, rule, s);
    case 32: return launch_batch_until_rows<32>(u, rule, s);
    case 64: return launch_batch_until_rows<64>(u, rule, s);
    default: return hipErrorInvalidValue;
    }
}

extern template hipError_t launch_batch_rules_rows<8>(const BatchRuleArgs&, hipStream_t);
extern template hipError_t launch_batch_rules_rows<16>(const BatchRuleArgs&, hipStream_t);
extern template hipError_t launch_batch_rules_rows<32>(const BatchRuleArgs&, hipStream_t);
extern template hipError_t launch_batch_rules_rows<64>(const BatchRuleArgs&, hipStream_t);

hipError_t launch_batch_rules(const BatchRuleArgs& ra, int rows, hipStream_t s)
{
    switch (rows) {
    case 8: return launch_batch_rules_rows<8>(ra, s);
    case 16: return launch_batch_rules_rows<16>(ra, s);
    case 32: return launch_batch_rules_rows<32>(ra, s);
    case 64: return launch_batch_rules_rows<64>(ra, s);
    default: return hipErrorInvalidValue;
    }
}

extern template hipError_t launch_batch_until_rules_rows<8>(const BatchUntilRuleArgs&, hipStream_t);
extern template hipError_t launch_batch_until_rules_rows<16>(const BatchUntilRuleArgs&, hipStream_t);
extern template hipError_t launch_batch_until_rules_rows<32>(const BatchUntilRuleArgs&, hipStream_t);
extern template hipError_t launch_batch_until_rules_rows<64>(const BatchUntilRuleArgs&, hipStream_t);

hipError_t launch_batch_until_rules(const BatchUntilRuleArgs& ru, int rows, hipStream_t s)
{
    switch (rows) {
    case 8: return launch_batch_until_rules_rows<8>(ru, s);
    case 16: return launch_batch_until_rules_rows<16>(ru, s);
    case 32: return launch_batch_until_rules_rows<32>(ru, s);
    case 64: return launch_batch_until_rules_rows<64>(ru, s);
    default: return hipErrorInvalidValue;
    }
}

extern template hipError_t launch_batch_trace_rows<8>(const BatchTraceArgs&, RuleKind, hipStream_t);
extern template hipError_t launch_batch_trace_rows<16>(const BatchTraceArgs&, RuleKind, hipStream_t);
extern template hipError_t launch_batch_trace_rows<32>(const BatchTraceArgs&, RuleKind, hipStream_t);
extern template hipError_t launch_batch_trace_rows<64>(const BatchTraceArgs&, RuleKind, hipStream_t);

hipError_t launch_batch_trace(const BatchTraceArgs& t, int rows, RuleKind rule, hipStream_t s)
{
    switch (rows) {
    case 8: return launch_batch_trace_rows<8>(t, rule, s);
    case 16: return launch_batch_trace_rows<16>(t, rule, s);
    case 32: return launch_batch_trace_rows<32>(t, rule, s);
    case 64: return launch_batch_trace_rows<64>(t, rule, s);
    default: return hipErrorInvalidValue;
    }
}

extern template hipError_t launch_batch_trace_rules_rows<8>(const BatchTraceRuleArgs&, hipStream_t);
extern template hipError_t launch_batch_trace_rules_rows<16>(const BatchTraceRuleArgs&, hipStream_t);
extern template hipError_t launch_batch_trace_rules_rows<32>(const BatchTraceRuleArgs&, hipStream_t);
extern template hipError_t launch_batch_trace_rules_rows<64>(const BatchTraceRuleArgs&, hipStream_t);

hipError_t launch_batch_trace_rules(const BatchTraceRuleArgs& rt, int rows, hipStream_t s)
{
    switch (rows) {
    case 8: return launch_batch_trace_rules_rows<8>(rt, s);
    case 16: return launch_batch_trace_rules_rows<16>(rt, s);
    case 32: return launch_batch_trace_rules_rows<32>(rt, s);
    case 64: return launch_batch_trace_rules_rows<64>(rt, s);
    default: return hipErrorInvalidValue;
    }
}

extern template hipError_t launch_batch_record_rows<8>(const BatchRecordArgs&, RuleKind, hipStream_t);
extern template hipError_t launch_batch_record_rows<16>(const BatchRecordArgs&, RuleKind, hipStream_t);
extern template hipError_t launch_batch_record_rows<32>(const BatchRecordArgs&, RuleKind, hipStream_t);
extern template hipError_t launch_batch_record_rows<64>(const BatchRecordArgs&, RuleKind, hipStream_t);

hipError_t launch_batch_record(const BatchRecordArgs& t, int rows, RuleKind rule, hipStream_t s)
{
    switch (rows) {
    case 8: return launch_batch_record_rows<8>(t, rule, s);
    case 16: return launch_batch_record_rows<16>(t, rule, s);
    case 32: return launch_batch_record_rows<32>(t, rule, s);
    case 64: return launch_batch_record_rows<64>(t, rule, s);
    default: return hipErrorInvalidValue;
    }
}

extern template hipError_t launch_batch_record_rules_rows<8>(const BatchRecordRuleArgs&, hipStream_t);
extern template hipError_t launch_batch_record_rules_rows<16>(const BatchRecordRuleArgs&, hipStream_t);
extern template hipError_t launch_batch_record_rules_rows<32>(const BatchRecordRuleArgs&, hipStream_t);
extern template hipError_t launch_batch_record_rules_rows<64>(const BatchRecordRuleArgs&, hipStream_t);

hipError_t launch_batch_record_rules(const BatchRecordRuleArgs& rt, int rows, hipStream_t s)
{
    switch (rows) {
    case 8: return launch_batch_record_rules_rows<8>(rt, s);
    case 16: return launch_batch_record_rules_rows<16>(rt, s);
    case 32: return launch_batch_record_rules_rows<32>(rt, s);
    case 64: return launch_batch_record_rules_rows<64>(rt, s);
    default: return hipErrorInvalidValue;
    }
}

namespace {

// (as life_aux.hip: the synthetic field and the digest are defined on the canonical
// word index r * wq + q of a field, gol.h)
__device__ __forceinline__ uint64_t splitmix64_at(uint64_t seed, uint64_t idx)
{
    uint64_t z = seed + (idx + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// One thread per canonical word of fields [first, first + count).
__global__ __launch_bounds__(256) void batch_load_kernel(BatchGeom g, int64_t first, int64_t count,
                                                         const uint64_t* words, int64_t fs,
                                                         int64_t rs)
{
    const int64_t per = (int64_t)g.h * g.wq, total = count * per;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total;
         k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = k / per, j = k - i * per;
        const int32_t r = (int32_t)(j / g.wq), q = (int32_t)(j - (int64_t)r * g.wq);
        uint64_t c = words[i * fs + (int64_t)r * rs + q];
        if (q == g.wq - 1) c &= g.lastmask;
        g.buf[batch_word_index(first + i, r, q, g.h, g.lpf_shift)] = gol_split64(c);
    }
}

__global__ __launch_bounds__(256) void batch_store_kernel(BatchGeom g, int64_t first,
                                                          int64_t count, uint64_t* words,
                                                          int64_t fs, int64_t rs)
{
    const int64_t per = (int64_t)g.h * g.wq, total = count * per;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total;
         k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = k / per, j = k - i * per;
        const int32_t r = (int32_t)(j / g.wq), q = (int32_t)(j - (int64_t)r * g.wq);
        uint64_t c = gol_join64(g.buf[batch_word_index(first + i, r, q, g.h, g.lpf_shift)]);
        if (q == g.wq - 1) c &= g.lastmask;
        words[i * fs + (int64_t)r * rs + q] = c;
    }
}

// One thread per canonical word of the whole batch.
__global__ __launch_bounds__(256) void batch_init_random_kernel(BatchGeom g, uint64_t seed)
{
    const int64_t per = (int64_t)g.h * g.wq, total = g.n * per;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total;
         k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = k / per, j = k - i * per;
        const int32_t r = (int32_t)(j / g.wq), q = (int32_t)(j - (int64_t)r * g.wq);
        uint64_t c = splitmix64_at(seed + (uint64_t)i, (uint64_t)j);
        if (q == g.wq - 1) c &= g.lastmask;
        g.buf[batch_word_index(i, r, q, g.h, g.lpf_shift)] = gol_split64(c);
    }
}

// One wavefront per field: its lanes share the field's words, add up with shuffles,
// and lane 0 stores the field's two sums.
__global__ __launch_bounds__(256) void batch_digest_kernel(BatchGeom g, int64_t first,
                                                           int64_t count, uint64_t* out)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int32_t per = g.h * g.wq;
    for (int64_t i = wave0; i < count; i += nwaves) {
        uint64_t live = 0, hash = 0;
        for (int32_t j = lane; j < per; j += 64) {
            const int32_t r = j / g.wq, q = j - r * g.wq;
            uint64_t c = gol_join64(g.buf[batch_word_index(first + i, r, q, g.h, g.lpf_shift)]);
            if (q == g.wq - 1) c &= g.lastmask;
            live += (uint64_t)__popcll(c);
            hash += splitmix64_at(c ^ splitmix64_at(0, (uint64_t)j), 0);
        }
        for (int off = 32; off > 0; off >>= 1) {
            live += __shfl_xor(live, off);
            hash += __shfl_xor(hash, off);
        }
        if (lane == 0) {
            out[2 * i] = live;
            out[2 * i + 1] = hash;
        }
    }
}

dim3 batch_grid(int64_t items, int64_t per_block, int64_t cap)
{
    int64_t blocks = (items + per_block - 1) / per_block;
    if (blocks > cap) blocks = cap;
    return dim3((unsigned)blocks);
}

}  // namespace

hipError_t launch_batch_load(const BatchGeom& g, int64_t first, int64_t count,
                             const uint64_t* words, int64_t fs, int64_t rs, hipStream_t s)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(batch_load_kernel, batch_grid(count * g.h * g.wq, 256, 8192), dim3(256), 0,
                       s, g, first, count, words, fs, rs);
    return hipGetLastError();
}

hipError_t launch_batch_store(const BatchGeom& g, int64_t first, int64_t count, uint64_t* words,
                              int64_t fs, int64_t rs, hipStream_t s)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(batch_store_kernel, batch_grid(count * g.h * g.wq, 256, 8192), dim3(256), 0,
                       s, g, first, count, words, fs, rs);
    return hipGetLastError();
}

hipError_t launch_batch_init_random(const BatchGeom& g, uint64_t seed, hipStream_t s)
{
    if (g.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(batch_init_random_kernel, batch_grid(g.n * g.h * g.wq, 256, 8192),
                       dim3(256), 0, s, g, seed);
    return hipGetLastError();
}

hipError_t launch_batch_digest(const BatchGeom& g, int64_t first, int64_t count, uint64_t* out,
                               hipStream_t s)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(batch_digest_kernel, batch_grid(count, 4, 8192), dim3(256), 0, s, g, first,
                       count, out);
    return hipGetLastError();
}

}  // namespace gol
