// life_copy.hip -- the copy pass (DESIGN §4 "Copy pass"): the rows of the calm
// units of a stencil launch, moved from the launch's input buffer to its output
// buffer by a kernel of its own instead of the copy loop inside life_tb_kernel.
// That loop inherits the stencil kernel's shape (240 VGPRs, 2 wavefronts per SIMD,
// one wavefront walking a unit's several hundred rows alone, 496-byte row pieces
// that share 128-byte lines with the next strip); this kernel holds a few dozen
// registers and no LDS, so it runs at full occupancy, gives every few rows to a
// wavefront of their own, walks the field band by band, and writes whole lines.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "life_internal.h"

namespace gol {

namespace {

constexpr int kStillStepThreads = 1024;  // life_still_step_kernel's one workgroup

// calm(U) as life_tb_kernel's prologue evaluates it: every streak_in of U's
// neighbour list is >= 1, and an empty list is not calm (uniform); *still: every
// one of them is >= 2, the condition on which a depth-K launch skips U.
__device__ __forceinline__ bool unit_calm(const CopyArgs& a, uint32_t unit, int lane, bool* still)
{
    const uint32_t o0 = a.nb_off[unit], o1 = a.nb_off[unit + 1];
    bool calm = o1 > o0, st2 = o1 > o0;
    for (uint32_t j = o0; j < o1; j += 64) {
        const uint32_t i = j + (uint32_t)lane;
        const uint32_t st = i < o1 ? a.streak_in[a.nb_ids[i]] : 2u;
        calm = calm && __builtin_amdgcn_ballot_w64(st < 1u) == 0;
        st2 = st2 && __builtin_amdgcn_ballot_w64(st < 2u) == 0;
    }
    *still = st2;
    return calm;
}

// The pass's first kernel: one wavefront per unit writes need[unit] (1 or 0), so
// that a tile's wavefront learns about its owners with two loads, not with a walk
// of their lists: on a field in motion, where every tile leaves after that test,
// the pass is bound by this chain of loads and nothing else.
// Copy elision (DESIGN §4 "Copy pass"): need = calm and the destination does not hold
// the unit's rows yet.  It holds them (a.elided set) when the unit probed through
// in the step's first launch and this pass goes before the second (a.held: dst was
// that launch's input, which the probe proved equal to its output on the unit),
// when the unit is still (it was calm in the launch before, whose input buffer is
// dst and whose output it left equal to it), or in every calm unit of the second
// and later launches of one remainder (a.all_held).  Only this kernel writes
// elided[], one lane per unit.
__global__ __launch_bounds__(256) void life_calm_kernel(CopyArgs a)
{
    const int lane = threadIdx.x & 63;
    const uint32_t unit =
        blockIdx.x * (uint32_t)kWavesPerBlock + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (unit >= (uint32_t)a.total_units) return;
    bool still;
    const bool calm = unit_calm(a, unit, lane, &still);
    if (lane == 0) {
        // Rows both buffers hold: before a step's last launch.  A calm unit's
        // output rows equal its input rows, however they get there, and the launch's
        // input buffer is the other one once the step has ended.  A unit that computes
        // gets 0, quiet or not.  twin_val: 2 before a remainder launch, whose calm units
        // are still one generation on as well (DESIGN §4 "Sure tiles"), else 1.
        if (a.twin) {
            a.twin[unit] = calm ? (a.twin_val == 2u ? 2u : 1u) : 0u;
            if (unit == 0) *a.twin_ok = 1u;
        }
        if (!a.need) return;
        const bool holds =
            a.elided && (a.all_held || still || (a.held && a.held[unit] != 0u));
        a.need[unit] = (calm && !holds) ? 1u : 0u;
        if (calm && holds) a.elided[unit] += 1u;
    }
}

// twin[] after a step whose only launch probed: a unit that took the still
// probe's quiet exit left its output rows equal to its input rows (copy elision's
// case P reads the same flag for the same reason); every other unit computed.
__global__ __launch_bounds__(256) void life_twin_held_kernel(const uint32_t* held, uint32_t* twin,
                                                             uint32_t* twin_ok, int32_t units)
{
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u >= (uint32_t)units) return;
    twin[u] = held[u] != 0u ? 1u : 0u;
    if (u == 0) *twin_ok = 1u;
}

// The short step's one node (DESIGN §4 "Short step"): stands for `count` depth-K launches
// from index first_idx on, each of which would take the one-load exit
// (life_stencil.h: busy[1] < launch_idx, none of them writes busy[1]) and add 1 to
// busy[0].  The same test; where it fails the replacement is not exact, the launches
// left out should have computed, and the next gol_sync reports it.
__global__ __launch_bounds__(64) void life_still_span_kernel(uint32_t* busy, int* err,
                                                             uint32_t first_idx, uint32_t count)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    if (busy[1] < first_idx)
        busy[0] += count;
    else
        *err = kErrShortStep;
}

// The fixed step (DESIGN §4 "Fixed step"): one workgroup, strided over the units, in
// place of every kernel of a step that starts on a proven fixed point.  Phase 1 is the
// proof itself, as gol_sync makes it on the host (step.cpp sync_observing): twin_ok
// set and a 2 in every unit's word.  Phase 2, behind the barrier that reduces phase 1,
// adds the step's increments and stores its final values, none of which depends on what
// a word held (step.cpp still_effect derives them from the kernels).  Where the proof
// fails one lane stores kErrShortStep and nothing else is written.  Plain vector loads
// and stores by one workgroup: no atomics, no scratch, no field word touched.
// Every index is below min(total_units, act_units), the length of every region.
__global__ __launch_bounds__(kStillStepThreads) void life_still_step_kernel(StillArgs a)
{
    if (blockIdx.x != 0) return;
    const uint32_t n = a.total_units;
    int ok = n > 0 && n <= a.act_units && *a.twin_ok != 0u;
    if (n <= a.act_units)
        for (uint32_t u = threadIdx.x; u < n; u += kStillStepThreads) ok = ok && a.twin[u] == 2u;
    if (!__syncthreads_and(ok)) {
        if (threadIdx.x == 0) *a.err = kErrShortStep;
        return;
    }
    for (uint32_t u = threadIdx.x; u < n; u += kStillStepThreads) {
        a.act[2 * u] += a.computed;
        a.act[2 * u + 1] += a.skipped;
        a.copied[u] += a.n_copied;
        a.probed[u] += a.n_probed;
        a.pass_probed[u] += a.n_pass_probed;
        a.elided[u] += a.n_elided;
        a.streak0[u] = a.v_streak0;
        a.streak1[u] = a.v_streak1;
        a.need[u] = a.v_need;
        a.held[u] = a.v_held;
        a.moved[u] = a.v_moved;
        a.twin[u] = a.v_twin;
    }
    if (threadIdx.x == 0) {
        a.busy[0] += a.busy0_add;
        a.busy[1] = a.busy1;
        *a.twin_ok = a.v_twin_ok;
    }
}

// One wavefront per tile of kCopyTileRows rows x kCopyTileWords words, lane l = word
// l of the tile's column segment, consecutive tiles along a row chunk.  The tile is
// copied when one of its owners has `need`, whole: the words of its other owners too.
// Writing the words of a calm unit whose rows dst holds stores equal values; writing
// the words of a unit that is not calm is safe because the pass runs only
// before launches none of whose units skips (engine.cpp launch checks it): such a
// unit stores every word of its rectangle after the pass, on the same stream, from
// the input buffer, which nobody writes.  A tile none of whose owners has `need` is left
// alone, so a field in motion costs the tiles' tests and no traffic.  The words
// stored are the ones the stencil kernel's put_row(row_in()) stores: the last group
// masked, rows outside [vlo, vhi) zero.  Loads and stores are non-temporal: each
// word is touched once, and 2 x 537 MB at 65536^2 would only sweep the caches.  The
// pass writes field words, its own need flags and the elided counters, no other
// counter and no streak.
// Every index is checked against the tables' and the plan's bounds before any access.
__global__ __launch_bounds__(256) void life_copy_kernel(CopyArgs a)
{
    const int lane = threadIdx.x & 63;
    const uint32_t tile =
        blockIdx.x * (uint32_t)kWavesPerBlock + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (tile >= (uint32_t)a.ntile) return;
    const uint32_t chunk = tile / (uint32_t)a.ncol, seg = tile - chunk * (uint32_t)a.ncol;
    const int32_t rb = a.out_lo + (int32_t)chunk * kCopyTileRows;
    const int32_t n = min(rb + kCopyTileRows, a.out_hi) - rb;
    if (rb < 0 || n <= 0) return;
    {
        uint32_t c = 0;
        if (lane < kCopyOwners) {
            const uint32_t unit = a.owners[(size_t)tile * kCopyOwners + lane];
            if (unit < (uint32_t)a.total_units) c = a.need[unit];
        }
        if (__builtin_amdgcn_ballot_w64(c != 0u) == 0) return;
    }
    const int32_t q = (int32_t)seg * kCopyTileWords + lane;
    if (q >= a.ng) return;
    const uint64_t cm = q == a.ng - 1 ? a.lastmask : ~0ull;
    const int64_t off = (a.base_row + rb) * a.stride + q;
    const uint64_t* src = a.src + off;
    uint64_t* dst = a.dst + off;
    uint64_t g[kCopyTileRows];
#pragma unroll
    for (int j = 0; j < kCopyTileRows; ++j)
        g[j] = __builtin_nontemporal_load(src + (int64_t)min(j, n - 1) * a.stride);
#pragma unroll
    for (int j = 0; j < kCopyTileRows; ++j) {
        const bool ok = rb + j >= a.vlo && rb + j < a.vhi;
        if (j < n) __builtin_nontemporal_store(ok ? (g[j] & cm) : 0ull, dst + (int64_t)j * a.stride);
    }
}

}  // namespace

hipError_t launch_copy_pass(const CopyArgs& a, hipStream_t s)
{
    if (a.ntile <= 0 || a.ncol <= 0 || a.total_units <= 0) return hipSuccess;
    const unsigned ublocks = ((unsigned)a.total_units + kWavesPerBlock - 1) / kWavesPerBlock;
    hipLaunchKernelGGL(life_calm_kernel, dim3(ublocks), dim3(64 * kWavesPerBlock), 0, s, a);
    if (a.all_held && a.elided) return hipGetLastError();
    const unsigned blocks = ((unsigned)a.ntile + kWavesPerBlock - 1) / kWavesPerBlock;
    hipLaunchKernelGGL(life_copy_kernel, dim3(blocks), dim3(64 * kWavesPerBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_twin_held(const uint32_t* held, uint32_t* twin, uint32_t* twin_ok, int32_t units,
                            hipStream_t s)
{
    if (units <= 0 || !held || !twin || !twin_ok) return hipErrorInvalidValue;
    hipLaunchKernelGGL(life_twin_held_kernel, dim3(((unsigned)units + 255) / 256), dim3(256), 0, s,
                       held, twin, twin_ok, units);
    return hipGetLastError();
}

hipError_t launch_still_span(uint32_t* busy, int* err, uint32_t first_idx, uint32_t count,
                             hipStream_t s)
{
    if (!busy || !err || count == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(life_still_span_kernel, dim3(1), dim3(64), 0, s, busy, err, first_idx, count);
    return hipGetLastError();
}

hipError_t launch_still_step(const StillArgs& a, hipStream_t s)
{
    if (!a.streak0 || !a.streak1 || !a.act || !a.copied || !a.busy || !a.probed || !a.need ||
        !a.held || !a.elided || !a.moved || !a.pass_probed || !a.twin || !a.twin_ok || !a.err ||
        a.total_units == 0 || a.total_units > a.act_units)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(life_still_step_kernel, dim3(1), dim3(kStillStepThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_twin_flags(const CopyArgs& a, hipStream_t s)
{
    if (a.total_units <= 0 || !a.twin || !a.twin_ok || a.need || a.elided) return hipErrorInvalidValue;
    const unsigned ublocks = ((unsigned)a.total_units + kWavesPerBlock - 1) / kWavesPerBlock;
    hipLaunchKernelGGL(life_calm_kernel, dim3(ublocks), dim3(64 * kWavesPerBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace gol
