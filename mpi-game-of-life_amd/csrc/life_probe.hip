// life_probe.hip -- the probe pass (DESIGN §4 "Probe pass"): one generation over the
// field before a step's first stencil launch, in the copy pass's shape instead of the
// stencil kernel's (life_copy.hip says what that shape costs): one wavefront per
// line-aligned tile of kCopyTileRows rows x kCopyTileWords words, a few dozen
// registers, no LDS, row bands, whole lines written once.
//
// The pass is a conservative accelerator of the still probe inside life_tb_kernel,
// which stays the authority.  It leaves moved[U] = 0 only for a unit U that is sure:
// no tile that meets U's output rectangles dilated by K - 1 cells (the device table,
// plan.cpp build_tile_units) holds a field cell whose generation 1 differs from its
// input.  The in-kernel probe compares on a subset of those cells, so it would take
// a sure unit through; life_tb_kernel does that on the word alone.  Every tile that
// meets a sure unit's rectangles found no difference and did not leave early (the
// unit is listed for it and never marked), so it stored its rows, the unit's among
// them, in the form the probe's quiet exit stores.  Every other unit probes in the
// launch as it does without the pass and stores its whole rectangle afterwards.
//
// Rows both buffers hold: a tile without a difference leaves its
// stores out where the destination holds its rows already, which the last launch of
// the step before recorded per unit (ActState::twin, valid while twin_ok is set).
// "Stored its rows" above then reads "the destination holds its rows": the same
// content, so everything that follows from it stands.
//
// Sure tiles: where that last launch was a remainder launch, its calm units
// got twin = 2, and a tile all of whose owners have it keeps its state for one
// generation by proof.  It ends as the twin tile it would turn out to be, before its
// field loads, and counts in sure[tile] as well.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "life_stencil.h"

namespace gol {

namespace {

// moved[] = 0, on the stream directly before the tile kernel and captured with it.
__global__ __launch_bounds__(256) void life_probe_zero_kernel(uint32_t* moved, int32_t units)
{
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u < (uint32_t)units) moved[u] = 0u;
}

// Lane l = word l of the tile's column segment, consecutive tiles along a row chunk.
// Every index is checked against the table's and the plan's bounds before any access.
// (8 wavefronts per SIMD, the copy kernel's occupancy: at most 64 registers, 52 used.
// The generic rule's 10-term mask sum spills at 64 and at 80: it stays uncapped, 96
// registers, 5 wavefronts per SIMD, no scratch.)
template <int RULE>
__global__ __launch_bounds__(256, RULE == RULE_GENERIC ? 1 : 8) void life_probe_kernel(ProbeArgs a)
{
    constexpr int NP = 2;
    constexpr int R = kCopyTileRows;
    constexpr bool kBirths = RULE != RULE_REF;
    const int lane = threadIdx.x & 63;
    const uint32_t tile =
        blockIdx.x * (uint32_t)kWavesPerBlock + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (tile >= (uint32_t)a.ntile) return;
    const uint32_t chunk = tile / (uint32_t)a.ncol, seg = tile - chunk * (uint32_t)a.ncol;
    const int32_t rb = a.out_lo + (int32_t)chunk * R;
    const int32_t n = min(rb + R, a.out_hi) - rb;
    if (rb < 0 || n <= 0) return;
    // The listed units (one per lane below kProbeSlots).  All of them marked already:
    // the tile can change nothing, and each of them stores its rectangles itself in
    // the launch, so the tile's rows need no store either.  A stale 0 only means that
    // the tile does its work.  (An agent-scope load, served by L2, so that a word set
    // from another CU is seen.  On a soup at 65536^2 the exit still catches few tiles:
    // a unit's 55-77 row chunks are in flight together)
    uint32_t unit = ~0u;
    if (lane < kProbeSlots) unit = a.tiles[(size_t)tile * kProbeSlots + lane];
    const bool listed = unit < (uint32_t)a.total_units;
    // Rows both buffers hold: the tile's owners (one per lane below
    // kCopyOwners) and their words, loaded beside the listed units' so that the two
    // chains of two loads run together.  twin_tile: dst holds every row of the tile.
    // Such a tile does not take the exit below, so that whether it counts in kept[]
    // does not hang on the order in which other tiles mark its units; it is a tile of
    // still units beside units in motion, and the exit catches few tiles anyway.
    uint32_t owner = ~0u;
    if (a.twin && lane < kCopyOwners) owner = a.owners[(size_t)tile * kCopyOwners + lane];
    const bool owned = owner < (uint32_t)a.total_units;
    const uint32_t tw = owned ? a.twin[owner] : 1u;
    const uint32_t tw_ok = a.twin ? *a.twin_ok : 0u;
    const bool twin_tile = tw_ok != 0u && __builtin_amdgcn_ballot_w64(owned) != 0 &&
                           __builtin_amdgcn_ballot_w64(tw == 0u) == 0;
    // Sure tiles: every owner was calm in a remainder launch that ended the
    // step before, so generation 1 equals the input on every word of the tile: the
    // loads below would find diff == 0 and the tile would end as a twin tile.  It ends
    // so here, leaving moved[], kept[] and the field as that path leaves them.
    if (a.sure && twin_tile && __builtin_amdgcn_ballot_w64(owned && tw != 2u) == 0) {
        if (lane == 0) {
            a.kept[tile] += 1u;
            a.sure[tile] += 1u;
        }
        return;
    }
    {
        const uint32_t m = listed ? __hip_atomic_load(a.moved + unit, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT)
                                  : 1u;
        const bool any = __builtin_amdgcn_ballot_w64(listed) != 0;
        if (any && !twin_tile && __builtin_amdgcn_ballot_w64(m == 0u) == 0) return;
    }
    const int32_t q0 = (int32_t)seg * kCopyTileWords;
    const int32_t q = q0 + lane;
    const bool qin = q < a.ng;
    const uint64_t cmw = !qin ? 0ull : (q == a.ng - 1 ? a.lastmask : ~0ull);
    Pl<NP> cm;
    cm.v[0] = (uint32_t)cmw;
    cm.v[1] = (uint32_t)(cmw >> 32);
    // The columns beside the tile, which the wave shifts cannot supply: lane 0 reads
    // the upper half (plane 1, odd columns: bit 31 = column 63) of word q0 - 1, lane
    // 63 the lower half (plane 0: bit 0 = column 0) of word q0 + 64.
    const int32_t qe = lane == 0 ? q0 - 1 : q0 + kCopyTileWords;
    const bool edge = (lane == 0 || lane == 63) && qe >= 0 && qe < a.ng;
    const uint32_t em = !edge ? 0u
                        : lane == 0 ? ~0u
                                    : (uint32_t)(qe == a.ng - 1 ? a.lastmask : ~0ull);
    // rows rb - 1 .. rb + n; a row outside [vlo, vhi) is dead and its load goes to a
    // row inside (masked to 0), so nothing outside the field's rows is read
    const int32_t vmax = max(a.vhi - 1, a.vlo);
    const int64_t row0 = a.base_row * a.stride;
    const uint64_t* src = a.src + row0 + (qin ? q : q0);
    const uint32_t* esrc =
        reinterpret_cast<const uint32_t*>(a.src + row0 + (edge ? qe : q0)) + (lane == 0 ? 1 : 0);
    uint64_t g[R + 2];
    uint32_t ge[R + 2];
#pragma unroll
    for (int j = 0; j < R + 2; ++j) {
        const int32_t r = min(max(rb - 1 + min(j, n + 1), a.vlo), vmax);
        const int64_t off = (int64_t)r * a.stride;
        // the tile's own rows are touched once more at most (by the tile above or
        // below, as its halo); the halo rows and the edge columns are other tiles' own
        g[j] = (j >= 1 && j <= R) ? __builtin_nontemporal_load(src + off) : src[off];
        ge[j] = edge ? esrc[2 * off] : 0u;
    }
    StageT<NP> st = {};
    uint32_t diff = 0;
#pragma unroll
    for (int j = 0; j < R + 2; ++j) {
        // step j ingests row rb - 1 + j and emits generation 1 of row rb + j - 2,
        // which the stage holds as `al`; exact for j in [2, n + 2)
        const int32_t r = rb - 1 + j;
        const bool ok = j <= n + 1 && r >= a.vlo && r < a.vhi;
        Pl<NP> x;
        x.v[0] = ok ? ((uint32_t)g[j] & cm.v[0]) : 0u;
        x.v[1] = ok ? ((uint32_t)(g[j] >> 32) & cm.v[1]) : 0u;
        const uint32_t e = ok ? (ge[j] & em) : 0u;
        const Pl<NP> was = st.al;
        Pl<NP> y = stage_step_ends<RULE>(st, x, ends(x, lane == 0 ? e : 0u, lane == 63 ? e : 0u),
                                         a.birth, a.survive, (j & 1) == 0);
        if constexpr (kBirths) {
            // dead rows and columns stay dead (the in-kernel probe's masks)
            const bool rok = r - 1 >= a.vlo && r - 1 < a.vhi;
#pragma unroll
            for (int k = 0; k < NP; ++k) y.v[k] = rok ? (y.v[k] & cm.v[k]) : 0u;
        }
        if (j >= 2 && j < n + 2) diff |= (y.v[0] ^ was.v[0]) | (y.v[1] ^ was.v[1]);
    }
    if (__builtin_amdgcn_ballot_w64(diff != 0u) != 0) {
        // plain vector stores of one value by every writer, as busy[1]: no atomics
        if (listed) a.moved[unit] = 1u;
        return;
    }
    // Every word of the tile belongs to one of its owners (their rectangles tile the
    // field), and dst holds every owner's rows as the stores below would write them:
    // nothing to store.  One wavefront per tile: a plain add by one lane.
    if (twin_tile) {
        if (lane == 0) a.kept[tile] += 1u;
        return;
    }
    if (!qin) return;
    uint64_t* dst = a.dst + row0 + (int64_t)rb * a.stride + q;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const bool ok = rb + j >= a.vlo && rb + j < a.vhi;
        if (j < n) __builtin_nontemporal_store(ok ? (g[j + 1] & cmw) : 0ull, dst + (int64_t)j * a.stride);
    }
}

}  // namespace

hipError_t launch_probe_pass(const ProbeArgs& a, RuleKind rule, hipStream_t s)
{
    if (a.ntile <= 0 || a.ncol <= 0 || a.total_units <= 0) return hipSuccess;
    // no word of an earlier step, load or timing pass survives
    hipLaunchKernelGGL(life_probe_zero_kernel, dim3(((unsigned)a.total_units + 255) / 256), dim3(256),
                       0, s, a.moved, a.total_units);
    const unsigned blocks = ((unsigned)a.ntile + kWavesPerBlock - 1) / kWavesPerBlock;
    const dim3 grid(blocks), block(64 * kWavesPerBlock);
    if (rule == RULE_REF)
        hipLaunchKernelGGL(life_probe_kernel<RULE_REF>, grid, block, 0, s, a);
    else if (rule == RULE_CONWAY)
        hipLaunchKernelGGL(life_probe_kernel<RULE_CONWAY>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(life_probe_kernel<RULE_GENERIC>, grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace gol
