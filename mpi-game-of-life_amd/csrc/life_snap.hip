// life_snap.hip -- the snapshot compare (DESIGN §4 "Snapshots"): the field words of
// an engine's current buffer against the same words of its snapshot, in the shape of
// the copy pass (life_copy.hip): one wavefront per tile of kCopyTileRows rows x
// kCopyTileWords words, lane l = word l of the tile's column segment, non-temporal
// loads of both buffers and a few dozen registers.  The stored format is a bit
// permutation of the canonical one within a lane group (bitlayout.h), so the XOR of
// two stored words has as many bits as the XOR of the cells they hold, and a masked
// last group (SnapArgs::mask: the split form of the field's columns) leaves out
// columns >= w and a torus interior's ghost columns; no word is joined.
//   same  one wavefront per tile.  Every wavefront first loads *flag and skips its
//         field loads if it is set (the one-load exit of StepArgs::busy); a workgroup
//         one of whose wavefronts' ballots finds a difference stores 1 there with a
//         plain vector store, and nothing else is stored (16 bytes of LDS gather the
//         four wavefronts' findings).  On a field in motion the grid drains after the
//         first tiles.
//   diff  a bounded grid, each wavefront walking tiles with a grid stride, popcounts
//         added up in registers, reduced across the lanes and then across the
//         workgroup's four wavefronts (32 bytes of LDS), and one 64-bit atomic add per
//         workgroup per launch at most.
// Every index is checked against the arguments' bounds before any access.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "life_internal.h"

namespace gol {

namespace {

// The XOR of the two buffers' words of tile `tile`, one word per lane and row, masked
// to the field's columns; rows beyond the tile's last repeat it and are zeroed.
// Returns false (uniform) for a tile outside the region.
__device__ __forceinline__ bool tile_xor(const SnapArgs& a, uint32_t tile, int lane,
                                         uint64_t x[kCopyTileRows])
{
    const uint32_t chunk = tile / (uint32_t)a.ncol, seg = tile - chunk * (uint32_t)a.ncol;
    const int64_t rb = (int64_t)chunk * kCopyTileRows;
    if (rb >= a.rows) return false;
    const int n = (int)min((int64_t)kCopyTileRows, a.rows - rb);
    const int64_t q = (int64_t)seg * kCopyTileWords + lane;
    const bool on = q < a.nwords;
    const uint64_t cm = q == a.nwords - 1 ? a.mask[1] : q == a.nwords - 2 ? a.mask[0] : ~0ull;
    // (a lane beyond the row's words reads word 0 of the region: in bounds, not used)
    const int64_t off = (a.row_base + rb) * a.stride + a.word0 + (on ? q : 0);
    const uint64_t* cur = a.cur + off;
    const uint64_t* snap = a.snap + off;
    uint64_t g[kCopyTileRows], s[kCopyTileRows];
#pragma unroll
    for (int j = 0; j < kCopyTileRows; ++j) {
        g[j] = __builtin_nontemporal_load(cur + (int64_t)min(j, n - 1) * a.stride);
        s[j] = __builtin_nontemporal_load(snap + (int64_t)min(j, n - 1) * a.stride);
    }
#pragma unroll
    for (int j = 0; j < kCopyTileRows; ++j) x[j] = (on && j < n) ? ((g[j] ^ s[j]) & cm) : 0ull;
    return true;
}

__global__ __launch_bounds__(256) void life_snap_same_kernel(SnapArgs a)
{
    const int lane = threadIdx.x & 63;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t tile = blockIdx.x * (uint32_t)kWavesPerBlock + wv;
    bool found = false;
    // (agent scope: the word another wavefront of this launch stored, not a line a
    // cache has held since the launch's first wavefronts)
    if (tile < (uint32_t)a.ntile &&
        __hip_atomic_load(a.flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
        uint64_t x[kCopyTileRows];
        if (tile_xor(a, tile, lane, x)) {
            uint64_t any = 0;
#pragma unroll
            for (int j = 0; j < kCopyTileRows; ++j) any |= x[j];
            found = __builtin_amdgcn_ballot_w64(any != 0ull) != 0ull;
        }
    }
    // One store per workgroup at most, after a second look at the word: stores to one
    // address run one after the other, and the wavefronts in flight when the first
    // difference is found all come here together.  Every wavefront of the
    // workgroup reaches the barrier: nothing above returns.
    __shared__ uint32_t part[kWavesPerBlock];
    if (lane == 0) part[wv] = found ? 1u : 0u;
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint32_t hit = 0;
#pragma unroll
    for (int i = 0; i < kWavesPerBlock; ++i) hit |= part[i];
    if (hit && __hip_atomic_load(a.flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u)
        __hip_atomic_store(a.flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void life_snap_diff_kernel(SnapArgs a)
{
    const int lane = threadIdx.x & 63;
    const uint32_t wave0 =
        blockIdx.x * (uint32_t)kWavesPerBlock + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nwaves = gridDim.x * (uint32_t)kWavesPerBlock;
    uint64_t cells = 0;
    // (ntile < 2^31 and nwaves <= 2^13: the sum does not wrap)
    for (uint32_t tile = wave0; tile < (uint32_t)a.ntile; tile += nwaves) {
        uint64_t x[kCopyTileRows];
        if (!tile_xor(a, tile, lane, x)) break;
        uint32_t c = 0;
#pragma unroll
        for (int j = 0; j < kCopyTileRows; ++j) c += (uint32_t)__popcll(x[j]);
        cells += c;
    }
    for (int off = 32; off > 0; off >>= 1) cells += __shfl_xor(cells, off);
    // one atomic per workgroup: adds to one address run one after the other, and the
    // grid's wavefronts all end together (32768 of them cost 0.3 ms at 65536^2)
    __shared__ uint64_t part[kWavesPerBlock];
    if (lane == 0) part[threadIdx.x >> 6] = cells;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t sum = 0;
#pragma unroll
        for (int i = 0; i < kWavesPerBlock; ++i) sum += part[i];
        if (sum) atomicAdd(a.count, (unsigned long long)sum);
    }
}

}  // namespace

hipError_t launch_snap_compare(const SnapArgs& in, bool count, hipStream_t s)
{
    SnapArgs a = in;
    if (a.rows <= 0 || a.nwords <= 0) return hipSuccess;
    if (!a.cur || !a.snap || a.stride <= 0 || a.word0 < 0 || a.word0 + a.nwords > a.stride ||
        (count ? !a.count : !a.flag))
        return hipErrorInvalidValue;
    const int64_t ncol = (a.nwords + kCopyTileWords - 1) / kCopyTileWords;
    const int64_t ntile = (a.rows + kCopyTileRows - 1) / kCopyTileRows * ncol;
    if (ntile > 0x7fffffffll) return hipErrorInvalidValue;  // (a field of 2^40 words)
    a.ncol = (int32_t)ncol;
    a.ntile = (int32_t)ntile;
    const int64_t blocks = (ntile + kWavesPerBlock - 1) / kWavesPerBlock;
    if (count) {
        // (2048 workgroups: the 8 a CU holds at once on each of 256 CUs)
        hipLaunchKernelGGL(life_snap_diff_kernel, dim3((unsigned)min(blocks, (int64_t)2048)),
                           dim3(64 * kWavesPerBlock), 0, s, a);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(life_snap_same_kernel, dim3((unsigned)blocks), dim3(64 * kWavesPerBlock), 0,
                       s, a);
    return hipGetLastError();
}

}  // namespace gol
