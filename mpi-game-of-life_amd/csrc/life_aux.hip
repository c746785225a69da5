// life_aux.hip -- memory-bound helper kernels (synthetic init, digest, ASCII
// codec, torus wrap, region I/O) and the depth dispatch of the stencil kernel
// (life_stencil.h, one translation unit per depth: life_tb_d<K>.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bitlayout.h"
#include "life_internal.h"
#include "rect_blit.h"
#include "torus_wrap.h"

namespace gol {

#define GOL_EXTERN_DEPTH(K)                                                                   \
    extern template hipError_t launch_depth<K>(const StepArgs&, RuleKind, int, bool,          \
                                               hipStream_t);                                  \
    extern template int occupancy_depth<K>(RuleKind, int, bool, bool);
GOL_EXTERN_DEPTH(1)
GOL_EXTERN_DEPTH(2)
GOL_EXTERN_DEPTH(4)
GOL_EXTERN_DEPTH(6)
GOL_EXTERN_DEPTH(7)
GOL_EXTERN_DEPTH(8)
GOL_EXTERN_DEPTH(12)
GOL_EXTERN_DEPTH(16)
#if GOL_DEV_KERNELS
GOL_EXTERN_DEPTH(20)
GOL_EXTERN_DEPTH(24)
GOL_EXTERN_DEPTH(32)
#endif
#undef GOL_EXTERN_DEPTH

hipError_t launch_life(const StepArgs& a, int depth, RuleKind rule, int planes, bool hand,
                       hipStream_t s)
{
    if (a.total_units <= 0) return hipSuccess;
    switch (depth) {
    case 1: return launch_depth<1>(a, rule, planes, hand, s);
    case 2: return launch_depth<2>(a, rule, planes, hand, s);
    case 4: return launch_depth<4>(a, rule, planes, hand, s);
    case 6: return launch_depth<6>(a, rule, planes, hand, s);
    case 7: return launch_depth<7>(a, rule, planes, hand, s);
    case 8: return launch_depth<8>(a, rule, planes, hand, s);
    case 12: return launch_depth<12>(a, rule, planes, hand, s);
    case 16: return launch_depth<16>(a, rule, planes, hand, s);
#if GOL_DEV_KERNELS
    case 20: return launch_depth<20>(a, rule, planes, hand, s);
    case 24: return launch_depth<24>(a, rule, planes, hand, s);
    case 32: return launch_depth<32>(a, rule, planes, hand, s);
#endif
    default: return hipErrorInvalidValue;
    }
}

int life_blocks_per_cu(int depth, RuleKind rule, int planes, bool hand, bool mp)
{
    switch (depth) {
    case 1: return occupancy_depth<1>(rule, planes, hand, mp);
    case 2: return occupancy_depth<2>(rule, planes, hand, mp);
    case 4: return occupancy_depth<4>(rule, planes, hand, mp);
    case 6: return occupancy_depth<6>(rule, planes, hand, mp);
    case 7: return occupancy_depth<7>(rule, planes, hand, mp);
    case 8: return occupancy_depth<8>(rule, planes, hand, mp);
    case 12: return occupancy_depth<12>(rule, planes, hand, mp);
    case 16: return occupancy_depth<16>(rule, planes, hand, mp);
#if GOL_DEV_KERNELS
    case 20: return occupancy_depth<20>(rule, planes, hand, mp);
    case 24: return occupancy_depth<24>(rule, planes, hand, mp);
    case 32: return occupancy_depth<32>(rule, planes, hand, mp);
#endif
    default: return 0;
    }
}

bool life_has_kernel(int depth, int planes)
{
    bool listed = false;
    for (int d : kDepthList) listed |= d == depth;
    if (!listed) return false;
    return planes == 2 || (kDevKernels && planes == 4 && depth <= 16);
}

namespace {

__device__ __forceinline__ uint64_t splitmix64_at(uint64_t seed, uint64_t idx)
{
    uint64_t z = seed + (idx + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The kernels below work per lane group of NP planes (NP/2 words, bitlayout.h);
// the canonical word index r*wq + c is what the synthetic field and the digest are
// defined on (gol.h), so they match the oracle's.

template <int NP>
__global__ __launch_bounds__(256) void init_random_kernel(uint64_t* buf, int64_t stride,
                                                          int64_t wq, uint64_t lastmask,
                                                          int64_t row_base, int64_t glob_row0,
                                                          int64_t nrows, uint64_t seed,
                                                          int64_t row_words)
{
    constexpr int G = NP / 2;
    const int64_t gpr = row_words / G;  // lane groups written per buffer row
    const int64_t total = nrows * gpr;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total;
         k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = k / gpr, gq = k - i * gpr;
        uint64_t c[2] = {0, 0}, s[2];
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const int64_t idx = gq * G + j;
            if (idx < wq) {
                c[j] = splitmix64_at(seed, (uint64_t)(glob_row0 + i) * (uint64_t)wq + (uint64_t)idx);
                if (idx == wq - 1) c[j] &= lastmask;  // canonical mask
            }
        }
        gol_split_group(c, s, NP);
#pragma unroll
        for (int j = 0; j < G; ++j) buf[(row_base + i) * stride + gq * G + j] = s[j];
    }
}

template <int NP>
__global__ __launch_bounds__(256) void digest_kernel(const uint64_t* buf, int64_t stride,
                                                     int64_t wq, int64_t ng, int64_t row_base,
                                                     int64_t glob_row0, int64_t nrows,
                                                     unsigned long long* acc, uint64_t lastmask)
{
    constexpr int G = NP / 2;
    const int64_t total = nrows * ng;
    uint64_t live = 0, hash = 0;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total;
         k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = k / ng, gq = k - i * ng;
        uint64_t s[2] = {0, 0}, c[2];
#pragma unroll
        for (int j = 0; j < G; ++j) s[j] = buf[(row_base + i) * stride + gq * G + j];
        gol_join_group(s, c, NP);
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const int64_t idx = gq * G + j;
            if (idx < wq) {
                // (a torus interior's last word also holds ghost columns)
                if (idx == wq - 1) c[j] &= lastmask;
                live += (uint64_t)__popcll(c[j]);
                const uint64_t h = (uint64_t)(glob_row0 + i) * (uint64_t)wq + (uint64_t)idx;
                hash += splitmix64_at(c[j] ^ splitmix64_at(0, h), 0);
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        live += __shfl_xor(live, off);
        hash += __shfl_xor(hash, off);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&acc[0], (unsigned long long)live);
        atomicAdd(&acc[1], (unsigned long long)hash);
    }
}

// ASCII codec (data.txt / output.txt bytes <-> stored lane groups), the
// device-side replacement of readGridFromFile's parse (:91-99) and
// writeDataToFile's serialisation (:157-164).  One wavefront per (row, lane
// group): lane j reads the byte of column 64c+j of each of the group's words
// (coalesced), __ballot forms the canonical words, lane 0 stores the group.
// Byte w of every row must be '\n'.
template <int NP>
__global__ __launch_bounds__(256) void ascii_pack_kernel(const char* src, int64_t rows, int64_t w,
                                                         int64_t ng, uint64_t* dst,
                                                         int64_t stride, int* bad)
{
    constexpr int G = NP / 2;
    const int lane = threadIdx.x & 63;
    const int64_t total = rows * ng;
    const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t k = wave0; k < total; k += nwaves) {
        const int64_t r = k / ng, gq = k - r * ng;
        const char* line = src + r * (w + 1);
        uint64_t c[2] = {0, 0}, s[2];
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const int64_t col = (gq * G + j) * 64 + lane;
            c[j] = __ballot(col < w && line[col] == '1');
        }
        if (lane == 0) {
            gol_split_group(c, s, NP);
#pragma unroll
            for (int j = 0; j < G; ++j) dst[r * stride + gq * G + j] = s[j];
            if (gq == ng - 1 && line[w] != '\n') atomicOr(bad, 1);
        }
    }
}

template <int NP>
__global__ __launch_bounds__(256) void ascii_unpack_kernel(const uint64_t* src, int64_t stride,
                                                           int64_t rows, int64_t w, int64_t ng,
                                                           char* dst)
{
    constexpr int G = NP / 2;
    const int lane = threadIdx.x & 63;
    const int64_t total = rows * ng;
    const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t k = wave0; k < total; k += nwaves) {
        const int64_t r = k / ng, gq = k - r * ng;
        uint64_t s[2] = {0, 0}, c[2];
#pragma unroll
        for (int j = 0; j < G; ++j) s[j] = src[r * stride + gq * G + j];
        gol_join_group(s, c, NP);
        char* line = dst + r * (w + 1);
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const int64_t col = (gq * G + j) * 64 + lane;
            if (col < w) line[col] = ((c[j] >> lane) & 1) ? '1' : '0';
        }
        if (gq == ng - 1 && lane == 0) line[w] = '\n';
    }
}

// Torus wrap: one thread per ghost or straddling word of the padded field (2-plane
// stored words).  The 2G ghost rows take all wq_pad words; an interior row takes
// its Gx left ghost words and the words from the one that holds column w on
// (`side` words: the straddling word, if w % 64 != 0, and the right ghosts).
// Sources are interior words only; the one word that is both source and target,
// the straddling word, keeps its interior bits (imask), and the gather never looks
// at a source bit at or beyond column w (torus_wrap.h), so the order in which the
// threads run does not matter.
__global__ __launch_bounds__(256) void torus_wrap_kernel(uint64_t* buf, int64_t stride, int64_t h,
                                                         int64_t w, int64_t G, int64_t Gx,
                                                         int64_t wq_pad)
{
    const int64_t full = w >> 6;             // interior words without ghost columns
    const int64_t side = wq_pad - full;      // words per interior row: Gx + (rest)
    const int64_t ghost_words = 2 * G * wq_pad;
    const int64_t total = ghost_words + h * side;
    const int64_t x_end = w + 64 * Gx;
    const uint64_t imask = (w & 63) ? ((1ull << (w & 63)) - 1ull) : 0ull;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total;
         k += (int64_t)gridDim.x * blockDim.x) {
        int64_t row, q;  // padded row and word
        if (k < ghost_words) {
            const int64_t i = k / wq_pad;
            q = k - i * wq_pad;
            row = i < G ? i : h + i;  // rows [0, G) and [h + G, h + 2G)
        } else {
            const int64_t j = k - ghost_words, i = j / side, c = j - i * side;
            row = G + i;
            q = c < Gx ? c : full + c;  // [0, Gx) and [Gx + full, wq_pad)
        }
        const uint64_t* src = buf + (G + gol_torus_mod(row - G, h)) * stride + Gx;
        uint64_t v = gol_torus_gather([src](int64_t i) { return gol_join64(src[i]); }, w, q - Gx,
                                      x_end);
        uint64_t* dst = buf + row * stride + q;
        if (row >= G && row < G + h && q == Gx + full && imask)
            v = (gol_join64(*dst) & imask) | (v & ~imask);
        *dst = gol_split64(v);
    }
}

// ---- Region I/O (gol_read_rect / gol_write_rect / gol_density; rect_blit.h) ----
// The three kernels see one non-wrapping piece of a rectangle: `rows` buffer rows
// from row_base on, field columns [x, x + cols) of a view `buf` whose word 0 is
// field column 0 (a torus interior: the inner buffer + its ghost words).  No bit at
// or beyond column x + cols is read for its value or changed.

// canonical word q of a stored row
template <int NP>
__device__ __forceinline__ uint64_t load_canonical(const uint64_t* row, int64_t q)
{
    constexpr int G = NP / 2;
    const int64_t g = q / G;
    uint64_t s[2] = {0, 0}, c[2] = {0, 0};
#pragma unroll
    for (int j = 0; j < G; ++j) s[j] = row[g * G + j];
    gol_join_group(s, c, NP);
    return (q - g * G) ? c[1] : c[0];
}

// One thread per word of the compact staging window dst (rows x ceil(cols/64)
// words): bit j of word dq of row i = field column x + 64 dq + j, 0 from cols on.
template <int NP>
__global__ __launch_bounds__(256) void rect_read_kernel(const uint64_t* buf, int64_t stride,
                                                        int64_t row_base, int64_t x, int64_t rows,
                                                        int64_t cols, uint64_t* dst,
                                                        int64_t dst_stride)
{
    const int64_t ww = (cols + 63) >> 6;
    const int64_t total = rows * ww;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total;
         k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = k / ww, dq = k - i * ww;
        const uint64_t* row = buf + (row_base + i) * stride;
        uint64_t m;
        dst[i * dst_stride + dq] = gol_rect_word(
            [row](int64_t q) { return load_canonical<NP>(row, q); }, x, 0, cols, dq, &m);
    }
}

// One thread per lane group of the field that holds a column of the piece, so no
// two threads touch the same word.  src is the compact staged window (bit 0 of a
// row = field column x).  A group wholly inside the piece under SET is not loaded.
template <int NP>
__global__ __launch_bounds__(256) void rect_write_kernel(uint64_t* buf, int64_t stride,
                                                         int64_t row_base, int64_t x, int64_t rows,
                                                         int64_t cols, const uint64_t* src,
                                                         int64_t src_stride, uint32_t op)
{
    constexpr int G = NP / 2;
    const int64_t g0 = x / (64 * G), ngr = (x + cols - 1) / (64 * G) - g0 + 1;
    const int64_t total = rows * ngr;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total;
         k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = k / ngr, gq = g0 + (k - i * ngr);
        const uint64_t* srow = src + i * src_stride;
        uint64_t* grp = buf + (row_base + i) * stride + gq * G;
        uint64_t v[2] = {0, 0}, m[2] = {0, 0}, c[2] = {0, 0}, s[2] = {0, 0};
        bool full = true;
#pragma unroll
        for (int j = 0; j < G; ++j) {
            v[j] = gol_rect_word([srow](int64_t q) { return srow[q]; }, 0, x, cols, gq * G + j,
                                 &m[j]);
            full &= m[j] == ~0ull;
        }
        if (op == GOL_RECT_OP_SET && full) {
            c[0] = v[0];
            c[1] = v[1];
        } else {
#pragma unroll
            for (int j = 0; j < G; ++j) s[j] = grp[j];
            gol_join_group(s, c, NP);
#pragma unroll
            for (int j = 0; j < G; ++j) c[j] = gol_rect_merge(c[j], v[j], m[j], op);
        }
        gol_split_group(c, s, NP);
#pragma unroll
        for (int j = 0; j < G; ++j) grp[j] = s[j];
    }
}

// bits [lo, hi) of the row that fall into the word starting at bit wb
__device__ __forceinline__ uint64_t range_mask(int64_t lo, int64_t hi, int64_t wb)
{
    const int64_t a = lo > wb ? lo - wb : 0, b = hi < wb + 64 ? hi - wb : 64;
    if (b <= a) return 0;
    return (b - a == 64 ? ~0ull : (1ull << (b - a)) - 1ull) << a;
}

// Live cells per by x bx block.  The piece's first cell is window cell (wrow0,
// wcol0); block (bi, bj) holds window rows [bi by, (bi + 1) by) and columns
// [bj bx, (bj + 1) bx), and its cells in this piece are added to
// counts[bi * cstride + bj].  One wavefront per work item = 64 consecutive lane
// groups x up to rpi rows of one block row: a lane keeps its group and therefore
// its block, loads one stored group per row (the wavefront 64 consecutive ones) and
// counts it without a join, the stored format being a bit permutation: a group cut
// by the piece's edge is masked with the split form of its column mask.  The lanes
// of one block then add up with shuffles (their keys rise along the wavefront, so
// equal keys are neighbours) and the first of them adds the sum to the block.  A
// group whose columns fall into several blocks (bx below the group's width, or a
// block edge inside it) is joined and counted per block instead.
template <int NP>
__global__ __launch_bounds__(256) void density_kernel(const uint64_t* buf, int64_t stride,
                                                      int64_t row_base, int64_t x, int64_t rows,
                                                      int64_t cols, int64_t wrow0, int64_t wcol0,
                                                      int64_t by, int64_t bx, uint32_t* counts,
                                                      int64_t cstride, int64_t rpi)
{
    constexpr int G = NP / 2;
    constexpr int64_t GC = 64 * G;
    const int lane = threadIdx.x & 63;
    const int64_t g0 = x / GC, g1 = (x + cols - 1) / GC;
    const int64_t nchunk = (g1 - g0 + 64) / 64;
    const int64_t bi0 = wrow0 / by, nbr = (wrow0 + rows - 1) / by - bi0 + 1;
    const int64_t ppb = (by + rpi - 1) / rpi;
    const int64_t total = nbr * ppb * nchunk;
    const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t k = wave0; k < total; k += nwaves) {
        const int64_t chunk = k % nchunk, t = k / nchunk;
        const int64_t bi = bi0 + t / ppb, p = t % ppb;
        // window rows of this item, clipped to the block row and the piece
        int64_t r0 = bi * by + p * rpi, r1 = r0 + rpi;
        if (r1 > (bi + 1) * by) r1 = (bi + 1) * by;
        if (r0 < wrow0) r0 = wrow0;
        if (r1 > wrow0 + rows) r1 = wrow0 + rows;
        if (r1 <= r0) continue;  // (uniform over the wavefront)
        const int64_t gq = g0 + chunk * 64 + lane;
        const bool on = gq <= g1;
        // field columns [c0, c1) of this group inside the piece, and their blocks
        const int64_t c0 = on ? (gq * GC > x ? gq * GC : x) : 0;
        const int64_t c1 = on ? ((gq + 1) * GC < x + cols ? (gq + 1) * GC : x + cols) : 0;
        const int64_t bj0 = on ? (wcol0 + c0 - x) / bx : 0;
        const int64_t bj1 = on ? (wcol0 + c1 - 1 - x) / bx : 0;
        const bool single = on && bj0 == bj1;
        const uint64_t* grp = buf + (row_base + (r0 - wrow0)) * stride + gq * G;
        uint32_t val = 0;
        if (single) {
            uint64_t cm[2] = {0, 0}, sm[2] = {0, 0};
#pragma unroll
            for (int j = 0; j < G; ++j) cm[j] = range_mask(c0, c1, (gq * G + j) * 64);
            gol_split_group(cm, sm, NP);
#pragma unroll 4
            for (int64_t r = 0; r < r1 - r0; ++r) {
#pragma unroll
                for (int j = 0; j < G; ++j) val += (uint32_t)__popcll(grp[r * stride + j] & sm[j]);
            }
        } else if (on) {
            for (int64_t r = 0; r < r1 - r0; ++r) {
                uint64_t s[2] = {0, 0}, c[2] = {0, 0};
#pragma unroll
                for (int j = 0; j < G; ++j) s[j] = grp[r * stride + j];
                gol_join_group(s, c, NP);
                for (int64_t bj = bj0; bj <= bj1; ++bj) {
                    // field columns of block bj inside this group
                    const int64_t lo = x - wcol0 + bj * bx, hi = lo + bx;
                    const int64_t a = lo > c0 ? lo : c0, b = hi < c1 ? hi : c1;
                    uint32_t n = 0;
#pragma unroll
                    for (int j = 0; j < G; ++j)
                        n += (uint32_t)__popcll(c[j] & range_mask(a, b, (gq * G + j) * 64));
                    if (n) atomicAdd(&counts[bi * cstride + bj], n);
                }
            }
        }
        long long key = single ? (long long)bj0 : -1ll;
        for (int off = 1; off < 64; off <<= 1) {
            const long long ok = __shfl_down(key, off);
            const uint32_t ov = __shfl_down(val, off);
            if (lane + off < 64 && ok == key) val += ov;
        }
        const long long prev = __shfl_up(key, 1);
        if (key >= 0 && val && (lane == 0 || prev != key))
            atomicAdd(&counts[bi * cstride + key], val);
    }
}

dim3 grid_for(int64_t items, int64_t per_block, int64_t cap)
{
    int64_t blocks = (items + per_block - 1) / per_block;
    if (blocks > cap) blocks = cap;
    return dim3((unsigned)blocks);
}

}  // namespace

hipError_t launch_init_random(uint64_t* buf, int64_t stride, int64_t wq, uint64_t lastmask,
                              int64_t row_base, int64_t glob_row0, int64_t nrows, uint64_t seed,
                              int planes, hipStream_t s, int64_t row_words)
{
    if (nrows <= 0) return hipSuccess;
    if (row_words <= 0) row_words = stride;
    const dim3 grid = grid_for(nrows * row_words / (planes / 2), 256, 8192);
    if (planes == 4)
        hipLaunchKernelGGL(init_random_kernel<4>, grid, dim3(256), 0, s, buf, stride, wq, lastmask,
                           row_base, glob_row0, nrows, seed, row_words);
    else
        hipLaunchKernelGGL(init_random_kernel<2>, grid, dim3(256), 0, s, buf, stride, wq, lastmask,
                           row_base, glob_row0, nrows, seed, row_words);
    return hipGetLastError();
}

hipError_t launch_ascii_pack(const char* src, int64_t rows, int64_t w, int64_t ng, uint64_t* dst,
                             int64_t stride, int* bad, int planes, hipStream_t s)
{
    if (rows <= 0) return hipSuccess;
    const dim3 grid = grid_for(rows * ng, 4, 16384);
    if (planes == 4)
        hipLaunchKernelGGL(ascii_pack_kernel<4>, grid, dim3(256), 0, s, src, rows, w, ng, dst,
                           stride, bad);
    else
        hipLaunchKernelGGL(ascii_pack_kernel<2>, grid, dim3(256), 0, s, src, rows, w, ng, dst,
                           stride, bad);
    return hipGetLastError();
}

hipError_t launch_ascii_unpack(const uint64_t* src, int64_t stride, int64_t rows, int64_t w,
                               int64_t ng, char* dst, int planes, hipStream_t s)
{
    if (rows <= 0) return hipSuccess;
    const dim3 grid = grid_for(rows * ng, 4, 16384);
    if (planes == 4)
        hipLaunchKernelGGL(ascii_unpack_kernel<4>, grid, dim3(256), 0, s, src, stride, rows, w, ng,
                           dst);
    else
        hipLaunchKernelGGL(ascii_unpack_kernel<2>, grid, dim3(256), 0, s, src, stride, rows, w, ng,
                           dst);
    return hipGetLastError();
}

hipError_t launch_digest(const uint64_t* buf, int64_t stride, int64_t wq, int64_t ng,
                         int64_t row_base, int64_t glob_row0, int64_t nrows,
                         unsigned long long* acc, int planes, hipStream_t s, uint64_t lastmask)
{
    if (nrows <= 0) return hipSuccess;
    const dim3 grid = grid_for(nrows * ng, 256, 8192);
    if (planes == 4)
        hipLaunchKernelGGL(digest_kernel<4>, grid, dim3(256), 0, s, buf, stride, wq, ng, row_base,
                           glob_row0, nrows, acc, lastmask);
    else
        hipLaunchKernelGGL(digest_kernel<2>, grid, dim3(256), 0, s, buf, stride, wq, ng, row_base,
                           glob_row0, nrows, acc, lastmask);
    return hipGetLastError();
}

hipError_t launch_torus_wrap(uint64_t* buf, int64_t stride, int64_t h, int64_t w, int64_t G,
                             int64_t Gx, hipStream_t s)
{
    if (h <= 0 || w <= 0 || G <= 0 || Gx <= 0) return hipErrorInvalidValue;
    const int64_t wq_pad = (w + 128 * Gx + 63) / 64;
    if (stride < wq_pad) return hipErrorInvalidValue;
    const int64_t total = 2 * G * wq_pad + h * (wq_pad - (w >> 6));
    hipLaunchKernelGGL(torus_wrap_kernel, grid_for(total, 256, 8192), dim3(256), 0, s, buf, stride,
                       h, w, G, Gx, wq_pad);
    return hipGetLastError();
}

// Region I/O launchers: one non-wrapping piece each (see the kernels above).
hipError_t launch_rect_read(const uint64_t* buf, int64_t stride, int64_t row_base, int64_t x,
                            int64_t rows, int64_t cols, uint64_t* dst, int64_t dst_stride,
                            int planes, hipStream_t s)
{
    if (rows <= 0 || cols <= 0) return hipSuccess;
    const dim3 grid = grid_for(rows * ((cols + 63) / 64), 256, 8192);
    if (planes == 4)
        hipLaunchKernelGGL(rect_read_kernel<4>, grid, dim3(256), 0, s, buf, stride, row_base, x,
                           rows, cols, dst, dst_stride);
    else
        hipLaunchKernelGGL(rect_read_kernel<2>, grid, dim3(256), 0, s, buf, stride, row_base, x,
                           rows, cols, dst, dst_stride);
    return hipGetLastError();
}

hipError_t launch_rect_write(uint64_t* buf, int64_t stride, int64_t row_base, int64_t x,
                             int64_t rows, int64_t cols, const uint64_t* src, int64_t src_stride,
                             uint32_t op, int planes, hipStream_t s)
{
    if (rows <= 0 || cols <= 0) return hipSuccess;
    if (op > GOL_RECT_OP_CLEAR) return hipErrorInvalidValue;
    const int64_t gc = 32 * planes;
    const dim3 grid = grid_for(rows * ((x + cols - 1) / gc - x / gc + 1), 256, 8192);
    if (planes == 4)
        hipLaunchKernelGGL(rect_write_kernel<4>, grid, dim3(256), 0, s, buf, stride, row_base, x,
                           rows, cols, src, src_stride, op);
    else
        hipLaunchKernelGGL(rect_write_kernel<2>, grid, dim3(256), 0, s, buf, stride, row_base, x,
                           rows, cols, src, src_stride, op);
    return hipGetLastError();
}

hipError_t launch_density(const uint64_t* buf, int64_t stride, int64_t row_base, int64_t x,
                          int64_t rows, int64_t cols, int64_t wrow0, int64_t wcol0, int64_t by,
                          int64_t bx, uint32_t* counts, int64_t cstride, int planes,
                          hipStream_t s)
{
    if (rows <= 0 || cols <= 0) return hipSuccess;
    if (by <= 0 || bx <= 0) return hipErrorInvalidValue;
    // rows per work item: up to 32 of one block row (a lane adds 32 x 64 x planes / 2
    // cells at most, and tall blocks still split into enough wavefronts)
    const int64_t rpi = by < 32 ? by : 32;
    const int64_t gc = 32 * planes;
    const int64_t nchunk = ((x + cols - 1) / gc - x / gc + 64) / 64;
    const int64_t nbr = (wrow0 + rows - 1) / by - wrow0 / by + 1;
    const int64_t items = nbr * ((by + rpi - 1) / rpi) * nchunk;
    const dim3 grid = grid_for(items, 4, 8192);
    if (planes == 4)
        hipLaunchKernelGGL(density_kernel<4>, grid, dim3(256), 0, s, buf, stride, row_base, x,
                           rows, cols, wrow0, wcol0, by, bx, counts, cstride, rpi);
    else
        hipLaunchKernelGGL(density_kernel<2>, grid, dim3(256), 0, s, buf, stride, row_base, x,
                           rows, cols, wrow0, wcol0, by, bx, counts, cstride, rpi);
    return hipGetLastError();
}

}  // namespace gol
