// rect_blit.h -- the bit blit of the region I/O (gol_read_rect, gol_write_rect,
// gol_rect_blit), host + device, no HIP dependence.
//
// A blit moves bits [sx, sx + cols) of a source row onto bits [dx, dx + cols) of a
// destination row, word by destination word: gol_rect_word gathers the source bits
// that land in one destination word (through gol_torus_bits, torus_wrap.h: two
// source words at most, and none at or beyond the word that holds bit sx + cols - 1)
// and gol_rect_merge combines them with the destination under the word's bit mask.
// The read kernel, the write kernel (life_aux.hip) and gol_rect_blit (engine.cpp)
// all call these two, so the CPU sweep (tests/rect_blit_sweep.cpp) covers the rule
// the kernels run.
#pragma once
#include <stdint.h>

#include "bitlayout.h"
#include "torus_wrap.h"

// gol_rect_op (gol.h)
#define GOL_RECT_OP_SET 0u
#define GOL_RECT_OP_OR 1u
#define GOL_RECT_OP_XOR 2u
#define GOL_RECT_OP_CLEAR 3u

// The bits of destination word dq (bits [64 dq, 64 dq + 64) of the row) that lie in
// [dx, dx + cols): returned in *mask, and the source bits that belong there as the
// result (0 outside the mask).  ld(i) returns canonical word i of the source row;
// it is called for the words that hold source bits of this destination word only.
template <class Load>
GOL_HD uint64_t gol_rect_word(Load ld, int64_t sx, int64_t dx, int64_t cols, int64_t dq,
                              uint64_t* mask)
{
    const int64_t w0 = 64 * dq;
    const int64_t b0 = dx > w0 ? dx : w0;
    const int64_t b1 = dx + cols < w0 + 64 ? dx + cols : w0 + 64;
    if (b1 <= b0) {
        *mask = 0;
        return 0;
    }
    const int lo = (int)(b0 - w0), n = (int)(b1 - b0);
    *mask = (n == 64 ? ~0ull : (1ull << n) - 1ull) << lo;
    return gol_torus_bits(ld, sx + (b0 - dx), n) << lo;
}

// dst combined with src under mask: SET copies, OR / XOR combine, CLEAR is
// dst AND NOT src.  Bits outside mask keep dst's value.  (op checked by the caller.)
GOL_HD uint64_t gol_rect_merge(uint64_t dst, uint64_t src, uint64_t mask, uint32_t op)
{
    const uint64_t s = src & mask;
    switch (op) {
    case GOL_RECT_OP_SET: return (dst & ~mask) | s;
    case GOL_RECT_OP_OR: return dst | s;
    case GOL_RECT_OP_XOR: return dst ^ s;
    default: return dst & ~s;
    }
}

// One row of a blit on canonical words: the host twin of the kernels.
inline void gol_rect_blit_row(const uint64_t* src, int64_t sx, uint64_t* dst, int64_t dx,
                              int64_t cols, uint32_t op)
{
    if (cols <= 0) return;
    for (int64_t dq = dx >> 6; dq <= (dx + cols - 1) >> 6; ++dq) {
        uint64_t m;
        const uint64_t v = gol_rect_word([src](int64_t i) { return src[i]; }, sx, dx, cols, dq, &m);
        dst[dq] = gol_rect_merge(dst[dq], v, m, op);
    }
}
