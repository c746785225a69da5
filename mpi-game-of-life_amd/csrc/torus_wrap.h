// torus_wrap.h -- the wrap rule of a torus engine (GOL_SEM_TORUS), host + device,
// no HIP dependence.
//
// A torus engine keeps its h x w interior inside a larger dead-border field with
// ghost cells around it (torus.cpp).  Ghost cell (y, x), with y and x
// relative to the interior's row 0 / column 0 (so negative above and to the left),
// takes interior cell (y mod h, x mod w).  The rule is written once, here, as a
// gather of one 64-column word of a row; the wrap kernel (life_aux.hip) and
// gol_torus_pad (torus.cpp) both call it.
#pragma once
#include <stdint.h>

#include "bitlayout.h"

// y mod n for any sign of y, n >= 1
GOL_HD int64_t gol_torus_mod(int64_t y, int64_t n)
{
    const int64_t m = y % n;
    return m < 0 ? m + n : m;
}

// Bits [x, x + n) of an interior row as the low n bits of the result; 1 <= n <= 64
// and x + n <= w, so no bit at or beyond column w is ever looked at: the word that
// holds column w - 1 may carry anything above it (in a torus buffer: ghost cells).
// ld(i) returns canonical word i of the row's interior, 0 <= i < ceil(w/64).
template <class Load>
GOL_HD uint64_t gol_torus_bits(Load ld, int64_t x, int n)
{
    const int64_t i = x >> 6;
    const int s = (int)(x & 63);
    uint64_t v = ld(i) >> s;
    if (s + n > 64) v |= ld(i + 1) << (64 - s);
    return n == 64 ? v : v & ((1ull << n) - 1ull);
}

// Word p of a row of the padded field, p counted from the interior's word 0 (the
// left ghost words have p < 0): bit j is interior column (64 p + j) mod w of that
// row.  Columns at or beyond x_end (the padded field's right edge, relative to the
// interior's column 0) are 0.  Any w >= 1: for w < 64 the word holds several
// periods, for w % 64 != 0 the periods are not word-aligned.
template <class Load>
GOL_HD uint64_t gol_torus_gather(Load ld, int64_t w, int64_t p, int64_t x_end)
{
    int64_t valid = x_end - 64 * p;  // columns of this word inside the padded field
    if (valid <= 0) return 0;
    if (valid > 64) valid = 64;
    uint64_t out = 0;
    int64_t x = gol_torus_mod(64 * p, w);
    for (int filled = 0; filled < (int)valid;) {
        int64_t n = w - x;
        if (n > valid - filled) n = valid - filled;
        out |= gol_torus_bits(ld, x, (int)n) << filled;
        filled += (int)n;
        x = 0;
    }
    return out;
}
