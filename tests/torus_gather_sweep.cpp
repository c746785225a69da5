// torus_gather_sweep.cpp -- stand-alone check of the torus wrap rule's word gather
// (mpi-game-of-life_amd/csrc/torus_wrap.h) against a per-bit loop, meant to be
// compiled with -fsanitize=address,undefined (tests/test_torus_host.py): the gather
// must never read a source word at or beyond ceil(w/64), so each row lives in a
// heap block of exactly that many words.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "torus_wrap.h"

int main()
{
    std::mt19937_64 rng(12345);
    long checked = 0;
    for (int64_t w = 1; w <= 200; ++w) {
        const int64_t wq = (w + 63) / 64;
        // (a fresh exact-size block per width: an over-read is an ASan error)
        std::vector<uint64_t> row((size_t)wq);
        for (int rep = 0; rep < 3; ++rep) {
            // bits at columns >= w are junk on purpose: the gather must ignore them
            for (auto& x : row) x = rep == 0 ? ~0ull : rng();
            const uint64_t* src = row.data();
            auto cell = [&](int64_t x) { return (src[x >> 6] >> (x & 63)) & 1ull; };
            for (int64_t G : {1, 16, 63, 64, 65, 70, 130}) {
                const int64_t Gx = (G + 63) / 64;
                const int64_t x_end = w + 64 * Gx;
                const int64_t wq_pad = wq + 2 * Gx;
                for (int64_t q = 0; q < wq_pad; ++q) {
                    const uint64_t got = gol_torus_gather([src](int64_t i) { return src[i]; }, w,
                                                          q - Gx, x_end);
                    uint64_t want = 0;
                    for (int j = 0; j < 64; ++j) {
                        const int64_t x = 64 * (q - Gx) + j;
                        if (x < x_end) want |= cell(gol_torus_mod(x, w)) << j;
                    }
                    if (got != want) {
                        std::printf("mismatch w=%lld G=%lld q=%lld got=%016llx want=%016llx\n",
                                    (long long)w, (long long)G, (long long)q,
                                    (unsigned long long)got, (unsigned long long)want);
                        return 1;
                    }
                    ++checked;
                }
            }
        }
    }
    // rows: y mod h for negative and large y
    for (int64_t h = 1; h <= 9; ++h)
        for (int64_t y = -300; y <= 300; ++y) {
            const int64_t m = gol_torus_mod(y, h);
            if (m < 0 || m >= h || (y - m) % h != 0) return 2;
        }
    std::printf("ok %ld\n", checked);
    return 0;
}
