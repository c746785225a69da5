// Pending fixed steps (csrc/still_pending.h) against the device words they stand for:
// a run of fixed steps folded by still_accumulate and applied once, as flush_still's
// one kernel does, must leave every word of a simulated activity state as the steps'
// kernels leave it one after the other.  The simulation is life_still_step_kernel's
// (life_copy.hip): the proof (twin_ok set, every twin 2), then increments added in
// uint32_t and final values stored; where the proof fails, the error word alone.
// argv[1]: a text file of real effects, one per line, the 18 numbers of
// gol_still_effect in the struct's order (tests/test_still_pending_host.py writes it
// from gol_plan_still_step for every depth and the lengths 5K .. 9K - 1); synthetic
// effects with increments near 2^32 join them.  Runs follow the engine's rule: a step
// whose effect leaves twin != 2 ends the run (the next step is no fixed step).  Start
// values include words within one increment of wrapping and states on which the proof
// fails.  Prints "ok <runs> <effects>".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "still_pending.h"

using golh::StillPending;
using golh::still_accumulate;

static const int kUnits = 3;

struct Words {
    uint32_t act[2 * kUnits], copied[kUnits], probed[kUnits], pass_probed[kUnits], elided[kUnits];
    uint32_t busy[2];
    uint32_t streak0[kUnits], streak1[kUnits], need[kUnits], held[kUnits], moved[kUnits], twin[kUnits];
    uint32_t twin_ok;
    uint32_t err;
};

// life_still_step_kernel on the simulated words
static void kernel(Words& w, const gol_still_effect& fx)
{
    bool ok = w.twin_ok != 0u;
    for (int u = 0; u < kUnits; ++u) ok = ok && w.twin[u] == 2u;
    if (!ok) {
        w.err = 2u;
        return;
    }
    for (int u = 0; u < kUnits; ++u) {
        w.act[2 * u] += fx.computed;
        w.act[2 * u + 1] += fx.skipped;
        w.copied[u] += fx.copied;
        w.probed[u] += fx.probed;
        w.pass_probed[u] += fx.pass_probed;
        w.elided[u] += fx.elided;
        w.streak0[u] = fx.streak0;
        w.streak1[u] = fx.streak1;
        w.need[u] = fx.need;
        w.held[u] = fx.held;
        w.moved[u] = fx.moved;
        w.twin[u] = fx.twin;
    }
    w.busy[0] += fx.busy0_add;
    w.busy[1] = fx.busy1;
    w.twin_ok = fx.twin_ok;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// a start value: anything, small, or within a few counts of wrapping
static uint32_t start_word()
{
    switch (rnd() % 4) {
    case 0: return (uint32_t)rnd();
    case 1: return (uint32_t)(rnd() % 8);
    case 2: return 0xFFFFFFFFu - (uint32_t)(rnd() % 8);
    default: return 0xFFFFFFFFu - (uint32_t)(rnd() % 100000);
    }
}

static Words start_state(bool proven)
{
    Words w;
    uint32_t* p = reinterpret_cast<uint32_t*>(&w);
    for (size_t i = 0; i < sizeof(Words) / sizeof(uint32_t); ++i) p[i] = start_word();
    w.err = 0;
    if (proven) {
        w.twin_ok = 1;
        for (int u = 0; u < kUnits; ++u) w.twin[u] = 2;
    } else {
        // one way for the proof to fail
        w.twin_ok = 1;
        for (int u = 0; u < kUnits; ++u) w.twin[u] = 2;
        if (rnd() % 2)
            w.twin_ok = 0;
        else
            w.twin[rnd() % kUnits] = (uint32_t)(rnd() % 2);
    }
    return w;
}

static gol_still_effect synthetic()
{
    gol_still_effect fx{};
    auto big = [] { return rnd() % 2 ? 0xFFFFFFFFu - (uint32_t)(rnd() % 4) : (uint32_t)rnd(); };
    fx.launches = rnd() >> (rnd() % 40);
    fx.computed = big();
    fx.skipped = big();
    fx.copied = big();
    fx.probed = big();
    fx.pass_probed = big();
    fx.elided = big();
    fx.busy0_add = big();
    fx.busy1 = (uint32_t)rnd();
    fx.streak0 = (uint32_t)rnd();
    fx.streak1 = (uint32_t)rnd();
    fx.need = (uint32_t)(rnd() % 2);
    fx.held = (uint32_t)(rnd() % 2);
    fx.moved = (uint32_t)(rnd() % 2);
    fx.twin = rnd() % 4 ? 2u : 1u;
    fx.twin_ok = 1;
    fx.kept_passes = (uint32_t)(rnd() % 3);
    fx.sure_passes = fx.kept_passes;
    return fx;
}

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s effects.txt\n", argv[0]);
        return 2;
    }
    std::vector<gol_still_effect> real;
    if (FILE* f = std::fopen(argv[1], "r")) {
        uint64_t v[18];
        for (;;) {
            int n = 0;
            for (; n < 18; ++n)
                if (std::fscanf(f, "%" SCNu64, &v[n]) != 1) break;
            if (n != 18) break;
            gol_still_effect fx{};
            fx.launches = v[0];
            uint32_t* w32[] = {&fx.computed, &fx.skipped, &fx.copied, &fx.probed, &fx.pass_probed,
                               &fx.elided, &fx.busy0_add, &fx.busy1, &fx.streak0, &fx.streak1,
                               &fx.need, &fx.held, &fx.moved, &fx.twin, &fx.twin_ok,
                               &fx.kept_passes, &fx.sure_passes};
            for (int i = 0; i < 17; ++i) *w32[i] = (uint32_t)v[1 + i];
            real.push_back(fx);
        }
        std::fclose(f);
    }
    if (real.empty()) {
        std::fprintf(stderr, "no effects read from %s\n", argv[1]);
        return 2;
    }
    uint64_t runs = 0, applied = 0;
    for (int iter = 0; iter < 20000; ++iter) {
        const bool proven = iter % 8 != 7;
        const int mode = iter % 3;  // real, synthetic, mixed
        const size_t want = 1 + rnd() % (iter % 5 == 0 ? 40 : 6);
        Words one = start_state(proven);
        Words all = one;
        StillPending p;
        uint64_t launches = 0, kept = 0, sure = 0;
        for (size_t i = 0; i < want; ++i) {
            const bool syn = mode == 1 || (mode == 2 && rnd() % 2);
            const gol_still_effect fx = syn ? synthetic() : real[rnd() % real.size()];
            kernel(one, fx);
            const StillPending q = still_accumulate(p, fx);
            if (q.steps != p.steps + 1) {
                std::printf("FAIL: the step count after a fold\n");
                return 1;
            }
            p = q;
            launches += fx.launches;
            kept += fx.kept_passes;
            sure += fx.sure_passes;
            ++applied;
            if (fx.twin != 2u) break;  // the host withdraws twin_two: the run ends here
        }
        kernel(all, p.fx);
        if (std::memcmp(&one, &all, sizeof(Words)) != 0) {
            std::printf("FAIL: run %d (%" PRIu64 " steps, proof %s): the words differ\n", iter,
                        p.steps, proven ? "holds" : "fails");
            return 1;
        }
        if (!proven && (one.err != 2u || all.err != 2u)) {
            std::printf("FAIL: run %d: a failed proof left no error word\n", iter);
            return 1;
        }
        if (p.fx.launches != launches || p.fx.kept_passes != (uint32_t)kept ||
            p.fx.sure_passes != (uint32_t)sure) {
            std::printf("FAIL: run %d: the host's sums differ\n", iter);
            return 1;
        }
        ++runs;
    }
    std::printf("ok %" PRIu64 " %" PRIu64 " %zu\n", runs, applied, real.size());
    return 0;
}
