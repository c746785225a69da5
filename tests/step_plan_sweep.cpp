// The step's schedule (csrc/step_plan.h) against a counter-driven walk of the rules it
// was written from: the step's loop over pick_depth and the passes, the three-way branch
// of a launch on `may`, the counters that branch keeps from launch to launch, and the
// conditions under which the copy pass, the calm kernel alone, the probe pass, the
// clearing of twin_ok and the copy of held[] run.  The walk is the reference: it does
// not change when the schedule does.  Built and run by tests/test_still_effect_host.py;
// prints "ok <cases>".
#include <cstdio>
#include <cstdlib>

#include "step_plan.h"

using golh::StepLaunch;
using golh::StepSchedule;
using golh::StepTraits;

static const int kDepths[] = {16, 12, 8, 7, 6, 4, 2, 1};  // the shipped library's kDepthList
static const int kNDepths = (int)(sizeof(kDepths) / sizeof(kDepths[0]));

// What one launch of the walk does, as the stream would show it.
struct Seen {
    uint32_t depth;
    int passes;
    bool last;
    int branch;  // 0 = leaves the streaks alone, 1 = depth K, 2 = remainder
    bool act;
    int streak_in;
    bool streak_out, no_hist, probe, held, busy;
    int through, launch_idx;
    bool copy_pass, c_held, c_all_held, c_elided, c_twin;
    uint32_t c_twin_val;
    bool calm_alone, probe_pass, probe_twin, probe_sure, twin_clear, twin_held, short_ok;
};

// The walk's state between launches: the fields a step used to keep.
struct Walk {
    int act_launch = 0, act_hist = -1, act_rem = 0;
    bool act_probed = false, act_last = false;
};

static bool hand_at(const StepTraits& t, uint32_t depth)
{
    for (int i = 0; i < t.ndepth; ++i)
        if ((uint32_t)t.depth[i] == depth) return t.hand[i];
    return false;
}

static bool shift_at(const StepTraits& t, uint32_t depth)
{
    for (int i = 0; i < t.ndepth; ++i)
        if ((uint32_t)t.depth[i] == depth) return t.shift[i];
    return false;
}

static Seen walk_launch(const StepTraits& e, Walk& w, uint32_t depth, int passes)
{
    Seen s{};
    s.depth = depth;
    s.passes = passes;
    s.last = w.act_last;
    s.streak_in = -1;
    const bool hand = hand_at(e, depth);
    const bool xcd_shift = shift_at(e, depth);
    bool pass = false, pass_held = false, pass_all = false;
    bool twin_drop = e.twin_on && e.tracked;
    bool twin_last = false, twin_set = false;
    uint32_t twin_val = 1;
    if (w.act_launch >= 0 && e.tracked) {
        s.act = true;
        const bool may = e.act_on && !e.timing_every && !hand && passes == 1 && e.has_nb &&
                         e.npass == 1 && e.nbuf == 2 && !xcd_shift && e.units_fit;
        if (may && depth == e.K) {
            const int par = w.act_launch & 1;
            s.branch = 1;
            s.streak_in = par;
            s.streak_out = true;
            s.no_hist = w.act_launch == 0;
            s.probe = s.no_hist && e.probe_on;
            s.held = s.probe && e.elide_on;
            if (s.no_hist) w.act_probed = s.held;
            s.through = e.through_on >= 1 ? 1 : 0;
            s.busy = e.still_on;
            s.launch_idx = w.act_launch;
            w.act_hist = par ^ 1;
            pass = s.through && w.act_launch == 1;
            pass_held = w.act_probed;
            twin_drop = e.twin_on && w.act_last;
            twin_last = twin_drop && !s.no_hist;
            s.short_ok = s.busy && !s.no_hist && s.launch_idx >= 3;
        } else if (may && depth < e.K && w.act_hist >= 0 && e.through_on >= 2) {
            s.branch = 2;
            s.streak_in = w.act_hist;
            s.through = 1;
            pass = true;
            pass_held = w.act_probed && w.act_launch == 1;
            pass_all = w.act_rem > 0;
            ++w.act_rem;
            twin_last = twin_drop = e.twin_on && w.act_last;
            if (e.sure_on) twin_val = 2;
        } else {
            w.act_hist = -1;
            w.act_probed = false;
        }
        ++w.act_launch;
    }
    if (pass && e.pass_on && e.has_own && e.one_seg) {
        s.copy_pass = true;
        s.c_elided = e.elide_on;
        s.c_held = e.elide_on && pass_held;
        s.c_all_held = e.elide_on && pass_all;
        if (twin_last) {
            s.c_twin = true;
            s.c_twin_val = twin_val;
            twin_set = true;
        }
        s.through = 2;
    }
    if (twin_last && !twin_set && s.streak_in >= 0 && e.has_nb && !s.no_hist) {
        s.calm_alone = true;
        twin_set = true;
    }
    if (s.probe && e.ppass_on && e.has_ptab && e.one_seg && e.planes2) {
        s.probe_pass = true;
        if (e.twin_on && e.has_own) {  // (d_kept: allocated where twin_on)
            s.probe_twin = true;
            s.probe_sure = e.sure_on;
        }
    }
    s.twin_held = twin_drop && !twin_set && s.no_hist && s.probe && s.held;
    s.twin_clear = twin_drop && !twin_set && !s.twin_held;
    return s;
}

static int fail(const char* what, const StepTraits& t, uint64_t gens, uint64_t index)
{
    std::printf("mismatch: %s (K %u, generations %llu, launch %llu, npass %d, through %d, pass %d, "
                "still %d, probe %d, elide %d, ppass %d, twin %d, sure %d, timing %u, act %d)\n",
                what, t.K, (unsigned long long)gens, (unsigned long long)index, t.npass, t.through_on,
                t.pass_on, t.still_on, t.probe_on, t.elide_on, t.ppass_on, t.twin_on, t.sure_on,
                t.timing_every, t.act_on);
    return 1;
}

#define SAME(cond, what) \
    if (!(cond)) return fail(what, t, gens, index)

static int check(const StepTraits& t, uint64_t gens)
{
    StepSchedule sched(t, gens);
    Walk w;
    uint64_t left = gens, index = 0, sum = 0;
    int lasts = 0;
    while (left > 0) {
        const uint32_t d = golh::pick_depth(kDepths, kNDepths, t.K, left);
        const int np = (t.npass <= 1 || d != t.K) ? 1 : (int)std::min<uint64_t>((uint64_t)t.npass, left / d);
        w.act_last = left == (uint64_t)d * np;
        const Seen s = walk_launch(t, w, d, np);
        StepLaunch r;
        SAME(sched.next(&r), "the schedule ends early");
        SAME(r.depth == s.depth && r.passes == s.passes, "depth or passes");
        SAME(r.index == index && r.last == s.last, "index or last");
        SAME((int)r.kind == s.branch, "kind");
        SAME(r.act == s.act, "counters");
        SAME(r.streak_in == s.streak_in && r.streak_out == s.streak_out, "streaks");
        SAME(r.no_hist == s.no_hist && r.probe == s.probe && r.held == s.held, "no_hist, probe or held");
        SAME(r.through == s.through && r.busy == s.busy, "through or busy");
        SAME(r.kind != StepLaunch::kDepthK || r.launch_idx == s.launch_idx, "launch_idx");
        SAME(r.copy_pass == s.copy_pass, "copy pass");
        SAME(!s.copy_pass || (r.pass_held == s.c_held && r.pass_all == s.c_all_held &&
                              r.pass_elide == s.c_elided),
             "copy pass: held, all_held or elided");
        SAME(!s.copy_pass || s.c_twin == (r.twin == StepLaunch::kTwinCalm), "copy pass: twin");
        SAME(r.calm_alone == s.calm_alone, "calm kernel alone");
        SAME(!(s.c_twin || s.calm_alone) || r.twin == StepLaunch::kTwinCalm, "twin by the calm kernel");
        SAME(!s.c_twin || r.twin_val == s.c_twin_val, "twin_val");
        SAME(!s.calm_alone || r.twin_val == 1, "twin_val of the calm kernel alone");
        SAME((r.twin == StepLaunch::kTwinCalm) == (s.c_twin || s.calm_alone), "twin by the calm kernel");
        SAME(r.probe_pass == s.probe_pass && r.probe_twin == s.probe_twin &&
                 r.probe_sure == s.probe_sure,
             "probe pass");
        SAME((r.twin == StepLaunch::kTwinClear) == s.twin_clear, "twin_clear");
        SAME((r.twin == StepLaunch::kTwinHeld) == s.twin_held, "launch_twin_held");
        SAME(r.short_ok == s.short_ok, "short_ok");
        sum += (uint64_t)r.depth * (uint64_t)r.passes;
        lasts += r.last ? 1 : 0;
        left -= (uint64_t)d * np;
        ++index;
    }
    StepLaunch r;
    SAME(!sched.next(&r), "the schedule goes on");
    SAME(sum == gens, "the depths do not sum to the generations");
    SAME(lasts == 1, "not exactly one last launch");
    return 0;
}

int main()
{
    unsigned long long cases = 0;
    for (int K : kDepths)
        for (int npass : {1, 3})
            for (int through = 0; through <= 2; ++through)
                for (int bits = 0; bits < 256; ++bits)
                    for (uint32_t timing : {0u, 8u})
                        for (int hands = 0; hands < 3; ++hands) {
                            StepTraits t;
                            t.K = (uint32_t)K;
                            t.npass = npass;
                            t.nbuf = npass > 1 ? 4 : 2;
                            t.tracked = t.has_err = true;
                            t.act_on = bits & 1;
                            t.through_on = through;
                            t.pass_on = bits & 2;
                            t.still_on = bits & 4;
                            t.probe_on = bits & 8;
                            t.elide_on = bits & 16;
                            t.ppass_on = bits & 32;
                            t.twin_on = bits & 64;
                            t.sure_on = bits & 128;
                            // what init_common can produce
                            if (!t.act_on && (through || (bits & ~1))) continue;
                            if (t.pass_on && through < 1) continue;
                            if (t.elide_on && !t.pass_on) continue;
                            if (t.ppass_on && !t.probe_on) continue;
                            if (t.twin_on && !(t.ppass_on && t.pass_on)) continue;
                            if (t.sure_on && !t.twin_on) continue;
                            t.has_nb = t.has_own = t.has_ptab = t.one_seg = t.planes2 = t.units_fit = true;
                            t.timing_every = timing;
                            for (int d : kDepths) {
                                // hand-off row blocks nowhere / at depth K / at the depths below
                                t.hand[t.ndepth] = hands == 1 ? d == K : hands == 2 ? d < K : false;
                                t.depth[t.ndepth++] = d;
                            }
                            for (uint64_t gens = 1; gens <= 9 * (uint64_t)K - 1; ++gens) {
                                if (check(t, gens)) return 1;
                                ++cases;
                            }
                        }
    // an engine without activity state: no record touches it
    for (int K : kDepths) {
        StepTraits t;
        t.K = (uint32_t)K;
        for (int d : kDepths) t.depth[t.ndepth++] = d;
        for (uint64_t gens = 1; gens <= 9 * (uint64_t)K - 1; ++gens) {
            if (check(t, gens)) return 1;
            ++cases;
        }
    }
    std::printf("ok %llu\n", cases);
    return 0;
}
