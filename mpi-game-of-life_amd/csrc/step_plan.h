// step_plan.h -- the launches of a single-stream gol_step, as a pure function of what
// the engine decided at create and of the step's length (DESIGN §4 "The step's
// schedule").  Host only: no HIP call, no engine pointer.  launch() (engine.cpp) issues
// what a record says, step.cpp walks the records to run or capture a step and folds
// them into the fixed step's effect, and tests/step_plan_sweep.cpp holds them against
// a counter-driven walk: the schedule is the one statement of the step's policy.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace golh __attribute__((visibility("hidden"))) {

// The largest kernel depth of `list` (descending) that fits K and what remains.
inline uint32_t pick_depth(const int* list, int n, uint32_t K, uint64_t remaining)
{
    for (int i = 0; i < n; ++i)
        if ((uint32_t)list[i] <= K && (uint64_t)list[i] <= remaining) return (uint32_t)list[i];
    return 1;
}

// What is constant from step to step: decided at create, but for timing_every, which
// gol_set_timing writes here as well.  The per-depth entries follow the engine's kernel depth list.
struct StepTraits {
    static constexpr int kMaxDepths = 16;
    uint32_t K = 0;
    int npass = 1;  // plan 0's passes per full-depth launch
    int nbuf = 2;
    // the engine keeps activity state and steps alone (d_streak, nranks <= 1), d_err
    bool tracked = false, has_err = false;
    // gol_engine's switches
    bool act_on = false, pass_on = false, still_on = false, probe_on = false, elide_on = false,
         ppass_on = false, twin_on = false, sure_on = false;
    int through_on = 0;
    // plan 0: neighbour lists, copy-pass owners, a probe table, one segment; 2 word
    // planes; the state has a word for every unit
    bool has_nb = false, has_own = false, has_ptab = false, one_seg = false, planes2 = false,
         units_fit = false;
    uint32_t timing_every = 0;
    // per kernel depth: a launch of plan 0 at that depth runs hand-off row blocks /
    // takes the dev row shift
    int ndepth = 0;
    int depth[kMaxDepths] = {};
    bool hand[kMaxDepths] = {}, shift[kMaxDepths] = {};

    uint32_t pick(uint64_t remaining) const { return pick_depth(depth, ndepth, K, remaining); }
    // Passes of the next launch at depth d with `left` generations to go: multi-pass
    // plans run up to npass full-depth passes per launch.
    int passes(uint32_t d, uint64_t left) const
    {
        if (npass <= 1 || d != K) return 1;
        return (int)std::min<uint64_t>((uint64_t)npass, left / d);
    }
    // A launch at depth d may track activity, event timing aside: classic single-pass
    // blocks on two buffers (a hand-off launch leaves the activity state alone).
    bool plan_tracks(uint32_t d) const
    {
        bool h = false, s = false;
        for (int i = 0; i < ndepth; ++i)
            if ((uint32_t)depth[i] == d) h = hand[i], s = shift[i];
        return act_on && !h && has_nb && npass == 1 && nbuf == 2 && !s && units_fit;
    }
    bool tracks(uint32_t d) const { return !timing_every && plan_tracks(d); }
};

// Every kernel the fixed step stands for is in the step: every launch of every depth up
// to K tracks activity and every switch of the skip is on (twin_on stands for the
// passes and their tables).  What only the plan's geometry can say (every unit owns
// rows, every tile has an owner) is init_common's to check.
inline bool every_kernel_on(const StepTraits& t)
{
    bool all = t.tracked && t.twin_on && t.through_on >= 2 && t.elide_on && t.sure_on && t.one_seg;
    for (int i = 0; i < t.ndepth; ++i)
        if ((uint32_t)t.depth[i] <= t.K && !t.plan_tracks((uint32_t)t.depth[i])) all = false;
    return all;
}

// A short step's shape (DESIGN §4 "Short step"): a captured step (no event timing, at
// least 4K generations) of n >= 5 depth-K launches, n - 3 of which fit the span kernel's
// count, on an engine with the twin record, the one-load exit and the error word.
// Whether the step is short, or fixed, then hangs on what the host knows of the field.
inline bool short_shape(const StepTraits& t, uint64_t generations)
{
    if (t.K == 0 || t.pick(t.K) != t.K) return false;
    const uint64_t nK = generations / t.K;  // pick(): depth K while it fits
    return t.timing_every == 0 && t.twin_on && t.still_on && t.tracked && t.has_err &&
           t.npass <= 1 && nK >= 5 && nK - 3 <= 0xFFFFFFFFull;
}

// One launch of the step: what launch() passes to the stencil kernel and which kernels
// it issues around it.
struct StepLaunch {
    enum Kind { kUntracked, kDepthK, kRemainder };
    // ActState::twin after this launch: untouched; twin_ok cleared; written by the calm
    // kernel before the launch (with the copy pass or alone), twin_val for a calm unit;
    // held[] copied behind the launch
    enum Twin { kTwinNone, kTwinClear, kTwinCalm, kTwinHeld };
    uint32_t depth = 0;
    int passes = 1;
    uint64_t index = 0;  // within the step
    bool last = false;
    Kind kind = kUntracked;
    bool act = false;    // the kernel gets the counters (act[], copied[])
    int streak_in = -1;  // parity of the streaks the launch reads, -1: none
    bool streak_out = false;  // ... and writes those of the other parity
    bool no_hist = false, probe = false, held = false, busy = false;
    int through = 0;  // StepArgs::through: 2 = behind the copy pass
    int32_t launch_idx = 0;
    // the copy pass goes before this launch; it takes held[] / every calm unit's rows are
    // in its destination already; it counts what it leaves (copy elision)
    bool copy_pass = false, pass_held = false, pass_all = false, pass_elide = false;
    bool calm_alone = false;  // the calm kernel runs for twin[] alone
    // the probe pass goes before this launch; with the twin record; with sure tiles
    bool probe_pass = false, probe_twin = false, probe_sure = false;
    Twin twin = kTwinNone;
    uint32_t twin_val = 1;
    bool short_ok = false;  // the short graph may leave the stencil kernel out
};

// The step's launches, one at a time (a step of 2^32 launches allocates nothing).
// The streaks live within one step: its first launch carries no history, the parity
// alternates from there, and a launch at another depth (the remainder, always last)
// never skips and leaves the streaks alone: it reads the ones the last depth-K launch
// wrote, and only to copy still units through (its depths add up to less than K, so the
// lists, dilated by K, cover every one of them).
class StepSchedule {
public:
    StepSchedule(const StepTraits& t, uint64_t generations) : t_(t), left_(generations) {}

    bool next(StepLaunch* out)
    {
        if (left_ == 0) return false;
        StepLaunch& r = *out = StepLaunch{};
        r.depth = t_.pick(left_);
        r.passes = t_.passes(r.depth, left_);
        r.index = index_;
        r.last = left_ == (uint64_t)r.depth * (uint64_t)r.passes;
        r.act = t_.tracked;
        // Rows both buffers hold: a launch writes the field, so it clears
        // twin_ok unless it tracks activity, where the step's last launch decides.
        r.twin = t_.tracked && t_.twin_on ? StepLaunch::kTwinClear : StepLaunch::kTwinNone;
        bool pass = false;  // the launch wants the copy pass before it
        const bool may = t_.tracked && r.passes == 1 && t_.tracks(r.depth);
        if (may && r.depth == t_.K) {
            const int par = (int)(index_ & 1);
            r.kind = StepLaunch::kDepthK;
            r.streak_in = par;
            r.streak_out = true;
            r.no_hist = index_ == 0;
            r.probe = r.no_hist && t_.probe_on;
            // (copy elision) a first launch that probes writes every unit's flag
            r.held = r.probe && t_.elide_on;
            if (r.no_hist) probed_ = r.held;
            r.through = t_.through_on >= 1 ? 1 : 0;
            r.busy = t_.still_on;
            r.launch_idx = (int32_t)index_;
            hist_ = par ^ 1;
            // the step's second launch: its streaks are 0 or 1, no unit can skip
            pass = r.through && index_ == 1;
            r.pass_held = probed_;
            // the last launch: reading history, the calm kernel writes twin[] before
            // it; the step's only launch, which probes and writes held[] for every
            // unit: twin[] is held[], copied behind it; else the flag goes
            r.twin = !(t_.twin_on && r.last) ? StepLaunch::kTwinNone
                     : !r.no_hist            ? StepLaunch::kTwinCalm
                     : r.held                ? StepLaunch::kTwinHeld
                                             : StepLaunch::kTwinClear;
            // a launch the short step leaves out would have taken the one-load exit
            r.short_ok = r.busy && !r.no_hist && r.launch_idx >= 3;
        } else if (may && r.depth < t_.K && hist_ >= 0 && t_.through_on >= 2) {
            r.kind = StepLaunch::kRemainder;
            r.streak_in = hist_;
            r.through = 1;
            pass = true;  // a remainder launch never skips
            // the step's second launch: the first one's input is this one's output
            r.pass_held = probed_ && index_ == 1;
            // a later launch of the same remainder: the same streaks, the buffers
            // swapped, and every calm unit's rows went across (or were there) in the
            // launch before
            r.pass_all = rem_ > 0;
            ++rem_;
            r.twin = t_.twin_on && r.last ? StepLaunch::kTwinCalm : StepLaunch::kTwinNone;
            // Sure tiles: 2 only here, where fewer than K generations have
            // run since the streaks were written
            if (t_.sure_on) r.twin_val = 2;
        } else {
            hist_ = -1;
            probed_ = false;
        }
        // Copy pass (life_copy.hip): the calm units' rows, stored by a kernel of its own;
        // the launch's calm units then store no row (through = 2)
        r.copy_pass = pass && t_.pass_on && t_.has_own && t_.one_seg;
        if (r.copy_pass) r.through = 2;
        r.pass_elide = r.copy_pass && t_.elide_on;
        r.pass_held = r.pass_elide && r.pass_held;
        r.pass_all = r.pass_elide && r.pass_all;
        // ... and where the last launch takes no copy pass (a depth-K launch after the
        // step's second), the calm kernel runs for twin[] alone
        r.calm_alone = r.twin == StepLaunch::kTwinCalm && !r.copy_pass;
        // Probe pass (life_probe.hip): before a first launch that probes
        r.probe_pass = r.probe && t_.ppass_on && t_.has_ptab && t_.one_seg && t_.planes2;
        r.probe_twin = r.probe_pass && t_.twin_on && t_.has_own;
        r.probe_sure = r.probe_twin && t_.sure_on;
        left_ -= (uint64_t)r.depth * (uint64_t)r.passes;
        ++index_;
        return true;
    }

    // After a depth-K record with history and no copy pass: the launches ahead that
    // differ from it in index, launch_idx and parity only (depth K, not the step's
    // last).  Jumps over them and returns their number.
    uint64_t skip_alike()
    {
        if (hist_ < 0 || index_ < 3) return 0;  // (not after such a record)
        uint64_t n = left_ / t_.K;
        if (n && left_ % t_.K == 0) --n;
        left_ -= n * t_.K;
        index_ += n;
        if (n & 1) hist_ ^= 1;
        return n;
    }

private:
    const StepTraits& t_;
    uint64_t left_;
    uint64_t index_ = 0;
    int hist_ = -1;  // the streak parity the step's last depth-K launch wrote, -1: none
    bool probed_ = false;  // the step's first launch probed and wrote held[]
    int rem_ = 0;          // remainder launches issued so far
};

}  // namespace golh
