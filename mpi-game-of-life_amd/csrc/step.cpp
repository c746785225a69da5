// step.cpp -- the single-stream step of libgol.so (engine_internal.h): gol_step on an
// engine that steps alone, its launches taken from the schedule of step_plan.h and
// issued one by one or captured into a graph; the short step and the fixed step
//  with what gol_sync observes for them; pending fixed steps and their one
// kernel (still_pending.h, flush_still); the activity counters' getters.
#include "engine_internal.h"

namespace golh __attribute__((visibility("hidden"))) {

// The schedule's traits with every switch of the activity skip on, over a plan that
// takes every pass: what gol_plan_still_step describes.
static StepTraits all_on_traits(uint32_t K)
{
    StepTraits t;
    t.K = K;
    t.tracked = t.has_err = true;
    t.act_on = t.pass_on = t.still_on = t.probe_on = t.elide_on = t.ppass_on = t.twin_on = t.sure_on = true;
    t.through_on = 2;
    t.has_nb = t.has_own = t.has_ptab = t.one_seg = t.planes2 = t.units_fit = true;
    for (int d : gol::kDepthList) t.depth[t.ndepth++] = d;
    return t;
}

// Fixed step: what a step of `generations` generations does to the activity
// state when it starts with twin_ok == 1 and twin[u] == 2 for every unit, every switch
// of the activity skip on.  A fold over the step's schedule, the one launch() issues
// from: every unit goes the same way through every kernel, so one record serves all of
// them, and each launch's part is chosen by what its record says.  False: not a short
// step's shape, or a launch that a still unit's way above does not cover.
static bool still_effect(const StepTraits& t, uint64_t generations, gol_still_effect* out)
{
    gol_still_effect fx{};
    if (!short_shape(t, generations)) return false;
    StepSchedule sched(t, generations);
    StepLaunch r;
    while (sched.next(&r)) {
        uint32_t& in = r.streak_in == 0 ? fx.streak0 : fx.streak1;
        uint32_t& outw = r.streak_in == 0 ? fx.streak1 : fx.streak0;
        if (r.kind == StepLaunch::kDepthK && r.no_hist) {
            // No history, it probes (the step's first launch).  The probe pass before it
            // zeroes moved[] (life_probe.hip life_probe_zero_kernel); every owned tile
            // has owners with twin == 2 under twin_ok and takes the sure-tile exit,
            // which adds 1 to kept[tile] and to sure[tile] and touches nothing else
            // (life_probe.hip:89-95), so moved[] stays 0.
            if (!r.probe_pass || !r.probe_sure || !r.held || !r.busy) return false;
            fx.moved = 0;
            fx.kept_passes += 1;
            fx.sure_passes += 1;
            // The launch: every unit that goes on writes busy[1] = launch_idx + 1
            // (life_stencil.h:564), finds moved[unit] == 0 and takes the quiet exit
            // (:902-908): streak_out = min(0 + 1, cap), computed, probed and
            // pass_probed + 1, held = 1.
            fx.busy1 = (uint32_t)r.launch_idx + 1;
            outw = 1;
            fx.computed += 1;
            fx.probed += 1;
            fx.pass_probed += 1;
            fx.held = 1;
        } else if (r.kind == StepLaunch::kDepthK && r.copy_pass && r.pass_held && in == 1) {
            // Behind the copy pass, which takes held[] (the step's second launch).
            // life_calm_kernel: every list entry has a streak of 1, so calm and not
            // still; held[unit] is 1, so the destination holds the rows: need = 0,
            // elided + 1.  No tile has need: the tile kernel writes nothing.  The
            // launch: busy[1] is not below its index, the lists say calm, not still:
            // busy[1] = launch_idx + 1 (:564) and the copy-through exit with `through`
            // == 2 (:844-846): streak_out = 1 + 1, computed + 1, copied + 1.
            if (r.through != 2 || !r.pass_elide || fx.busy1 < (uint32_t)r.launch_idx) return false;
            fx.need = 0;
            fx.elided += 1;
            fx.busy1 = (uint32_t)r.launch_idx + 1;
            outw = in + 1;
            fx.computed += 1;
            fx.copied += 1;
        } else if (r.kind == StepLaunch::kDepthK && r.short_ok && fx.busy1 < (uint32_t)r.launch_idx) {
            // busy[1] below a launch_idx >= 3: the one-load exit (:540-543): busy[0] +
            // 1, no streak written (the short graph's span kernel adds them up in one
            // go).  The schedule still alternates the parity.  Before the step's last
            // launch life_calm_kernel runs alone (launch_twin_flags), calm on streaks
            // of 2 or 3, twin_val 1 (below).  Those that follow alike: all at once.
            if (r.copy_pass) return false;
            fx.busy0_add += 1;
            if (!r.last) {
                const uint64_t more = sched.skip_alike();
                fx.busy0_add += (uint32_t)more;
                fx.launches += more;
            }
        } else if (r.kind == StepLaunch::kDepthK && !r.copy_pass && in >= 2) {
            // busy[1] is not below the index; every list entry has a streak of 2: the
            // unit skips (:555-560), streak_out = 2 + 1, skipped + 1.  Nobody writes
            // busy[1] (the step's third launch).
            if (fx.busy1 < (uint32_t)r.launch_idx) return false;
            outw = in + 1;
            fx.skipped += 1;
        } else if (r.kind == StepLaunch::kRemainder && r.copy_pass && in >= 2) {
            // A remainder launch, behind the copy pass on the streaks the last depth-K
            // launch wrote (2 or 3 everywhere).  life_calm_kernel: calm and still, so
            // need = 0 and elided + 1 (from the second remainder launch on all_held
            // says the same and the tile kernel is left out); before the step's last
            // launch twin = 2 (sure tiles) and twin_ok = 1 (below).  The launch has no
            // busy[] and no streak_out: it neither takes the one-load exit nor skips,
            // and every unit copies through with `through` == 2 (:844-846): computed +
            // 1, copied + 1, no streak written.
            if (r.through != 2 || !r.pass_elide) return false;
            fx.need = 0;
            fx.elided += 1;
            fx.computed += 1;
            fx.copied += 1;
        } else {
            return false;
        }
        // the calm kernel before the step's last launch: every unit is calm
        if (r.twin == StepLaunch::kTwinCalm) {
            fx.twin = r.twin_val;
            fx.twin_ok = 1;
        } else if (r.twin != StepLaunch::kTwinNone) {
            return false;
        }
        fx.launches += 1;
    }
    *out = fx;
    return true;
}

// Pending fixed steps (still_pending.h) reach the device: life_still_step_kernel once,
// with the increments summed over the steps and the final values of the last one.  It
// repeats the proof on the state as the first pending step found it; where that fails
// it writes the error word alone, as each of the steps' kernels would have.  The
// record is cleared whether or not the kernel launches: a failure is the caller's to
// report, and what the host believed of twin[] goes with it.
gol_status flush_still_launch(gol_engine* e)
{
    const gol_still_effect fx = e->pending.fx;
    const bool any = e->pending.steps != 0;
    e->pending = StillPending{};
    if (!any) return GOL_OK;
    const ActState st{e->d_streak, (size_t)e->act_units};
    gol::StillArgs a{};
    a.streak0 = st.streak(0);
    a.streak1 = st.streak(1);
    a.act = st.act();
    a.copied = st.copied();
    a.busy = st.busy();
    a.probed = st.probed();
    a.need = st.need();
    a.held = st.held();
    a.elided = st.elided();
    a.moved = st.moved();
    a.pass_probed = st.pass_probed();
    a.twin = st.twin();
    a.twin_ok = st.twin_ok();
    a.err = e->d_err;
    a.total_units = (uint32_t)e->plans[0].total_units;
    a.act_units = (uint32_t)std::min<int64_t>(e->act_units, 0xFFFFFFFFll);
    a.computed = fx.computed;
    a.skipped = fx.skipped;
    a.n_copied = fx.copied;
    a.n_probed = fx.probed;
    a.n_pass_probed = fx.pass_probed;
    a.n_elided = fx.elided;
    a.busy0_add = fx.busy0_add;
    a.busy1 = fx.busy1;
    a.v_streak0 = fx.streak0;
    a.v_streak1 = fx.streak1;
    a.v_need = fx.need;
    a.v_held = fx.held;
    a.v_moved = fx.moved;
    a.v_twin = fx.twin;
    a.v_twin_ok = fx.twin_ok;
    const hipError_t he = gol::launch_still_step(a, e->stream);
    if (he != hipSuccess) {
        (void)twin_clear(e);
        return fail(GOL_EHIP, std::string("fixed step: the kernel did not launch: ") +
                                  hipGetErrorString(he));
    }
    ++e->fixed_launches;
    return GOL_OK;
}

// The step's launches in the schedule's order, on the engine's stream (issued, or
// captured by the caller).  shorty: the stencil kernels of the depth-K launches from
// index 3 on are left out, and one span kernel stands behind the first of them.
static gol_status issue_launches(gol_engine* e, const StepTraits& t, uint64_t generations, bool shorty)
{
    StepSchedule sched(t, generations);
    StepLaunch r;
    while (sched.next(&r)) {
        const bool skip = shorty && r.depth == e->K && r.index >= 3;
        GOL_TRY(launch(e, 0, r.depth, true, nullptr, r.passes, &r, skip));
        if (skip && r.index == 3) {
            const ActState as{e->d_streak, (size_t)e->act_units};
            const uint64_t nK = generations / (uint64_t)e->K;
            if (gol::launch_still_span(as.busy(), e->d_err, 3u, (uint32_t)(nK - 3), e->stream) !=
                hipSuccess)
                return fail(GOL_EHIP, "short step: the span kernel did not launch");
        }
    }
    return GOL_OK;
}

// Single-stream engines: the launch sequence of gol_step(gens) as a captured
// hipGraph, replayed from the second call on (LRU cache keyed by gens and the
// starting buffer).
static gol_status step_single_launches(gol_engine* e, uint64_t generations)
{
    const StepTraits& t = step_traits(e);
    const bool graphable = e->timing_every == 0 && generations >= 4 * (uint64_t)e->K;
    // Short step: the step has a short step's shape (step_plan.h) and the
    // host knows the field is a fixed point (still_seen; or GOL_DEV_SHORT_STEP=2).
    // Launch 1 takes the quiet exit, launch 2 is calm, launch 3 skips on the lists and
    // launches 4 .. n take the one-load exit: the short graph leaves those n - 3 stencil
    // kernels out and puts one node in their place.  The graph cache's key gains the bit.
    const bool shape = short_shape(t, generations);
    const bool shorty = shape && (e->short_on == 2 || (e->short_on == 1 && e->still_seen));
    // Fixed step: the short step's shape, and the host knows that twin[]
    // holds 2.  One kernel, launched directly (flush_still_launch): no capture, no graph.
    // It repeats the proof on the device; where that fails it writes nothing but the
    // error word, and the next gol_sync reports it (check_err).
    if (shape && ((e->fixed_on == 1 && e->short_on == 1 && e->still_seen && e->twin_two) ||
                  (e->fixed_on == 2 && e->rem_ended))) {
        // the effect is a function of the length alone: the last one is kept
        if (e->still_memo_gens != generations) {
            gol_still_effect one;
            if (!still_effect(t, generations, &one))
                return fail(GOL_ESTATE, "fixed step: not a short step's shape");
            e->still_memo = one;
            e->still_memo_gens = generations;
        }
        const gol_still_effect& fx = e->still_memo;
        // Pending steps (still_pending.h): the step's part on the device waits, folded
        // into the record, until somebody looks (flush_still); GOL_DEV_FIXED_DEFER=0:
        // at once, one kernel per step.  A kernel that does not launch leaves no step.
        e->pending = still_accumulate(e->pending, fx);
        if (!e->defer_on) GOL_TRY(flush_still_launch(e));
        // every launch swaps the buffers, which hold the same field
        e->cur = (int)(((uint64_t)e->cur + fx.launches) % (uint64_t)e->nbuf);
        ++e->short_steps;
        ++e->fixed_steps;
        e->fixed_passes += fx.kept_passes;  // (= sure_passes: one probe pass, all sure)
        e->twin_two = e->twin_two && fx.twin == 2;
        return GOL_OK;
    }
    // any other step's kernels read and write the activity state: pending fixed steps
    // go first, before a capture begins
    GOL_TRY(flush_still(e));
    // it keeps the host's word on twin[] only where it replays a short graph that ends
    // with a remainder launch, which writes the 2s again
    e->twin_two = e->twin_two && shorty && generations % (uint64_t)e->K != 0;
    if (graphable) {
        const auto key = std::make_pair(generations, e->cur | (shorty ? 0x100 : 0));
        auto it = e->graphs.find(key);
        if (it == e->graphs.end()) {
            if (e->graphs.size() >= kGraphCache) {
                auto lru = e->graphs.begin();
                for (auto j = e->graphs.begin(); j != e->graphs.end(); ++j)
                    if (j->second.used < lru->second.used) lru = j;
                HIP_TRY(hipStreamSynchronize(e->stream));
                (void)hipGraphExecDestroy(lru->second.exec);
                e->graphs.erase(lru);
            }
            hipGraph_t g = nullptr;
            HIP_TRY(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
            const int cur0 = e->cur;
            // the host flag as it stands: nothing issued while capturing touches the field
            const bool seen0 = e->still_seen, two0 = e->twin_two;
            const gol_status st = issue_launches(e, t, generations, shorty);
            e->still_seen = seen0;
            e->twin_two = two0;
            const hipError_t ce = hipStreamEndCapture(e->stream, &g);
            if (st != GOL_OK) {
                if (g) (void)hipGraphDestroy(g);
                e->cur = cur0;
                return st;
            }
            if (ce != hipSuccess) {
                e->cur = cur0;
                return fail(GOL_EHIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
            }
            hipGraphExec_t x = nullptr;
            const hipError_t ie = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (ie != hipSuccess) {
                e->cur = cur0;
                return fail(GOL_EHIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ie));
            }
            it = e->graphs.emplace(key, gol_engine::GraphEntry{x, e->cur, 0}).first;
            e->cur = cur0;
        }
        it->second.used = ++e->graph_clock;
        HIP_TRY(hipGraphLaunch(it->second.exec, e->stream));
        e->cur = it->second.cur_after;
        if (shorty) ++e->short_steps;
        return GOL_OK;
    }
    return issue_launches(e, t, generations, false);
}

gol_status step_single(gol_engine* e, uint64_t generations)
{
    if (e->res.on) return step_resident(e, generations);
    e->twin_fresh = true;  // (short step) twin[] may change: gol_sync looks again
    const gol_status st = step_single_launches(e, generations);
    // a step that failed half-way leaves no statement about the buffers
    if (st != GOL_OK) (void)twin_clear(e);
    // (fixed step, GOL_DEV_FIXED_STEP=2) depth-K launches, then a remainder launch
    e->rem_ended = st == GOL_OK && generations > (uint64_t)e->K && generations % (uint64_t)e->K != 0;
    return st;
}

// Short step, the observation: with the engine's stream idle, gol_sync
// reads twin[] and twin_ok (they lie one after the other, act_units + 1 words) where a
// step has run since it last looked.  twin_ok set and a 2 in every unit's word: every
// unit was calm in the remainder launch that ended the last step, so the whole field
// equals its generation before, and stays so until somebody writes it.  The words
// come into pinned memory together with the error word, behind the stream's work, so
// that gol_sync waits once and issues no blocking copy.
static bool observe_wanted(const gol_engine* e)
{
    // (fixed step) ... and where the field is known still but not that twin[] holds 2
    const bool news = !e->still_seen || (e->fixed_on == 1 && !e->twin_two);
    return e->short_on == 1 && e->sync_host && news && e->twin_fresh && e->d_streak &&
           !e->plans.empty() && e->plans[0].total_units > 0 &&
           e->plans[0].total_units <= e->act_units;
}

gol_status sync_observing(gol_engine* e)
{
    GOL_TRY(flush_still(e));  // pending fixed steps write the words copied below
    const ActState st{e->d_streak, (size_t)e->act_units};
    const bool look = observe_wanted(e);
    uint32_t* host = e->sync_host;
    host[0] = 0;
    HIP_TRY(hipMemcpyAsync(host, e->d_err, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    if (look)
        HIP_TRY(hipMemcpyAsync(host + 1, st.twin(), (st.units + 1) * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (host[0]) return check_err(e);
    if (!look) return GOL_OK;
    e->twin_fresh = false;
    const uint32_t* twin = host + 1;
    if (twin[st.units] == 0) return GOL_OK;
    const size_t units = (size_t)e->plans[0].total_units;
    for (size_t u = 0; u < units; ++u)
        if (twin[u] != 2u) return GOL_OK;
    e->still_seen = true;
    e->twin_two = true;  // (fixed step) until a step ends with a depth-K launch
    return GOL_OK;
}

// The activity counters of an engine, summed over its units (and over the parts
// of a composite engine), after everything issued on its stream has run.
struct ActTotals {
    uint64_t computed = 0, skipped = 0, copied = 0, probed = 0, elided = 0, pass_probed = 0;
    uint64_t pass_kept = 0;  // probe-pass tiles that left their rows (gol_engine::d_kept)
    uint64_t pass_sure = 0;  // ... of them, those that left before their field loads (d_sure)
};
static gol_status read_activity(gol_engine* e, ActTotals& t)
{
    if (e->inner) return read_activity(e->inner, t);
    for (auto* part : e->parts) GOL_TRY(read_activity(part, t));
    if (!e->parts.empty() || !e->d_streak) return GOL_OK;
    HIP_TRY(hipSetDevice(e->device));
    GOL_TRY(flush_still(e));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const ActState dev{e->d_streak, (size_t)e->act_units};
    std::vector<uint32_t> host(dev.words());
    HIP_TRY(hipMemcpy(host.data(), dev.base, host.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    const ActState st{host.data(), dev.units};
    for (size_t u = 0; u < st.units; ++u) {
        t.computed += st.act()[2 * u];
        t.skipped += st.act()[2 * u + 1];
        t.copied += st.copied()[u];
        t.probed += st.probed()[u];
        t.elided += st.elided()[u];
        t.pass_probed += st.pass_probed()[u];
    }
    // launches that every unit skipped at the one-load exit (only plan 0's
    // launches of a step ever skip)
    if (!e->plans.empty()) t.skipped += (uint64_t)st.busy()[0] * (uint64_t)e->plans[0].total_units;
    if (e->d_kept && e->kept_tiles > 0) {
        std::vector<uint32_t> kept((size_t)e->kept_tiles);
        HIP_TRY(hipMemcpy(kept.data(), e->d_kept, kept.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (uint32_t k : kept) t.pass_kept += k;
        if (e->d_sure) {
            HIP_TRY(hipMemcpy(kept.data(), e->d_sure, kept.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
            for (uint32_t k : kept) t.pass_sure += k;
        }
    }
    // (fixed step) its probe passes, each of which would have counted every owned tile
    // in both arrays
    t.pass_kept += e->fixed_passes * (uint64_t)e->owned_tiles;
    if (e->d_sure) t.pass_sure += e->fixed_passes * (uint64_t)e->owned_tiles;
    return GOL_OK;
}


// One or two of those totals for a getter of the C ABI.
static gol_status activity_total(gol_engine* e, uint64_t ActTotals::*m, uint64_t* out,
                                 uint64_t ActTotals::*m2 = nullptr, uint64_t* out2 = nullptr)
{
    if (!e) return fail(GOL_EINVAL, "null engine");
    ActTotals t;
    GOL_TRY(read_activity(e, t));
    if (out) *out = t.*m;
    if (m2 && out2) *out2 = t.*m2;
    return GOL_OK;
}

}  // namespace golh

extern "C" {

gol_status gol_activity(gol_engine* e, uint64_t* computed_units, uint64_t* skipped_units)
{
    return activity_total(e, &ActTotals::computed, computed_units, &ActTotals::skipped, skipped_units);
}

gol_status gol_activity_copied(gol_engine* e, uint64_t* copied_units)
{
    return activity_total(e, &ActTotals::copied, copied_units);
}

gol_status gol_activity_probed(gol_engine* e, uint64_t* probed_units)
{
    return activity_total(e, &ActTotals::probed, probed_units);
}

gol_status gol_activity_elided(gol_engine* e, uint64_t* elided_units)
{
    return activity_total(e, &ActTotals::elided, elided_units);
}

gol_status gol_activity_pass_probed(gol_engine* e, uint64_t* pass_probed_units)
{
    return activity_total(e, &ActTotals::pass_probed, pass_probed_units);
}

gol_status gol_activity_pass_kept(gol_engine* e, uint64_t* kept_tiles)
{
    return activity_total(e, &ActTotals::pass_kept, kept_tiles);
}

gol_status gol_activity_pass_sure(gol_engine* e, uint64_t* sure_tiles)
{
    return activity_total(e, &ActTotals::pass_sure, sure_tiles);
}

gol_status gol_activity_short_steps(gol_engine* e, uint64_t* steps)
{
    if (!e) return fail(GOL_EINVAL, "null engine");
    // a host count: torus, composite, rank, group and resident engines never arm it
    if (steps) *steps = (e->inner || !e->parts.empty()) ? 0 : e->short_steps;
    return GOL_OK;
}

gol_status gol_activity_fixed_steps(gol_engine* e, uint64_t* steps)
{
    if (!e) return fail(GOL_EINVAL, "null engine");
    // a host count, as gol_activity_short_steps
    if (steps) *steps = (e->inner || !e->parts.empty()) ? 0 : e->fixed_steps;
    return GOL_OK;
}

gol_status gol_activity_fixed_launches(gol_engine* e, uint64_t* launches)
{
    if (!e) return fail(GOL_EINVAL, "null engine");
    // a host count, as gol_activity_short_steps
    if (launches) *launches = (e->inner || !e->parts.empty()) ? 0 : e->fixed_launches;
    return GOL_OK;
}

gol_status gol_activity_state(gol_engine* e, uint32_t* out, size_t cap, size_t* words)
{
    if (!e) return fail(GOL_EINVAL, "null engine");
    if (e->inner || !e->parts.empty() || !e->d_streak)
        return fail(GOL_ESTATE, "the engine keeps no activity state");
    const ActState dev{e->d_streak, (size_t)e->act_units};
    if (words) *words = dev.words();
    if (!out) return GOL_OK;
    if (cap < dev.words()) return fail(GOL_EINVAL, "activity state: the buffer is too small");
    HIP_TRY(hipSetDevice(e->device));
    GOL_TRY(flush_still(e));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(out, dev.base, dev.words() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return GOL_OK;
}

gol_status gol_plan_still_step(uint32_t tb_depth, uint64_t generations, gol_still_effect* out)
{
    if (!out) return fail(GOL_EINVAL, "null argument");
    if (!still_effect(all_on_traits(tb_depth), generations, out))
        return fail(GOL_EINVAL, "not a short step: fewer than 5 launches of a kernel depth");
    return GOL_OK;
}

}  // extern "C"
