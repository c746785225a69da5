// still_pending.h -- fixed steps that have not reached the device yet (DESIGN §4 "Fixed
// step": pending steps).  Host only: no HIP call, no engine pointer.  A fixed step on a
// proven fixed point adds constants to the counter words and stores constants to the
// state words of the activity state, and two of them in a row do not interact: the
// second one's proof reads the 2s the first one stored, its increments add to the
// first one's and its state values overwrite them.  So a run of them is one
// gol_still_effect: the sums of the increments modulo 2^32, as the device words wrap,
// and the state values of the run's last step.  step.cpp keeps one such record per
// engine and launches life_still_step_kernel with it when somebody looks
// (flush_still); tests/still_pending_sweep.cpp holds the fold against applying the
// effects one by one to simulated words.
#pragma once

#include <cstdint>

#include "../../include/gol.h"

namespace golh __attribute__((visibility("hidden"))) {

struct StillPending {
    uint64_t steps = 0;   // fixed steps folded into fx; 0: nothing pending
    gol_still_effect fx;  // (meaningful while steps > 0)
};

// The record after one more fixed step with the effect `fx`.  Pure.  Increments add up
// in uint32_t, modulo 2^32; the final values are the new step's; `launches`, the
// stencil launches stood for, and the probe passes add up too (the host's books).
inline StillPending still_accumulate(const StillPending& p, const gol_still_effect& fx)
{
    StillPending q;
    q.steps = p.steps + 1;
    q.fx = fx;  // every final value: the last step's
    if (p.steps == 0) return q;
    q.fx.launches = p.fx.launches + fx.launches;
    q.fx.computed = p.fx.computed + fx.computed;
    q.fx.skipped = p.fx.skipped + fx.skipped;
    q.fx.copied = p.fx.copied + fx.copied;
    q.fx.probed = p.fx.probed + fx.probed;
    q.fx.pass_probed = p.fx.pass_probed + fx.pass_probed;
    q.fx.elided = p.fx.elided + fx.elided;
    q.fx.busy0_add = p.fx.busy0_add + fx.busy0_add;
    q.fx.kept_passes = p.fx.kept_passes + fx.kept_passes;
    q.fx.sure_passes = p.fx.sure_passes + fx.sure_passes;
    return q;
}

}  // namespace golh
