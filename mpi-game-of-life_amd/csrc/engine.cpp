// engine.cpp -- host side of libgol.so: the C ABI of include/gol.h.  This unit:
// engine lifecycle, load/store, the resident step, launches and timing, digests
// and plan queries; planning is plan.cpp, the single-stream step step.cpp, multi-GPU
// stripes stripes.cpp, torus engines torus.cpp (engine_internal.h).
//
// Owns device memory, the HIP streams, the halo transport (RCCL communicator,
// a caller's host transport, or device copies inside a group) and the launch
// plans.  Mirrors main()'s flow in Parallel_Life_MPI.cpp:190-240: create
// (readGridFromFile's allocation :88-89) -> load (:91-99) -> step (the epoch loop
// :215-221 with the halo exchange :104-145) -> store (:157-164).
#include "engine_internal.h"

namespace golh __attribute__((visibility("hidden"))) {

thread_local std::string g_last_error;

#if GOL_WAVE_LOG
uint64_t* g_dev_wave_log = nullptr;
#endif

}  // namespace golh

namespace golh __attribute__((visibility("hidden"))) {


gol_status check_cfg(const gol_config* cfg)
{
    if (!cfg) return fail(GOL_EINVAL, "null config");
    if (cfg->birth_mask >= 512 || cfg->survive_mask >= 512)
        return fail(GOL_EINVAL, "rule masks must be 9-bit");
    // (the resident kernel takes any epoch length K <= 63: resident = 2 with tb_depth)
    if (cfg->tb_depth != 0 && !(cfg->resident == 2 && cfg->tb_depth <= 63) &&
        std::find(std::begin(gol::kDepthList), std::end(gol::kDepthList),
                  (int)cfg->tb_depth) == std::end(gol::kDepthList))
        return fail(GOL_EINVAL, gol::kDevKernels
                                    ? "tb_depth must be 0 (auto) or one of 1,2,4,6,7,8,12,16,20,24,32"
                                    : "tb_depth must be 0 (auto) or one of 1,2,4,6,7,8,12,16 "
                                      "(20/24/32: dev build)");
    if (cfg->handoff > 2) return fail(GOL_EINVAL, "handoff must be 0 (auto), 1 (off) or 2 (on)");
    if (cfg->handoff == 2 && cfg->tb_depth != 0 && cfg->tb_depth < (uint32_t)gol::kHandoffMinDepth)
        return fail(GOL_EINVAL, "handoff on needs tb_depth >= 4");
    if (cfg->strip_lanes != 0 && cfg->strip_lanes != 64 && cfg->strip_lanes != 32 &&
        cfg->strip_lanes != 16)
        return fail(GOL_EINVAL, "strip_lanes must be 0 (auto), 64, 32 or 16");
    if (cfg->semantics > GOL_SEM_TORUS) return fail(GOL_EINVAL, "bad semantics");
    if (cfg->resident > 2) return fail(GOL_EINVAL, "resident must be 0 (auto), 1 (off) or 2 (on)");
    if (cfg->exchange_overlap > 2)
        return fail(GOL_EINVAL, "exchange_overlap must be 0 (auto), 1 (blocking) or 2 (overlapped)");
    if (cfg->word_planes != 0 && cfg->word_planes != 2 && cfg->word_planes != 4)
        return fail(GOL_EINVAL, "word_planes must be 0 (auto), 2 or 4");
    if (cfg->word_planes == 4 && !gol::kDevKernels)
        return fail(GOL_EINVAL, "word_planes 4 is built only in the dev library (make dev)");
    if (cfg->word_planes == 4 && cfg->tb_depth > 16)
        return fail(GOL_EINVAL, "word_planes 4 needs tb_depth <= 16");
    return GOL_OK;
}



// Kernels that wait for other wavefronts of their own launch -- hand-off row blocks
// (life_stencil.h) and the resident kernel -- need every wavefront they wait for
// to get a slot.  Their plans guarantee it for the launch alone on the device:
// hand-off launches are one round of the occupancy query (pick_rows_per_wave), the
// resident grid is at most one workgroup per CU (plan_resident).  Launches of
// other engines of this process would share the slots, so the process keeps, per
// device: at most one engine with hand-off blocks, and none while a resident engine
// lives (resident launches of several engines are ordered on one stream,
// resident_stream; classic blocks and composite parts never wait, so they may run
// beside either).  An engine that cannot get the kind it would plan runs classic
// blocks / the streaming kernel instead (gol_plan_handoff, gol_plan_resident
// report it).  GOL_DEV_SHARED_WAITS=1 turns the registry off (dev sweeps that
// step their engines one at a time).
struct WaitReg {
    gol_engine* hand = nullptr;
    int resident = 0;
};
std::mutex g_wait_mu;
std::map<int, WaitReg> g_wait_reg;

bool wait_registry_off()
{
    const char* v = std::getenv("GOL_DEV_SHARED_WAITS");
    return v && v[0] == '1';
}

void wait_release(gol_engine* e)
{
    if (!e->reg_hand && !e->reg_res) return;
    std::lock_guard<std::mutex> lock(g_wait_mu);
    WaitReg& r = g_wait_reg[e->device];
    if (e->reg_hand && r.hand == e) r.hand = nullptr;
    if (e->reg_res) r.resident--;
    e->reg_hand = e->reg_res = false;
}

// Host-side layout of an engine (no GPU): rule kind, depth and lane-group
// layout, row stride and the last group's mask.  Geometry (row0, R, Hx, rank)
// already set.
gol_status host_layout(gol_engine* e, uint64_t h, uint64_t w, const gol_config* cfg)
{
    e->H = h;
    e->W = w;
    e->wq = (w + 63) / 64;
    e->stride = (e->wq + 7) / 8 * 8;
    e->lastmask = last_mask(w);
    e->birth = cfg->birth_mask;
    e->survive = cfg->survive_mask;
    if (e->birth == GOL_REF_BIRTH && e->survive == GOL_REF_SURVIVE)
        e->rule = gol::RULE_REF;
    else if (e->birth == GOL_CONWAY_BIRTH && e->survive == GOL_CONWAY_SURVIVE)
        e->rule = gol::RULE_CONWAY;
    else
        e->rule = gol::RULE_GENERIC;
    const Layout lay = auto_layout(e->R, cfg);
    e->K = lay.K;
    e->rows_per_wave = cfg->rows_per_wave;
    e->lane_shift = cfg->strip_lanes == 64 ? 0 : cfg->strip_lanes == 32 ? 1
                  : cfg->strip_lanes == 16 ? 2 : -1;
    e->handoff = cfg->handoff;
    e->planes = lay.planes;
    if (!gol::life_has_kernel((int)e->K, e->planes))
        return fail(GOL_EINVAL, "no stencil kernel for this tb_depth / word_planes");
    {
        const uint64_t G = (uint64_t)e->planes / 2;
        e->ng = (e->wq + G - 1) / G;
        uint64_t c[2] = {0, 0};
        for (uint64_t j = 0; j < G; ++j) {
            const uint64_t idx = (e->ng - 1) * G + j;
            c[j] = idx + 1 < e->wq ? ~0ull : idx + 1 == e->wq ? e->lastmask : 0ull;
        }
        gol_split_group(c, e->lastmask_split, e->planes);
    }
    e->sem = cfg->semantics;
    return GOL_OK;
}

// The raw launch regions of an engine (host only): rank engines the round's
// regions (rank_geometry), REF_STRIPES the P independent stripes, GLOBAL the
// field; with the load/store row mappings.
gol_status raw_regions(gol_engine* e, uint64_t h, const gol_config* cfg, const RankGeom* geom,
                       std::vector<std::vector<SegDesc>>& raw)
{
    if (e->nranks > 1) {
        e->buf_rows = geom->buf_rows;
        e->overlap = geom->overlap;
        e->band_plans = geom->band;
        e->xchg_tune = geom->tune;
        raw = geom->raw;
        e->user_regions.push_back({e->Hx, e->row0, 0, e->R});
        e->load_regions = e->user_regions;
    } else if (e->sem == GOL_SEM_REF_STRIPES) {
        e->P = cfg->ref_ranks ? cfg->ref_ranks : 1;
        if (h / e->P == 0) return fail(GOL_EINVAL, "REF_STRIPES needs h >= ref_ranks");
        std::vector<SegDesc> segs;
        uint64_t base = 0;
        const uint64_t c = h / e->P;
        for (uint32_t r = 0; r < e->P; ++r) {
            uint64_t s0, n;
            ref_stripe(h, e->P, r, &s0, &n);
            SegDesc s{};
            s.base_row = (int64_t)base;
            s.in_rows = (int64_t)n;
            s.glob0 = 0;
            s.field_h = (int64_t)n;
            s.out_lo = 0;
            s.out_hi = (int64_t)n;
            segs.push_back(s);
            e->load_regions.push_back({base, s0, s0, n});
            // writeDataToFile (:149-175): own rows [r*c, (r+1)*c), last rank to h
            const uint64_t lo = r * c, hi = (r == e->P - 1) ? h : (r + 1) * c;
            e->user_regions.push_back({base + (lo - s0), lo, lo, hi - lo});
            base += n;
        }
        e->buf_rows = base;
        raw.push_back(segs);
    } else {
        e->buf_rows = h;
        SegDesc s{};
        s.base_row = 0;
        s.in_rows = (int64_t)h;
        s.glob0 = 0;
        s.field_h = (int64_t)h;
        s.out_lo = 0;
        s.out_hi = (int64_t)h;
        raw.push_back({s});
        e->user_regions.push_back({0, 0, 0, h});
        e->load_regions = e->user_regions;
    }
    return GOL_OK;
}

// Common construction; geometry (row0, R, Hx, rank) already set.
gol_status init_common(gol_engine* e, uint64_t h, uint64_t w, const gol_config* cfg,
                       const RankGeom* geom)
{
    GOL_TRY(host_layout(e, h, w, cfg));
    if (cfg->device >= 0) HIP_TRY(hipSetDevice(cfg->device));
    HIP_TRY(hipGetDevice(&e->device));
    HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    if (e->nranks > 1) {
        HIP_TRY(hipStreamCreateWithFlags(&e->comm_stream, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&e->band_stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&e->ev_band, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&e->ev_in, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&e->ev_xdone, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
    }

    std::vector<std::vector<SegDesc>> raw;
    GOL_TRY(raw_regions(e, h, cfg, geom, raw));

    const size_t words = (size_t)(e->buf_rows + 2 * gol::kGuardRows) * e->stride;
    decide_passes(e, words);
    // (r06 dev A/B) GOL_DEV_XCD_SHIFT = "c0c1...c7:m": speed class 0-3 of the
    // workgroups with blockIdx mod 8 == x, and the strip modulus m (life_stencil.h)
    if (const char* v = gol::kDevKernels ? std::getenv("GOL_DEV_XCD_SHIFT") : nullptr) {
        uint32_t code = 0;
        int i = 0;
        for (; i < 8 && v[i] >= '0' && v[i] <= '3'; ++i) code |= (uint32_t)(v[i] - '0') << (2 * i);
        const int m = (i == 8 && v[8] == ':') ? std::atoi(v + 9) : 0;
        if (m >= 1 && m <= 255) e->xcd_shift = code | ((uint32_t)m << 16);
    }
    const size_t halves = e->npass > 1 ? 2 : 1;
    e->nbuf = e->npass > 1 ? 4 : 2;
    e->shadow_off = e->npass > 1 ? (uint32_t)(words * sizeof(uint64_t)) : 0u;
    for (int b = 0; b < e->nbuf; ++b) {
        HIP_TRY(hipMalloc(&e->alloc[b], halves * words * sizeof(uint64_t)));
        HIP_TRY(hipMemsetAsync(e->alloc[b], 0, halves * words * sizeof(uint64_t), e->stream));
        e->buf[b] = e->alloc[b] + (size_t)gol::kGuardRows * e->stride;
    }
    HIP_TRY(hipMalloc(&e->d_acc, 2 * sizeof(unsigned long long)));
    HIP_TRY(hipMalloc(&e->d_flag, sizeof(int)));
    gol_status st = GOL_OK;
    {
        // plan and register under the lock, so that engines created by several
        // threads see each other (wait_release).  The registry entry covers every
        // candidate the autotuner may pick; the timing itself runs after the lock
        // is released (it takes tens of ms), and the entry is narrowed to the pick.
        std::lock_guard<std::mutex> lock(g_wait_mu);
        const bool off = wait_registry_off();
        const WaitReg reg = g_wait_reg[e->device];
        gol_config c = *cfg;
        if (!off && (reg.hand || reg.resident)) e->handoff = 1;
        if (!off && reg.hand) c.resident = 1;
        st = build_plans(e, raw);
        if (st == GOL_OK) st = plan_resident(e, &c);
        if (st == GOL_OK && !off) {
            WaitReg& r = g_wait_reg[e->device];
            if (e->res.on) {
                e->reg_res = true;
                r.resident++;
            } else {
                bool hand = false;
                for (const auto& pl : e->plans) hand |= (pl.hand && pl.multi_blk) || pl.npass > 1;
                for (const auto& alts : e->plan_alts)
                    for (const auto& pl : alts) hand |= (pl.hand && pl.multi_blk) || pl.npass > 1;
                if (hand && e->side[0]) {
                    e->reg_hand = true;
                    r.hand = e;
                }
            }
        }
    }
    if (st == GOL_OK) st = autotune_plans(e);
    if (st != GOL_OK) return st;
    resolve_aliases(e);
    if (e->reg_hand) {
        bool hand = false;
        for (const auto& pl : e->plans) hand |= (pl.hand && pl.multi_blk) || pl.npass > 1;
        if (!hand) {  // the autotuner picked classic blocks: free the device's entry
            std::lock_guard<std::mutex> lock(g_wait_mu);
            WaitReg& r = g_wait_reg[e->device];
            if (r.hand == e) r.hand = nullptr;
            e->reg_hand = false;
        }
    }
    // activity skip: engines of gol_create on one stream (e->act_on so far: the
    // caller allows it) whose plan has neighbour lists, i.e. classic single-pass
    // blocks; GOL_DEV_ACTIVITY_SKIP=0 turns it off (A/B runs, tests)
    {
        const char* v = std::getenv("GOL_DEV_ACTIVITY_SKIP");
        // (two field buffers: a skipped unit relies on launch m writing the buffer
        // launch m - 2 wrote, so an engine that may run multi-pass launches, with
        // its 4 rotating buffers, never skips, even on a plan that fell back to
        // single passes; nor one with the dev row shift, whose moved block
        // boundaries unit_rects does not model)
        e->act_on = e->act_on && !(v && std::atoi(v) == 0) && !e->res.on && e->d_streak &&
                    !e->plans.empty() && e->plans[0].d_nb && !e->shared_device && !e->grouped &&
                    e->nbuf == 2 && e->npass <= 1 && !e->xcd_shift;
        // copy-through of still units (GOL_DEV_COPY_THROUGH: 0 = off, 1 = in the
        // depth-K launches only, default: in the remainder launches too) and the
        // one-load exit of a launch after a wholly skipped one
        // (GOL_DEV_STILL_EXIT=0 = off); neither touches the skip itself
        const char* t = std::getenv("GOL_DEV_COPY_THROUGH");
        e->through_on = !e->act_on ? 0 : !t ? 2 : std::max(0, std::min(2, std::atoi(t)));
        const char* x = std::getenv("GOL_DEV_STILL_EXIT");
        e->still_on = e->act_on && !(x && std::atoi(x) == 0);
        // the copy pass: where copy-through is on, its rows move in a kernel of
        // their own before a step's second launch and before its remainder launches
        // (GOL_DEV_COPY_PASS=0 = off: the stencil kernel's copy loop, as before)
        const char* cp = std::getenv("GOL_DEV_COPY_PASS");
        e->pass_on = e->through_on >= 1 && !(cp && std::atoi(cp) == 0);
        // the still probe of a step's first launch (GOL_DEV_STILL_PROBE=0 = off)
        const char* pr = std::getenv("GOL_DEV_STILL_PROBE");
        e->probe_on = e->act_on && !(pr && std::atoi(pr) == 0);
        // copy elision: the pass leaves the rows its destination already holds
        // (GOL_DEV_COPY_ELIDE=0 = off: the pass copies every calm unit, as before)
        const char* el = std::getenv("GOL_DEV_COPY_ELIDE");
        e->elide_on = e->pass_on && !(el && std::atoi(el) == 0);
        // the probe pass: the first launch's still probe, run tile by tile in a kernel
        // of its own before it (GOL_DEV_PROBE_PASS=0 = off: the in-kernel probe alone)
        const char* pp = std::getenv("GOL_DEV_PROBE_PASS");
        e->ppass_on = e->probe_on && !(pp && std::atoi(pp) == 0);
        // rows both buffers hold: the probe pass stores no tile whose rows the other
        // buffer holds already, on the word of the copy pass's calm kernel before the
        // last launch of the step before (GOL_DEV_TWIN=0 = off: every tile without a
        // difference stores, as in r12).  One counter word per tile of the pass.
        const char* tw = std::getenv("GOL_DEV_TWIN");
        e->twin_on = e->ppass_on && e->pass_on && !(tw && std::atoi(tw) == 0);  // (act_on: a plan)
        if (e->twin_on) {
            const auto& p0 = e->plans[0];
            e->twin_on = p0.d_own && p0.d_ptab && e->planes == 2 &&
                         p0.owners.size() / gol::kCopyOwners ==
                             p0.probe_tiles.size() / gol::kProbeSlots;
        }
        if (e->twin_on) {
            const auto& p0 = e->plans[0];
            e->kept_tiles = (int64_t)(p0.owners.size() / gol::kCopyOwners);
            HIP_TRY(hipMalloc(&e->d_kept, (size_t)e->kept_tiles * sizeof(uint32_t)));
            HIP_TRY(hipMemsetAsync(e->d_kept, 0, (size_t)e->kept_tiles * sizeof(uint32_t), e->stream));
            // sure tiles: a tile whose owners a remainder launch proved still leaves
            // before its field loads (GOL_DEV_TWIN_SURE=0 = off: twin is 0 or 1 and
            // every kept tile loads, as in r13).  One more counter word per tile.
            const char* su = std::getenv("GOL_DEV_TWIN_SURE");
            e->sure_on = !(su && std::atoi(su) == 0);
            if (e->sure_on) {
                HIP_TRY(hipMalloc(&e->d_sure, (size_t)e->kept_tiles * sizeof(uint32_t)));
                HIP_TRY(hipMemsetAsync(e->d_sure, 0, (size_t)e->kept_tiles * sizeof(uint32_t), e->stream));
            }
            // short step: once gol_sync has seen every unit's twin at 2, a captured step
            // leaves out the depth-K launches from the fourth on (GOL_DEV_SHORT_STEP=0 =
            // off; 2 = without having seen it, for the error-code test).  It stands on
            // the one-load exit, whose test its one node repeats, and on the 2s.
            const char* ss = std::getenv("GOL_DEV_SHORT_STEP");
            const int sv = ss ? std::atoi(ss) : 1;
            e->short_on = !e->still_on ? 0 : sv == 2 ? 2 : (sv != 0 && e->sure_on) ? 1 : 0;
            // gol_sync's look: the error word, twin[] and twin_ok, pinned
            if (e->short_on == 1)
                HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&e->sync_host),
                                      ((size_t)e->act_units + 2) * sizeof(uint32_t), hipHostMallocDefault));
            // fixed step: one kernel for the whole step (GOL_DEV_FIXED_STEP=0 = off; 2 =
            // unseen, for the error-status test).  It stands for the kernels of a step
            // in which every one of these is on, over a plan whose launches all track
            // activity, whose units all own rows and whose tiles all have an owner:
            // anything else keeps the short graph.
            const char* fx = std::getenv("GOL_DEV_FIXED_STEP");
            const int fv = fx ? std::atoi(fx) : 1;
            bool whole = e->short_on != 0 && every_kernel_on(step_traits(e)) &&
                         p0.total_units > 0 && p0.total_units <= 0xFFFFFFFFll;
            if (whole) {
                // every unit owns rows (life_stencil.h: a unit without rows neither
                // probes nor writes held = 1) ...
                std::vector<URect> rc;
                unit_rects(p0, (int64_t)e->ng, rc);
                for (int64_t u = 0; u < p0.total_units; ++u)
                    if (rc[(size_t)(2 * u)].r1 <= rc[(size_t)(2 * u)].r0) whole = false;
                // ... and every tile with a row has an owner (life_probe.hip: a tile
                // without one is no twin tile, and would load and store its rows)
                const SegDesc& sg = p0.segs[0];
                int64_t owned = 0;
                for (int64_t t = 0; t < e->kept_tiles; ++t) {
                    const int64_t rb = sg.out_lo + t / p0.copy_ncol * gol::kCopyTileRows;
                    bool own = false;
                    for (int k = 0; k < gol::kCopyOwners; ++k)
                        own = own || (int64_t)p0.owners[(size_t)(t * gol::kCopyOwners + k)] < p0.total_units;
                    if (rb >= 0 && rb < sg.out_hi && own) ++owned;
                }
                e->owned_tiles = owned;
                if (sg.out_lo < 0 || owned != e->kept_tiles) whole = false;
            }
            e->fixed_on = !whole ? 0 : fv == 2 ? 2 : (fv != 0 && e->short_on == 1) ? 1 : 0;
            // pending fixed steps: the kernel waits for the next look at the state
            // (GOL_DEV_FIXED_DEFER=0 = off: one kernel per fixed step)
            const char* fd = std::getenv("GOL_DEV_FIXED_DEFER");
            e->defer_on = e->fixed_on != 0 && !(fd && std::atoi(fd) == 0);
        }
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    return GOL_OK;
}

gol_status flush_timing(gol_engine* e)
{
    for (size_t i = 0; i < e->ev_pending.size(); ++i) {
        auto& p = e->ev_pending[i];
        HIP_TRY(hipEventSynchronize(p.second));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, p.first, p.second));
        e->tm.launches += 1;
        e->tm.kernel_ms += ms;
        e->tm.cell_gens += e->pending_cells[i];
        e->tm.cell_gens_computed += e->pending_cells_comp[i];
        e->tm.launch_rows += e->pending_rows[i];
        e->ev_free.push_back(p.first);
        e->ev_free.push_back(p.second);
    }
    // an overlapped exchange is exposed for the part that ends after its round's
    // compute span (the next round's launches wait for it); a blocking one sits
    // between two rounds on the compute stream, all of it exposed
    std::map<hipEvent_t, float> round_end_to_xend;
    for (auto& r : e->ev_rpending) {
        HIP_TRY(hipEventSynchronize(r.end));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, r.start, r.end));
        e->tm.rounds += 1;
        e->tm.round_ms += ms;
        if (r.xend) {
            HIP_TRY(hipEventSynchronize(r.xend));
            float tail = 0.f;
            HIP_TRY(hipEventElapsedTime(&tail, r.end, r.xend));
            round_end_to_xend[r.xend] = tail;
        }
        e->ev_free.push_back(r.start);
        e->ev_free.push_back(r.end);
    }
    for (size_t i = 0; i < e->ev_xpending.size(); ++i) {
        auto& p = e->ev_xpending[i];
        HIP_TRY(hipEventSynchronize(p.second));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, p.first, p.second));
        e->tm.exchanges += 1;
        e->tm.exchange_ms += ms;
        float exposed = ms;
        if (!e->xpending_blocking[i]) {
            auto it = round_end_to_xend.find(p.second);
            exposed = it == round_end_to_xend.end() ? ms : std::min(ms, std::max(0.f, it->second));
        }
        e->tm.exchange_exposed_ms += exposed;
        e->ev_free.push_back(p.first);
        e->ev_free.push_back(p.second);
    }
    e->ev_pending.clear();
    e->ev_xpending.clear();
    e->xpending_blocking.clear();
    e->ev_rpending.clear();
    e->pending_cells.clear();
    e->pending_cells_comp.clear();
    e->pending_rows.clear();
    return GOL_OK;
}

gol_status get_event(gol_engine* e, hipEvent_t* ev)
{
    if (e->ev_free.empty()) {
        HIP_TRY(hipEventCreate(ev));
        return GOL_OK;
    }
    *ev = e->ev_free.back();
    e->ev_free.pop_back();
    return GOL_OK;
}

// HIP events around every `timing_every`-th kernel launch (gol_set_timing).
gol_status timing_begin(gol_engine* e, hipStream_t s, hipEvent_t* e0, hipEvent_t* e1)
{
    *e0 = *e1 = nullptr;
    if (e->timing_every) e->tm.launches_issued += 1;
    if (!e->timing_every || (e->launch_count++ % e->timing_every) != 0) return GOL_OK;
    GOL_TRY(get_event(e, e0));
    GOL_TRY(get_event(e, e1));
    HIP_TRY(hipEventRecord(*e0, s));
    return GOL_OK;
}

gol_status timing_end(gol_engine* e, hipStream_t s, hipEvent_t e0, hipEvent_t e1, double own,
                      double computed, double rows = 0)
{
    if (!e0) return GOL_OK;
    HIP_TRY(hipEventRecord(e1, s));
    e->ev_pending.push_back({e0, e1});
    e->pending_cells.push_back(own);
    e->pending_cells_comp.push_back(computed);
    e->pending_rows.push_back(rows);
    return GOL_OK;
}

// Resident plan: tiles of `band_rows` rows x one 64-lane strip, one 1024-thread
// workgroup each (at most one per CU: every workgroup of the launch must be
// resident at once, since tiles wait for their neighbours), each wavefront
// holding `rows` rows, so a tile holds 16 rows >= band + 2K halo rows.  Cost per
// generation, in us, fitted to 12 (rows, K, band) shapes at 4096^2
// (profiles/r02/c2_resident_sweep.jsonl, within 8%): 0.17 + 0.046 (B + K) / 16
// (the rows still exact, averaged over an epoch, per wavefront) + 0.068 rows
// (barrier, LDS edge exchange, per-row fixed work) + 3.3 / K (the epoch hand-off:
// publish, flag, neighbour wait, halo reload).
gol_status plan_resident(gol_engine* e, const gol_config* cfg)
{
    if (cfg->resident == 1 || e->nranks > 1 || e->sem != GOL_SEM_GLOBAL || e->planes != 2)
        return GOL_OK;
    const bool knobs = cfg->tb_depth || cfg->rows_per_wave || cfg->handoff || cfg->strip_lanes ||
                       cfg->word_planes;
    if (cfg->resident == 0 && knobs) return GOL_OK;
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device));
    const int64_t strips = e->ng <= 64 ? 1 : ((int64_t)e->ng + 61) / 62;
    if (strips > cus) return GOL_OK;
    const int64_t h = (int64_t)e->H;
    double best = 1e300;
    for (int M : gol::kResRowsList) {
        if (cfg->resident == 2 && cfg->rows_per_wave && (uint32_t)M != cfg->rows_per_wave) continue;
        if (gol::resident_blocks_per_cu(M, e->rule) < 1) continue;
        // the generic-mask rule keeps 8 rows per wavefront only with spills
        if (e->rule == gol::RULE_GENERIC && M > 6 && cfg->rows_per_wave != (uint32_t)M) continue;
        const int64_t NR = (int64_t)gol::kResWaves * M;
        const int64_t max_bands = std::min<int64_t>(cus / strips, h);
        for (int64_t nb = 1; nb <= max_bands; ++nb) {
            const int64_t B = (h + nb - 1) / nb;
            const int64_t bands = (h + B - 1) / B;
            int64_t kmax = (NR - B) / 2;
            if (strips > 1) kmax = std::min<int64_t>(kmax, 63);
            int64_t K = (cfg->resident == 2 && cfg->tb_depth) ? (int64_t)cfg->tb_depth : kmax;
            if (K < 1 || K > kmax || (cfg->resident == 0 && K < 8)) continue;
            const int64_t span = (K + B - 1) / B;  // bands a K-row halo reaches
            if ((2 * span + 1) * (strips > 1 ? 3 : 1) - 1 > 64) continue;
            const double cost = 0.17 + 0.046 * (double)(B + K) / gol::kResWaves + 0.068 * M +
                                3.3 / (double)K;
            if (cost < best * 0.999) {
                best = cost;
                e->res.rows = M;
                e->res.strips = (int32_t)strips;
                e->res.bands = (int32_t)bands;
                e->res.band_rows = (int32_t)B;
                e->res.K = (int32_t)K;
            }
        }
    }
    if (best >= 1e300) {
        if (cfg->resident == 2 && (cfg->tb_depth || cfg->rows_per_wave))
            return fail(GOL_EINVAL, "resident: the field does not fit with this tb_depth / rows_per_wave");
        return GOL_OK;
    }
    const size_t tiles = (size_t)e->res.bands * (size_t)e->res.strips;
    HIP_TRY(hipMalloc(&e->res.flags, tiles * sizeof(uint32_t)));
    HIP_TRY(hipMemset(e->res.flags, 0, tiles * sizeof(uint32_t)));
    HIP_TRY(hipEventCreateWithFlags(&e->res.ev_in, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&e->res.ev_out, hipEventDisableTiming));
    e->res.on = true;
    {
        const char* v = std::getenv("GOL_DEV_RES_COOP");
        e->res.coop = v && std::atoi(v) == 1;
    }
#if GOL_DEV_KERNELS
    // dev build: the wave-level temporal blocking of life_resident_mb.hip (r06,
    // measured slower at every MB: DESIGN §4)
    if (const char* v = std::getenv("GOL_DEV_RES_MB")) {
        const int mb = std::atoi(v);
        if (mb >= 2 && gol::resident_mb_exists(e->res.rows, mb, e->rule) &&
            gol::resident_mb_blocks_per_cu(e->res.rows, mb, e->rule) >= 1)
            e->res.mb = mb;
    }
#endif
    e->K = (uint32_t)e->res.K;
    return GOL_OK;
}

// The resident launches of every engine of this process on one device run on one
// shared stream, in order: each needs all its tiles resident at once, one per CU,
// so two side by side could each hold CUs the other's tiles wait for.  (Engines
// of different processes on one GPU are not ordered: their resident waits are
// bounded and a timeout is reported by gol_sync.)
hipStream_t resident_stream(int device)
{
    static std::mutex mu;
    static std::map<int, hipStream_t> streams;
    std::lock_guard<std::mutex> lock(mu);
    auto it = streams.find(device);
    if (it != streams.end()) return it->second;
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
    streams[device] = s;
    return s;
}

// gol_step on a resident engine: one launch (per 2^30 generations).
gol_status step_resident(gol_engine* e, uint64_t generations)
{
    auto& r = e->res;
    hipStream_t rs = resident_stream(e->device);
    if (!rs) return fail(GOL_EHIP, "resident launch stream");
    HIP_TRY(hipEventRecord(r.ev_in, e->stream));
    HIP_TRY(hipStreamWaitEvent(rs, r.ev_in, 0));
    uint64_t left = generations;
    while (left > 0) {
        const int32_t g = (int32_t)std::min<uint64_t>(left, 1u << 30);
        gol::ResArgs a{};
        a.buf0 = e->buf[e->cur];
        a.buf1 = e->buf[e->cur ^ 1];
        a.flags = r.flags;
        a.err = e->d_err;
        a.stride = (int64_t)e->stride;
        a.h = (int64_t)e->H;
        a.ng = (int64_t)e->ng;
        a.lastmask = e->lastmask_split[0];
        a.strips = r.strips;
        a.bands = r.bands;
        a.band_rows = r.band_rows;
        a.K = r.K;
        a.span = (r.K + r.band_rows - 1) / r.band_rows;
        a.gens = g;
        a.flag_base = r.flag_base;
        a.birth = e->birth;
        a.survive = e->survive;
#if GOL_WAVE_LOG
        a.wlog = g_dev_wave_log;
#endif
        hipEvent_t e0, e1;
        GOL_TRY(timing_begin(e, rs, &e0, &e1));
#if GOL_DEV_KERNELS
        if (r.mb > 1)
            HIP_TRY(gol::launch_resident_mb(a, r.rows, r.mb, e->rule, r.bands * r.strips, rs));
        else
#endif
            HIP_TRY(gol::launch_resident(a, r.rows, e->rule, r.bands * r.strips, rs, r.coop));
        // lanes process every held row of every tile, every generation (wave-level
        // blocking: rows + mb - 1 per generation on average over a super-step)
        const double comp = (double)g * r.bands * r.strips * gol::kResWaves * (r.rows + r.mb - 1) *
                            64.0 * 64.0;
        GOL_TRY(timing_end(e, rs, e0, e1, (double)e->H * (double)e->W * g, comp));
        const uint32_t epochs = (uint32_t)((g + r.K - 1) / r.K);
        r.flag_base += epochs;
        if (epochs & 1) e->cur ^= 1;
        left -= (uint64_t)g;
    }
    HIP_TRY(hipEventRecord(r.ev_out, rs));
    HIP_TRY(hipStreamWaitEvent(e->stream, r.ev_out, 0));
    return GOL_OK;
}

// A launch of plan `p` at `depth` on the stream of `region` runs hand-off row blocks.
static bool launch_hands(const gol_engine* e, const gol_engine::Plan& p, int region, uint32_t depth)
{
    return p.hand && p.multi_blk && e->side[region] && handoff_fits(p.rpw, (int)depth, e->planes) &&
           gol::handoff_kernel_exists((int)depth, e->rule);
}

// (r06 dev A/B, GOL_DEV_XCD_SHIFT) per-XCD row shift between paired blocks: blocks
// keep >= the length their closure needs after giving up 8 rows
static bool launch_shifts(const gol_engine* e, const gol_engine::Plan& p, bool hand, uint32_t depth)
{
    if (!e->xcd_shift || p.segs.size() != 1) return false;
    const int64_t shortest = p.rows_old ? std::min<int64_t>(p.rows_old, p.rows_young) : p.rpw;
    return hand ? handoff_fits(shortest - 8, (int)depth, e->planes) : shortest - 8 >= 2;
}

// What the step's schedule (step_plan.h) reads of the engine and of plan 0.
const StepTraits& step_traits(gol_engine* e)
{
    if (e->traits_ok) return e->traits;
    StepTraits t;
    t.K = e->K;
    t.nbuf = e->nbuf;
    t.tracked = e->d_streak && e->nranks <= 1;
    t.has_err = e->d_err != nullptr;
    t.act_on = e->act_on;
    t.through_on = e->through_on;
    t.pass_on = e->pass_on;
    t.still_on = e->still_on;
    t.probe_on = e->probe_on;
    t.elide_on = e->elide_on;
    t.ppass_on = e->ppass_on;
    t.twin_on = e->twin_on;
    t.sure_on = e->sure_on;
    t.timing_every = e->timing_every;
    t.planes2 = e->planes == 2;
    static_assert(std::size(gol::kDepthList) <= (size_t)StepTraits::kMaxDepths, "depth list");
    for (int d : gol::kDepthList) t.depth[t.ndepth++] = d;
    if (!e->plans.empty()) {
        const auto& p = e->plans[0];
        t.npass = p.npass;
        t.has_nb = p.d_nb != nullptr;
        t.has_own = p.d_own != nullptr;
        t.has_ptab = p.d_ptab != nullptr;
        t.one_seg = p.segs.size() == 1;
        t.units_fit = p.total_units <= e->act_units;
        for (int i = 0; i < t.ndepth; ++i) {
            t.hand[i] = launch_hands(e, p, 0, (uint32_t)t.depth[i]);
            t.shift[i] = launch_shifts(e, p, t.hand[i], (uint32_t)t.depth[i]);
        }
    }
    e->traits = t;
    e->traits_ok = true;
    return e->traits;
}

// The arguments every stencil launch takes, whoever issues it.
static gol_status fill_step_args(const gol_engine* e, const gol_engine::Plan& p, uint32_t depth,
                                 int passes, int region, bool hand, StepArgs& a)
{
    for (int i = 0; i <= passes; ++i) a.pbuf[i] = e->buf[(e->cur + i) % e->nbuf];
    a.npass = passes;
    a.shadow_off = e->shadow_off;
    a.mpflags = e->mpflags;
    a.err = e->d_err;
    a.segs = p.dev;
    a.nseg = (int32_t)p.segs.size() + (p.pair_units ? 1 : 0);
    if (p.segs.size() == 1) {
        a.seg0_only = 1;
        a.seg0 = p.segs[0];
    }
    a.strips = p.groups;
    a.lane_shift = p.lane_shift;
    a.stride = (int64_t)e->stride;
    a.ng = (int64_t)e->ng;
    a.lastmask[0] = e->lastmask_split[0];  // the kernel works on stored (split) words
    a.lastmask[1] = e->lastmask_split[1];
    a.rows_per_wave = p.rpw;
    a.total_units = p.total_units;
    a.birth = e->birth;
    a.survive = e->survive;
    if (hand) {
        a.side = e->side[region];
        a.flags = e->flags[region];
        a.side_slot = (int64_t)2 * (depth - 1) * 64 * (e->planes / 2);
        a.tail_off = gol::handoff_toff(p.rpw, (int)depth, e->planes);
        // The pair forms (life_stencil.h stage_rm) take a step's pair parity from
        // its unrolled index, which holds only while a consumer's tail starts at an
        // even step t_side = R + 2: every hand-off block length must be even.
        if ((p.rpw & 1) || (p.rows_old && ((p.rows_old | p.rows_young) & 1)))
            return fail(GOL_ESTATE, "hand-off plan with an odd block length");
    }
    if (p.rows_old) {
        a.rows_per_wave = p.rows_young;
        a.rows_old = p.rows_old;
        a.units_old = p.units_old;
    }
    if (launch_shifts(e, p, hand, depth)) a.xcd_shift = e->xcd_shift;
    a.edge = p.edge;
    a.right_q0 = p.right_q0;
    a.half_q0 = p.half_q0;
    a.half_hi = p.half_hi;
    a.pair_units = p.pair_units;
    a.pair0 = p.total_units - p.pair_units;
    a.pairs = p.dpairs;
#if GOL_WAVE_LOG
    a.wlog = g_dev_wave_log;
#endif
    return GOL_OK;
}

// ... and what a launch of a single-stream step does with the activity state, as its
// record says.
static void fill_activity_args(const gol_engine* e, const gol_engine::Plan& p, const StepLaunch& r,
                               StepArgs& a)
{
    if (!r.act) return;
    const ActState st{e->d_streak, (size_t)e->act_units};
    a.act = st.act();
    a.copied = st.copied();
    if (r.streak_in < 0) return;
    a.streak_in = st.streak(r.streak_in);
    a.nb_off = p.d_nb;
    a.nb_ids = p.d_nb + p.nb_off.size();
    if (r.streak_out) {
        a.streak_out = st.streak(r.streak_in ^ 1);
        a.probed = st.probed();
    }
    a.no_hist = r.no_hist ? 1 : 0;
    a.probe = r.probe ? 1 : 0;
    a.held = r.held ? st.held() : nullptr;
    a.through = r.through;
    a.busy = r.busy ? st.busy() : nullptr;
    a.launch_idx = r.launch_idx;
}

// The tile grid of plan p's one segment, which the copy pass and the probe pass share.
template <class Args>
static void fill_tile_args(const gol_engine* e, const gol_engine::Plan& p, const StepArgs& a,
                           size_t ntile, Args& c)
{
    const SegDesc& sg = p.segs[0];
    c.src = a.pbuf[0];
    c.dst = a.pbuf[1];
    c.stride = a.stride;
    c.base_row = sg.base_row;
    c.lastmask = e->lastmask_split[0];
    c.ntile = (int32_t)ntile;
    c.ncol = p.copy_ncol;
    c.total_units = (int32_t)p.total_units;
    c.out_lo = (int32_t)sg.out_lo;
    c.out_hi = (int32_t)sg.out_hi;
    c.ng = (int32_t)e->ng;
    c.vlo = (int32_t)std::max<int64_t>(0, -sg.glob0);
    c.vhi = (int32_t)std::max<int64_t>(0, std::min(sg.in_rows, sg.field_h - sg.glob0));
}

// Copy pass (life_copy.hip): the calm units' rows, stored by a kernel of its
// own on this stream (captured into the step's graph with the launch); the launch's
// calm units then store no row (through = 2).  Both read the same streaks, which
// neither writes before the launch's units have read them.
static gol_status issue_copy_pass(gol_engine* e, const gol_engine::Plan& p, const StepLaunch& r,
                                  const StepArgs& a, hipStream_t s)
{
    // The pass writes whole tiles, words of units that are not calm among them.
    // That is safe only where every such unit stores its whole rectangle in
    // the launch that follows: no unit of it may skip.  A remainder launch
    // writes no streaks and never skips; a depth-K launch skips on streaks >= 2,
    // which the step's second launch cannot see (the first wrote 0 or 1).
    const bool none_skips = !a.streak_out || (a.launch_idx == 1 && !a.no_hist);
    if (!none_skips || !a.streak_in || a.through != 2 || !p.d_own || s != e->stream ||
        p.segs.size() != 1)
        return fail(GOL_ESTATE, "copy pass before a launch whose units may skip");
    const ActState st{e->d_streak, (size_t)e->act_units};
    gol::CopyArgs c{};
    fill_tile_args(e, p, a, p.owners.size() / gol::kCopyOwners, c);
    c.owners = p.d_own;
    c.need = st.need();
    // copy elision (GOL_DEV_COPY_ELIDE=0: elided null, every calm unit copies)
    c.elided = r.pass_elide ? st.elided() : nullptr;
    c.held = r.pass_held ? st.held() : nullptr;
    c.all_held = r.pass_all ? 1 : 0;
    c.streak_in = a.streak_in;
    c.nb_off = a.nb_off;
    c.nb_ids = a.nb_ids;
    // the step's last launch: the calm kernel writes twin[] as well
    if (r.twin == StepLaunch::kTwinCalm) {
        c.twin = st.twin();
        c.twin_ok = st.twin_ok();
        c.twin_val = r.twin_val;
    }
    HIP_TRY(gol::launch_copy_pass(c, s));
    return GOL_OK;
}

// ... and where the step's last launch takes no copy pass (a depth-K launch after the
// step's second), the calm kernel runs for twin[] alone, on the streaks the launch reads
static gol_status issue_calm_alone(gol_engine* e, const gol_engine::Plan& p, const StepArgs& a,
                                   hipStream_t s)
{
    const ActState st{e->d_streak, (size_t)e->act_units};
    gol::CopyArgs c{};
    c.streak_in = a.streak_in;
    c.nb_off = a.nb_off;
    c.nb_ids = a.nb_ids;
    c.total_units = (int32_t)p.total_units;
    c.twin = st.twin();
    c.twin_ok = st.twin_ok();
    HIP_TRY(gol::launch_twin_flags(c, s));
    return GOL_OK;
}

// Probe pass (life_probe.hip): before a step's first launch, where that
// launch probes, under the copy pass's conditions.  The launch has no history, so
// none of its units skips or copies: a unit the pass leaves unmarked ends quiet on
// the pass's word, every other one stores its whole rectangle after the pass.
static gol_status issue_probe_pass(gol_engine* e, const gol_engine::Plan& p, const StepLaunch& r,
                                   StepArgs& a, hipStream_t s)
{
    if (!a.no_hist || !a.streak_out || !a.probe || !p.d_ptab || s != e->stream ||
        p.segs.size() != 1 || e->planes != 2)
        return fail(GOL_ESTATE, "probe pass before a launch with history");
    const ActState st{e->d_streak, (size_t)e->act_units};
    gol::ProbeArgs c{};
    fill_tile_args(e, p, a, p.probe_tiles.size() / gol::kProbeSlots, c);
    c.tiles = p.d_ptab;
    c.moved = st.moved();
    c.birth = e->birth;
    c.survive = e->survive;
    // rows both buffers hold: the copy pass's owners, over the same tile grid
    if (r.probe_twin) {
        if (!p.d_own || !e->d_kept || p.owners.size() / gol::kCopyOwners != (size_t)c.ntile ||
            e->kept_tiles != (int64_t)c.ntile || p.copy_ncol != c.ncol)
            return fail(GOL_ESTATE, "probe pass and copy pass over different tiles");
        c.owners = p.d_own;
        c.twin = st.twin();
        c.twin_ok = st.twin_ok();
        c.kept = e->d_kept;
        c.sure = r.probe_sure ? e->d_sure : nullptr;
    }
    HIP_TRY(gol::launch_probe_pass(c, e->rule, s));
    a.moved = st.moved();
    a.pass_probed = st.pass_probed();
    return GOL_OK;
}

// The end of the timing bracket around a stencil launch, with the launch's work.
static gol_status timing_end_launch(gol_engine* e, hipStream_t s, hipEvent_t e0, hipEvent_t e1,
                                    const gol_engine::Plan& p, uint32_t depth, int passes, bool hand)
{
    // cell-generations the lanes actually process: every stage of a block
    // computes its rows, a classic block (and the last block of a hand-off
    // segment) also d(d-1) stage-rows of vertical halo, and every strip also
    // its 2 halo lanes
    double comp = 0;
    for (const auto& sg : p.segs) {
        const double n = (double)std::max<int64_t>(0, sg.out_hi - sg.out_lo);
        const double classic = hand ? (double)std::min<int64_t>(1, sg.nblk) : (double)sg.nblk;
        comp += depth * n + classic * depth * (depth - 1.0);
    }
    // (the half strip's units: 64 lanes over one block's rows each, classic)
    double comp_half = 0;
    for (size_t i = 0; i + 2 < p.pairs.size(); i += 3)
        comp_half += depth * (double)p.pairs[i + 2] + depth * (depth - 1.0);
    const double cols = 64.0 * 32.0 * e->planes;  // per strip or unit
    double rows = 0;
    for (const auto& sg : p.segs) rows += (double)std::max<int64_t>(0, sg.out_hi - sg.out_lo);
    return timing_end(e, s, e0, e1, p.own_rows * (double)e->W * depth * passes,
                      (comp * p.groups + comp_half) * cols * passes, rows * passes);
}

// `passes` > 1: a multi-pass launch of that many depth-K passes (plans with npass
// >= passes), reading buf[cur] and writing buf[cur + 1 .. cur + passes]

gol_status launch(gol_engine* e, int plan, uint32_t depth, bool swap, hipStream_t stream,
                  int passes, const StepLaunch* rec, bool skip_stencil)
{
    hipStream_t s = stream ? stream : e->stream;
    const int region = (e->band_stream && s == e->band_stream) ? 1 : 0;
    const auto& p = e->plans[plan];
    // (a step flushes before it captures; whoever else launches finds steps pending here)
    GOL_TRY(flush_still(e));
    if (passes < 1 || (passes > 1 && (passes > p.npass || depth != e->K || !e->mpflags)))
        return fail(GOL_ESTATE, "multi-pass launch of a plan without passes");
    const bool hand = launch_hands(e, p, region, depth);
    StepArgs a{};
    GOL_TRY(fill_step_args(e, p, depth, passes, region, hand, a));
    // Rows both buffers hold: a launch of plan 0 writes the field, so it
    // clears twin_ok; within a step the record says what becomes of twin[].
    StepLaunch::Twin twin =
        e->twin_on && e->d_streak && plan == 0 ? StepLaunch::kTwinClear : StepLaunch::kTwinNone;
    if (rec) {
        if (plan != 0 || (rec->act && !e->d_streak) || depth != rec->depth || passes != rec->passes)
            return fail(GOL_ESTATE, "a step's record before a launch that is not the step's");
        fill_activity_args(e, p, *rec, a);
        twin = rec->twin;
        // copy pass, else the calm kernel alone; probe pass
        if (rec->copy_pass) GOL_TRY(issue_copy_pass(e, p, *rec, a, s));
        if (rec->calm_alone) GOL_TRY(issue_calm_alone(e, p, a, s));
        if (rec->probe_pass) GOL_TRY(issue_probe_pass(e, p, *rec, a, s));
    }
    // after the probe pass, which reads the flag as the step before left it
    if (twin == StepLaunch::kTwinClear) GOL_TRY(twin_clear(e, s));
    hipEvent_t e0, e1;
    GOL_TRY(timing_begin(e, s, &e0, &e1));
    // Short step: everything around the launch has happened as in the full
    // step, the calm kernel for twin[] before a last depth-K launch included; the
    // stencil kernel, which would exit on one load, is left out (the step puts one
    // node in place of all of them).
    if (skip_stencil) {
        if (!rec || !rec->short_ok || !a.busy || e0 || s != e->stream)
            return fail(GOL_ESTATE, "short step over a launch without the one-load exit");
    } else {
        HIP_TRY(gol::launch_life(a, (int)depth, e->rule, e->planes, hand, s));
    }
    if (e0) GOL_TRY(timing_end_launch(e, s, e0, e1, p, depth, passes, hand));
    // the step's only launch, which probes and writes held[] for every unit: twin[] is
    // held[], copied behind the launch
    if (twin == StepLaunch::kTwinHeld) {
        const ActState st{e->d_streak, (size_t)e->act_units};
        HIP_TRY(gol::launch_twin_held(a.held, st.twin(), st.twin_ok(), (int32_t)p.total_units, s));
    }
    if (swap) e->cur = (e->cur + passes) % e->nbuf;
    return GOL_OK;
}


// Order everything the side streams of a stripe engine have enqueued (band
// launches, overlapped exchanges) before the next work on its compute stream, so
// reads of the field on `stream` (store, digest) see the band rows.
gol_status join_side_streams(gol_engine* e)
{
    if (e->band_stream) {
        HIP_TRY(hipEventRecord(e->ev_join, e->band_stream));
        HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_join, 0));
    }
    if (e->comm_stream) {
        HIP_TRY(hipEventRecord(e->ev_join, e->comm_stream));
        HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_join, 0));
    }
    return GOL_OK;
}

// Before a load replaces the field: finish every stream of this engine and the
// neighbours' exchange streams that may still be copying from its buffers.
gol_status quiesce(gol_engine* e)
{
    HIP_TRY(hipSetDevice(e->device));
    if (e->comm_stream) HIP_TRY(hipStreamSynchronize(e->comm_stream));
    if (e->band_stream) HIP_TRY(hipStreamSynchronize(e->band_stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (gol_engine* n : {e->up, e->down})
        if (n && n->comm_stream) HIP_TRY(hipStreamSynchronize(n->comm_stream));
    e->halo_fresh = false;
    return GOL_OK;
}

gol_status twin_clear(gol_engine* e, hipStream_t s)
{
    // (short step) whoever withdraws the record may have written the field: what
    // gol_sync saw no longer holds, on whatever stream the write goes
    e->still_seen = false;
    e->twin_two = false;  // (fixed step) twin[] says nothing any more
    // pending fixed steps prove themselves on the flag as it stands, and write it
    GOL_TRY(flush_still(e));
    if (!e->d_streak || !e->twin_on) return GOL_OK;  // nobody reads the flag
    const ActState st{e->d_streak, (size_t)e->act_units};
    HIP_TRY(hipMemsetAsync(st.twin_ok(), 0, sizeof(uint32_t), s ? s : e->stream));
    return GOL_OK;
}

// The kernel's hand-off wait gives up after a bounded time and flags it: report.
gol_status check_err(gol_engine* e)
{
    if (!e->d_err) return GOL_OK;
    // pending fixed steps may write the word: their kernel runs before the look
    if (e->pending.steps) {
        GOL_TRY(flush_still(e));
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    int err = 0;
    HIP_TRY(hipMemcpy(&err, e->d_err, sizeof(int), hipMemcpyDeviceToHost));
    if (!err) return GOL_OK;
    HIP_TRY(hipMemset(e->d_err, 0, sizeof(int)));
    if (err == gol::kErrShortStep) {
        // the short step's node found a unit busy in the step's third launch: the
        // launches left out should have computed (only GOL_DEV_SHORT_STEP=2 gets here
        // unless the host's flag was wrong)
        (void)twin_clear(e);
        e->rem_ended = false;
        return fail(GOL_ESTATE, "short step on a field that was not still; the field is not valid");
    }
    for (int r = 0; r < 2; ++r)
        if (e->flags[r]) {
            const int64_t n = [&] {
                int64_t m = 0;
                for (const auto& p : e->plans) m = std::max(m, p.total_units);
                return m;
            }();
            HIP_TRY(hipMemset(e->flags[r], 0, (size_t)n * sizeof(uint32_t)));
        }
    return fail(GOL_EHIP, "a wait for a neighbour's rows timed out in the stencil kernel; "
                          "the field is not valid");
}


}  // namespace golh

extern "C" {

void gol_config_init(gol_config* cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->birth_mask = GOL_REF_BIRTH;
    cfg->survive_mask = GOL_REF_SURVIVE;
    cfg->device = -1;
    cfg->semantics = GOL_SEM_GLOBAL;
    cfg->ref_ranks = 1;
}

const char* gol_last_error(void) { return g_last_error.c_str(); }

gol_status gol_create(uint64_t h, uint64_t w, const gol_config* cfg, gol_engine** out)
{
    if (!out) return fail(GOL_EINVAL, "null out");
    *out = nullptr;
    gol_status st = check_cfg(cfg);
    if (st != GOL_OK) return st;
    if (h == 0 || w == 0) return fail(GOL_EINVAL, "h and w must be >= 1");
    if (h > (1ull << 40) || w > (1ull << 40)) return fail(GOL_EINVAL, "field too large");
    if (cfg->semantics == GOL_SEM_TORUS) return torus_create(h, w, cfg, out);
    gol_engine* e = new (std::nothrow) gol_engine();
    if (!e) return fail(GOL_ENOMEM, "host allocation");
    e->R = h;
    uint32_t S = cfg->streams;
    if (S == 0)
        S = (cfg->semantics == GOL_SEM_GLOBAL && h >= kCompositeMinRows && !single_stream_skews(h, w, cfg))
                ? 2
                : 1;
    if (S > 1 && cfg->semantics == GOL_SEM_GLOBAL && h / S >= 256) {
        // composite: S same-device stripes with deep halos, advanced together
        gol_config c = *cfg;
        c.streams = 1;
        // the stripes run side by side on one device, so at most one of them could
        // keep hand-off blocks (gol_create_group); unbalanced stripes lose more than
        // that one gains (profiles/r02/ab_handoff_policy.jsonl): classic blocks
        if (c.handoff == 0) c.handoff = 1;
        const Layout lay = auto_layout(h / S, cfg);
        c.tb_depth = lay.K;
        c.word_planes = (uint32_t)lay.planes;
        if (!c.halo_depth) c.halo_depth = 16 * c.tb_depth;
        int dev = cfg->device;
        if (dev < 0) {
            hipError_t he = hipGetDevice(&dev);
            if (he != hipSuccess) {
                delete e;
                return fail(GOL_EHIP, std::string("hipGetDevice: ") + hipGetErrorString(he));
            }
        }
        std::vector<int> devs(S, dev);
        e->parts.assign(S, nullptr);
        st = gol_create_group(h, w, &c, (int)S, devs.data(), e->parts.data());
        if (st != GOL_OK) {
            e->parts.clear();
            delete e;
            return st;
        }
        e->H = h;
        e->W = w;
        e->wq = (w + 63) / 64;
        e->device = dev;
        e->K = e->parts[0]->K;
        *out = e;
        return GOL_OK;
    }
    e->act_on = true;  // (activity skip) allowed; init_common decides
    st = init_common(e, h, w, cfg, nullptr);
    if (st != GOL_OK) {
        std::string msg = g_last_error;
        gol_destroy(e);
        g_last_error = msg;
        return st;
    }
    *out = e;
    return GOL_OK;
}


gol_status gol_plan_model(uint64_t h, uint64_t w, const gol_config* cfg, int rank, int nranks,
                          int cus, int occ_classic, int occ_hand, gol_plan_summary* out)
{
    if (!out) return fail(GOL_EINVAL, "null out");
    *out = gol_plan_summary{};
    gol_status st = check_cfg(cfg);
    if (st != GOL_OK) return st;
    if (h == 0 || w == 0) return fail(GOL_EINVAL, "h and w must be >= 1");
    if (h > (1ull << 40) || w > (1ull << 40)) return fail(GOL_EINVAL, "field too large");
    if (cus <= 0 || occ_classic <= 0 || occ_hand < 0)
        return fail(GOL_EINVAL, "cus and occ_classic must be >= 1, occ_hand >= 0");
    if (nranks > 1 && cfg->semantics != GOL_SEM_GLOBAL)
        return fail(GOL_EINVAL, "rank engines implement GLOBAL semantics only");
    if (cfg->semantics == GOL_SEM_TORUS) {  // the inner engine's plan (padded field)
        TorusGeom tg;
        GOL_TRY(torus_geometry(h, w, cfg, &tg));
        gol_config ic = *cfg;
        ic.semantics = GOL_SEM_GLOBAL;
        ic.streams = 1;
        ic.halo_depth = 0;
        GOL_TRY(gol_plan_model(tg.ph, tg.pw, &ic, rank, nranks, cus, occ_classic, occ_hand, out));
        out->halo_depth = tg.G;
        return GOL_OK;
    }
    RankGeom g;
    gol_config c = *cfg;
    if (nranks > 1) {
        st = rank_geometry(h, cfg, rank, nranks, &g);
        if (st != GOL_OK) return st;
        c.resident = 1;
        c.tb_depth = g.K;
    } else if (nranks != 1 || rank != 0) {
        return fail(GOL_EINVAL, "rank must be 0 of 1, or 0 <= rank < nranks");
    }
    std::unique_ptr<gol_engine> e(new (std::nothrow) gol_engine());
    if (!e) return fail(GOL_ENOMEM, "host allocation");
    e->model.on = true;
    e->model.cus = cus;
    e->model.occ_c = occ_classic;
    e->model.occ_h = occ_hand;
    if (nranks > 1) {
        e->rank = rank;
        e->nranks = nranks;
        e->row0 = g.row0;
        e->R = g.R;
        e->Hx = g.Hx;
    } else {
        e->R = h;
    }
    GOL_TRY(host_layout(e.get(), h, w, &c));
    std::vector<std::vector<SegDesc>> raw;
    GOL_TRY(raw_regions(e.get(), h, &c, nranks > 1 ? &g : nullptr, raw));
    decide_passes(e.get(), (size_t)(e->buf_rows + 2 * gol::kGuardRows) * e->stride);
    GOL_TRY(build_plans(e.get(), raw));
    if (e->plans.empty()) return fail(GOL_ESTATE, "no launch plan");
    const size_t pi = nranks > 1 ? std::min<size_t>(e->plans.size() - 1, e->K - 1) : 0;
    const auto& p = e->plans[pi];
    out->tb_depth = e->K;
    out->halo_depth = (uint32_t)e->Hx;
    out->plans = (uint32_t)e->plans.size();
    for (int a : e->plan_alias) out->distinct_plans += a < 0 ? 1u : 0u;
    out->rows_lo = p.segs.empty() ? 0 : p.segs[0].out_lo;
    out->rows_hi = p.segs.empty() ? 0 : p.segs.back().out_hi;
    out->rows_per_wave = p.rows_old ? p.rows_young : p.rpw;
    out->rows_old = p.rows_old;
    out->units_old = p.units_old;
    out->strips = p.groups;
    out->lane_shift = p.lane_shift;
    out->total_units = p.total_units;
    out->half_units = p.pair_units;
    for (const auto& sg : p.segs) out->blocks += sg.nblk;
    out->handoff = (p.hand && p.multi_blk) ? 1 : 0;
    out->tail_off = out->handoff ? gol::handoff_toff(p.rpw, (int)e->K, e->planes) : -1;
    out->passes = (uint32_t)p.npass;
    out->candidates = pi < e->plan_alts.size() ? (uint32_t)e->plan_alts[pi].size() : 0u;
    return GOL_OK;
}

// The plans gol_create would build for an h x w GLOBAL field on a device of `cus`
// CUs with those occupancies, on the host alone (gol_plan_neighbours,
// gol_plan_probe_tiles).
static gol_status model_plans(gol_engine* e, uint64_t h, uint64_t w, const gol_config* cfg, int cus,
                              int occ_classic, int occ_hand)
{
    e->model.on = true;
    e->model.cus = cus;
    e->model.occ_c = occ_classic;
    e->model.occ_h = occ_hand;
    e->R = h;
    GOL_TRY(host_layout(e, h, w, cfg));
    std::vector<std::vector<SegDesc>> raw;
    GOL_TRY(raw_regions(e, h, cfg, nullptr, raw));
    decide_passes(e, (size_t)(e->buf_rows + 2 * gol::kGuardRows) * e->stride);
    GOL_TRY(build_plans(e, raw));
    if (e->plans.empty()) return fail(GOL_ESTATE, "no launch plan");
    return GOL_OK;
}

gol_status gol_plan_probe_tiles(uint64_t h, uint64_t w, const gol_config* cfg, int cus,
                                int occ_classic, int occ_hand, uint32_t* table, uint64_t cap,
                                uint32_t* tile_rows, uint32_t* tile_words, uint32_t* slots,
                                uint64_t* ntile, uint64_t* ncol)
{
    if (!ntile || !ncol) return fail(GOL_EINVAL, "null out");
    *ntile = *ncol = 0;
    if (tile_rows) *tile_rows = (uint32_t)gol::kCopyTileRows;
    if (tile_words) *tile_words = (uint32_t)gol::kCopyTileWords;
    if (slots) *slots = (uint32_t)gol::kProbeSlots;
    gol_status st = check_cfg(cfg);
    if (st != GOL_OK) return st;
    if (h == 0 || w == 0) return fail(GOL_EINVAL, "h and w must be >= 1");
    if (h > (1ull << 40) || w > (1ull << 40)) return fail(GOL_EINVAL, "field too large");
    if (cus <= 0 || occ_classic <= 0 || occ_hand < 0)
        return fail(GOL_EINVAL, "cus and occ_classic must be >= 1, occ_hand >= 0");
    if (cfg->semantics == GOL_SEM_TORUS) {  // the inner engine's plan (padded field)
        TorusGeom tg;
        GOL_TRY(torus_geometry(h, w, cfg, &tg));
        gol_config ic = *cfg;
        ic.semantics = GOL_SEM_GLOBAL;
        ic.streams = 1;
        ic.halo_depth = 0;
        return gol_plan_probe_tiles(tg.ph, tg.pw, &ic, cus, occ_classic, occ_hand, table, cap,
                                    tile_rows, tile_words, slots, ntile, ncol);
    }
    std::unique_ptr<gol_engine> e(new (std::nothrow) gol_engine());
    if (!e) return fail(GOL_ENOMEM, "host allocation");
    GOL_TRY(model_plans(e.get(), h, w, cfg, cus, occ_classic, occ_hand));
    const auto& p = e->plans[0];
    if (p.probe_tiles.empty() || p.nb_off.empty()) return GOL_OK;  // no pass
    *ntile = p.probe_tiles.size() / gol::kProbeSlots;
    *ncol = (uint64_t)p.copy_ncol;
    if (table && cap >= p.probe_tiles.size())
        std::memcpy(table, p.probe_tiles.data(), p.probe_tiles.size() * sizeof(uint32_t));
    return GOL_OK;
}

gol_status gol_plan_neighbours(uint64_t h, uint64_t w, const gol_config* cfg, int cus,
                               int occ_classic, int occ_hand, int64_t* rects, uint32_t* offsets,
                               uint64_t unit_cap, uint32_t* ids, uint64_t id_cap, uint64_t* units,
                               uint64_t* nids)
{
    if (!units || !nids) return fail(GOL_EINVAL, "null out");
    *units = *nids = 0;
    gol_status st = check_cfg(cfg);
    if (st != GOL_OK) return st;
    if (h == 0 || w == 0) return fail(GOL_EINVAL, "h and w must be >= 1");
    if (h > (1ull << 40) || w > (1ull << 40)) return fail(GOL_EINVAL, "field too large");
    if (cus <= 0 || occ_classic <= 0 || occ_hand < 0)
        return fail(GOL_EINVAL, "cus and occ_classic must be >= 1, occ_hand >= 0");
    if (cfg->semantics == GOL_SEM_TORUS) {  // the inner engine's plan (padded field)
        TorusGeom tg;
        GOL_TRY(torus_geometry(h, w, cfg, &tg));
        gol_config ic = *cfg;
        ic.semantics = GOL_SEM_GLOBAL;
        ic.streams = 1;
        ic.halo_depth = 0;
        return gol_plan_neighbours(tg.ph, tg.pw, &ic, cus, occ_classic, occ_hand, rects, offsets,
                                   unit_cap, ids, id_cap, units, nids);
    }
    std::unique_ptr<gol_engine> e(new (std::nothrow) gol_engine());
    if (!e) return fail(GOL_ENOMEM, "host allocation");
    GOL_TRY(model_plans(e.get(), h, w, cfg, cus, occ_classic, occ_hand));
    const auto& p = e->plans[0];
    *units = (uint64_t)p.total_units;
    *nids = p.nb_ids.size();
    if (rects && unit_cap >= *units) {
        std::vector<URect> rc;
        unit_rects(p, (int64_t)e->ng, rc);
        std::memcpy(rects, rc.data(), rc.size() * sizeof(URect));
    }
    if (offsets && ids && unit_cap >= *units && id_cap >= *nids && !p.nb_off.empty()) {
        std::memcpy(offsets, p.nb_off.data(), p.nb_off.size() * sizeof(uint32_t));
        std::memcpy(ids, p.nb_ids.data(), p.nb_ids.size() * sizeof(uint32_t));
    }
    return GOL_OK;
}

}  // extern "C"


extern "C" {

void gol_destroy(gol_engine* e)
{
    if (!e) return;
    if (e->inner) {
        gol_destroy(e->inner);
        delete e;
        return;
    }
    if (!e->parts.empty()) {
        for (auto* p : e->parts) (void)hipStreamSynchronize(p->stream);
        for (auto* p : e->parts) gol_destroy(p);
        delete e;
        return;
    }
    (void)hipSetDevice(e->device);
    e->pending = StillPending{};  // pending fixed steps: nobody is left to look
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->comm_stream) (void)hipStreamSynchronize(e->comm_stream);
    if (e->band_stream) (void)hipStreamSynchronize(e->band_stream);
    // group neighbours may still be copying from this engine's buffers
    for (gol_engine* n : {e->up, e->down}) {
        if (!n) continue;
        if (n->stream) (void)hipStreamSynchronize(n->stream);
        if (n->comm_stream) (void)hipStreamSynchronize(n->comm_stream);
        if (n->band_stream) (void)hipStreamSynchronize(n->band_stream);
    }
    wait_release(e);
    if (e->comm) (void)ncclCommDestroy(e->comm);
    if (e->host_xfer) (void)hipHostFree(e->host_xfer);
    if (e->up) e->up->down = nullptr;
    if (e->down) e->down->up = nullptr;
    if (e->ev_ready) (void)hipEventDestroy(e->ev_ready);
    if (e->ev_copied) (void)hipEventDestroy(e->ev_copied);
    for (hipEvent_t ev : {e->ev_band, e->ev_in, e->ev_xdone, e->ev_join})
        if (ev) (void)hipEventDestroy(ev);
    if (e->band_stream) (void)hipStreamDestroy(e->band_stream);
    if (e->comm_stream) (void)hipStreamDestroy(e->comm_stream);
    for (auto& p : e->plans) free_plan(p);
    for (auto& alts : e->plan_alts)
        for (auto& p : alts) free_plan(p);
    for (int b = 0; b < 4; ++b)
        if (e->alloc[b]) (void)hipFree(e->alloc[b]);
    for (int b = 0; b < 2; ++b) {
        if (e->side[b]) (void)hipFree(e->side[b]);
        if (e->flags[b]) (void)hipFree(e->flags[b]);
    }
    if (e->mpflags) (void)hipFree(e->mpflags);
    if (e->d_streak) (void)hipFree(e->d_streak);
    if (e->d_kept) (void)hipFree(e->d_kept);
    if (e->d_sure) (void)hipFree(e->d_sure);
    if (e->sync_host) (void)hipHostFree(e->sync_host);
    if (e->d_err) (void)hipFree(e->d_err);
    if (e->res.flags) (void)hipFree(e->res.flags);
    for (hipEvent_t ev : {e->res.ev_in, e->res.ev_out})
        if (ev) (void)hipEventDestroy(ev);
    for (auto& kv : e->graphs) (void)hipGraphExecDestroy(kv.second.exec);
    if (e->d_acc) (void)hipFree(e->d_acc);
    if (e->d_flag) (void)hipFree(e->d_flag);
    if (e->rect_stage) (void)hipFree(e->rect_stage);
    snapshot_free(e);
    for (const auto* pend : {&e->ev_pending, &e->ev_xpending})
        for (auto& p : *pend) {
            (void)hipEventDestroy(p.first);
            (void)hipEventDestroy(p.second);
        }
    for (auto& r : e->ev_rpending) {  // (xend belongs to ev_xpending)
        (void)hipEventDestroy(r.start);
        (void)hipEventDestroy(r.end);
    }
    for (auto ev : e->ev_free) (void)hipEventDestroy(ev);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

static uint64_t user_rows(const gol_engine* e)
{
    uint64_t n = 0;
    for (const auto& r : e->user_regions) n += r.rows;
    return n;
}

static uint64_t load_rows_needed(const gol_engine* e)
{
    // rows of the caller's buffer that a load reads: the whole field for
    // GLOBAL/REF_STRIPES, own rows for a rank engine
    return e->nranks > 1 ? e->R : e->H;
}

}  // extern "C"

// Host <-> device transfer of the load/store regions.  The caller's words use the
// public bit order (bit j = column 64q+j) and are converted to/from the
// engine's lane groups (bitlayout.h).
static gol_status upload(gol_engine* e, const uint64_t* words, uint64_t rs)
{
    GOL_TRY(quiesce(e));
    GOL_TRY(twin_clear(e));
    // clear everything (halos, unused rows) then copy each region, masking pad bits
    const size_t words_all = (size_t)(e->buf_rows + 2 * gol::kGuardRows) * e->stride;
    HIP_TRY(hipMemsetAsync(e->alloc[e->cur], 0, words_all * 8, e->stream));
    std::vector<uint64_t> tmp;
    for (const auto& r : e->load_regions) {
        tmp.assign((size_t)r.rows * e->stride, 0);
        const uint64_t urow = e->nranks > 1 ? 0 : r.user_row;
        for (uint64_t i = 0; i < r.rows; ++i) {
            const uint64_t* src = words + (urow + i) * rs;
            uint64_t* dst = tmp.data() + i * e->stride;
            const uint64_t G = (uint64_t)e->planes / 2;
            for (uint64_t gq = 0; gq < e->ng; ++gq) {
                uint64_t c[2] = {0, 0};
                for (uint64_t j = 0; j < G; ++j) {
                    const uint64_t q = gq * G + j;
                    if (q < e->wq) c[j] = q == e->wq - 1 ? (src[q] & e->lastmask) : src[q];
                }
                gol_split_group(c, dst + gq * G, e->planes);
            }
        }
        HIP_TRY(hipMemcpyAsync(e->buf[e->cur] + r.buf_row * e->stride, tmp.data(),
                               tmp.size() * 8, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    return GOL_OK;
}

static gol_status download(gol_engine* e, uint64_t* words, uint64_t rs)
{
    HIP_TRY(hipSetDevice(e->device));
    GOL_TRY(join_side_streams(e));
    std::vector<uint64_t> tmp;
    for (const auto& r : e->user_regions) {
        tmp.resize((size_t)r.rows * e->stride);
        HIP_TRY(hipMemcpyAsync(tmp.data(), e->buf[e->cur] + r.buf_row * e->stride,
                               tmp.size() * 8, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        const uint64_t urow = e->nranks > 1 ? 0 : r.user_row;
        for (uint64_t i = 0; i < r.rows; ++i) {
            uint64_t* dst = words + (urow + i) * rs;
            const uint64_t* src = tmp.data() + i * e->stride;
            const uint64_t G = (uint64_t)e->planes / 2;
            for (uint64_t gq = 0; gq < e->ng; ++gq) {
                uint64_t c[2];
                gol_join_group(src + gq * G, c, e->planes);
                for (uint64_t j = 0; j < G; ++j)
                    if (gq * G + j < e->wq) dst[gq * G + j] = c[j];
            }
        }
    }
    return check_err(e);
}

// composite engines: part r holds field rows [row0_r, row0_r + rows_r)
static void part_rows(const gol_engine* e, size_t r, uint64_t* row0, uint64_t* rows)
{
    gol_rank_rows(e->H, (int)e->parts.size(), (int)r, row0, rows);
}

extern "C" {

gol_status gol_load_packed(gol_engine* e, const uint64_t* words, uint64_t rs)
{
    if (!e || !words) return fail(GOL_EINVAL, "null argument");
    if (e->inner) return torus_load_packed(e, words, rs);
    if (!e->parts.empty()) {
        for (size_t r = 0; r < e->parts.size(); ++r) {
            uint64_t r0, n;
            part_rows(e, r, &r0, &n);
            gol_status st = gol_load_packed(e->parts[r], words + r0 * rs, rs);
            if (st != GOL_OK) return st;
        }
        return GOL_OK;
    }
    if (rs < e->wq) return fail(GOL_EINVAL, "row stride smaller than ceil(w/64)");
    return upload(e, words, rs);
}

gol_status gol_load_ascii(gol_engine* e, const char* buf, size_t len)
{
    if (!e || !buf) return fail(GOL_EINVAL, "null argument");
    if (e->inner) return torus_load_ascii(e, buf, len);
    if (!e->parts.empty()) {
        if (len != e->H * (e->W + 1))
            return fail(GOL_EINVAL, "ASCII length must be rows*(w+1) = " +
                                        std::to_string(e->H * (e->W + 1)));
        for (size_t r = 0; r < e->parts.size(); ++r) {
            uint64_t r0, n;
            part_rows(e, r, &r0, &n);
            gol_status st = gol_load_ascii(e->parts[r], buf + r0 * (e->W + 1), n * (e->W + 1));
            if (st != GOL_OK) return st;
        }
        return GOL_OK;
    }
    const uint64_t rows = load_rows_needed(e);
    if (len != rows * (e->W + 1))
        return fail(GOL_EINVAL, "ASCII length must be rows*(w+1) = " +
                                    std::to_string(rows * (e->W + 1)) + ", got " +
                                    std::to_string(len));
    // raw bytes to the device, packed there by the ASCII codec kernel
    GOL_TRY(quiesce(e));
    GOL_TRY(twin_clear(e));
    DeviceBytes bytes;
    HIP_TRY(hipMalloc(&bytes.p, len));
    HIP_TRY(hipMemcpyAsync(bytes.p, buf, len, hipMemcpyHostToDevice, e->stream));
    const size_t words_all = (size_t)(e->buf_rows + 2 * gol::kGuardRows) * e->stride;
    HIP_TRY(hipMemsetAsync(e->alloc[e->cur], 0, words_all * 8, e->stream));
    HIP_TRY(hipMemsetAsync(e->d_flag, 0, sizeof(int), e->stream));
    for (const auto& r : e->load_regions) {
        const uint64_t urow = e->nranks > 1 ? 0 : r.user_row;
        HIP_TRY(gol::launch_ascii_pack(bytes.p + urow * (e->W + 1), (int64_t)r.rows,
                                       (int64_t)e->W, (int64_t)e->ng,
                                       e->buf[e->cur] + r.buf_row * e->stride,
                                       (int64_t)e->stride, e->d_flag, e->planes, e->stream));
    }
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, e->d_flag, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (bad) return fail(GOL_EINVAL, "malformed ASCII: a line is not w cells followed by '\\n'");
    return GOL_OK;
}

gol_status gol_store_packed(gol_engine* e, uint64_t* words, uint64_t rs)
{
    if (!e || !words) return fail(GOL_EINVAL, "null argument");
    if (e->inner) return torus_store_packed(e, words, rs);
    if (!e->parts.empty()) {
        for (size_t r = 0; r < e->parts.size(); ++r) {
            uint64_t r0, n;
            part_rows(e, r, &r0, &n);
            gol_status st = gol_store_packed(e->parts[r], words + r0 * rs, rs);
            if (st != GOL_OK) return st;
        }
        return GOL_OK;
    }
    if (rs < e->wq) return fail(GOL_EINVAL, "row stride smaller than ceil(w/64)");
    return download(e, words, rs);
}

gol_status gol_store_ascii(gol_engine* e, char* buf, size_t len)
{
    if (!e || !buf) return fail(GOL_EINVAL, "null argument");
    if (e->inner) return torus_store_ascii(e, buf, len);
    if (!e->parts.empty()) {
        if (len != e->H * (e->W + 1))
            return fail(GOL_EINVAL, "ASCII length must be rows*(w+1) = " +
                                        std::to_string(e->H * (e->W + 1)));
        for (size_t r = 0; r < e->parts.size(); ++r) {
            uint64_t r0, n;
            part_rows(e, r, &r0, &n);
            gol_status st = gol_store_ascii(e->parts[r], buf + r0 * (e->W + 1), n * (e->W + 1));
            if (st != GOL_OK) return st;
        }
        return GOL_OK;
    }
    const uint64_t rows = user_rows(e);
    if (len != rows * (e->W + 1))
        return fail(GOL_EINVAL, "ASCII length must be rows*(w+1) = " +
                                    std::to_string(rows * (e->W + 1)));
    HIP_TRY(hipSetDevice(e->device));
    GOL_TRY(join_side_streams(e));
    DeviceBytes bytes;
    HIP_TRY(hipMalloc(&bytes.p, len));
    for (const auto& r : e->user_regions) {
        const uint64_t urow = e->nranks > 1 ? 0 : r.user_row;
        HIP_TRY(gol::launch_ascii_unpack(e->buf[e->cur] + r.buf_row * e->stride,
                                         (int64_t)e->stride, (int64_t)r.rows, (int64_t)e->W,
                                         (int64_t)e->ng, bytes.p + urow * (e->W + 1), e->planes,
                                         e->stream));
    }
    HIP_TRY(hipMemcpyAsync(buf, bytes.p, len, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return check_err(e);
}

gol_status gol_init_random(gol_engine* e, uint64_t seed)
{
    if (!e) return fail(GOL_EINVAL, "null engine");
    if (e->inner) return torus_init_random(e, seed);
    if (!e->parts.empty()) {
        for (auto* p : e->parts) {
            gol_status st = gol_init_random(p, seed);
            if (st != GOL_OK) return st;
        }
        return GOL_OK;
    }
    GOL_TRY(quiesce(e));
    GOL_TRY(twin_clear(e));
    const size_t words_all = (size_t)(e->buf_rows + 2 * gol::kGuardRows) * e->stride;
    HIP_TRY(hipMemsetAsync(e->alloc[e->cur], 0, words_all * 8, e->stream));
    for (const auto& r : e->load_regions)
        HIP_TRY(gol::launch_init_random(e->buf[e->cur], (int64_t)e->stride, (int64_t)e->wq,
                                        e->lastmask, (int64_t)r.buf_row, (int64_t)r.glob_row,
                                        (int64_t)r.rows, seed, e->planes, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return GOL_OK;
}


gol_status gol_step(gol_engine* e, uint64_t generations)
{
    if (!e) return fail(GOL_EINVAL, "null engine");
    if (e->inner) return torus_step(e, generations);
    if (!e->parts.empty()) return gol_group_step(e->parts.data(), (int)e->parts.size(), generations);
    if (e->grouped) return fail(GOL_ESTATE, "group members advance with gol_group_step");
    HIP_TRY(hipSetDevice(e->device));
    if (e->nranks <= 1) return step_single(e, generations);
    return step_stripe(e, generations);
}


gol_status gol_sync(gol_engine* e)
{
    if (!e) return fail(GOL_EINVAL, "null engine");
    if (e->inner) return gol_sync(e->inner);
    if (!e->parts.empty()) {
        for (auto* p : e->parts) {
            gol_status st = gol_sync(p);
            if (st != GOL_OK) return st;
        }
        return GOL_OK;
    }
    HIP_TRY(hipSetDevice(e->device));
    // (short step) a single-stream engine that may arm the short graph: one wait for
    // the work, the error word and, where a step has run, twin[]
    if (e->sync_host && e->d_err && !e->band_stream && !e->comm_stream) return sync_observing(e);
    GOL_TRY(flush_still(e));  // (GOL_DEV_FIXED_STEP=2 without the short step's look)
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->band_stream) HIP_TRY(hipStreamSynchronize(e->band_stream));
    if (e->comm_stream) HIP_TRY(hipStreamSynchronize(e->comm_stream));
    return check_err(e);
}

gol_status gol_digest(gol_engine* e, uint64_t* live, uint64_t* hash)
{
    if (!e || !live || !hash) return fail(GOL_EINVAL, "null argument");
    if (e->inner) return torus_digest_rows(e, 0, e->H, live, hash);
    if (!e->parts.empty()) {
        uint64_t L = 0, Hs = 0;
        for (auto* p : e->parts) {
            uint64_t l, h;
            gol_status st = gol_digest(p, &l, &h);
            if (st != GOL_OK) return st;
            L += l;
            Hs += h;
        }
        *live = L;
        *hash = Hs;
        return GOL_OK;
    }
    HIP_TRY(hipSetDevice(e->device));
    GOL_TRY(join_side_streams(e));
    HIP_TRY(hipMemsetAsync(e->d_acc, 0, 2 * sizeof(unsigned long long), e->stream));
    for (const auto& r : e->user_regions)
        HIP_TRY(gol::launch_digest(e->buf[e->cur], (int64_t)e->stride, (int64_t)e->wq,
                                   (int64_t)e->ng, (int64_t)r.buf_row, (int64_t)r.glob_row,
                                   (int64_t)r.rows, e->d_acc, e->planes, e->stream));
    unsigned long long acc[2];
    HIP_TRY(hipMemcpyAsync(acc, e->d_acc, sizeof(acc), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    *live = acc[0];
    *hash = acc[1];
    return check_err(e);
}

gol_status gol_digest_rows(gol_engine* e, uint64_t row0, uint64_t rows, uint64_t* live,
                           uint64_t* hash)
{
    if (!e || !live || !hash) return fail(GOL_EINVAL, "null argument");
    if (row0 > e->H || rows > e->H - row0) return fail(GOL_EINVAL, "rows outside the field");
    if (e->inner) return torus_digest_rows(e, row0, rows, live, hash);
    if (!e->parts.empty()) {
        uint64_t L = 0, Hs = 0;
        for (auto* p : e->parts) {
            uint64_t l, h;
            gol_status st = gol_digest_rows(p, row0, rows, &l, &h);
            if (st != GOL_OK) return st;
            L += l;
            Hs += h;
        }
        *live = L;
        *hash = Hs;
        return GOL_OK;
    }
    HIP_TRY(hipSetDevice(e->device));
    GOL_TRY(join_side_streams(e));
    HIP_TRY(hipMemsetAsync(e->d_acc, 0, 2 * sizeof(unsigned long long), e->stream));
    for (const auto& r : e->user_regions) {
        // the field rows of this region inside [row0, row0 + rows)
        const uint64_t lo = std::max<uint64_t>(r.glob_row, row0);
        const uint64_t hi = std::min<uint64_t>(r.glob_row + r.rows, row0 + rows);
        if (hi <= lo) continue;
        HIP_TRY(gol::launch_digest(e->buf[e->cur], (int64_t)e->stride, (int64_t)e->wq,
                                   (int64_t)e->ng, (int64_t)(r.buf_row + (lo - r.glob_row)),
                                   (int64_t)lo, (int64_t)(hi - lo), e->d_acc, e->planes,
                                   e->stream));
    }
    unsigned long long acc[2];
    HIP_TRY(hipMemcpyAsync(acc, e->d_acc, sizeof(acc), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    *live = acc[0];
    *hash = acc[1];
    return check_err(e);
}

}  // extern "C"

// ---- Region I/O: gol_read_rect / gol_write_rect / gol_density.  A call
// becomes non-wrapping pieces in the coordinates of a leaf engine (one with
// buffers); a piece is cut along the leaf's regions, whose rows are contiguous in
// the buffer, and each cut runs one kernel on a staging buffer of the cut's size.
namespace golh __attribute__((visibility("hidden"))) {

// Device staging of one cut.  Up to kRectStageKeep bytes it is the engine's own
// buffer, kept and grown between calls (every use ends with the stream idle), so a
// small read, write or density pays no allocation; a larger one is transient.
constexpr size_t kRectStageKeep = 64u << 20;
struct RectStage {
    char* p = nullptr;
    bool own = false;
    ~RectStage()
    {
        if (own && p) (void)hipFree(p);
    }
};

static gol_status rect_stage(gol_engine* e, size_t bytes, RectStage* s)
{
    if (bytes > kRectStageKeep) {
        HIP_TRY(hipMalloc(&s->p, bytes));
        s->own = true;
        return GOL_OK;
    }
    if (e->rect_stage_bytes < bytes) {
        if (e->rect_stage) HIP_TRY(hipFree(e->rect_stage));
        e->rect_stage = nullptr;
        e->rect_stage_bytes = 0;
        HIP_TRY(hipMalloc(&e->rect_stage, bytes));
        e->rect_stage_bytes = bytes;
    }
    s->p = e->rect_stage;
    return GOL_OK;
}

// rows of region r inside the piece: field rows [*lo, *hi)
static bool piece_rows(const Region& r, const RectPiece& p, uint64_t* lo, uint64_t* hi)
{
    *lo = std::max<uint64_t>(r.glob_row, p.frow);
    *hi = std::min<uint64_t>(r.glob_row + r.rows, p.frow + p.rows);
    return *hi > *lo;
}

gol_status leaf_read(gol_engine* e, const std::vector<Region>& regs, uint64_t word_off,
                     const RectPiece* pcs, size_t npc, uint64_t* words, uint64_t rs)
{
    HIP_TRY(hipSetDevice(e->device));
    GOL_TRY(join_side_streams(e));
    std::vector<uint64_t> tmp;
    for (size_t k = 0; k < npc; ++k) {
        const RectPiece& p = pcs[k];
        const uint64_t pw = (p.cols + 63) / 64;
        for (const auto& r : regs) {
            uint64_t lo, hi;
            if (!piece_rows(r, p, &lo, &hi) || !p.cols) continue;
            const uint64_t n = hi - lo;
            RectStage d;
            GOL_TRY(rect_stage(e, (size_t)n * pw * 8, &d));
            HIP_TRY(gol::launch_rect_read(e->buf[e->cur] + word_off, (int64_t)e->stride,
                                          (int64_t)(r.buf_row + (lo - r.glob_row)),
                                          (int64_t)p.fcol, (int64_t)n, (int64_t)p.cols,
                                          (uint64_t*)d.p, (int64_t)pw, e->planes, e->stream));
            tmp.resize((size_t)n * pw);
            HIP_TRY(hipMemcpyAsync(tmp.data(), d.p, tmp.size() * 8, hipMemcpyDeviceToHost,
                                   e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
            for (uint64_t i = 0; i < n; ++i)
                gol_rect_blit_row(tmp.data() + i * pw, 0, words + (p.wrow + lo - p.frow + i) * rs,
                                  (int64_t)p.wcol, (int64_t)p.cols, GOL_RECT_SET);
        }
    }
    return check_err(e);
}

gol_status leaf_write(gol_engine* e, const std::vector<Region>& regs, uint64_t word_off,
                      const RectPiece* pcs, size_t npc, const uint64_t* words, uint64_t rs,
                      uint32_t op)
{
    // as a load: every stream of the engine finished, and the next step of a stripe
    // engine exchanges halos first (whether or not the rectangle meets its rows)
    GOL_TRY(quiesce(e));
    GOL_TRY(twin_clear(e));
    std::vector<uint64_t> tmp;
    for (size_t k = 0; k < npc; ++k) {
        const RectPiece& p = pcs[k];
        const uint64_t pw = (p.cols + 63) / 64;
        for (const auto& r : regs) {
            uint64_t lo, hi;
            if (!piece_rows(r, p, &lo, &hi) || !p.cols) continue;
            const uint64_t n = hi - lo;
            tmp.assign((size_t)n * pw, 0);
            for (uint64_t i = 0; i < n; ++i)
                gol_rect_blit_row(words + (p.wrow + lo - p.frow + i) * rs, (int64_t)p.wcol,
                                  tmp.data() + i * pw, 0, (int64_t)p.cols, GOL_RECT_SET);
            RectStage d;
            GOL_TRY(rect_stage(e, tmp.size() * 8, &d));
            HIP_TRY(hipMemcpyAsync(d.p, tmp.data(), tmp.size() * 8, hipMemcpyHostToDevice,
                                   e->stream));
            HIP_TRY(gol::launch_rect_write(e->buf[e->cur] + word_off, (int64_t)e->stride,
                                           (int64_t)(r.buf_row + (lo - r.glob_row)),
                                           (int64_t)p.fcol, (int64_t)n, (int64_t)p.cols,
                                           (const uint64_t*)d.p, (int64_t)pw, op, e->planes,
                                           e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
        }
    }
    return GOL_OK;
}

// Adds the pieces' live cells to counts (nby x nbx blocks, row stride cs).
gol_status leaf_density(gol_engine* e, const std::vector<Region>& regs, uint64_t word_off,
                        const RectPiece* pcs, size_t npc, uint64_t by, uint64_t bx, uint64_t nby,
                        uint64_t nbx, uint32_t* counts, uint64_t cs)
{
    HIP_TRY(hipSetDevice(e->device));
    GOL_TRY(join_side_streams(e));
    RectStage d;
    const size_t bytes = (size_t)nby * nbx * sizeof(uint32_t);
    GOL_TRY(rect_stage(e, bytes, &d));
    HIP_TRY(hipMemsetAsync(d.p, 0, bytes, e->stream));
    bool any = false;
    for (size_t k = 0; k < npc; ++k) {
        const RectPiece& p = pcs[k];
        for (const auto& r : regs) {
            uint64_t lo, hi;
            if (!piece_rows(r, p, &lo, &hi) || !p.cols) continue;
            any = true;
            HIP_TRY(gol::launch_density(e->buf[e->cur] + word_off, (int64_t)e->stride,
                                        (int64_t)(r.buf_row + (lo - r.glob_row)), (int64_t)p.fcol,
                                        (int64_t)(hi - lo), (int64_t)p.cols,
                                        (int64_t)(p.wrow + lo - p.frow), (int64_t)p.wcol,
                                        (int64_t)by, (int64_t)bx, (uint32_t*)d.p, (int64_t)nbx,
                                        e->planes, e->stream));
        }
    }
    if (any) {
        std::vector<uint32_t> tmp((size_t)nby * nbx);
        HIP_TRY(hipMemcpyAsync(tmp.data(), d.p, bytes, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        for (uint64_t i = 0; i < nby; ++i)
            for (uint64_t j = 0; j < nbx; ++j) counts[i * cs + j] += tmp[i * nbx + j];
    }
    return check_err(e);
}

// The call on an engine of gol_create / gol_create_rank / a group: a composite
// engine hands the piece to every part, a leaf applies it to its own rows.
static gol_status read_own(gol_engine* e, const RectPiece& p, uint64_t* words, uint64_t rs)
{
    for (auto* part : e->parts) GOL_TRY(read_own(part, p, words, rs));
    if (!e->parts.empty()) return GOL_OK;
    return leaf_read(e, e->user_regions, 0, &p, 1, words, rs);
}

static gol_status write_own(gol_engine* e, const RectPiece& p, const uint64_t* words, uint64_t rs,
                            uint32_t op)
{
    for (auto* part : e->parts) GOL_TRY(write_own(part, p, words, rs, op));
    if (!e->parts.empty()) return GOL_OK;
    return leaf_write(e, e->user_regions, 0, &p, 1, words, rs, op);
}

static gol_status density_own(gol_engine* e, const RectPiece& p, uint64_t by, uint64_t bx,
                              uint64_t nby, uint64_t nbx, uint32_t* counts, uint64_t cs)
{
    for (auto* part : e->parts) GOL_TRY(density_own(part, p, by, bx, nby, nbx, counts, cs));
    if (!e->parts.empty()) return GOL_OK;
    return leaf_density(e, e->user_regions, 0, &p, 1, by, bx, nby, nbx, counts, cs);
}

// Bounds of a rectangle: inside the field, or on a torus any start inside it and
// at most one period each way.
static gol_status rect_bounds(const gol_engine* e, uint64_t y, uint64_t x, uint64_t rh, uint64_t rw)
{
    const bool ok = e->inner ? (y < e->H && x < e->W && rh <= e->H && rw <= e->W)
                             : (y <= e->H && rh <= e->H - y && x <= e->W && rw <= e->W - x);
    if (ok) return GOL_OK;
    return fail(GOL_EINVAL, "rectangle " + std::to_string(rh) + " x " + std::to_string(rw) +
                                " at (" + std::to_string(y) + ", " + std::to_string(x) +
                                ") is outside the " + std::to_string(e->H) + " x " +
                                std::to_string(e->W) + (e->inner ? " torus" : " field"));
}

// The plan that the gol_plan_* getters and gol_info describe, and in `e` the
// engine that owns it: the inner engine of a torus, the first part of a composite
// engine; of a rank engine plans[Hx - 1], the full-round launch over its own rows
// (the band and interior plans come after it), else plans[0].  Null: no plan.
static const gol_engine::Plan* described_plan(gol_engine*& e)
{
    while (e->inner || !e->parts.empty()) e = e->inner ? e->inner : e->parts[0];
    if (e->plans.empty()) return nullptr;
    return e->nranks > 1 ? &e->plans[e->Hx - 1] : &e->plans[0];
}

}  // namespace golh

extern "C" {

gol_status gol_read_rect(gol_engine* e, uint64_t y, uint64_t x, uint64_t rh, uint64_t rw,
                         uint64_t* words, uint64_t rs)
{
    if (!e) return fail(GOL_EINVAL, "null engine");
    GOL_TRY(rect_bounds(e, y, x, rh, rw));
    const uint64_t ww = (rw + 63) / 64;
    if (rs < ww) return fail(GOL_EINVAL, "row stride smaller than ceil(rw/64)");
    if (rh == 0 || rw == 0) return GOL_OK;
    if (!words) return fail(GOL_EINVAL, "null argument");
    // pad bits and the rows of a rank engine that are not its own read as 0
    for (uint64_t i = 0; i < rh; ++i) std::memset(words + i * rs, 0, ww * 8);
    if (e->inner) return torus_read_rect(e, y, x, rh, rw, words, rs);
    return read_own(e, RectPiece{y, x, rh, rw, 0, 0}, words, rs);
}

gol_status gol_write_rect(gol_engine* e, uint64_t y, uint64_t x, uint64_t rh, uint64_t rw,
                          const uint64_t* words, uint64_t rs, uint32_t op)
{
    if (!e) return fail(GOL_EINVAL, "null engine");
    if (op > GOL_RECT_CLEAR) return fail(GOL_EINVAL, "unknown rectangle op " + std::to_string(op));
    if (e->sem == GOL_SEM_REF_STRIPES)
        return fail(GOL_ESTATE, "REF_STRIPES keeps the stripes' overlap rows twice: a cell to "
                                "write is ambiguous");
    GOL_TRY(rect_bounds(e, y, x, rh, rw));
    if (rs < (rw + 63) / 64) return fail(GOL_EINVAL, "row stride smaller than ceil(rw/64)");
    if (rh == 0 || rw == 0) return GOL_OK;
    if (!words) return fail(GOL_EINVAL, "null argument");
    if (e->inner) return torus_write_rect(e, y, x, rh, rw, words, rs, op);
    return write_own(e, RectPiece{y, x, rh, rw, 0, 0}, words, rs, op);
}

gol_status gol_density(gol_engine* e, uint64_t y, uint64_t x, uint64_t rh, uint64_t rw,
                       uint64_t by, uint64_t bx, uint32_t* counts, uint64_t cs)
{
    if (!e || !counts) return fail(GOL_EINVAL, "null argument");
    if (by == 0 || bx == 0 || rh == 0 || rw == 0)
        return fail(GOL_EINVAL, "density needs a window and blocks of at least one cell");
    if (by > UINT32_MAX / bx) return fail(GOL_EINVAL, "density blocks of more than 2^32 - 1 cells");
    GOL_TRY(rect_bounds(e, y, x, rh, rw));
    const uint64_t nby = (rh + by - 1) / by, nbx = (rw + bx - 1) / bx;
    if (cs < nbx) return fail(GOL_EINVAL, "row stride smaller than ceil(rw/bx)");
    for (uint64_t i = 0; i < nby; ++i) std::memset(counts + i * cs, 0, nbx * sizeof(uint32_t));
    if (e->inner) return torus_density(e, y, x, rh, rw, by, bx, nby, nbx, counts, cs);
    return density_own(e, RectPiece{y, x, rh, rw, 0, 0}, by, bx, nby, nbx, counts, cs);
}

gol_status gol_rect_blit(const uint64_t* src, uint64_t src_stride, uint64_t sx, uint64_t* dst,
                         uint64_t dst_stride, uint64_t dx, uint64_t rows, uint64_t cols,
                         uint32_t op)
{
    if (op > GOL_RECT_CLEAR) return fail(GOL_EINVAL, "unknown rectangle op " + std::to_string(op));
    if (sx > (1ull << 62) || dx > (1ull << 62) || cols > (1ull << 62))
        return fail(GOL_EINVAL, "bit offsets too large");
    if (src_stride < (sx + cols + 63) / 64 || dst_stride < (dx + cols + 63) / 64)
        return fail(GOL_EINVAL, "row stride smaller than the words that hold the bits");
    if (rows == 0 || cols == 0) return GOL_OK;
    if (!src || !dst) return fail(GOL_EINVAL, "null argument");
    for (uint64_t i = 0; i < rows; ++i)
        gol_rect_blit_row(src + i * src_stride, (int64_t)sx, dst + i * dst_stride, (int64_t)dx,
                          (int64_t)cols, op);
    return GOL_OK;
}


gol_status gol_plan_tuning(gol_engine* e, uint32_t* variant, float* tuned_us, float* model_us)
{
    if (!e) return fail(GOL_EINVAL, "null engine");
    if (e->inner) return gol_plan_tuning(e->inner, variant, tuned_us, model_us);
    if (!e->parts.empty()) return gol_plan_tuning(e->parts[0], variant, tuned_us, model_us);
    if (e->plans.empty()) return fail(GOL_ESTATE, "no launch plan");
    const bool rk = e->nranks > 1 && e->Hx >= e->K;
    const auto& p = rk ? e->plans[e->K - 1] : e->plans[0];
    const bool on = !e->res.on;
    if (variant) *variant = on ? (uint32_t)p.tuned : 0u;
    if (tuned_us) *tuned_us = on ? 1e3f * p.tune_ms : 0.f;
    if (model_us) *model_us = on ? 1e3f * p.tune_ms_model : 0.f;
    return GOL_OK;
}


gol_status gol_plan_passes(gol_engine* e, uint32_t* passes)
{
    if (!e || !passes) return fail(GOL_EINVAL, "null argument");
    if (e->inner) return gol_plan_passes(e->inner, passes);
    if (!e->parts.empty()) return gol_plan_passes(e->parts[0], passes);
    if (e->plans.empty()) return fail(GOL_ESTATE, "no launch plan");
    const bool rk = e->nranks > 1 && e->Hx >= e->K;
    const auto& p = rk ? e->plans[e->K - 1] : e->plans[0];
    *passes = e->res.on ? 1u : (uint32_t)p.npass;
    return GOL_OK;
}

gol_status gol_set_timing(gol_engine* e, int every)
{
    if (!e) return fail(GOL_EINVAL, "null engine");
    if (e->inner) return gol_set_timing(e->inner, every);
    if (!e->parts.empty()) {
        for (auto* p : e->parts) {
            gol_status st = gol_set_timing(p, every);
            if (st != GOL_OK) return st;
        }
        return GOL_OK;
    }
    if (every < 0) return fail(GOL_EINVAL, "timing sample interval must be >= 0");
    e->timing_every = (uint32_t)every;
    e->traits.timing_every = e->timing_every;  // the one trait of a step that changes after create
    e->launch_count = 0;
    return GOL_OK;
}

// Copy a timing record into the caller's struct: all of it when the caller says it
// has this header's layout (struct_size), else the r04 prefix only.
static void put_timing(gol_timing* out, const gol_timing& t)
{
    if (out->struct_size == (uint32_t)sizeof(gol_timing)) {
        *out = t;
        out->struct_size = (uint32_t)sizeof(gol_timing);
    } else {
        static_assert(offsetof(gol_timing, struct_size) + sizeof(uint32_t) == GOL_TIMING_R04_BYTES,
                      "r04 gol_timing prefix");
        std::memcpy(out, &t, offsetof(gol_timing, struct_size));
        out->struct_size = GOL_TIMING_R04_BYTES;
    }
}

gol_status gol_get_timing(gol_engine* e, gol_timing* out)
{
    if (!e || !out) return fail(GOL_EINVAL, "null argument");
    if (e->inner) return gol_get_timing(e->inner, out);
    if (!e->parts.empty()) {
        gol_timing t{};
        for (auto* p : e->parts) {
            gol_timing pt{};
            pt.struct_size = (uint32_t)sizeof(gol_timing);
            gol_status st = gol_get_timing(p, &pt);
            if (st != GOL_OK) return st;
            t.launches += pt.launches;
            t.kernel_ms += pt.kernel_ms;
            t.cell_gens += pt.cell_gens;
            t.cell_gens_computed += pt.cell_gens_computed;
            t.launches_issued += pt.launches_issued;
            t.launch_rows += pt.launch_rows;
            t.exchanges += pt.exchanges;
            t.exchange_ms += pt.exchange_ms;
            t.rounds += pt.rounds;
            t.round_ms += pt.round_ms;
            t.exchange_exposed_ms += pt.exchange_exposed_ms;
        }
        t.streams = (uint32_t)e->parts.size();
        put_timing(out, t);
        return GOL_OK;
    }
    gol_status st = flush_timing(e);
    if (st != GOL_OK) return st;
    gol_timing t = e->tm;
    t.streams = 1;
    put_timing(out, t);
    return GOL_OK;
}

gol_status gol_reset_timing(gol_engine* e)
{
    if (!e) return fail(GOL_EINVAL, "null engine");
    if (e->inner) return gol_reset_timing(e->inner);
    if (!e->parts.empty()) {
        for (auto* p : e->parts) {
            gol_status st = gol_reset_timing(p);
            if (st != GOL_OK) return st;
        }
        return GOL_OK;
    }
    gol_status st = flush_timing(e);
    if (st != GOL_OK) return st;
    e->tm = gol_timing{};
    if (e->d_streak) {
        HIP_TRY(hipSetDevice(e->device));
        // pending fixed steps count before the reset, and leave their state words
        GOL_TRY(flush_still(e));
        // Every counter: computed / skipped, copied and busy[0] lie one after the
        // other, the probed ones behind busy[1], the elided ones behind the pass's and
        // the probe's flags, the probe pass's behind its words.  The streaks, the
        // flags, the words and busy[1] are not statistics but the skip's own state
        // within a step, which each step's first launch starts afresh: a reset
        // leaves them alone.
        const ActState as{e->d_streak, (size_t)e->act_units};
        HIP_TRY(hipMemsetAsync(as.act(), 0, (size_t)(as.busy() + 1 - as.act()) * sizeof(uint32_t),
                               e->stream));
        HIP_TRY(hipMemsetAsync(as.probed(), 0, as.units * sizeof(uint32_t), e->stream));
        HIP_TRY(hipMemsetAsync(as.elided(), 0, as.units * sizeof(uint32_t), e->stream));
        HIP_TRY(hipMemsetAsync(as.pass_probed(), 0, as.units * sizeof(uint32_t), e->stream));
        // (twin[] and twin_ok are state across steps, not statistics: left alone too)
        if (e->d_kept)
            HIP_TRY(hipMemsetAsync(e->d_kept, 0, (size_t)e->kept_tiles * sizeof(uint32_t), e->stream));
        if (e->d_sure)
            HIP_TRY(hipMemsetAsync(e->d_sure, 0, (size_t)e->kept_tiles * sizeof(uint32_t), e->stream));
    }
    e->short_steps = 0;
    e->fixed_steps = 0;
    e->fixed_passes = 0;
    e->fixed_launches = 0;
    return GOL_OK;
}

gol_status gol_info(gol_engine* e, uint64_t* h, uint64_t* w, uint64_t* row0, uint64_t* rows,
                    uint32_t* tb_depth, uint32_t* halo_depth, uint32_t* rows_per_wave)
{
    if (!e) return fail(GOL_EINVAL, "null engine");
    if (e->inner) {  // the interior, the inner engine's depth, G
        GOL_TRY(gol_info(e->inner, nullptr, nullptr, nullptr, nullptr, tb_depth, nullptr,
                         rows_per_wave));
        if (h) *h = e->H;
        if (w) *w = e->W;
        if (row0) *row0 = 0;
        if (rows) *rows = e->H;
        if (halo_depth) *halo_depth = (uint32_t)e->tG;
        return GOL_OK;
    }
    if (!e->parts.empty()) {
        gol_status st = gol_info(e->parts[0], nullptr, nullptr, nullptr, nullptr, tb_depth,
                                 halo_depth, rows_per_wave);
        if (st != GOL_OK) return st;
        if (h) *h = e->H;
        if (w) *w = e->W;
        if (row0) *row0 = 0;
        if (rows) *rows = e->H;
        return GOL_OK;
    }
    // (a rank engine that holds fewer than its Hx round plans: the last it has)
    const bool last =
        e->nranks > 1 && !(e->Hx >= 1 && e->plans.size() >= e->Hx) && !e->plans.empty();
    const gol_engine::Plan* p = last ? &e->plans.back() : described_plan(e);
    if (rows_per_wave) *rows_per_wave = e->res.on ? (uint32_t)e->res.rows : p ? (uint32_t)p->rpw : 0;
    if (h) *h = e->H;
    if (w) *w = e->W;
    if (row0) *row0 = e->row0;
    if (rows) *rows = e->nranks > 1 ? e->R : e->H;
    if (tb_depth) *tb_depth = e->K;
    if (halo_depth) *halo_depth = (uint32_t)e->Hx;
    return GOL_OK;
}

gol_status gol_plan_info(gol_engine* e, uint32_t* strip_lanes, uint32_t* rows_per_wave,
                         uint32_t* word_planes)
{
    if (!e) return fail(GOL_EINVAL, "null engine");
    const gol_engine::Plan* pp = described_plan(e);
    if (word_planes) *word_planes = (uint32_t)e->planes;
    if (!pp) return fail(GOL_ESTATE, "no launch plan");
    const auto& p = *pp;
    if (strip_lanes) *strip_lanes = e->res.on ? 64u : (uint32_t)(64 >> p.lane_shift);
    if (rows_per_wave) *rows_per_wave = e->res.on ? (uint32_t)e->res.rows : (uint32_t)p.rpw;
    return GOL_OK;
}

gol_status gol_plan_skew(gol_engine* e, uint32_t* rows_old, uint32_t* rows_young,
                         uint32_t* units_old)
{
    if (!e) return fail(GOL_EINVAL, "null engine");
    const gol_engine::Plan* pp = described_plan(e);
    if (!pp) return fail(GOL_ESTATE, "no launch plan");
    const auto& p = *pp;
    const bool on = !e->res.on && p.rows_old;
    if (rows_old) *rows_old = on ? (uint32_t)p.rows_old : 0u;
    if (rows_young) *rows_young = on ? (uint32_t)p.rows_young : 0u;
    if (units_old) *units_old = on ? (uint32_t)p.units_old : 0u;
    return GOL_OK;
}
gol_status gol_plan_columns(gol_engine* e, uint32_t* strips, uint32_t* half_units,
                            uint32_t* half_groups)
{
    if (!e) return fail(GOL_EINVAL, "null engine");
    const gol_engine::Plan* pp = described_plan(e);
    if (!pp) return fail(GOL_ESTATE, "no launch plan");
    const auto& p = *pp;
    const bool on = !e->res.on;
    if (strips) *strips = on ? (uint32_t)p.groups : (uint32_t)e->res.strips;
    if (half_units) *half_units = on ? (uint32_t)p.pair_units : 0u;
    if (half_groups)
        *half_groups = on && p.pair_units ? (uint32_t)(p.half_hi - p.half_q0) : 0u;
    return GOL_OK;
}

gol_status gol_plan_resident(gol_engine* e, uint32_t* on, uint32_t* bands, uint32_t* strips)
{
    if (!e || !on) return fail(GOL_EINVAL, "null argument");
    if (e->inner) return gol_plan_resident(e->inner, on, bands, strips);
    if (!e->parts.empty()) {
        *on = 0;
        if (bands) *bands = 0;
        if (strips) *strips = 0;
        return GOL_OK;
    }
    *on = e->res.on ? 1u : 0u;
    if (bands) *bands = (uint32_t)e->res.bands;
    if (strips) *strips = (uint32_t)e->res.strips;
    return GOL_OK;
}

gol_status gol_plan_resident_rows(gol_engine* e, uint32_t* rows, uint32_t* band_rows,
                                  uint32_t* epoch, uint32_t* swap_every)
{
    if (!e) return fail(GOL_EINVAL, "null engine");
    if (e->inner) return gol_plan_resident_rows(e->inner, rows, band_rows, epoch, swap_every);
    const bool on = e->parts.empty() && e->res.on;
    if (rows) *rows = on ? (uint32_t)e->res.rows : 0u;
    if (band_rows) *band_rows = on ? (uint32_t)e->res.band_rows : 0u;
    if (epoch) *epoch = on ? (uint32_t)e->res.K : 0u;
    if (swap_every) *swap_every = on ? (uint32_t)e->res.mb : 0u;
    return GOL_OK;
}

gol_status gol_plan_handoff(gol_engine* e, uint32_t* handoff)
{
    if (!e || !handoff) return fail(GOL_EINVAL, "null argument");
    const gol_engine::Plan* pp = described_plan(e);
    if (!pp) return fail(GOL_ESTATE, "no launch plan");
    const auto& p = *pp;
    *handoff = (!e->res.on && p.hand && p.multi_blk && e->side[0] && handoff_fits(p.rpw, (int)e->K, e->planes))
                   ? 1u
                   : 0u;
    return GOL_OK;
}

}  // extern "C"

#if GOL_WAVE_LOG
// GOL_WAVE_LOG builds only: the kernels log 8 words per wavefront into `dev`
// (StepArgs::wlog, ResArgs::wlog; null turns the log off).  Not part of include/gol.h.
extern "C" __attribute__((visibility("default"))) void gol_dev_set_wave_log(void* dev)
{
    g_dev_wave_log = static_cast<uint64_t*>(dev);
}
#endif
