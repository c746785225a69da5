// snapshot.cpp -- the snapshot slot (DESIGN §4 "Snapshots"): gol_snapshot, _same,
// _diff, _restore, _drop, and gol_step_until_periodic built from them and gol_step.
//
// A leaf engine (one with buffers) keeps a device copy of its whole current buffer:
// guard rows, a stripe's halo rows and a torus's ghost cells included, so a restore
// is one copy back and puts the ghosts back too.  The comparisons look at field cells
// only: a leaf's own rows (user_regions) from word 0, or a torus interior at row tG,
// word tGx of its inner engine, the last lane group masked to the field's columns
// (life_snap.hip).  Composite engines route every call to their stripes, which share
// one device, and add the answers up; torus engines route to the inner engine.
#include "engine_internal.h"

namespace golh __attribute__((visibility("hidden"))) {

namespace {

// What one leaf compares: rows of `regs` (field row -> buffer row), `nwords` stored
// words per row from word `word_off` on, the last lane group masked with `mask`
// (gol::SnapArgs::mask).
struct SnapView {
    gol_engine* leaf;
    std::vector<Region> regs;
    uint64_t word_off, nwords;
    uint64_t mask[2];
};

SnapView leaf_view(gol_engine* e)
{
    SnapView v{e, e->user_regions, 0, e->ng * (uint64_t)(e->planes / 2), {~0ull, ~0ull}};
    if (e->planes == 4) {
        v.mask[0] = e->lastmask_split[0];
        v.mask[1] = e->lastmask_split[1];
    } else {
        v.mask[1] = e->lastmask_split[0];
    }
    return v;
}

// The leaves behind an engine of a kind that has a snapshot slot, else GOL_ESTATE.
gol_status snap_views(gol_engine* e, std::vector<SnapView>& out)
{
    if (!e) return fail(GOL_EINVAL, "null engine");
    if (e->inner) {
        // (the interior's last word also holds ghost columns: masked like a store)
        out.push_back(SnapView{e->inner, {Region{e->tG, 0, 0, e->H}}, e->tGx, e->wq,
                               {~0ull, gol_split64(e->lastmask)}});
        return GOL_OK;
    }
    if (!e->parts.empty()) {
        for (auto* p : e->parts) out.push_back(leaf_view(p));
        return GOL_OK;
    }
    if (e->sem == GOL_SEM_REF_STRIPES)
        return fail(GOL_ESTATE, "snapshots: REF_STRIPES keeps the stripes' overlap rows twice; "
                                "there is no one field to keep or compare");
    if (e->grouped || e->nranks > 1)
        return fail(GOL_ESTATE, "snapshots: a rank engine or group member holds a part of the "
                                "field; whether the field repeats is a collective decision");
    out.push_back(leaf_view(e));
    return GOL_OK;
}

size_t slot_bytes(const gol_engine* e)
{
    const size_t words = (size_t)(e->buf_rows + 2 * gol::kGuardRows) * e->stride;
    return (e->npass > 1 ? 2 : 1) * words * sizeof(uint64_t);
}

gol_status need_snapshot(const std::vector<SnapView>& vs)
{
    for (const auto& v : vs)
        if (!v.leaf->snap || !v.leaf->snap_host || !v.leaf->snap_set)
            return fail(GOL_ESTATE, "no snapshot: call gol_snapshot first");
    return GOL_OK;
}

gol_status leaf_snapshot(gol_engine* e)
{
    HIP_TRY(hipSetDevice(e->device));
    if (!e->snap) HIP_TRY(hipMalloc(&e->snap, slot_bytes(e)));
    if (!e->snap_host) HIP_TRY(hipHostMalloc(&e->snap_host, 4 * sizeof(unsigned long long)));
    GOL_TRY(join_side_streams(e));
    HIP_TRY(hipMemcpyAsync(e->snap, e->alloc[e->cur], slot_bytes(e), hipMemcpyDeviceToDevice,
                           e->stream));
    e->snap_set = true;
    return GOL_OK;
}

// A writer of the field like leaf_write: every stream of the engine finished, the
// "rows both buffers hold" record withdrawn, and a stripe's next step exchanges halos
// first (quiesce: halo_fresh = false).  The copy itself is left enqueued.
gol_status leaf_restore(gol_engine* e)
{
    GOL_TRY(quiesce(e));
    GOL_TRY(twin_clear(e));
    HIP_TRY(hipMemcpyAsync(e->alloc[e->cur], e->snap, slot_bytes(e), hipMemcpyDeviceToDevice,
                           e->stream));
    return GOL_OK;
}

// Enqueues the comparison of one leaf on its stream.  The answer lands in the leaf's
// d_acc: word 0 the cell count, the low half of word 1 the "differs" flag.
gol_status compare_begin(const SnapView& v, bool count)
{
    gol_engine* e = v.leaf;
    HIP_TRY(hipSetDevice(e->device));
    GOL_TRY(flush_still(e));  // compare_end reads the error word behind this work
    GOL_TRY(join_side_streams(e));
    HIP_TRY(hipMemsetAsync(e->d_acc, 0, 2 * sizeof(unsigned long long), e->stream));
    for (const auto& r : v.regs) {
        if (r.buf_row + r.rows > e->buf_rows || v.word_off + v.nwords > e->stride)
            return fail(GOL_ESTATE, "snapshot compare: region outside the buffer");
        gol::SnapArgs a{};
        a.cur = e->buf[e->cur];
        a.snap = e->snap + (size_t)gol::kGuardRows * e->stride;
        a.stride = (int64_t)e->stride;
        a.row_base = (int64_t)r.buf_row;
        a.word0 = (int64_t)v.word_off;
        a.nwords = (int64_t)v.nwords;
        a.rows = (int64_t)r.rows;
        a.mask[0] = v.mask[0];
        a.mask[1] = v.mask[1];
        a.flag = reinterpret_cast<uint32_t*>(e->d_acc + 1);
        a.count = e->d_acc;
        HIP_TRY(gol::launch_snap_compare(a, count, e->stream));
    }
    return GOL_OK;
}

gol_status compare_end(const SnapView& v, bool count, uint64_t* out)
{
    gol_engine* e = v.leaf;
    HIP_TRY(hipSetDevice(e->device));
    // one wait for the answer and the kernels' error word, both into pinned memory: a
    // check costs a look, not two blocking copies
    unsigned long long* acc = e->snap_host;
    int* err = reinterpret_cast<int*>(acc + 2);
    *err = 0;
    HIP_TRY(hipMemcpyAsync(acc, e->d_acc, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                           e->stream));
    if (e->d_err)
        HIP_TRY(hipMemcpyAsync(err, e->d_err, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    *out = count ? (uint64_t)acc[0] : (uint64_t)((acc[1] & 0xFFFFFFFFull) != 0);
    return *err ? check_err(e) : GOL_OK;
}

// Every leaf's comparison enqueued before the first is waited for: a composite
// engine's stripes compare side by side on their streams.
gol_status compare(gol_engine* e, bool count, uint64_t* total)
{
    std::vector<SnapView> vs;
    GOL_TRY(snap_views(e, vs));
    GOL_TRY(need_snapshot(vs));
    for (const auto& v : vs) GOL_TRY(compare_begin(v, count));
    uint64_t sum = 0;
    for (const auto& v : vs) {
        uint64_t one = 0;
        GOL_TRY(compare_end(v, count, &one));
        sum += one;
    }
    *total = sum;
    return GOL_OK;
}

}  // namespace

void snapshot_free(gol_engine* e)
{
    if (e->snap) (void)hipFree(e->snap);
    if (e->snap_host) (void)hipHostFree(e->snap_host);
    e->snap = nullptr;
    e->snap_host = nullptr;
    e->snap_set = false;
}

}  // namespace golh

extern "C" {

gol_status gol_snapshot(gol_engine* e)
{
    std::vector<SnapView> vs;
    GOL_TRY(snap_views(e, vs));
    for (const auto& v : vs) GOL_TRY(leaf_snapshot(v.leaf));
    return GOL_OK;
}

gol_status gol_snapshot_same(gol_engine* e, uint32_t* same)
{
    if (!same) return fail(GOL_EINVAL, "null argument");
    uint64_t differing = 0;  // leaves with a difference
    GOL_TRY(compare(e, false, &differing));
    *same = differing == 0 ? 1u : 0u;
    return GOL_OK;
}

gol_status gol_snapshot_diff(gol_engine* e, uint64_t* cells)
{
    if (!cells) return fail(GOL_EINVAL, "null argument");
    return compare(e, true, cells);
}

gol_status gol_snapshot_restore(gol_engine* e)
{
    std::vector<SnapView> vs;
    GOL_TRY(snap_views(e, vs));
    GOL_TRY(need_snapshot(vs));
    for (const auto& v : vs) GOL_TRY(leaf_restore(v.leaf));
    return GOL_OK;
}

gol_status gol_snapshot_drop(gol_engine* e)
{
    std::vector<SnapView> vs;
    GOL_TRY(snap_views(e, vs));
    for (const auto& v : vs) {
        if (!v.leaf->snap) continue;
        // (the slot may still be read or written by work on the leaf's stream)
        HIP_TRY(hipSetDevice(v.leaf->device));
        HIP_TRY(hipStreamSynchronize(v.leaf->stream));
        snapshot_free(v.leaf);
    }
    return GOL_OK;
}

// Only public calls from here on: the driver knows nothing of plans or launches.
gol_status gol_step_until_periodic(gol_engine* e, uint64_t max_generations, uint32_t lag,
                                   uint32_t check_every, uint32_t flags, gol_until* out)
{
    if (!e || !out) return fail(GOL_EINVAL, "null argument");
    if (out->struct_size != sizeof(gol_until))
        return fail(GOL_EINVAL, "gol_until.struct_size must be sizeof(gol_until)");
    if (flags & ~GOL_UNTIL_FINISH) return fail(GOL_EINVAL, "unknown gol_step_until_periodic flag");
    if (lag < 1 || lag > 65536) return fail(GOL_EINVAL, "lag must be 1..65536");
    if (check_every == 0)
        check_every = (lag + 63) / 64 * 64;
    else if (check_every < lag)
        return fail(GOL_EINVAL, "check_every must be 0 or >= lag");
    {
        std::vector<SnapView> vs;  // (an engine kind without a slot: before any step)
        GOL_TRY(snap_views(e, vs));
    }
    gol_until r{};
    r.struct_size = sizeof(gol_until);
    r.lag = lag;
    r.check_every = check_every;
    uint64_t g = 0;
    for (;;) {
        if (check_every > max_generations - g) {  // the next check lies beyond the limit
            if (max_generations > g) GOL_TRY(gol_step(e, max_generations - g));
            r.advanced = max_generations;
            break;
        }
        if (check_every > lag) GOL_TRY(gol_step(e, check_every - lag));
        GOL_TRY(gol_snapshot(e));
        GOL_TRY(gol_step(e, lag));
        uint32_t same = 0;
        GOL_TRY(gol_snapshot_same(e, &same));
        r.checks++;
        g += check_every;
        if (!same) continue;
        // field(g) = field(g - lag), the snapshot: the minimal period divides lag.  Walk
        // on to g + d for lag's proper divisors d, ascending; the first field equal to
        // the snapshot gives it.
        uint32_t p = lag, at = 0;
        for (uint32_t d = 1; d <= lag / 2; ++d) {
            if (lag % d) continue;
            GOL_TRY(gol_step(e, d - at));
            at = d;
            GOL_TRY(gol_snapshot_same(e, &same));
            if (same) {
                p = d;
                break;
            }
        }
        r.extra_generations = at;
        if (at) GOL_TRY(gol_snapshot_restore(e));
        r.period = p;
        r.advanced = g;
        if (flags & GOL_UNTIL_FINISH) {
            const uint64_t rest = (max_generations - g) % p;
            if (rest) GOL_TRY(gol_step(e, rest));
        }
        break;
    }
    *out = r;
    return GOL_OK;
}

}  // extern "C"
