// batch.cpp -- gol_batch: n independent h x w fields of one rule and one boundary,
// held on the device in the batch kernel's order and advanced together by one
// life_batch_kernel launch per (at most) launch_generations generations (life_batch.h,
// DESIGN §4 "life_batch_kernel").  Argument checks and the fixed geometry are host
// code that never touches the GPU; the host forms of load and store are the device
// forms behind a compact staging buffer.  gol_batch_step_until_periodic drives
// life_batch_until_kernel (life_batch_until.h) launch by launch, by the host-only plan
// of gol_batch_until_plan_of.  With a rule table (gol_batch_set_rules) both step by
// life_batch_rules.h's kernels, which read every field's rule from the table.
// gol_batch_step_trace drives life_batch_trace_kernel (life_batch_trace.h) by the host-only
// plan of gol_batch_trace_plan_of; gol_batch_step_record drives life_batch_record_kernel
// (life_batch_record.h) by the same plan.
#include <cstdlib>
#include <cstring>
#include <new>

#include "engine_internal.h"
#include "life_batch.h"
#include "life_batch_until.h"
#include "life_batch_rules.h"
#include "life_batch_trace.h"
#include "life_batch_record.h"

struct gol_batch {
    int device = 0;
    hipStream_t stream = nullptr;
    uint64_t n = 0, h = 0, w = 0, wq = 0, waves = 0;
    uint32_t lpf = 1, lpf_shift = 0, fpw = 64, rows = 8;
    uint32_t launch_gens = 0;
    uint32_t birth = 0, survive = 0, sem = GOL_SEM_GLOBAL;
    gol::RuleKind rule = gol::RULE_REF;
    uint64_t* buf = nullptr;
    // staging for the host forms of load / store and for the digests, kept between calls
    uint64_t* stage = nullptr;
    size_t stage_words = 0;
    // gol_batch_step_until_periodic, allocated by its first call: the snapshot buffer (as
    // large as buf) and one block of [counters | generation[n] | period[n] | done[waves]];
    // `counters`: where the block's counters start from and are read back to
    uint64_t* snap = nullptr;
    unsigned char* until = nullptr;
    gol::BatchUntilCounters counters = {};
    // gol_batch_set_rules: field f's birth | survive << 16, [n] words; null = every field
    // steps by the create rule
    uint32_t* rules = nullptr;
    // gol_batch_step_trace's host form: the samples on the device ([samples][n] words),
    // allocated by its first call and grown on demand
    uint32_t* trace = nullptr;
    size_t trace_words = 0;
    // gol_batch_step_record's host form: the frames on the device, compact
    // ([samples][count][h][wq] words), allocated by its first call and grown on demand
    uint64_t* record = nullptr;
    size_t record_words = 0;
};

namespace golh __attribute__((visibility("hidden"))) {

namespace {

// Generations per launch unless GOL_DEV_BATCH_LAUNCH_GENS says otherwise: a launch of
// the 64-row B3/S23 kernel stays far below 100 ms.
constexpr uint32_t kBatchLaunchGens = 4096;

struct BatchShape {
    uint32_t lpf, lpf_shift, fpw, rows;
    uint64_t wq, waves;
};

// The checks and the geometry gol_batch_geometry and gol_batch_create share.
gol_status batch_shape(uint64_t n, uint64_t h, uint64_t w, const gol_config* cfg, BatchShape* s)
{
    if (!cfg) return fail(GOL_EINVAL, "null config");
    if (cfg->birth_mask >= 512 || cfg->survive_mask >= 512)
        return fail(GOL_EINVAL, "rule masks are 9-bit");
    if (cfg->semantics != GOL_SEM_GLOBAL && cfg->semantics != GOL_SEM_TORUS)
        return fail(GOL_EINVAL, "a batch is GOL_SEM_GLOBAL (dead border per field) or "
                                "GOL_SEM_TORUS (torus per field)");
    if (cfg->ref_ranks > 1 || cfg->tb_depth || cfg->halo_depth || cfg->rows_per_wave ||
        cfg->handoff || cfg->streams || cfg->strip_lanes || cfg->word_planes || cfg->resident ||
        cfg->exchange_overlap)
        return fail(GOL_EINVAL, "a batch has no plan knobs: every gol_config field but the rule, "
                                "device and semantics must be 0");
    if (n == 0 || h == 0 || w == 0) return fail(GOL_EINVAL, "n, h and w must be >= 1");
    if (h > 64 || w > 4096)
        return fail(GOL_EINVAL, "a batch holds fields of at most 64 rows x 4096 columns; "
                                "gol_create is the engine for larger fields");
    s->wq = (w + 63) / 64;
    s->lpf = 1;
    s->lpf_shift = 0;
    while (s->lpf < s->wq) {
        s->lpf *= 2;
        s->lpf_shift += 1;
    }
    s->fpw = 64 / s->lpf;
    s->rows = 8;
    while (s->rows < h) s->rows *= 2;
    if (n > (1ull << 31) / s->lpf)
        return fail(GOL_EINVAL, "batch too large: n * lanes_per_field must be <= 2^31; "
                                "gol_create is the engine for larger fields");
    s->waves = (n + s->fpw - 1) / s->fpw;
    return GOL_OK;
}

gol::BatchGeom geom_of(const gol_batch* b)
{
    return gol::BatchGeom{b->buf, (int64_t)b->n, (int32_t)b->h, (int32_t)b->wq,
                          (int32_t)b->lpf_shift, last_mask(b->w)};
}

gol_status check_range(const gol_batch* b, uint64_t first, uint64_t count, const void* words,
                       uint64_t fs, uint64_t rs)
{
    if (!b) return fail(GOL_EINVAL, "null batch");
    if (first > b->n || count > b->n - first)
        return fail(GOL_EINVAL, "first + count exceeds the batch's fields");
    if (rs < b->wq) return fail(GOL_EINVAL, "row_stride_words < ceil(w/64)");
    if (fs < b->h * rs) return fail(GOL_EINVAL, "field_stride_words < h * row_stride_words");
    if (count && !words) return fail(GOL_EINVAL, "null words");
    return GOL_OK;
}

gol_status need_stage(gol_batch* b, size_t words)
{
    if (b->stage_words >= words) return GOL_OK;
    if (b->stage) {
        HIP_TRY(hipStreamSynchronize(b->stream));
        (void)hipFree(b->stage);
        b->stage = nullptr;
        b->stage_words = 0;
    }
    HIP_TRY(hipMalloc(&b->stage, words * sizeof(uint64_t)));
    b->stage_words = words;
    return GOL_OK;
}

// Host words <-> the compact staging image ([count][h][wq] words): one linear copy when
// the caller's image has no padding, one 2-D copy when its fields follow each other row
// after row, else one 2-D copy per field.
gol_status stage_copy(gol_batch* b, uint64_t count, uint64_t* host, uint64_t fs, uint64_t rs,
                      bool to_device)
{
    const size_t rowb = b->wq * 8;
    if (rs == b->wq && fs == b->h * rs) {
        // the caller's image is the staging image: one linear copy
        const size_t bytes = (size_t)count * b->h * rowb;
        if (to_device)
            HIP_TRY(hipMemcpyAsync(b->stage, host, bytes, hipMemcpyHostToDevice, b->stream));
        else
            HIP_TRY(hipMemcpyAsync(host, b->stage, bytes, hipMemcpyDeviceToHost, b->stream));
        return GOL_OK;
    }
    const bool flat = fs == b->h * rs;
    const uint64_t pieces = flat ? 1 : count, rows = flat ? count * b->h : b->h;
    for (uint64_t i = 0; i < pieces; ++i) {
        uint64_t* hp = host + i * fs;
        uint64_t* dp = b->stage + i * b->h * b->wq;
        if (to_device)
            HIP_TRY(hipMemcpy2DAsync(dp, rowb, hp, rs * 8, rowb, rows, hipMemcpyHostToDevice,
                                     b->stream));
        else
            HIP_TRY(hipMemcpy2DAsync(hp, rs * 8, dp, rowb, rowb, rows, hipMemcpyDeviceToHost,
                                     b->stream));
    }
    return GOL_OK;
}

gol::BatchArgs args_of(const gol_batch* b)
{
    gol::BatchArgs a{};
    a.buf = b->buf;
    a.waves = (int64_t)b->waves;
    a.n = (int64_t)b->n;
    a.h = (int32_t)b->h;
    a.w = (int32_t)b->w;
    a.wq = (int32_t)b->wq;
    a.lpf_shift = (int32_t)b->lpf_shift;
    a.torus = b->sem == GOL_SEM_TORUS;
    a.birth = b->birth;
    a.survive = b->survive;
    a.lastmask = gol_split64(last_mask(b->w));
    return a;
}

// The checks gol_batch_step_until_periodic and gol_batch_until_plan_of share;
// *check_every: resolved from 0.
gol_status until_args(uint32_t lag, uint32_t* check_every)
{
    if (lag < 1 || lag > gol::kBatchUntilMaxLag)
        return fail(GOL_EINVAL, "a batch's lag must be 1..1024 (its proper divisors travel in "
                                "the kernel's arguments)");
    if (*check_every == 0)
        *check_every = (lag + 63) / 64 * 64;
    else if (*check_every < lag)
        return fail(GOL_EINVAL, "check_every must be 0 or >= lag");
    if (*check_every > 65536) return fail(GOL_EINVAL, "a batch's check_every must be <= 65536");
    return GOL_OK;
}

// The checks gol_batch_step_trace, its device form and gol_batch_trace_plan_of share.
gol_status trace_every(uint32_t every)
{
    if (every == 0 || every > gol::kBatchTraceMaxEvery)
        return fail(GOL_EINVAL, "a batch trace's `every` must be 1..65536");
    return GOL_OK;
}

// Every GOL_EINVAL of gol_batch_step_trace and its device form, in the header's order;
// *plan: the call's launches.
gol_status trace_check(const gol_batch* b, uint64_t generations, uint32_t every,
                       const uint32_t* live, uint64_t stride, const gol_batch_trace* out,
                       gol_batch_trace_plan* plan)
{
    if (!b) return fail(GOL_EINVAL, "null batch");
    if (!out) return fail(GOL_EINVAL, "null out");
    if (out->struct_size != sizeof(gol_batch_trace))
        return fail(GOL_EINVAL, "gol_batch_trace.struct_size must be sizeof(gol_batch_trace)");
    GOL_TRY(trace_every(every));
    GOL_TRY(gol_batch_trace_plan_of(generations, every, b->launch_gens, plan));
    if (plan->samples > 0) {
        if (stride < b->n) return fail(GOL_EINVAL, "sample_stride < n");
        if (!live) return fail(GOL_EINVAL, "null live");
        // (in bytes too: the words are addressed in a buffer)
        if (stride > (UINT64_MAX / sizeof(uint32_t)) / plan->samples)
            return fail(GOL_EINVAL, "samples * sample_stride is not representable");
    }
    return GOL_OK;
}

// The plan's launches, samples to dev[s * stride + i]; waits for them.
gol_status trace_run(gol_batch* b, const gol_batch_trace_plan& plan, uint32_t every,
                     uint32_t* dev, uint64_t stride, gol_batch_trace* out)
{
    gol_batch_trace r = {};
    r.struct_size = sizeof(gol_batch_trace);
    r.every = every;
    r.samples = plan.samples;
    if (plan.launches > 0) {
        gol::BatchTraceArgs t{};
        t.a = args_of(b);
        t.trace = dev;
        t.stride = stride;
        t.every = every;
        for (uint64_t j = 0; j < plan.launches; ++j) {
            t.s0 = j * plan.samples_per_launch;
            t.intervals =
                (uint32_t)std::min<uint64_t>(plan.samples_per_launch, plan.samples - t.s0);
            t.tail = j + 1 == plan.launches ? plan.tail : 0;
            if (b->rules)
                HIP_TRY(gol::launch_batch_trace_rules(gol::BatchTraceRuleArgs{t, b->rules},
                                                      (int)b->rows, b->stream));
            else
                HIP_TRY(gol::launch_batch_trace(t, (int)b->rows, b->rule, b->stream));
            r.launches += 1;
        }
        HIP_TRY(hipStreamSynchronize(b->stream));
    }
    *out = r;
    return GOL_OK;
}

// Every GOL_EINVAL of gol_batch_step_record and its device form, in the header's order;
// *plan: the call's launches (gol_batch_trace_plan_of's: there is no second plan).
gol_status record_check(const gol_batch* b, uint64_t generations, uint32_t every, uint64_t first,
                        uint64_t count, const uint64_t* frames, uint64_t ss, uint64_t fs,
                        uint64_t rs, const gol_batch_record* out, gol_batch_trace_plan* plan)
{
    if (!b) return fail(GOL_EINVAL, "null batch");
    if (!out) return fail(GOL_EINVAL, "null out");
    if (out->struct_size != sizeof(gol_batch_record))
        return fail(GOL_EINVAL, "gol_batch_record.struct_size must be sizeof(gol_batch_record)");
    if (every == 0 || every > gol::kBatchRecordMaxEvery)
        return fail(GOL_EINVAL, "a batch record's `every` must be 1..65536");
    if (first > b->n || count > b->n - first)
        return fail(GOL_EINVAL, "first + count exceeds the batch's fields");
    GOL_TRY(gol_batch_trace_plan_of(generations, every, b->launch_gens, plan));
    if (plan->samples > 0 && count > 0) {
        // (a product that does not fit 64 bits is above every stride)
        if (rs < b->wq) return fail(GOL_EINVAL, "row_stride_words < ceil(w/64)");
        if (rs > UINT64_MAX / b->h || fs < b->h * rs)
            return fail(GOL_EINVAL, "field_stride_words < h * row_stride_words");
        if (fs > UINT64_MAX / count || ss < count * fs)
            return fail(GOL_EINVAL, "sample_stride_words < count * field_stride_words");
        if (!frames) return fail(GOL_EINVAL, "null frames");
        // (in bytes: the words are addressed in a buffer)
        if (ss > (UINT64_MAX / sizeof(uint64_t)) / plan->samples)
            return fail(GOL_EINVAL, "samples * sample_stride_words is not representable");
    }
    return GOL_OK;
}

// The plan's launches, sample s of field first + j to dev[s * ss + j * fs + r * rs + q];
// waits for them.
gol_status record_run(gol_batch* b, const gol_batch_trace_plan& plan, uint32_t every,
                      uint64_t first, uint64_t count, uint64_t* dev, uint64_t ss, uint64_t fs,
                      uint64_t rs, gol_batch_record* out)
{
    gol_batch_record r = {};
    r.struct_size = sizeof(gol_batch_record);
    r.every = every;
    r.samples = plan.samples;
    if (plan.launches > 0) {
        gol::BatchRecordArgs t{};
        t.a = args_of(b);
        t.frames = dev;
        t.ss = ss;
        t.fs = fs;
        t.rs = rs;
        t.first = (int64_t)first;
        t.count = (int64_t)count;
        t.every = every;
        for (uint64_t j = 0; j < plan.launches; ++j) {
            t.s0 = j * plan.samples_per_launch;
            t.intervals =
                (uint32_t)std::min<uint64_t>(plan.samples_per_launch, plan.samples - t.s0);
            t.tail = j + 1 == plan.launches ? plan.tail : 0;
            if (b->rules)
                HIP_TRY(gol::launch_batch_record_rules(gol::BatchRecordRuleArgs{t, b->rules},
                                                       (int)b->rows, b->stream));
            else
                HIP_TRY(gol::launch_batch_record(t, (int)b->rows, b->rule, b->stream));
            r.launches += 1;
        }
        HIP_TRY(hipStreamSynchronize(b->stream));
    }
    *out = r;
    return GOL_OK;
}

}  // namespace

}  // namespace golh

extern "C" {

gol_status gol_batch_geometry(uint64_t n, uint64_t h, uint64_t w, const gol_config* cfg,
                              uint32_t* lanes_per_field, uint32_t* fields_per_wave,
                              uint32_t* rows_in_regs, uint64_t* waves)
{
    BatchShape s{};
    GOL_TRY(batch_shape(n, h, w, cfg, &s));
    if (lanes_per_field) *lanes_per_field = s.lpf;
    if (fields_per_wave) *fields_per_wave = s.fpw;
    if (rows_in_regs) *rows_in_regs = s.rows;
    if (waves) *waves = s.waves;
    return GOL_OK;
}

gol_status gol_batch_create(uint64_t n, uint64_t h, uint64_t w, const gol_config* cfg,
                            gol_batch** out)
{
    if (!out) return fail(GOL_EINVAL, "null out");
    *out = nullptr;
    BatchShape s{};
    GOL_TRY(batch_shape(n, h, w, cfg, &s));
    uint32_t launch_gens = kBatchLaunchGens;
    if (const char* v = std::getenv("GOL_DEV_BATCH_LAUNCH_GENS")) {
        const long k = std::atol(v);
        if (k < 1 || k > (1l << 30))
            return fail(GOL_EINVAL, "GOL_DEV_BATCH_LAUNCH_GENS must be in 1..2^30");
        launch_gens = (uint32_t)k;
    }
    gol_batch* b = new (std::nothrow) gol_batch();
    if (!b) return fail(GOL_ENOMEM, "host allocation");
    b->n = n;
    b->h = h;
    b->w = w;
    b->wq = s.wq;
    b->waves = s.waves;
    b->lpf = s.lpf;
    b->lpf_shift = s.lpf_shift;
    b->fpw = s.fpw;
    b->rows = s.rows;
    b->launch_gens = launch_gens;
    b->birth = cfg->birth_mask;
    b->survive = cfg->survive_mask;
    b->sem = cfg->semantics;
    b->rule = (b->birth == GOL_REF_BIRTH && b->survive == GOL_REF_SURVIVE) ? gol::RULE_REF
              : (b->birth == GOL_CONWAY_BIRTH && b->survive == GOL_CONWAY_SURVIVE)
                  ? gol::RULE_CONWAY
                  : gol::RULE_GENERIC;
    auto init = [&]() -> gol_status {
        if (cfg->device >= 0) HIP_TRY(hipSetDevice(cfg->device));
        HIP_TRY(hipGetDevice(&b->device));
        HIP_TRY(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
        const size_t bytes = (size_t)b->waves * b->h * 64 * sizeof(uint64_t);
        HIP_TRY(hipMalloc(&b->buf, bytes));
        // padding lanes and the lanes beyond field n - 1 stay 0 from here on
        HIP_TRY(hipMemsetAsync(b->buf, 0, bytes, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
        return GOL_OK;
    };
    const gol_status st = init();
    if (st != GOL_OK) {
        const std::string msg = g_last_error;
        gol_batch_destroy(b);
        g_last_error = msg;
        return st;
    }
    *out = b;
    return GOL_OK;
}

void gol_batch_destroy(gol_batch* b)
{
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    if (b->buf) (void)hipFree(b->buf);
    if (b->stage) (void)hipFree(b->stage);
    if (b->snap) (void)hipFree(b->snap);
    if (b->until) (void)hipFree(b->until);
    if (b->rules) (void)hipFree(b->rules);
    if (b->trace) (void)hipFree(b->trace);
    if (b->record) (void)hipFree(b->record);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}

gol_status gol_batch_info(gol_batch* b, uint64_t* n, uint64_t* h, uint64_t* w,
                          uint32_t* lanes_per_field, uint32_t* fields_per_wave,
                          uint32_t* rows_in_regs, uint32_t* launch_generations)
{
    if (!b) return fail(GOL_EINVAL, "null batch");
    if (n) *n = b->n;
    if (h) *h = b->h;
    if (w) *w = b->w;
    if (lanes_per_field) *lanes_per_field = b->lpf;
    if (fields_per_wave) *fields_per_wave = b->fpw;
    if (rows_in_regs) *rows_in_regs = b->rows;
    if (launch_generations) *launch_generations = b->launch_gens;
    return GOL_OK;
}

gol_status gol_batch_load_device(gol_batch* b, uint64_t first, uint64_t count,
                                 const uint64_t* words, uint64_t field_stride_words,
                                 uint64_t row_stride_words)
{
    GOL_TRY(check_range(b, first, count, words, field_stride_words, row_stride_words));
    if (count == 0) return GOL_OK;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(gol::launch_batch_load(geom_of(b), (int64_t)first, (int64_t)count, words,
                                   (int64_t)field_stride_words, (int64_t)row_stride_words,
                                   b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return GOL_OK;
}

gol_status gol_batch_store_device(gol_batch* b, uint64_t first, uint64_t count, uint64_t* words,
                                  uint64_t field_stride_words, uint64_t row_stride_words)
{
    GOL_TRY(check_range(b, first, count, words, field_stride_words, row_stride_words));
    if (count == 0) return GOL_OK;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(gol::launch_batch_store(geom_of(b), (int64_t)first, (int64_t)count, words,
                                    (int64_t)field_stride_words, (int64_t)row_stride_words,
                                    b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return GOL_OK;
}

gol_status gol_batch_load_packed(gol_batch* b, uint64_t first, uint64_t count,
                                 const uint64_t* words, uint64_t field_stride_words,
                                 uint64_t row_stride_words)
{
    GOL_TRY(check_range(b, first, count, words, field_stride_words, row_stride_words));
    if (count == 0) return GOL_OK;
    HIP_TRY(hipSetDevice(b->device));
    GOL_TRY(need_stage(b, (size_t)(count * b->h * b->wq)));
    GOL_TRY(stage_copy(b, count, const_cast<uint64_t*>(words), field_stride_words,
                       row_stride_words, true));
    HIP_TRY(gol::launch_batch_load(geom_of(b), (int64_t)first, (int64_t)count, b->stage,
                                   (int64_t)(b->h * b->wq), (int64_t)b->wq, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return GOL_OK;
}

gol_status gol_batch_store_packed(gol_batch* b, uint64_t first, uint64_t count, uint64_t* words,
                                  uint64_t field_stride_words, uint64_t row_stride_words)
{
    GOL_TRY(check_range(b, first, count, words, field_stride_words, row_stride_words));
    if (count == 0) return GOL_OK;
    HIP_TRY(hipSetDevice(b->device));
    GOL_TRY(need_stage(b, (size_t)(count * b->h * b->wq)));
    HIP_TRY(gol::launch_batch_store(geom_of(b), (int64_t)first, (int64_t)count, b->stage,
                                    (int64_t)(b->h * b->wq), (int64_t)b->wq, b->stream));
    GOL_TRY(stage_copy(b, count, words, field_stride_words, row_stride_words, false));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return GOL_OK;
}

gol_status gol_batch_init_random(gol_batch* b, uint64_t seed)
{
    if (!b) return fail(GOL_EINVAL, "null batch");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(gol::launch_batch_init_random(geom_of(b), seed, b->stream));
    return GOL_OK;
}

gol_status gol_batch_step(gol_batch* b, uint64_t generations)
{
    if (!b) return fail(GOL_EINVAL, "null batch");
    if (generations == 0) return GOL_OK;
    HIP_TRY(hipSetDevice(b->device));
    gol::BatchArgs a = args_of(b);
    for (uint64_t left = generations; left > 0;) {
        const uint64_t g = std::min<uint64_t>(left, b->launch_gens);
        a.gens = (int32_t)g;
        if (b->rules)
            HIP_TRY(gol::launch_batch_rules(gol::BatchRuleArgs{a, b->rules}, (int)b->rows,
                                            b->stream));
        else
            HIP_TRY(gol::launch_batch(a, (int)b->rows, b->rule, b->stream));
        left -= g;
    }
    return GOL_OK;
}

gol_status gol_batch_until_plan_of(uint64_t max_generations, uint32_t lag, uint32_t check_every,
                                   uint32_t launch_generations, gol_batch_until_plan* out)
{
    if (!out) return fail(GOL_EINVAL, "null out");
    GOL_TRY(until_args(lag, &check_every));
    gol_batch_until_plan p = {};
    p.check_every = check_every;
    for (uint32_t d = 1; d <= lag / 2; ++d)
        if (lag % d == 0) p.divisors[p.ndivisors++] = d;  // (at most 31: lag <= 1024)
    p.checks = max_generations / check_every;
    p.tail = (uint32_t)(max_generations % check_every);
    p.checks_per_launch = std::max<uint32_t>(1, launch_generations / check_every);
    p.launches = (p.checks + p.checks_per_launch - 1) / p.checks_per_launch;
    if (p.launches == 0 && max_generations > 0) p.launches = 1;
    *out = p;
    return GOL_OK;
}

gol_status gol_batch_step_until_periodic(gol_batch* b, uint64_t max_generations, uint32_t lag,
                                         uint32_t check_every, uint32_t* period,
                                         uint64_t* generation, gol_batch_until* out)
{
    if (!out) return fail(GOL_EINVAL, "null out");
    if (out->struct_size != sizeof(gol_batch_until))
        return fail(GOL_EINVAL, "gol_batch_until.struct_size must be sizeof(gol_batch_until)");
    GOL_TRY(until_args(lag, &check_every));
    if (!b) return fail(GOL_EINVAL, "null batch");
    gol_batch_until_plan plan;
    GOL_TRY(gol_batch_until_plan_of(max_generations, lag, check_every, b->launch_gens, &plan));
    gol_batch_until r = {};
    r.struct_size = sizeof(gol_batch_until);
    r.lag = lag;
    r.check_every = check_every;
    if (max_generations == 0) {
        for (uint64_t i = 0; i < b->n; ++i) {
            if (period) period[i] = 0;
            if (generation) generation[i] = 0;
        }
        *out = r;
        return GOL_OK;
    }
    HIP_TRY(hipSetDevice(b->device));
    const size_t gen_off = sizeof(gol::BatchUntilCounters), per_off = gen_off + b->n * 8,
                 done_off = per_off + b->n * 4, block = done_off + b->waves * 4;
    if (!b->snap) {
        if (hipMalloc(&b->snap, (size_t)b->waves * b->h * 64 * sizeof(uint64_t)) != hipSuccess) {
            (void)hipGetLastError();
            b->snap = nullptr;
            return fail(GOL_ENOMEM, "the batch's snapshot buffer");
        }
    }
    if (!b->until) {
        if (hipMalloc(&b->until, block) != hipSuccess) {
            (void)hipGetLastError();
            b->until = nullptr;
            return fail(GOL_ENOMEM, "the batch's period results");
        }
    }
    // results, done words and counters start from 0, the pending waves from all of them
    HIP_TRY(hipMemsetAsync(b->until, 0, block, b->stream));
    b->counters = gol::BatchUntilCounters{0ull, (uint32_t)b->waves, 0u};
    // (b->counters is next written by the copy back after the first launch, on this stream)
    HIP_TRY(hipMemcpyAsync(b->until, &b->counters, sizeof(b->counters), hipMemcpyHostToDevice,
                           b->stream));
    gol::BatchUntilArgs u{};
    u.a = args_of(b);
    u.snap = b->snap;
    u.ctr = reinterpret_cast<gol::BatchUntilCounters*>(b->until);
    u.generation = reinterpret_cast<uint64_t*>(b->until + gen_off);
    u.period = reinterpret_cast<uint32_t*>(b->until + per_off);
    u.done = reinterpret_cast<uint32_t*>(b->until + done_off);
    u.max_g = max_generations;
    u.lag = lag;
    u.check_every = check_every;
    u.ndiv = plan.ndivisors;
    for (uint32_t k = 0; k < plan.ndivisors; ++k) u.div[k] = plan.divisors[k];
    for (uint64_t j = 0; j < plan.launches; ++j) {
        const uint64_t c0 = j * plan.checks_per_launch;
        u.g0 = c0 * check_every;
        u.intervals = (uint32_t)std::min<uint64_t>(plan.checks_per_launch, plan.checks - c0);
        u.tail = j + 1 == plan.launches ? plan.tail : 0;
        if (b->rules)
            HIP_TRY(gol::launch_batch_until_rules(gol::BatchUntilRuleArgs{u, b->rules},
                                                  (int)b->rows, b->stream));
        else
            HIP_TRY(gol::launch_batch_until(u, (int)b->rows, b->rule, b->stream));
        r.launches += 1;
        // a few bytes per launch: once no wavefront is pending, every field already holds
        // generation max_generations and nothing more is launched
        HIP_TRY(hipMemcpyAsync(&b->counters, b->until, sizeof(b->counters), hipMemcpyDeviceToHost,
                               b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
        if (b->counters.pending == 0) break;
    }
    r.wave_generations = b->counters.wave_generations;
    std::vector<uint32_t> per(b->n);
    std::vector<uint64_t> gen(generation ? b->n : 0);
    HIP_TRY(hipMemcpyAsync(per.data(), b->until + per_off, b->n * 4, hipMemcpyDeviceToHost,
                           b->stream));
    if (generation)
        HIP_TRY(hipMemcpyAsync(gen.data(), b->until + gen_off, b->n * 8, hipMemcpyDeviceToHost,
                               b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    for (uint64_t i = 0; i < b->n; ++i) {
        if (per[i]) r.found += 1;
        if (period) period[i] = per[i];
        if (generation) generation[i] = per[i] ? gen[i] : max_generations;
    }
    *out = r;
    return GOL_OK;
}

gol_status gol_batch_trace_plan_of(uint64_t generations, uint32_t every,
                                   uint32_t launch_generations, gol_batch_trace_plan* out)
{
    if (!out) return fail(GOL_EINVAL, "null out");
    GOL_TRY(trace_every(every));
    gol_batch_trace_plan p = {};
    p.samples = generations / every;
    p.tail = (uint32_t)(generations % every);
    p.samples_per_launch = std::max<uint32_t>(1, launch_generations / every);
    p.launches = (p.samples + p.samples_per_launch - 1) / p.samples_per_launch;
    if (p.launches == 0 && generations > 0) p.launches = 1;
    *out = p;
    return GOL_OK;
}

gol_status gol_batch_step_trace_device(gol_batch* b, uint64_t generations, uint32_t every,
                                       uint32_t* live, uint64_t sample_stride,
                                       gol_batch_trace* out)
{
    gol_batch_trace_plan plan;
    GOL_TRY(trace_check(b, generations, every, live, sample_stride, out, &plan));
    HIP_TRY(hipSetDevice(b->device));
    return trace_run(b, plan, every, live, sample_stride, out);
}

gol_status gol_batch_step_trace(gol_batch* b, uint64_t generations, uint32_t every,
                                uint32_t* live, uint64_t sample_stride, gol_batch_trace* out)
{
    gol_batch_trace_plan plan;
    GOL_TRY(trace_check(b, generations, every, live, sample_stride, out, &plan));
    HIP_TRY(hipSetDevice(b->device));
    // (samples * n <= samples * sample_stride, which trace_check has bounded)
    const size_t words = (size_t)(plan.samples * b->n);
    if (b->trace_words < words) {
        if (b->trace) {
            HIP_TRY(hipStreamSynchronize(b->stream));
            (void)hipFree(b->trace);
            b->trace = nullptr;
            b->trace_words = 0;
        }
        if (hipMalloc(&b->trace, words * sizeof(uint32_t)) != hipSuccess) {
            (void)hipGetLastError();
            b->trace = nullptr;
            return fail(GOL_ENOMEM, "the batch's trace buffer");
        }
        b->trace_words = words;
    }
    GOL_TRY(trace_run(b, plan, every, b->trace, b->n, out));
    if (words == 0) return GOL_OK;
    const size_t rowb = b->n * sizeof(uint32_t);
    if (sample_stride == b->n)
        HIP_TRY(hipMemcpyAsync(live, b->trace, words * sizeof(uint32_t), hipMemcpyDeviceToHost,
                               b->stream));
    else
        HIP_TRY(hipMemcpy2DAsync(live, sample_stride * sizeof(uint32_t), b->trace, rowb, rowb,
                                 plan.samples, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return GOL_OK;
}

gol_status gol_batch_step_record_device(gol_batch* b, uint64_t generations, uint32_t every,
                                        uint64_t first, uint64_t count, uint64_t* frames,
                                        uint64_t sample_stride_words,
                                        uint64_t field_stride_words, uint64_t row_stride_words,
                                        gol_batch_record* out)
{
    gol_batch_trace_plan plan;
    GOL_TRY(record_check(b, generations, every, first, count, frames, sample_stride_words,
                         field_stride_words, row_stride_words, out, &plan));
    HIP_TRY(hipSetDevice(b->device));
    return record_run(b, plan, every, first, count, frames, sample_stride_words,
                      field_stride_words, row_stride_words, out);
}

gol_status gol_batch_step_record(gol_batch* b, uint64_t generations, uint32_t every,
                                 uint64_t first, uint64_t count, uint64_t* frames,
                                 uint64_t sample_stride_words, uint64_t field_stride_words,
                                 uint64_t row_stride_words, gol_batch_record* out)
{
    gol_batch_trace_plan plan;
    GOL_TRY(record_check(b, generations, every, first, count, frames, sample_stride_words,
                         field_stride_words, row_stride_words, out, &plan));
    HIP_TRY(hipSetDevice(b->device));
    // (samples * count * h * wq <= samples * sample_stride_words, which record_check has
    // bounded)
    const uint64_t fw = b->h * b->wq, sw = count * fw;
    const size_t words = (size_t)(plan.samples * sw);
    const bool compact = row_stride_words == b->wq && field_stride_words == fw &&
                         sample_stride_words == sw;
    // a caller's image with gaps is filled row by row from a host copy of the compact one,
    // which is taken before anything is stepped too
    uint64_t* host = nullptr;
    if (words > 0 && !compact) {
        host = new (std::nothrow) uint64_t[words];
        if (!host) return fail(GOL_ENOMEM, "the host copy of the batch's record buffer");
    }
    struct Free {
        uint64_t* p;
        ~Free() { delete[] p; }
    } free_host{host};
    if (b->record_words < words) {
        if (b->record) {
            HIP_TRY(hipStreamSynchronize(b->stream));
            (void)hipFree(b->record);
            b->record = nullptr;
            b->record_words = 0;
        }
        if (hipMalloc(&b->record, words * sizeof(uint64_t)) != hipSuccess) {
            (void)hipGetLastError();
            b->record = nullptr;
            return fail(GOL_ENOMEM, "the batch's record buffer");
        }
        b->record_words = words;
    }
    GOL_TRY(record_run(b, plan, every, first, count, b->record, sw, fw, b->wq, out));
    if (words == 0) return GOL_OK;
    HIP_TRY(hipMemcpyAsync(compact ? frames : host, b->record, words * sizeof(uint64_t),
                           hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (!compact) {
        const uint64_t* src = host;
        for (uint64_t s = 0; s < plan.samples; ++s)
            for (uint64_t j = 0; j < count; ++j)
                for (uint64_t r = 0; r < b->h; ++r, src += b->wq)
                    std::memcpy(frames + s * sample_stride_words + j * field_stride_words +
                                    r * row_stride_words,
                                src, b->wq * sizeof(uint64_t));
    }
    return GOL_OK;
}

gol_status gol_batch_set_rules(gol_batch* b, uint64_t first, uint64_t count,
                               const uint32_t* birth, const uint32_t* survive)
{
    if (!b) return fail(GOL_EINVAL, "null batch");
    if (first > b->n || count > b->n - first)
        return fail(GOL_EINVAL, "first + count exceeds the batch's fields");
    if (count == 0) return GOL_OK;
    if (!birth || !survive) return fail(GOL_EINVAL, "null birth or survive");
    for (uint64_t i = 0; i < count; ++i)
        if (birth[i] > 0x1FFu || survive[i] > 0x1FFu)
            return fail(GOL_EINVAL, "rule masks are 9-bit");
    HIP_TRY(hipSetDevice(b->device));
    // the first table: every field's create rule around the caller's range, in one copy
    const bool fresh = !b->rules;
    const uint64_t lo = fresh ? 0 : first, words = fresh ? b->n : count;
    std::vector<uint32_t> host(words, b->birth | b->survive << 16);
    for (uint64_t i = 0; i < count; ++i) host[first - lo + i] = birth[i] | survive[i] << 16;
    uint32_t* table = b->rules;
    if (fresh && hipMalloc(&table, b->n * sizeof(uint32_t)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(GOL_ENOMEM, "the batch's rule table");
    }
    // on the batch's stream: behind the steps already enqueued
    hipError_t e = hipMemcpyAsync(table + lo, host.data(), words * sizeof(uint32_t),
                                  hipMemcpyHostToDevice, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    if (e != hipSuccess) {
        if (fresh) (void)hipFree(table);
        HIP_TRY(e);
    }
    b->rules = table;
    return GOL_OK;
}

gol_status gol_batch_get_rules(gol_batch* b, uint64_t first, uint64_t count, uint32_t* birth,
                               uint32_t* survive)
{
    if (!b) return fail(GOL_EINVAL, "null batch");
    if (first > b->n || count > b->n - first)
        return fail(GOL_EINVAL, "first + count exceeds the batch's fields");
    if (count == 0) return GOL_OK;
    std::vector<uint32_t> host(count, b->birth | b->survive << 16);
    if (b->rules) {
        HIP_TRY(hipSetDevice(b->device));
        HIP_TRY(hipMemcpyAsync(host.data(), b->rules + first, count * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
    }
    for (uint64_t i = 0; i < count; ++i) {
        if (birth) birth[i] = host[i] & 0xFFFFu;
        if (survive) survive[i] = host[i] >> 16;
    }
    return GOL_OK;
}

gol_status gol_batch_drop_rules(gol_batch* b)
{
    if (!b) return fail(GOL_EINVAL, "null batch");
    if (!b->rules) return GOL_OK;
    HIP_TRY(hipSetDevice(b->device));
    // (steps already enqueued still read the table)
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipFree(b->rules));
    b->rules = nullptr;
    return GOL_OK;
}

gol_status gol_batch_has_rules(gol_batch* b, uint32_t* on)
{
    if (!b) return fail(GOL_EINVAL, "null batch");
    if (!on) return fail(GOL_EINVAL, "null on");
    *on = b->rules ? 1u : 0u;
    return GOL_OK;
}

gol_status gol_batch_sync(gol_batch* b)
{
    if (!b) return fail(GOL_EINVAL, "null batch");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return GOL_OK;
}

gol_status gol_batch_digest(gol_batch* b, uint64_t first, uint64_t count, uint64_t* live,
                            uint64_t* hash)
{
    if (!b) return fail(GOL_EINVAL, "null batch");
    if (first > b->n || count > b->n - first)
        return fail(GOL_EINVAL, "first + count exceeds the batch's fields");
    if (count == 0) return GOL_OK;
    HIP_TRY(hipSetDevice(b->device));
    GOL_TRY(need_stage(b, (size_t)(2 * count)));
    HIP_TRY(gol::launch_batch_digest(geom_of(b), (int64_t)first, (int64_t)count, b->stage,
                                     b->stream));
    std::vector<uint64_t> pairs(2 * count);
    HIP_TRY(hipMemcpyAsync(pairs.data(), b->stage, 2 * count * sizeof(uint64_t),
                           hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    for (uint64_t i = 0; i < count; ++i) {
        if (live) live[i] = pairs[2 * i];
        if (hash) hash[i] = pairs[2 * i + 1];
    }
    return GOL_OK;
}

}  // extern "C"
