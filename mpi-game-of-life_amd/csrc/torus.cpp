// torus.cpp -- torus engines (GOL_SEM_TORUS): one h x w field whose opposite edges
// are joined, built on an ordinary dead-border engine ("Torus").
//
// The torus engine owns one single-stream GLOBAL engine, the inner engine, whose
// field is the interior padded with ghost cells: G ghost rows above and below,
// Gx = ceil(G/64) ghost words (64 columns each) on the left, so the interior starts
// word-aligned at word Gx of each row, and 64 Gx ghost columns on the right from
// column w of the interior on: (h + 2G) x (w + 128 Gx) cells.  gol_step runs
// rounds of at most G generations: the wrap kernel (life_aux.hip, the rule of
// torus_wrap.h) rewrites every ghost cell of the inner engine's current buffer
// from the interior, then the inner engine advances g <= G generations on the
// same stream.  After g generations the dead border's error has moved at most g
// cells into the ghosts, so it never reaches the interior.  Every round starts
// with a wrap, the first of every gol_step too: nothing relies on what the ghosts
// hold between calls, and load / init only write the interior.
//
// The interior's last word also holds ghost columns unless w % 64 == 0, so every
// reader of the interior masks it (store, digest), and the wrap keeps its interior
// bits.  The load, init and digest kernels see the interior as a view of the inner
// engine's buffer: buf + Gx, the padded stride, row_base = G.
#include "engine_internal.h"
#include "torus_wrap.h"

namespace golh __attribute__((visibility("hidden"))) {

namespace {

uint32_t lcm_u32(uint32_t a, uint32_t b)
{
    uint32_t x = a, y = b;
    while (y) {
        const uint32_t t = x % y;
        x = y;
        y = t;
    }
    return a / x * b;
}

// Auto G for inner depth K: the largest multiple of K that is <= cap and
// <= max(K, min(h, w) / 4), cap = 256 for fields of at most 2^25 cells, else 128.
// The trade (measured, DESIGN §6 "Torus"): a round costs a fixed 25-40 us -- the
// wrap, 5-12 us, and the restart of the inner engine's launches -- and the ghosts
// cost area, (h + 2G)(w + 128 Gx) / (h w).  Fields up to 2^25 cells usually run
// the resident kernel, well under 1 us per generation and almost flat in area, so
// the round cost dominates and G = 256 beats 128 by 10-15% (512 gains 4-8% more
// for 2-4x the memory: not taken).  Larger fields stream at 4-40 us per
// generation: G from 32 to 256 is within +-3%, and area favours the smaller.
// min(h, w) / 4 bounds the ghosts' share of a small field.
uint32_t auto_round(uint32_t K, uint64_t h, uint64_t w)
{
    const uint64_t top = h <= (1ull << 25) / w ? 256 : 128;  // h w <= 2^25, no overflow
    const uint64_t cap = std::min<uint64_t>(top, std::max<uint64_t>(K, std::min(h, w) / 4));
    return (uint32_t)std::max<uint64_t>(K, cap / K * K);
}

}  // namespace

gol_status torus_geometry(uint64_t h, uint64_t w, const gol_config* cfg, TorusGeom* g)
{
    GOL_TRY(check_cfg(cfg));
    if (cfg->semantics != GOL_SEM_TORUS) return fail(GOL_EINVAL, "not a torus config");
    if (h == 0 || w == 0) return fail(GOL_EINVAL, "h and w must be >= 1");
    if (h > (1ull << 40) || w > (1ull << 40)) return fail(GOL_EINVAL, "field too large");
    if (cfg->streams > 1)
        return fail(GOL_EINVAL, "a torus engine runs on one stream: streams must be 0 or 1");
    if (cfg->word_planes == 4) return fail(GOL_EINVAL, "a torus engine needs word_planes 0 or 2");
    if (cfg->halo_depth > (1u << 16))
        return fail(GOL_EINVAL, "torus: halo_depth (generations per wrap round) must be <= 65536");
    uint32_t G = cfg->halo_depth, K = auto_layout(h, cfg).K;
    if (!G) {
        // the inner engine picks its depth from the padded rows, which depend on G
        // in turn: where the ghosts move the field across auto_layout's threshold,
        // G is a multiple of both depths
        G = auto_round(K, h, w);
        const uint32_t K1 = auto_layout(h + 2ull * G, cfg).K;
        if (K1 != K) G = auto_round(lcm_u32(K, K1), h, w);
    }
    g->G = G;
    g->Gx = (G + 63) / 64;
    g->ph = h + 2ull * G;
    g->pw = w + 128ull * g->Gx;
    g->K = auto_layout(g->ph, cfg).K;
    return GOL_OK;
}

// The inner engine's config: the caller's launch knobs, one stream, dead border.
static gol_config inner_config(const gol_config* cfg)
{
    gol_config c = *cfg;
    c.semantics = GOL_SEM_GLOBAL;
    c.ref_ranks = 1;
    c.streams = 1;
    c.halo_depth = 0;
    return c;
}

gol_status torus_create(uint64_t h, uint64_t w, const gol_config* cfg, gol_engine** out)
{
    TorusGeom g;
    GOL_TRY(torus_geometry(h, w, cfg, &g));
    gol_engine* e = new (std::nothrow) gol_engine();
    if (!e) return fail(GOL_ENOMEM, "host allocation");
    const gol_config c = inner_config(cfg);
    const gol_status st = gol_create(g.ph, g.pw, &c, &e->inner);
    if (st != GOL_OK) {
        delete e;
        return st;
    }
    const gol_engine* in = e->inner;
    if (!in->parts.empty() || in->planes != 2 || in->nbuf != 2 || in->buf_rows != g.ph ||
        in->stride < (g.pw + 63) / 64) {
        gol_destroy(e->inner);
        delete e;
        return fail(GOL_ESTATE, "torus: unexpected inner engine layout");
    }
    // (short step) the wrap withdraws the record before every round: the
    // inner engine's gol_sync has nothing to look for
    e->inner->short_on = 0;
    e->inner->fixed_on = 0;  // (fixed step) stands on the short step
    if (e->inner->sync_host) {
        (void)hipHostFree(e->inner->sync_host);
        e->inner->sync_host = nullptr;
    }
    e->sem = GOL_SEM_TORUS;
    e->H = e->R = h;
    e->W = w;
    e->wq = (w + 63) / 64;
    e->lastmask = last_mask(w);
    e->device = in->device;
    e->K = in->K;
    e->tG = g.G;
    e->tGx = g.Gx;
    *out = e;
    return GOL_OK;
}

// Word 0 of interior row 0 in the inner engine's current buffer.
static uint64_t* interior(const gol_engine* e)
{
    const gol_engine* in = e->inner;
    return in->buf[in->cur] + e->tG * in->stride + e->tGx;
}

static gol_status clear_current(gol_engine* in)
{
    GOL_TRY(quiesce(in));
    GOL_TRY(twin_clear(in));
    const size_t words_all = (size_t)(in->buf_rows + 2 * gol::kGuardRows) * in->stride;
    HIP_TRY(hipMemsetAsync(in->alloc[in->cur], 0, words_all * 8, in->stream));
    return GOL_OK;
}

gol_status torus_step(gol_engine* e, uint64_t generations)
{
    gol_engine* in = e->inner;
    HIP_TRY(hipSetDevice(in->device));
    for (uint64_t left = generations; left > 0;) {
        const uint64_t g = std::min<uint64_t>(left, e->tG);
        // (the wrap writes ghost cells of the current buffer alone)
        GOL_TRY(twin_clear(in));
        HIP_TRY(gol::launch_torus_wrap(in->buf[in->cur], (int64_t)in->stride, (int64_t)e->H,
                                       (int64_t)e->W, (int64_t)e->tG, (int64_t)e->tGx, in->stream));
        GOL_TRY(gol_step(in, g));
        left -= g;
    }
    return GOL_OK;
}

gol_status torus_load_packed(gol_engine* e, const uint64_t* words, uint64_t rs)
{
    if (rs < e->wq) return fail(GOL_EINVAL, "row stride smaller than ceil(w/64)");
    gol_engine* in = e->inner;
    GOL_TRY(clear_current(in));
    std::vector<uint64_t> tmp((size_t)e->H * e->wq);
    for (uint64_t i = 0; i < e->H; ++i)
        for (uint64_t q = 0; q < e->wq; ++q) {
            const uint64_t c = words[i * rs + q];
            tmp[i * e->wq + q] = gol_split64(q == e->wq - 1 ? (c & e->lastmask) : c);
        }
    HIP_TRY(hipMemcpy2DAsync(interior(e), in->stride * 8, tmp.data(), e->wq * 8, e->wq * 8, e->H,
                             hipMemcpyHostToDevice, in->stream));
    HIP_TRY(hipStreamSynchronize(in->stream));
    return GOL_OK;
}

gol_status torus_store_packed(gol_engine* e, uint64_t* words, uint64_t rs)
{
    if (rs < e->wq) return fail(GOL_EINVAL, "row stride smaller than ceil(w/64)");
    gol_engine* in = e->inner;
    HIP_TRY(hipSetDevice(in->device));
    std::vector<uint64_t> tmp((size_t)e->H * e->wq);
    HIP_TRY(hipMemcpy2DAsync(tmp.data(), e->wq * 8, interior(e), in->stride * 8, e->wq * 8, e->H,
                             hipMemcpyDeviceToHost, in->stream));
    HIP_TRY(hipStreamSynchronize(in->stream));
    for (uint64_t i = 0; i < e->H; ++i)
        for (uint64_t q = 0; q < e->wq; ++q) {
            const uint64_t c = gol_join64(tmp[i * e->wq + q]);
            // (the last word's columns >= w are ghost cells in the buffer)
            words[i * rs + q] = q == e->wq - 1 ? (c & e->lastmask) : c;
        }
    return check_err(in);
}

gol_status torus_load_ascii(gol_engine* e, const char* buf, size_t len)
{
    if (len != e->H * (e->W + 1))
        return fail(GOL_EINVAL, "ASCII length must be rows*(w+1) = " +
                                    std::to_string(e->H * (e->W + 1)) + ", got " +
                                    std::to_string(len));
    gol_engine* in = e->inner;
    GOL_TRY(clear_current(in));
    DeviceBytes bytes;
    HIP_TRY(hipMalloc(&bytes.p, len));
    HIP_TRY(hipMemcpyAsync(bytes.p, buf, len, hipMemcpyHostToDevice, in->stream));
    HIP_TRY(hipMemsetAsync(in->d_flag, 0, sizeof(int), in->stream));
    HIP_TRY(gol::launch_ascii_pack(bytes.p, (int64_t)e->H, (int64_t)e->W, (int64_t)e->wq,
                                   interior(e), (int64_t)in->stride, in->d_flag, 2, in->stream));
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, in->d_flag, sizeof(int), hipMemcpyDeviceToHost, in->stream));
    HIP_TRY(hipStreamSynchronize(in->stream));
    if (bad) return fail(GOL_EINVAL, "malformed ASCII: a line is not w cells followed by '\\n'");
    return GOL_OK;
}

gol_status torus_store_ascii(gol_engine* e, char* buf, size_t len)
{
    if (len != e->H * (e->W + 1))
        return fail(GOL_EINVAL, "ASCII length must be rows*(w+1) = " +
                                    std::to_string(e->H * (e->W + 1)));
    gol_engine* in = e->inner;
    HIP_TRY(hipSetDevice(in->device));
    DeviceBytes bytes;
    HIP_TRY(hipMalloc(&bytes.p, len));
    // (the codec writes columns < w only: the last word's ghost columns never show)
    HIP_TRY(gol::launch_ascii_unpack(interior(e), (int64_t)in->stride, (int64_t)e->H,
                                     (int64_t)e->W, (int64_t)e->wq, bytes.p, 2, in->stream));
    HIP_TRY(hipMemcpyAsync(buf, bytes.p, len, hipMemcpyDeviceToHost, in->stream));
    HIP_TRY(hipStreamSynchronize(in->stream));
    return check_err(in);
}

gol_status torus_init_random(gol_engine* e, uint64_t seed)
{
    gol_engine* in = e->inner;
    GOL_TRY(clear_current(in));
    // the interior's own word index r*ceil(w/64) + q: the field of a dead-border
    // engine of the same h x w and seed
    HIP_TRY(gol::launch_init_random(in->buf[in->cur] + e->tGx, (int64_t)in->stride,
                                    (int64_t)e->wq, e->lastmask, (int64_t)e->tG, 0,
                                    (int64_t)e->H, seed, 2, in->stream, (int64_t)e->wq));
    HIP_TRY(hipStreamSynchronize(in->stream));
    return GOL_OK;
}

gol_status torus_digest_rows(gol_engine* e, uint64_t row0, uint64_t rows, uint64_t* live,
                             uint64_t* hash)
{
    gol_engine* in = e->inner;
    HIP_TRY(hipSetDevice(in->device));
    HIP_TRY(hipMemsetAsync(in->d_acc, 0, 2 * sizeof(unsigned long long), in->stream));
    HIP_TRY(gol::launch_digest(in->buf[in->cur] + e->tGx, (int64_t)in->stride, (int64_t)e->wq,
                               (int64_t)e->wq, (int64_t)(e->tG + row0), (int64_t)row0,
                               (int64_t)rows, in->d_acc, 2, in->stream, e->lastmask));
    unsigned long long acc[2];
    HIP_TRY(hipMemcpyAsync(acc, in->d_acc, sizeof(acc), hipMemcpyDeviceToHost, in->stream));
    HIP_TRY(hipStreamSynchronize(in->stream));
    *live = acc[0];
    *hash = acc[1];
    return check_err(in);
}

// Region I/O: window cell (i, j) is interior cell ((y + i) mod h, (x + j) mod w), so
// a rectangle splits at the seams into at most 2 x 2 non-wrapping pieces of the
// interior, which sits at buffer row tG, word tGx of the inner engine.
static size_t torus_pieces(const gol_engine* e, uint64_t y, uint64_t x, uint64_t rh, uint64_t rw,
                           RectPiece out[4])
{
    const uint64_t h0 = std::min(rh, e->H - y), w0 = std::min(rw, e->W - x);
    const uint64_t rows[2][3] = {{y, h0, 0}, {0, rh - h0, h0}};  // start, count, window row
    const uint64_t cols[2][3] = {{x, w0, 0}, {0, rw - w0, w0}};
    size_t n = 0;
    for (const auto& r : rows)
        for (const auto& c : cols)
            if (r[1] && c[1]) out[n++] = RectPiece{r[0], c[0], r[1], c[1], r[2], c[2]};
    return n;
}

static std::vector<Region> interior_regions(const gol_engine* e)
{
    return {Region{e->tG, 0, 0, e->H}};
}

gol_status torus_read_rect(gol_engine* e, uint64_t y, uint64_t x, uint64_t rh, uint64_t rw,
                           uint64_t* words, uint64_t rs)
{
    RectPiece pcs[4];
    const size_t n = torus_pieces(e, y, x, rh, rw, pcs);
    return leaf_read(e->inner, interior_regions(e), e->tGx, pcs, n, words, rs);
}

gol_status torus_write_rect(gol_engine* e, uint64_t y, uint64_t x, uint64_t rh, uint64_t rw,
                            const uint64_t* words, uint64_t rs, uint32_t op)
{
    // (the ghosts go stale; the wrap at the start of the next round rewrites them)
    RectPiece pcs[4];
    const size_t n = torus_pieces(e, y, x, rh, rw, pcs);
    return leaf_write(e->inner, interior_regions(e), e->tGx, pcs, n, words, rs, op);
}

gol_status torus_density(gol_engine* e, uint64_t y, uint64_t x, uint64_t rh, uint64_t rw,
                         uint64_t by, uint64_t bx, uint64_t nby, uint64_t nbx, uint32_t* counts,
                         uint64_t cs)
{
    RectPiece pcs[4];
    const size_t n = torus_pieces(e, y, x, rh, rw, pcs);
    return leaf_density(e->inner, interior_regions(e), e->tGx, pcs, n, by, bx, nby, nbx, counts,
                        cs);
}

}  // namespace golh

extern "C" {

gol_status gol_torus_geometry(uint64_t h, uint64_t w, const gol_config* cfg, uint32_t* round_gens,
                              uint32_t* ghost_rows, uint32_t* ghost_words, uint64_t* padded_h,
                              uint64_t* padded_w)
{
    TorusGeom g;
    GOL_TRY(torus_geometry(h, w, cfg, &g));
    if (round_gens) *round_gens = g.G;
    if (ghost_rows) *ghost_rows = g.G;
    if (ghost_words) *ghost_words = (uint32_t)g.Gx;
    if (padded_h) *padded_h = g.ph;
    if (padded_w) *padded_w = g.pw;
    return GOL_OK;
}

gol_status gol_torus_pad(const uint64_t* field, uint64_t row_stride_words, uint64_t h, uint64_t w,
                         uint32_t ghost_rows, uint32_t ghost_words, uint64_t* out,
                         uint64_t out_stride_words)
{
    if (!field || !out) return fail(GOL_EINVAL, "null argument");
    if (h == 0 || w == 0) return fail(GOL_EINVAL, "h and w must be >= 1");
    if (h > (1ull << 40) || w > (1ull << 40)) return fail(GOL_EINVAL, "field too large");
    const uint64_t wq = (w + 63) / 64, wq_pad = wq + 2ull * ghost_words;
    if (row_stride_words < wq) return fail(GOL_EINVAL, "row stride smaller than ceil(w/64)");
    if (out_stride_words < wq_pad)
        return fail(GOL_EINVAL, "out stride smaller than ceil(w/64) + 2 ghost_words");
    const int64_t G = ghost_rows, Gx = ghost_words;
    const int64_t x_end = (int64_t)w + 64 * Gx;
    for (int64_t y = 0; y < (int64_t)h + 2 * G; ++y) {
        const uint64_t* src = field + (uint64_t)gol_torus_mod(y - G, (int64_t)h) * row_stride_words;
        uint64_t* dst = out + (uint64_t)y * out_stride_words;
        for (uint64_t q = 0; q < out_stride_words; ++q)
            dst[q] = q < wq_pad ? gol_torus_gather([src](int64_t i) { return src[i]; }, (int64_t)w,
                                                   (int64_t)q - Gx, x_end)
                                : 0ull;
    }
    return GOL_OK;
}

}  // extern "C"
