// api_adapt.cpp -- adaptive sampling for pt: akr_film_tile_error, akr_pt_adaptive_render (C ABI of libakari_hip.so,
// include/akari_hip.h; shared internals: api_internal.h). The arithmetic is csrc/device/dadapt.h: the kernels of adapt_kernels.hip run it on
// the device, akr_host_tile_error / akr_host_half_bracket (test hooks) run the same text here.
#include "api_internal.h"
#include "../adapt_kernels.h"
#if defined(AKR_TEST_HOOKS) && AKR_TEST_HOOKS
#include "../../../include/akari_hip_test.h"
#endif

namespace {
// the frame's tile grid as the kernels and the hooks take it; refuses what the tree cannot hold
AdaptFrame adapt_frame(const char* who, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h) {
    const TileGrid g = tile_grid(tile_w, tile_h, width, height, 0, 1);
    if ((g.tile_w % 8) || (g.tile_h % 8)) throw std::invalid_argument(std::string(who) + ": tile_w and tile_h must be multiples of 8");
    if ((uint64_t)g.tile_w * g.tile_h > kAdaptMaxTilePixels)
        throw std::invalid_argument(std::string(who) + ": tile_w * tile_h = " + std::to_string((uint64_t)g.tile_w * g.tile_h) + " (adaptive sampling takes tiles of at most 4096 pixels)");
    return AdaptFrame{width, height, g.tile_w, g.tile_h, g.tiles_x};
}
void check_tiles(const char* who, const AdaptFrame& fr, const uint32_t* tiles, uint32_t n) {
    const uint32_t n_tiles = fr.tiles_x * ((fr.height + fr.tile_h - 1) / fr.tile_h);
    for (uint32_t j = 0; j < n; j++)
        if (tiles[j] >= n_tiles) throw std::invalid_argument(std::string(who) + ": tile " + std::to_string(tiles[j]) + " is out of range (the grid has " + std::to_string(n_tiles) + " tiles)");
}
void check_films(const char* who, akr_context* ctx, const akr_film* film, const akr_film* half) {
    if (film->ctx != ctx || half->ctx != ctx) throw std::invalid_argument(std::string(who) + ": every film must belong to the context");
    if (film->width != half->width || film->height != half->height) throw std::invalid_argument(std::string(who) + ": the films differ in size");
    if (film == half || film->data == half->data) throw std::invalid_argument(std::string(who) + ": the half film cannot be the film itself");
}

void host_tile_error(const AdaptFrame& fr, const float* film, const float* half, const uint32_t* tiles, uint32_t n, float* err) {
    const uint32_t P = ad_tree_leaves(fr.tile_w * fr.tile_h);
    std::vector<float> s(P);
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t ty = tiles[j] / fr.tiles_x, tx = tiles[j] - ty * fr.tiles_x;
        uint32_t n_est = 0;
        for (uint32_t i = 0; i < P; i++) {
            bool has;
            s[i] = ad_tile_leaf(film, half, fr.width, fr.height, fr.tile_w, fr.tile_h, tx, ty, i, has);
            n_est += has ? 1u : 0u;
        }
        for (uint32_t stride = P >> 1; stride >= 1; stride >>= 1)
            for (uint32_t i = 0; i < stride; i++) s[i] = s[i] + s[i + stride];
        err[j] = ad_tile_error(s[0], n_est);
    }
}

// a failed call of the C ABI inside another: the same status and message for the outer call's guarded()
void rethrow(int32_t rc) {
    if (rc == AKR_OK) return;
    const std::string m = g_last_error;
    switch (rc) {
        case AKR_ERR_INVALID_ARGUMENT: throw std::invalid_argument(m);
        case AKR_ERR_HIP: throw HipError(m);
        case AKR_ERR_UNSUPPORTED: throw Unsupported(m);
        case AKR_ERR_IO: throw IoError(m);
        case AKR_ERR_RENDER: throw RenderError(m);
        case AKR_ERR_OUT_OF_MEMORY: throw std::bad_alloc();
        default: throw std::runtime_error(m);
    }
}

struct FilmHolder {  // a film that dies with its scope
    akr_film* f = nullptr;
    ~FilmHolder() { if (f) akr_film_destroy(f); }
};
}  // namespace

extern "C" {

AKR_API int32_t akr_adaptive_config_default(akr_adaptive_config* c) {
    if (!c) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_adaptive_config_default: NULL argument");
    std::memset(c, 0, sizeof *c);
    c->threshold = 0.0625f;  // the row of DESIGN.md 4.11's table with the best relMSE ratio against its uniform neighbour
    c->min_spp = 16;          // a choice: two checks' worth of the table's rounds before a tile may retire
    c->round_passes = 1;      // a choice: a check after every second pass
    return AKR_OK;
}

AKR_API int32_t akr_film_tile_error(akr_context* ctx, akr_film* film, akr_film* half, uint32_t tile_w, uint32_t tile_h, const uint32_t* tiles, uint32_t n,
                                    float* err_out_host) {
    if (!ctx || !film || !half || (n && (!tiles || !err_out_host))) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_film_tile_error: NULL argument");
    return guarded([&] {
        check_films("akr_film_tile_error", ctx, film, half);
        const AdaptFrame fr = adapt_frame("akr_film_tile_error", film->width, film->height, tile_w, tile_h);
        check_tiles("akr_film_tile_error", fr, tiles, n);
        if (n == 0) return;
        ctx->bind();
        DevBuf d_tiles, d_err;
        d_tiles.upload(std::vector<uint32_t>(tiles, tiles + n));
        d_err.alloc((size_t)n * sizeof(float));
        HIP_CHECK(launch_tile_error(fr, film->data, half->data, d_tiles.as<uint32_t>(), n, d_err.as<float>(), ctx->stream));
        HIP_CHECK(hipMemcpyAsync(err_out_host, d_err.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

AKR_API int32_t akr_pt_adaptive_render(akr_context* ctx, akr_scene* scene, const akr_pt_config* cfg, const akr_adaptive_config* acfg, akr_film* film,
                                       akr_film* half_in, uint32_t* tile_spp, akr_adaptive_stats* stats) {
    if (!ctx || !scene || !cfg || !acfg || !film) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_pt_adaptive_render: NULL argument");
    akr_pt_session* se = nullptr;
    int32_t rc = guarded([&] {
        auto check = [](int32_t r) { rethrow(r); };
        if (!(acfg->threshold >= 0.0f)) throw std::invalid_argument("akr_pt_adaptive_render: threshold must be >= 0 (+inf allowed), not NaN");
        if (acfg->round_passes == 0) throw std::invalid_argument("akr_pt_adaptive_render: round_passes must be >= 1");
        if (cfg->spp_per_pass == 0) throw std::invalid_argument("akr_pt_config: spp_per_pass must be > 0");
        if (cfg->sample_begin != 0 || cfg->sample_count != 0) throw std::invalid_argument("akr_pt_adaptive_render: a sample range cannot be rendered adaptively");
        const uint64_t round_samples = (uint64_t)acfg->round_passes * cfg->spp_per_pass;
        if (cfg->spp <= round_samples)
            throw std::invalid_argument("akr_pt_adaptive_render: needs a task of at least two rounds: spp = " + std::to_string(cfg->spp) + " is one round at round_passes = " +
                                        std::to_string(acfg->round_passes) + ", spp_per_pass = " + std::to_string(cfg->spp_per_pass));
        const AdaptFrame fr = adapt_frame("akr_pt_adaptive_render", film->width, film->height, cfg->tile_w, cfg->tile_h);
        FilmHolder own_half;
        akr_film* half = half_in;
        if (!half) {
            check(akr_film_create(ctx, film->width, film->height, &own_half.f));
            half = own_half.f;
        }
        check_films("akr_pt_adaptive_render", ctx, film, half);
        ctx->bind();
        HIP_CHECK(hipMemsetAsync(half->data, 0, half->n_floats() * sizeof(float), ctx->stream));
        half->splat_scale = film->splat_scale;
        check(akr_pt_begin(ctx, scene, cfg, film, &se));
        const TileGrid& grid = se->grid;
        const uint32_t n_tiles = grid.tiles_x * grid.tiles_y;
        const uint32_t count = cfg->shard_count > 1 ? cfg->shard_count : 1, rank = cfg->shard_count > 1 ? cfg->shard_rank : 0;
        std::vector<uint32_t> active = count > 1 ? owned_tiles(grid.tiles_x, grid.tiles_y, rank, count) : std::vector<uint32_t>();
        if (count == 1)
            for (uint32_t t = 0; t < n_tiles; t++) active.push_back(t);
        auto tile_pixels = [&](uint32_t t) {  // in-frame pixels of a tile
            const uint32_t ty = t / grid.tiles_x, tx = t - ty * grid.tiles_x;
            return (uint64_t)std::min(grid.tile_w, film->width - tx * grid.tile_w) * std::min(grid.tile_h, film->height - ty * grid.tile_h);
        };
        uint64_t owned_pixels = 0;
        for (uint32_t t : active) owned_pixels += tile_pixels(t);
        std::vector<uint32_t> spp_of(n_tiles, 0);
        DevBuf d_tiles, d_err;
        d_tiles.alloc((size_t)std::max(1u, n_tiles) * sizeof(uint32_t));
        d_err.alloc((size_t)std::max(1u, n_tiles) * sizeof(float));
        std::vector<float> err(n_tiles);
        auto upload_active = [&] {
            if (!active.empty()) HIP_CHECK(hipMemcpy(d_tiles.p, active.data(), active.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        };
        upload_active();
        uint32_t done = 0, rounds = 0, retired = 0;
        uint64_t drawn = 0;
        while (!active.empty() && done < cfg->spp) {
            const bool a_round = (rounds & 1u) == 0;
            const uint32_t n = (uint32_t)active.size();
            if (a_round) HIP_CHECK(launch_half_bracket(fr, film->data, half->data, d_tiles.as<uint32_t>(), n, false, ctx->stream));
            uint32_t now = done;
            check(akr_pt_passes(se, acfg->round_passes, 1, &now));
            if (a_round) HIP_CHECK(launch_half_bracket(fr, film->data, half->data, d_tiles.as<uint32_t>(), n, true, ctx->stream));
            const bool full = now - done == round_samples;
            for (uint32_t t : active) drawn += (uint64_t)(now - done) * tile_pixels(t);
            done = now;
            rounds++;
            for (uint32_t t : active) spp_of[t] = done;
            if (a_round || !full || done >= cfg->spp || done < acfg->min_spp) continue;  // a check follows every full B-round short of spp (no tile can retire before min_spp)
            HIP_CHECK(launch_tile_error(fr, film->data, half->data, d_tiles.as<uint32_t>(), n, d_err.as<float>(), ctx->stream));
            HIP_CHECK(hipMemcpyAsync(err.data(), d_err.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
            HIP_CHECK(hipStreamSynchronize(ctx->stream));
            std::vector<uint32_t> left;
            for (uint32_t j = 0; j < n; j++)
                if (!(is_finite(err[j]) && err[j] <= acfg->threshold)) left.push_back(active[j]);  // NaN and +inf stay
            if (left.size() == active.size()) continue;
            retired += (uint32_t)(active.size() - left.size());
            active.swap(left);
            check(akr_pt_set_active_tiles(se, active.data(), (uint32_t)active.size()));
            upload_active();
        }
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (tile_spp) std::copy(spp_of.begin(), spp_of.end(), tile_spp);
        akr_pt_stats st;
        akr_pt_session* ended = se;
        se = nullptr;
        check(akr_pt_end(ended, &st));
        if (stats) {
            std::memset(stats, 0, sizeof *stats);
            stats->rounds = rounds;
            stats->tiles_retired = retired;
            stats->samples_drawn = drawn;
            stats->samples_uniform = owned_pixels * cfg->spp;
            stats->pt = st;
        }
    });
    if (se) rc = end_keeping_first_error(rc, [&] { return akr_pt_end(se, nullptr); });
    return rc;
}

#if defined(AKR_TEST_HOOKS) && AKR_TEST_HOOKS
AKR_TEST_API int32_t akr_host_tile_error(uint32_t width, uint32_t height, const float* film, const float* half_film, uint32_t tile_w, uint32_t tile_h,
                                         const uint32_t* tiles, uint32_t n, float* err_out) {
    if (!film || !half_film || !width || !height || (n && (!tiles || !err_out))) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_tile_error: bad argument");
    return guarded([&] {
        if (film == half_film) throw std::invalid_argument("akr_host_tile_error: the half film cannot be the film itself");
        const AdaptFrame fr = adapt_frame("akr_host_tile_error", width, height, tile_w, tile_h);
        check_tiles("akr_host_tile_error", fr, tiles, n);
        host_tile_error(fr, film, half_film, tiles, n, err_out);
    });
}

AKR_TEST_API int32_t akr_host_half_bracket(uint32_t width, uint32_t height, const float* film, float* half_film, uint32_t tile_w, uint32_t tile_h,
                                           const uint32_t* tiles, uint32_t n, int32_t close) {
    if (!film || !half_film || !width || !height || (n && !tiles)) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_half_bracket: bad argument");
    return guarded([&] {
        if (film == half_film) throw std::invalid_argument("akr_host_half_bracket: the half film cannot be the film itself");
        const AdaptFrame fr = adapt_frame("akr_host_half_bracket", width, height, tile_w, tile_h);
        check_tiles("akr_host_half_bracket", fr, tiles, n);
        const uint64_t N = (uint64_t)width * height;
        for (uint32_t j = 0; j < n; j++) {
            const uint32_t ty = tiles[j] / fr.tiles_x, tx = tiles[j] - ty * fr.tiles_x;
            for (uint32_t yt = 0; yt < fr.tile_h; yt++)
                for (uint32_t xt = 0; xt < fr.tile_w; xt++) {
                    const uint32_t px = tx * fr.tile_w + xt, py = ty * fr.tile_h + yt;
                    if (px < width && py < height) ad_half_pixel(film, half_film, N, (uint64_t)py * width + px, close != 0);
                }
        }
    });
}

AKR_TEST_API int32_t akr_probe_adapt_times(akr_context* ctx, akr_film* film, akr_film* half, uint32_t tile_w, uint32_t tile_h, const uint32_t* tiles, uint32_t n,
                                           float* times3) {
    if (!ctx || !film || !half || !tiles || !n || !times3) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_adapt_times: bad argument");
    return guarded([&] {
        check_films("akr_probe_adapt_times", ctx, film, half);
        const AdaptFrame fr = adapt_frame("akr_probe_adapt_times", film->width, film->height, tile_w, tile_h);
        check_tiles("akr_probe_adapt_times", fr, tiles, n);
        ctx->bind();
        DevBuf d_tiles, d_err;
        d_tiles.upload(std::vector<uint32_t>(tiles, tiles + n));
        d_err.alloc((size_t)n * sizeof(float));
        StreamMarks marks(ctx->stream, true);
        marks.mark();
        HIP_CHECK(launch_tile_error(fr, film->data, half->data, d_tiles.as<uint32_t>(), n, d_err.as<float>(), ctx->stream));
        marks.mark();
        HIP_CHECK(launch_half_bracket(fr, film->data, half->data, d_tiles.as<uint32_t>(), n, false, ctx->stream));
        marks.mark();
        HIP_CHECK(launch_half_bracket(fr, film->data, half->data, d_tiles.as<uint32_t>(), n, true, ctx->stream));
        marks.mark();
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        for (int k = 0; k < 3; k++) times3[k] = marks.ms(k, k + 1);
    });
}
#endif

}  // extern "C"
