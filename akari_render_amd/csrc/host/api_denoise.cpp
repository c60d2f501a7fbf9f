// api_denoise.cpp -- akr_denoise: the edge-avoiding a-trous filter over a colour film and its albedo / normal guides
// (C ABI of libakari_hip.so, include/akari_hip.h; shared internals: api_internal.h). The arithmetic is csrc/device/ddenoise.h: the kernels
// of denoise_kernels.hip run it on the device, host_denoise (behind two test hooks) runs the same text here.
#include "api_internal.h"
#include "../denoise_kernels.h"
#if defined(AKR_TEST_HOOKS) && AKR_TEST_HOOKS
#include "../../../include/akari_hip_test.h"
#endif

namespace {
constexpr uint32_t kMaxIterations = 8;

// variance: akr_denoise's refusals, then those of sigma_variance. kv / (g + 1e-10f) has to stay finite for g = 0
void check_config(const akr_denoise_config& c, bool variance) {
    auto sigma_ok = [](float s) { return s >= 0.0f && s <= 3.4028235e38f; };  // (false for NaN and inf)
    if (c.iterations > kMaxIterations) throw std::invalid_argument("akr_denoise: iterations = " + std::to_string(c.iterations) + " (at most 8)");
    if (!sigma_ok(c.sigma_color) || !sigma_ok(c.sigma_normal) || !sigma_ok(c.sigma_albedo))
        throw std::invalid_argument("akr_denoise: sigma_color, sigma_normal and sigma_albedo must be finite and >= 0");
    if (!(c.albedo_floor > 0.0f)) throw std::invalid_argument("akr_denoise: albedo_floor must be > 0");
    // a positive sigma so small that its square underflows or 1 / sigma^2 overflows would make k = inf and the centre tap 0 * inf = NaN
    const uint32_t last = c.iterations ? c.iterations - 1 : 0;
    auto k_ok = [](float s) { return s == 0.0f || 1.0f / (s * s) <= 3.4028235e38f; };
    if (!k_ok(c.sigma_color * (1.0f / (float)(1u << last))) || !k_ok(c.sigma_normal) || !k_ok(c.sigma_albedo))
        throw std::invalid_argument("akr_denoise: a sigma is too small: 1 / sigma^2 (sigma_color at the last level: sigma_color 2^-(iterations - 1)) is not finite in f32");
    if (!variance) return;
    if (!(c.sigma_variance > 0.0f && c.sigma_variance <= 3.4028235e38f)) throw std::invalid_argument("akr_denoise_variance: sigma_variance must be finite and > 0");
    const float kv = 1.0f / (c.sigma_variance * c.sigma_variance);
    if (!(kv / 1e-10f <= 3.4028235e38f))
        throw std::invalid_argument("akr_denoise_variance: sigma_variance is too small: (1 / sigma_variance^2) / 1e-10 is not finite in f32");
}

// k = 1 / sigma^2 in f32; a sigma of exactly 0 switches the term off
float inv_sigma2(float sigma) { return sigma == 0.0f ? 0.0f : 1.0f / (sigma * sigma); }

// variance: kc = kv = 1 / sigma_variance^2 at every level (the variance shrinks by itself)
DenoiseLevel level_params(const akr_denoise_config& c, uint32_t w, uint32_t h, uint32_t i, bool have_albedo, bool have_normal, bool variance) {
    DenoiseLevel lv;
    lv.width = w;
    lv.height = h;
    lv.step = 1u << i;
    lv.kc = variance ? 1.0f / (c.sigma_variance * c.sigma_variance) : inv_sigma2(c.sigma_color * (1.0f / (float)(1u << i)));  // sigma_color 2^-i: an exact scaling
    lv.kn = have_normal ? inv_sigma2(c.sigma_normal) : 0.0f;
    lv.ka = have_albedo ? inv_sigma2(c.sigma_albedo) : 0.0f;
    return lv;
}

// Which level kernel runs step s when option denoise_kernel leaves it to the library ("Cost": at 1920 x 1080 the tiled
// kernel takes 0.47 / 0.49 / 0.59 of the gathering kernel's time at steps 1 / 2 / 4, 1.16 at step 8, the same at step 16)
bool tiled_by_default(uint32_t step) { return step <= 4; }

// The whole stage on the context's stream. kernel: -1 the library decides per step, 0 the gathering kernel, 1 the tiled one.
// times (or nullptr): milliseconds of prepare, the levels [8], finish, the whole call [11] -- HIP events on the stream.
// half = nullptr: akr_denoise. Else akr_denoise_variance: prepare is followed by the prefilter (both in times[0]) and the levels are the
// variance-guided ones.
void denoise_run(akr_context* ctx, const akr_denoise_config& cfg, akr_film* color, akr_film* half, akr_film* albedo, akr_film* normal, akr_film* out, int kernel,
                 float* times) {
    const bool variance = half != nullptr;
    check_config(cfg, variance);
    if (half && half == out) throw std::invalid_argument("akr_denoise_variance: the half film cannot be the output film");
    for (akr_film* f : {half, albedo, normal, out}) {
        if (!f) continue;
        if (f->ctx != ctx || color->ctx != ctx) throw std::invalid_argument("akr_denoise: every film must belong to the context");
        if (f->width != color->width || f->height != color->height) throw std::invalid_argument("akr_denoise: the films differ in size");
    }
    ctx->bind();
    const uint32_t w = color->width, h = color->height;
    const uint64_t n = (uint64_t)w * h;
    const uint32_t demodulate = cfg.demodulate && albedo ? 1u : 0u;
    auto level = [&](uint32_t i) { return level_params(cfg, w, h, i, albedo != nullptr, normal != nullptr, variance); };
    DevBuf bx0, bx1, bn, ba;  // the call's work buffers: x ping, x pong, n, a
    bx0.alloc(n * sizeof(float4));
    bx1.alloc(n * sizeof(float4));
    bn.alloc(n * sizeof(float4));
    ba.alloc(n * sizeof(float4));
    StreamMarks marks(ctx->stream, times != nullptr);
    DenoiseRecords rec{bx0.as<float4>(), bn.as<float4>(), ba.as<float4>()};
    float4* other = bx1.as<float4>();
    marks.mark();
    HIP_CHECK(launch_denoise_prepare(color->data, color->splat_scale, half ? half->data : nullptr, albedo ? albedo->data : nullptr, albedo ? albedo->splat_scale : 0.0f,
                                     normal ? normal->data : nullptr, normal ? normal->splat_scale : 0.0f, n, demodulate, cfg.albedo_floor, rec, ctx->stream));
    if (variance) HIP_CHECK(launch_denoise_variance(level(0), rec, ctx->stream));
    marks.mark();
    for (uint32_t i = 0; i < cfg.iterations; i++) {
        const DenoiseLevel lv = level(i);
        const bool tiled = kernel < 0 ? tiled_by_default(lv.step) : kernel != 0;
        HIP_CHECK(launch_denoise_level(lv, rec, other, tiled, variance, ctx->stream));
        std::swap(rec.x, other);
        marks.mark();
    }
    HIP_CHECK(launch_denoise_finish(rec.x, rec.a, n, demodulate, cfg.albedo_floor, out->data, ctx->stream));
    marks.mark();
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    out->splat_scale = 1.0f;
    if (times) {
        for (int k = 0; k < 11; k++) times[k] = 0.0f;
        times[0] = marks.ms(0, 1);
        for (uint32_t i = 0; i < cfg.iterations; i++) times[1 + i] = marks.ms(1 + i, 2 + i);
        times[9] = marks.ms(1 + cfg.iterations, 2 + cfg.iterations);
        times[10] = marks.ms(0, 2 + cfg.iterations);
    }
}

#if defined(AKR_TEST_HOOKS) && AKR_TEST_HOOKS
// What denoise_run computes, on the host from the same text, under guide G (ddenoise.h; half is read by DnVariance alone) -> out_rgb[3 N]
template <class G>
void host_denoise(const akr_denoise_config& cfg, uint32_t width, uint32_t height, const float* color, float color_scale, const float* half, const float* albedo,
                  float albedo_scale, const float* normal, float normal_scale, float* out_rgb) {
    check_config(cfg, G::kVariance);
    const uint64_t n = (uint64_t)width * height;
    const bool demodulate = cfg.demodulate && albedo;
    auto level = [&](uint32_t i) { return level_params(cfg, width, height, i, albedo != nullptr, normal != nullptr, G::kVariance); };
    std::vector<float4> x(n), y(n), nn(n), a(n);
    for (uint64_t i = 0; i < n; i++)
        dn_prepare_pixel<G>(color, color_scale, half, albedo, albedo_scale, normal, normal_scale, n, i, demodulate, cfg.albedo_floor, x[i], nn[i], a[i]);
    if constexpr (G::kVariance) {
        const DenoiseLevel lv0 = level(0);
        for (int py = 0; py < (int)height; py++)
            for (int px = 0; px < (int)width; px++) {
                const size_t p = (size_t)py * width + px;
                if (!G::valid(x[p])) continue;
                x[p].w = dn_prefilter_pixel(px, py, lv0, [&](int dx, int dy, float4& nq, float4& aq) {
                    const size_t q = (size_t)(py + dy) * width + (px + dx);
                    nq = nn[q];
                    aq = a[q];
                    return !(nq.w < 0.0f);
                });
            }
    }
    for (uint32_t it = 0; it < cfg.iterations; it++) {
        const DenoiseLevel lv = level(it);
        const int s = (int)lv.step;
        for (int py = 0; py < (int)height; py++)
            for (int px = 0; px < (int)width; px++)
                y[(size_t)py * width + px] = dn_level_pixel<G>(px, py, lv, [&](int dx, int dy, float4& xq, float4& nq, float4& aq) {
                    const size_t q = (size_t)(py + s * dy) * width + (px + s * dx);
                    xq = x[q];
                    nq = nn[q];
                    aq = a[q];
                    return G::valid(xq);
                });
        x.swap(y);
    }
    for (uint64_t i = 0; i < n; i++) dn_finish_pixel(x[i], a[i], demodulate, cfg.albedo_floor, out_rgb + 3 * i);
}
#endif
}  // namespace

extern "C" {

AKR_API int32_t akr_denoise_config_default(akr_denoise_config* c) {
    if (!c) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_denoise_config_default: NULL argument");
    std::memset(c, 0, sizeof *c);
    c->iterations = 5;
    c->demodulate = 1;
    // the grid point of lowest relMSE of DESIGN.md 4.10's table (cbox, 16 spp against 2048 spp)
    c->sigma_color = 2.0f;
    c->sigma_normal = 0.125f;
    c->sigma_albedo = 0.0625f;
    c->albedo_floor = 1e-3f;
    c->sigma_variance = 8.0f;  // the lowest point of DESIGN.md 4.10's sigma_variance table (read by akr_denoise_variance alone)
    return AKR_OK;
}

AKR_API int32_t akr_denoise(akr_context* ctx, const akr_denoise_config* cfg, akr_film* color, akr_film* albedo, akr_film* normal, akr_film* out) {
    if (!ctx || !cfg || !color || !out) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_denoise: NULL argument");
    return guarded([&] { denoise_run(ctx, *cfg, color, nullptr, albedo, normal, out, tuning().denoise_kernel, nullptr); });
}

AKR_API int32_t akr_denoise_variance(akr_context* ctx, const akr_denoise_config* cfg, akr_film* color, akr_film* half, akr_film* albedo, akr_film* normal,
                                     akr_film* out) {
    if (!ctx || !cfg || !color || !half || !out) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_denoise_variance: NULL argument");
    return guarded([&] { denoise_run(ctx, *cfg, color, half, albedo, normal, out, tuning().denoise_kernel, nullptr); });
}

#if defined(AKR_TEST_HOOKS) && AKR_TEST_HOOKS
AKR_TEST_API int32_t akr_probe_denoise_times(akr_context* ctx, const akr_denoise_config* cfg, akr_film* color, akr_film* albedo, akr_film* normal, akr_film* out,
                                             int32_t kernel, float* times11) {
    if (!ctx || !cfg || !color || !out || !times11) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_denoise_times: NULL argument");
    if (kernel < -1 || kernel > 1) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_denoise_times: kernel is -1, 0 or 1");
    return guarded([&] { denoise_run(ctx, *cfg, color, nullptr, albedo, normal, out, kernel, times11); });
}

AKR_TEST_API int32_t akr_probe_denoise_variance_times(akr_context* ctx, const akr_denoise_config* cfg, akr_film* color, akr_film* half, akr_film* albedo,
                                                      akr_film* normal, akr_film* out, int32_t kernel, float* times11) {
    if (!ctx || !cfg || !color || !half || !out || !times11) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_denoise_variance_times: NULL argument");
    if (kernel < -1 || kernel > 1) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_denoise_variance_times: kernel is -1, 0 or 1");
    return guarded([&] { denoise_run(ctx, *cfg, color, half, albedo, normal, out, kernel, times11); });
}

AKR_TEST_API int32_t akr_host_denoise(const akr_denoise_config* cfg, uint32_t width, uint32_t height, const float* color_film, float color_splat_scale,
                                      const float* albedo_film, float albedo_splat_scale, const float* normal_film, float normal_splat_scale, float* out_rgb) {
    if (!cfg || !color_film || !out_rgb || !width || !height) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_denoise: bad argument");
    return guarded([&] {
        host_denoise<DnPlain>(*cfg, width, height, color_film, color_splat_scale, nullptr, albedo_film, albedo_splat_scale, normal_film, normal_splat_scale, out_rgb);
    });
}

AKR_TEST_API int32_t akr_host_denoise_variance(const akr_denoise_config* cfg, uint32_t width, uint32_t height, const float* color_film, float color_splat_scale,
                                               const float* half_film, const float* albedo_film, float albedo_splat_scale, const float* normal_film,
                                               float normal_splat_scale, float* out_rgb) {
    if (!cfg || !color_film || !half_film || !out_rgb || !width || !height) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_denoise_variance: bad argument");
    return guarded([&] {
        host_denoise<DnVariance>(*cfg, width, height, color_film, color_splat_scale, half_film, albedo_film, albedo_splat_scale, normal_film, normal_splat_scale, out_rgb);
    });
}
#endif

}  // extern "C"
