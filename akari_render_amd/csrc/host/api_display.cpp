// api_display.cpp -- akr_display_transform: exposure (manual or from a log-luminance histogram), bloom and a tone curve over a film
//  (C ABI of libakari_hip.so, include/akari_hip.h; shared internals: api_internal.h). The arithmetic is
// csrc/device/ddisplay.h: the kernels of display_kernels.hip run it on the device, akr_host_display_transform (a test hook) runs the same
// text here. The end of the auto-exposure (histogram -> k) is host code in both: dp_exposure below.
#include "api_internal.h"
#include "../display_kernels.h"
#if defined(AKR_TEST_HOOKS) && AKR_TEST_HOOKS
#include "../../../include/akari_hip_test.h"
#endif

namespace {
constexpr uint32_t kMaxLevels = 8;
constexpr float kMaxExposure = 1.2676506e30f;  // 2^100: k s(c) and every sum of the pyramid stay finite

bool finite_f(float v) { return v >= -3.4028235e38f && v <= 3.4028235e38f; }  // (false for NaN and inf)

void check_config(const akr_display_config& c) {
    if (c.curve < kDpLinear || c.curve > kDpHable) throw std::invalid_argument("akr_display: unknown curve " + std::to_string(c.curve) + " (1 linear, 2 reinhard, 3 aces, 4 hable)");
    if (!finite_f(c.exposure_ev)) throw std::invalid_argument("akr_display: exposure_ev must be finite");
    if (!(c.bloom_strength >= 0.0f) || !finite_f(c.bloom_strength) || !(c.bloom_threshold >= 0.0f) || !finite_f(c.bloom_threshold))
        throw std::invalid_argument("akr_display: bloom_strength and bloom_threshold must be finite and >= 0");
    if (c.bloom_strength > 0.0f && (c.bloom_levels < 1 || c.bloom_levels > kMaxLevels))
        throw std::invalid_argument("akr_display: bloom_levels = " + std::to_string(c.bloom_levels) + " (1 to 8)");
    if (!finite_f(c.key) || !(c.key > 0.0f)) throw std::invalid_argument("akr_display: key must be finite and > 0");
    if (!finite_f(c.white) || !(c.white >= 0.0f)) throw std::invalid_argument("akr_display: white must be finite and >= 0 (0 = the curve's default)");
    if ((uint64_t)c.low_permille + (uint64_t)c.high_permille >= 1000) throw std::invalid_argument("akr_display: low_permille + high_permille must be < 1000");
}

// k of manual exposure: exp_f(exposure_ev ln2)
float manual_exposure(const akr_display_config& c) { return exp_f(c.exposure_ev * kDpLn2); }

// The end of the auto-exposure, a pure function of the configuration and the 256 counts (DESIGN.md 4.12 "Exposure")
float dp_exposure(const akr_display_config& c, const uint32_t* counts) {
    uint64_t cnt[kDpBins], total = 0;
    for (int i = 0; i < kDpBins; i++) total += (cnt[i] = counts[i]);
    uint64_t lo = total * c.low_permille / 1000, hi = total * c.high_permille / 1000;
    for (int i = 0; i < kDpBins && lo; i++) {
        const uint64_t t = cnt[i] < lo ? cnt[i] : lo;
        cnt[i] -= t;
        lo -= t;
    }
    for (int i = kDpBins - 1; i >= 0 && hi; i--) {
        const uint64_t t = cnt[i] < hi ? cnt[i] : hi;
        cnt[i] -= t;
        hi -= t;
    }
    double num = 0.0;
    uint64_t den = 0;
    for (int i = 0; i < kDpBins; i++) {
        num += (double)cnt[i] * ((double)i + 0.5);
        den += cnt[i];
    }
    if (!den) return manual_exposure(c);
    const double m = num / (double)den;
    const float avg = (float)(m / 8.0 - 20.0);
    return (c.key * exp_f(-avg * kDpLn2)) * manual_exposure(c);
}

void check_exposure(float k) {
    if (!(k >= 0.0f && k <= kMaxExposure)) throw std::invalid_argument("akr_display: the exposure (key 2^(exposure_ev - average log2 luminance)) is beyond 2^100");
}

DisplayParams dp_params(const akr_display_config& c, float k) {
    DisplayParams p;
    p.curve = c.curve;
    p.k = k;
    const float white = c.white == 0.0f ? (c.curve == kDpHable ? 11.2f : 4.0f) : c.white;
    p.white2 = white * white;
    p.hable_norm = dp_hable(white);
    p.strength = c.bloom_strength;
    p.threshold = c.bloom_threshold;
    p.inv_levels = c.bloom_strength != 0.0f ? 1.0f / (float)c.bloom_levels : 0.0f;
    if (c.curve == kDpReinhard && !(1.0f / p.white2 <= 3.4028235e38f)) throw std::invalid_argument("akr_display: white is too small: 1 / white^2 is not finite in f32");
    if (c.curve == kDpHable && !(p.hable_norm > 0.0f && 1.0f / p.hable_norm <= 3.4028235e38f)) throw std::invalid_argument("akr_display: white is too small: hable(white) is 0 in f32");
    return p;
}

// level l (1 .. levels) of a w x h frame: ceil(/2) of level l - 1, level 0 the frame; 1 x 1 stays 1 x 1
struct Pyramid {
    uint32_t w[kMaxLevels + 1], h[kMaxLevels + 1];
    uint64_t records = 0;  // of levels 1 .. levels
    Pyramid(uint32_t width, uint32_t height, uint32_t levels) {
        w[0] = width;
        h[0] = height;
        for (uint32_t l = 1; l <= levels; l++) {
            w[l] = (w[l - 1] + 1) / 2;
            h[l] = (h[l - 1] + 1) / 2;
            records += (uint64_t)w[l] * h[l];
        }
    }
};

void check_film(const akr_context* ctx, const akr_film* f) {
    if (f->ctx != ctx) throw std::invalid_argument("akr_display: every film must belong to the context");
    if ((uint64_t)f->width * f->height > 0xffffffffull) throw std::invalid_argument("akr_display: a film of 2^32 pixels or more");
}

// around_kernel (or empty): called on the stream right before and right after the kernel's launch
void histogram_run(akr_context* ctx, akr_film* film, uint32_t* counts257, const std::function<void()>& around_kernel = {}) {
    DevBuf dev;
    dev.alloc((kDpBins + 1) * sizeof(uint32_t));
    HIP_CHECK(hipMemsetAsync(dev.p, 0, (kDpBins + 1) * sizeof(uint32_t), ctx->stream));
    if (around_kernel) around_kernel();
    HIP_CHECK(launch_lum_histogram(film->data, film->splat_scale, (uint64_t)film->width * film->height, dev.as<uint32_t>(), ctx->stream));
    if (around_kernel) around_kernel();
    HIP_CHECK(hipMemcpyAsync(counts257, dev.p, (kDpBins + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

// Which blur runs when option display_kernel leaves it to the library ("Cost": over the five levels of a 1920 x 1080 frame
// the LDS kernel takes 0.65 of the two gathering passes' time, 0.59 at 3840 x 2160, and less at level 1 alone)
bool tiled_by_default() { return true; }

// The whole transform on the context's stream. kernel: -1 the library decides, 0 the two gathering blur passes, 1 the LDS blur.
// times (or nullptr): milliseconds of the histogram kernel, source, all downs, all blurs, all ups, apply, the whole call (the histogram's
// read-back and the host's part included), the blur of level 1 [8].
void display_run(akr_context* ctx, const akr_display_config& cfg, akr_film* film, akr_film* out, float* exposure_used, int kernel, float* times) {
    check_config(cfg);
    check_film(ctx, film);
    check_film(ctx, out);
    if (film->width != out->width || film->height != out->height) throw std::invalid_argument("akr_display: the films differ in size");
    ctx->bind();
    const uint32_t w = film->width, h = film->height;
    const bool bloom = cfg.bloom_strength != 0.0f;
    const bool tiled = kernel < 0 ? tiled_by_default() : kernel != 0;
    StreamMarks marks(ctx->stream, times != nullptr);
    // the bloom's work buffers in one allocation: the unblurred levels D, the blurred levels G (U after the recombination), one pass's temporary
    const Pyramid pyr(w, h, bloom ? cfg.bloom_levels : 0);
    DevBuf work;
    float4 *D[kMaxLevels + 1] = {}, *G[kMaxLevels + 1] = {}, *tmp = nullptr;
    const uint32_t L = bloom ? cfg.bloom_levels : 0;
    if (bloom) {
        const uint64_t first = (uint64_t)pyr.w[1] * pyr.h[1];
        work.alloc((2 * pyr.records + first) * sizeof(float4));
        float4* at = work.as<float4>();
        for (uint32_t l = 1; l <= L; l++) {
            D[l] = at;
            at += (uint64_t)pyr.w[l] * pyr.h[l];
        }
        for (uint32_t l = 1; l <= L; l++) {
            G[l] = at;
            at += (uint64_t)pyr.w[l] * pyr.h[l];
        }
        tmp = at;
    }
    marks.mark();  // 0
    float k = manual_exposure(cfg);
    if (cfg.auto_exposure) {
        uint32_t counts[kDpBins + 1];
        histogram_run(ctx, film, counts, [&] { marks.mark(); });  // 1, 2
        k = dp_exposure(cfg, counts);
    } else {
        marks.mark();
        marks.mark();
    }
    check_exposure(k);
    const DisplayParams p = dp_params(cfg, k);
    marks.mark();  // 3
    if (bloom) HIP_CHECK(launch_bloom_source(film->data, film->splat_scale, w, h, k, cfg.bloom_threshold, D[1], ctx->stream));
    marks.mark();  // 4
    for (uint32_t l = 1; l < L; l++) HIP_CHECK(launch_bloom_down(D[l], pyr.w[l], pyr.h[l], D[l + 1], ctx->stream));
    marks.mark();  // 5
    if (bloom) HIP_CHECK(launch_bloom_blur(D[1], tmp, G[1], pyr.w[1], pyr.h[1], tiled, ctx->stream));
    marks.mark();  // 6
    for (uint32_t l = 2; l <= L; l++) HIP_CHECK(launch_bloom_blur(D[l], tmp, G[l], pyr.w[l], pyr.h[l], tiled, ctx->stream));
    marks.mark();  // 7
    for (uint32_t l = L; l-- > 1;) HIP_CHECK(launch_bloom_up(G[l], pyr.w[l], pyr.h[l], G[l + 1], pyr.w[l + 1], pyr.h[l + 1], ctx->stream));
    marks.mark();  // 8
    HIP_CHECK(launch_display_apply(film->data, film->splat_scale, w, h, p, bloom ? G[1] : nullptr, bloom ? pyr.w[1] : 1, bloom ? pyr.h[1] : 1, out->data, ctx->stream));
    marks.mark();  // 9
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    out->splat_scale = 1.0f;
    if (exposure_used) *exposure_used = k;
    if (times) {
        times[0] = marks.ms(1, 2);
        times[1] = marks.ms(3, 4);
        times[2] = marks.ms(4, 5);
        times[3] = marks.ms(5, 7);
        times[4] = marks.ms(7, 8);
        times[5] = marks.ms(8, 9);
        times[6] = marks.ms(0, 9);
        times[7] = marks.ms(5, 6);
    }
}
}  // namespace

extern "C" {

AKR_API int32_t akr_display_config_default(akr_display_config* c) {
    if (!c) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_display_config_default: NULL argument");
    std::memset(c, 0, sizeof *c);
    // choices, not measurements
    c->curve = AKR_DISPLAY_ACES;
    c->auto_exposure = 0;
    c->exposure_ev = 0.0f;
    c->key = 0.18f;
    c->low_permille = 50;
    c->high_permille = 20;
    c->white = 0.0f;
    c->bloom_strength = 0.0f;
    c->bloom_threshold = 1.0f;
    c->bloom_levels = 5;
    return AKR_OK;
}

AKR_API int32_t akr_film_luminance_histogram(akr_context* ctx, akr_film* film, uint32_t* counts256, uint32_t* skipped) {
    if (!ctx || !film || !counts256) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_film_luminance_histogram: NULL argument");
    return guarded([&] {
        check_film(ctx, film);
        ctx->bind();
        uint32_t counts[kDpBins + 1];
        histogram_run(ctx, film, counts);
        std::memcpy(counts256, counts, kDpBins * sizeof(uint32_t));
        if (skipped) *skipped = counts[kDpBins];
    });
}

AKR_API int32_t akr_display_exposure(const akr_display_config* cfg, const uint32_t* counts256, float* k) {
    if (!cfg || !counts256 || !k) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_display_exposure: NULL argument");
    return guarded([&] {
        check_config(*cfg);
        *k = dp_exposure(*cfg, counts256);
    });
}

AKR_API int32_t akr_display_transform(akr_context* ctx, const akr_display_config* cfg, akr_film* film, akr_film* out, float* exposure_used) {
    if (!ctx || !cfg || !film || !out) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_display_transform: NULL argument");
    return guarded([&] { display_run(ctx, *cfg, film, out, exposure_used, tuning().display_kernel, nullptr); });
}

#if defined(AKR_TEST_HOOKS) && AKR_TEST_HOOKS
AKR_TEST_API int32_t akr_probe_display_times(akr_context* ctx, const akr_display_config* cfg, akr_film* film, akr_film* out, int32_t kernel, float* times8) {
    if (!ctx || !cfg || !film || !out || !times8) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_display_times: NULL argument");
    if (kernel < -1 || kernel > 1) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_probe_display_times: kernel is -1, 0 or 1");
    return guarded([&] { display_run(ctx, *cfg, film, out, nullptr, kernel, times8); });
}

AKR_TEST_API int32_t akr_host_luminance_histogram(uint32_t width, uint32_t height, const float* film, float splat_scale, uint32_t* counts256, uint32_t* skipped) {
    if (!film || !counts256 || !skipped || !width || !height) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_luminance_histogram: bad argument");
    return guarded([&] {
        const uint64_t n = (uint64_t)width * height;
        std::memset(counts256, 0, kDpBins * sizeof(uint32_t));
        *skipped = 0;
        for (uint64_t i = 0; i < n; i++) {
            const int b = dp_bin(dp_lum(dp_load(film, n, i, splat_scale)));
            if (b < 0) (*skipped)++;
            else counts256[b]++;
        }
    });
}

AKR_TEST_API int32_t akr_host_display_transform(const akr_display_config* cfg, uint32_t width, uint32_t height, const float* film, float splat_scale, float* out_rgb,
                                                float* exposure_used) {
    if (!cfg || !film || !out_rgb || !width || !height) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_display_transform: bad argument");
    return guarded([&] {
        check_config(*cfg);
        const uint64_t n = (uint64_t)width * height;
        float k = manual_exposure(*cfg);
        if (cfg->auto_exposure) {
            uint32_t counts[kDpBins] = {};
            for (uint64_t i = 0; i < n; i++) {
                const int b = dp_bin(dp_lum(dp_load(film, n, i, splat_scale)));
                if (b >= 0) counts[b]++;
            }
            k = dp_exposure(*cfg, counts);
        }
        check_exposure(k);
        const DisplayParams p = dp_params(*cfg, k);
        const uint32_t L = cfg->bloom_strength != 0.0f ? cfg->bloom_levels : 0;
        const Pyramid pyr(width, height, L);
        std::vector<std::vector<float4>> D(L + 1), G(L + 1);
        for (uint32_t l = 1; l <= L; l++) {
            const int sw = (int)pyr.w[l - 1], sh = (int)pyr.h[l - 1], dw = (int)pyr.w[l], dh = (int)pyr.h[l];
            D[l].resize((size_t)dw * dh);
            for (int y = 0; y < dh; y++)
                for (int x = 0; x < dw; x++) {
                    const int x0 = 2 * x, y0 = 2 * y, x1 = dp_clampi(x0 + 1, sw - 1), y1 = dp_clampi(y0 + 1, sh - 1);
                    auto at = [&](int px, int py) {
                        const size_t q = (size_t)py * sw + px;
                        return l == 1 ? dp_bright(dp_load(film, n, q, splat_scale), k, cfg->bloom_threshold) : D[l - 1][q];
                    };
                    D[l][(size_t)y * dw + x] = dp_box(at(x0, y0), at(x1, y0), at(x0, y1), at(x1, y1));
                }
            std::vector<float4> t((size_t)dw * dh);
            G[l].resize((size_t)dw * dh);
            for (int y = 0; y < dh; y++)
                for (int x = 0; x < dw; x++) t[(size_t)y * dw + x] = dp_blur5([&](int d) { return D[l][(size_t)y * dw + dp_clampi(x + d, dw - 1)]; });
            for (int y = 0; y < dh; y++)
                for (int x = 0; x < dw; x++) G[l][(size_t)y * dw + x] = dp_blur5([&](int d) { return t[(size_t)dp_clampi(y + d, dh - 1) * dw + x]; });
        }
        for (uint32_t l = L; l-- > 1;) {
            const int dw = (int)pyr.w[l], dh = (int)pyr.h[l], sw = (int)pyr.w[l + 1], sh = (int)pyr.h[l + 1];
            for (int y = 0; y < dh; y++)
                for (int x = 0; x < dw; x++)
                    G[l][(size_t)y * dw + x] = dp_add(G[l][(size_t)y * dw + x], dp_up(x, y, sw, sh, [&](int sx, int sy) { return G[l + 1][(size_t)sy * sw + sx]; }));
        }
        for (uint64_t i = 0; i < n; i++) {
            float4 u = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (L) u = dp_up((int)(i % width), (int)(i / width), (int)pyr.w[1], (int)pyr.h[1], [&](int sx, int sy) { return G[1][(size_t)sy * pyr.w[1] + sx]; });
            dp_apply(dp_load(film, n, i, splat_scale), u, p, out_rgb + 3 * i);
        }
        if (exposure_used) *exposure_used = k;
    });
}
#endif

}  // extern "C"
