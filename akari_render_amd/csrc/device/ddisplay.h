// ddisplay.h -- the display transform of akr_display_transform: exposure, bloom and a tone curve between a resolved
// film and the 8-bit file, written once for the device (display_kernels.hip) and the host (host/api_display.cpp akr_host_display_transform).
// Under the AKR-F32 contract: no contraction, IEEE division, exp_f / log_f of dmath.h. Every operand order below is the normative one.
//
// A pixel of a bloom level is one 16-byte record {r, g, b, 0}.
#pragma once
#include "ddenoise.h"  // dn_resolve: the film resolve, shared with the denoiser

namespace akr {

constexpr float kDpLn2 = 0.6931471805599453f, kDpInvLn2 = 1.4426950408889634f;
constexpr int kDpBins = 256;  // 1/8 EV each over [-20, 12)

// the curves: the values of akr_display_config.curve and of option "display"
enum : uint32_t { kDpLinear = 1, kDpReinhard = 2, kDpAces = 3, kDpHable = 4 };

// What the per-pixel stages need, derived once per call by the host (dp_params in api_display.cpp)
struct DisplayParams {
    uint32_t curve;
    float k;           // the exposure
    float white2;      // Reinhard: white^2
    float hable_norm;  // Hable: f(white)
    float strength, threshold, inv_levels;  // bloom: strength (0 = off), bright-pass threshold, 1 / bloom_levels
};

// s(x) = clamp_f(x, 0, 65504): NaN and negatives -> 0, +inf -> 65504
AKR_HD float dp_sanitise(float x) { return clamp_f(x, 0.0f, 65504.0f); }

// pixel i of a film accumulator, resolved as akr_film_resolve does and sanitised
AKR_HD float4 dp_load(const float* film, uint64_t n, uint64_t i, float splat_scale) {
    float4 c = dn_resolve(film, n, i, splat_scale);
    c.x = dp_sanitise(c.x);
    c.y = dp_sanitise(c.y);
    c.z = dp_sanitise(c.z);
    c.w = 0.0f;
    return c;
}

// L = (0.2126 r + 0.7152 g) + 0.0722 b
AKR_HD float dp_lum(const float4& c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

// The histogram bin of a sanitised pixel's luminance: -1 = skipped (L < 2^-20), else clamp((int)floor((log_f(L) (1 / ln2) + 20) 8), 0, 255)
AKR_HD int dp_bin(float L) {
    if (L < 9.5367431640625e-07f) return -1;
    const float b = __builtin_floorf((log_f(L) * kDpInvLn2 + 20.0f) * 8.0f);
    const int i = (int)b;
    return i < 0 ? 0 : (i > kDpBins - 1 ? kDpBins - 1 : i);
}

AKR_HD float4 dp_scale(const float4& c, float f) {
    float4 r;
    r.x = c.x * f;
    r.y = c.y * f;
    r.z = c.z * f;
    r.w = 0.0f;
    return r;
}

// e = k s(c)
AKR_HD float4 dp_expose(const float4& c, float k) {
    float4 e;
    e.x = k * c.x;
    e.y = k * c.y;
    e.z = k * c.z;
    e.w = 0.0f;
    return e;
}

// The bright pass of a sanitised pixel: b = e (max_f(Le - threshold, 0) / max_f(Le, 1e-4f))
AKR_HD float4 dp_bright(const float4& c, float k, float threshold) {
    const float4 e = dp_expose(c, k);
    const float Le = dp_lum(e);
    return dp_scale(e, max_f(Le - threshold, 0.0f) / max_f(Le, 1e-4f));
}

// The 2 x 2 box: ((p00 + p10) + (p01 + p11)) 0.25 -- pXY the pixel at (2x + X, 2y + Y), clamped to the edge by the caller
AKR_HD float4 dp_box(const float4& p00, const float4& p10, const float4& p01, const float4& p11) {
    float4 r;
    r.x = ((p00.x + p10.x) + (p01.x + p11.x)) * 0.25f;
    r.y = ((p00.y + p10.y) + (p01.y + p11.y)) * 0.25f;
    r.z = ((p00.z + p10.z) + (p01.z + p11.z)) * 0.25f;
    r.w = 0.0f;
    return r;
}

AKR_HD int dp_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// One pass of [1 4 6 4 1] / 16: ((a-2 + a2) 0.0625 + (a-1 + a1) 0.25) + a0 0.375
AKR_HD float dp_blur1(float m2, float m1, float a0, float p1, float p2) { return ((m2 + p2) * 0.0625f + (m1 + p1) * 0.25f) + a0 * 0.375f; }
// fetch(d) -> the record at offset d (-2 .. 2) along the pass's axis, already clamped to the edge
template <class Fetch>
AKR_HD float4 dp_blur5(Fetch&& fetch) {
    const float4 m2 = fetch(-2), m1 = fetch(-1), a0 = fetch(0), p1 = fetch(1), p2 = fetch(2);
    float4 r;
    r.x = dp_blur1(m2.x, m1.x, a0.x, p1.x, p2.x);
    r.y = dp_blur1(m2.y, m1.y, a0.y, p1.y, p2.y);
    r.z = dp_blur1(m2.z, m1.z, a0.z, p1.z, p2.z);
    r.w = 0.0f;
    return r;
}

// up(U)(x, y): the centre-aligned bilinear x 2 of a level of sw x sh records. The destination pixel x lies between the source columns
// x0 = floor((x - 1) / 2) and x0 + 1 with weights 1/4, 3/4 (x even) or 3/4, 1/4 (x odd), both clamped to the edge; the same in y.
// wy0 (wx0 c00 + wx1 c10) + wy1 (wx0 c01 + wx1 c11). fetch(sx, sy) -> the source record.
template <class Fetch>
AKR_HD float4 dp_up(int x, int y, int sw, int sh, Fetch&& fetch) {
    const int x0 = dp_clampi((x - 1) >> 1, sw - 1), x1 = dp_clampi(((x - 1) >> 1) + 1, sw - 1);
    const int y0 = dp_clampi((y - 1) >> 1, sh - 1), y1 = dp_clampi(((y - 1) >> 1) + 1, sh - 1);
    const float wx0 = (x & 1) ? 0.75f : 0.25f, wx1 = (x & 1) ? 0.25f : 0.75f;
    const float wy0 = (y & 1) ? 0.75f : 0.25f, wy1 = (y & 1) ? 0.25f : 0.75f;
    const float4 c00 = fetch(x0, y0), c10 = fetch(x1, y0), c01 = fetch(x0, y1), c11 = fetch(x1, y1);
    float4 r;
    r.x = wy0 * (wx0 * c00.x + wx1 * c10.x) + wy1 * (wx0 * c01.x + wx1 * c11.x);
    r.y = wy0 * (wx0 * c00.y + wx1 * c10.y) + wy1 * (wx0 * c01.y + wx1 * c11.y);
    r.z = wy0 * (wx0 * c00.z + wx1 * c10.z) + wy1 * (wx0 * c01.z + wx1 * c11.z);
    r.w = 0.0f;
    return r;
}

AKR_HD float4 dp_add(const float4& a, const float4& b) {
    float4 r;
    r.x = a.x + b.x;
    r.y = a.y + b.y;
    r.z = a.z + b.z;
    r.w = 0.0f;
    return r;
}

// Hable's curve before normalisation: (x (A x + C B) + D E) / (x (A x + B) + D F) - (D E) / (D F). The constant term is written as the
// quotient the first term has at x = 0, so that f(0) is 0 exactly
AKR_HD float dp_hable(float x) {
    const float A = 0.15f, B = 0.5f, Cc = 0.1f, D = 0.2f, E = 0.02f, F = 0.3f;
    return (x * (A * x + Cc * B) + D * E) / (x * (A * x + B) + D * F) - (D * E) / (D * F);
}

// The tone curve of one channel x >= 0, then clamp_f(y, 0, 1)
AKR_HD float dp_curve(float x, const DisplayParams& p) {
    float y = x;
    if (p.curve == kDpReinhard) y = (x * (1.0f + x / p.white2)) / (1.0f + x);
    else if (p.curve == kDpAces) y = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
    else if (p.curve == kDpHable) y = dp_hable(x) / p.hable_norm;
    return clamp_f(y, 0.0f, 1.0f);
}

// The output of a sanitised pixel c with bloom term u = up(U_1) at the pixel (read only when the bloom is on):
// curve(e + strength (u (1 / bloom_levels))) per channel
AKR_HD void dp_apply(const float4& c, const float4& u, const DisplayParams& p, float out[3]) {
    float4 e = dp_expose(c, p.k);
    if (p.strength != 0.0f) {
        e.x = e.x + p.strength * (u.x * p.inv_levels);
        e.y = e.y + p.strength * (u.y * p.inv_levels);
        e.z = e.z + p.strength * (u.z * p.inv_levels);
    }
    out[0] = dp_curve(e.x, p);
    out[1] = dp_curve(e.y, p);
    out[2] = dp_curve(e.z, p);
}

}  // namespace akr
