// ddenoise.h -- the edge-avoiding a-trous filter of akr_denoise and akr_denoise_variance, written once for the device
// (denoise_kernels.hip) and the host (host/api_denoise.cpp host_denoise). Under the AKR-F32 contract: no contraction, IEEE division, exp_f of dmath.h.
//
// A pixel is three 16-byte records: {x.rgb, x.w}, {n.xyz, n.w}, {a.rgb, -} -- x the (demodulated) colour, n and a the guides as resolved.
// One level at step s reads the 5 x 5 taps q = p + s (dx, dy) of the previous level's x and writes the next x; n and a never change.
// What the fourth components hold is the guide policy's (below): the one thing akr_denoise and akr_denoise_variance differ in.
#pragma once
#include "dmath.h"

namespace akr {

// What a level needs besides the records: k = 1 / sigma^2 per term (0 = the term is off), kc already scaled for the level
struct DenoiseLevel {
    uint32_t width, height, step;
    float kc, kn, ka;
};

// The guide policies. akr_denoise: x.w = 1 for a valid pixel, 0 for an invalid one; n.w is not read; lv.kc = 1 / (sigma_color 2^-i)^2.
struct DnPlain {
    static constexpr bool kVariance = false;
    static constexpr float kValidW = 1.0f, kInvalidW = 0.0f;  // x.w as prepare writes it; kInvalidW is an out-of-image record's too
    static AKR_HD bool valid(const float4& x) { return x.w != 0.0f; }
};
// akr_denoise_variance ("Variance guide"): x.w = v, the variance of the pixel's colour, and -1 for an invalid pixel; n.w = r, the pixel's own
// two-half estimate, and -1 where there is none. A level reads lv.kc as kv = 1 / sigma_variance^2.
struct DnVariance {
    static constexpr bool kVariance = true;
    static constexpr float kValidW = 0.0f, kInvalidW = -1.0f;
    static AKR_HD bool valid(const float4& x) { return !(x.w < 0.0f); }
};

// dot(v, v) = (vx vx + vy vy) + vz vz of v = p - q
AKR_HD float dn_dist2(const float4& p, const float4& q) {
    const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
    return (dx * dx + dy * dy) + dz * dz;
}

// B = {1/16, 1/4, 3/8, 1/4, 1/16}: the B3 spline, every product of two entries exact
AKR_HD float dn_b3(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }

// G = {1/4, 1/2, 1/4}
AKR_HD float dn_g3(int d) { return d == 0 ? 0.5f : 0.25f; }

// w = h exp(-e), e = (|x_p - x_q|^2 kc + |n_p - n_q|^2 kn) + |a_p - a_q|^2 ka
AKR_HD float dn_tap_weight(float h, const float4& xp, const float4& np_, const float4& ap, const float4& xq, const float4& nq, const float4& aq,
                           const DenoiseLevel& lv) {
    const float e = (dn_dist2(xp, xq) * lv.kc + dn_dist2(np_, nq) * lv.kn) + dn_dist2(ap, aq) * lv.ka;
    return h * exp_f(-e);
}

// The record x of pixel (px, py) after one level under guide G. fetch(dx, dy, xq, nq, aq) -> bool reads the records of the in-image pixel
// (px, py) + step (dx, dy) and says whether it is valid (G::valid(xq)): the two level kernels and the host differ in nothing but where the
// records lie. DnVariance: kc is divided by g, the variance smoothed over the 3 x 3 taps of the level's own lattice, and x.w becomes v'.
template <class G, class Fetch>
AKR_HD float4 dn_level_pixel(int px, int py, const DenoiseLevel& lv, Fetch&& fetch) {
    float4 xp, np_, ap;
    if (!fetch(0, 0, xp, np_, ap)) return xp;  // an invalid centre passes through unchanged
    const int s = (int)lv.step;
    DenoiseLevel lp = lv;
    if constexpr (G::kVariance) {
        float gn = 0.0f, gd = 0.0f;
        for (int dy = -1; dy <= 1; dy++) {
            const int qy = py + s * dy;
            for (int dx = -1; dx <= 1; dx++) {
                const int qx = px + s * dx;
                if (qx < 0 || qy < 0 || qx >= (int)lv.width || qy >= (int)lv.height) continue;
                float4 xq, nq, aq;
                if (!fetch(dx, dy, xq, nq, aq)) continue;
                const float gw = dn_g3(dx) * dn_g3(dy);
                gn = gn + gw * xq.w;
                gd = gd + gw;
            }
        }
        const float g = gn / gd;
        lp.kc = lv.kc / (g + 1e-10f);
    }
    [[maybe_unused]] float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f, vacc = 0.0f, wsum = 0.0f;  // (vacc: DnVariance alone)
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = py + s * dy;
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = px + s * dx;
            if (qx < 0 || qy < 0 || qx >= (int)lv.width || qy >= (int)lv.height) continue;  // no clamping, no mirroring
            float4 xq, nq, aq;
            if (!fetch(dx, dy, xq, nq, aq)) continue;
            const float w = dn_tap_weight(dn_b3(dx) * dn_b3(dy), xp, np_, ap, xq, nq, aq, lp);
            acc0 = acc0 + w * xq.x;
            acc1 = acc1 + w * xq.y;
            acc2 = acc2 + w * xq.z;
            if constexpr (G::kVariance) vacc = vacc + (w * w) * xq.w;
            wsum = wsum + w;
        }
    }
    float4 y;
    y.x = acc0 / wsum;
    y.y = acc1 / wsum;
    y.z = acc2 / wsum;
    if constexpr (G::kVariance) y.w = vacc / (wsum * wsum);
    else y.w = xp.w;
    return y;
}

// Film resolve of pixel i of an accumulator [rgb 3N | splat 3N | weight N] = k_film_resolve; a NULL film reads as 0
AKR_HD float4 dn_resolve(const float* film, uint64_t n, uint64_t i, float splat_scale) {
    float4 r;
    r.x = r.y = r.z = r.w = 0.0f;
    if (!film) return r;
    const float w = film[6 * n + i];
    const float inv = w == 0.0f ? 1.0f : w;
    r.x = film[3 * i + 0] / inv + film[3 * n + 3 * i + 0] * splat_scale;
    r.y = film[3 * i + 1] / inv + film[3 * n + 3 * i + 1] * splat_scale;
    r.z = film[3 * i + 2] / inv + film[3 * n + 3 * i + 2] * splat_scale;
    return r;
}

AKR_HD bool dn_finite(float v) { return (f2u(v) & 0x7f800000u) != 0x7f800000u; }

// d = max(a, albedo_floor) per channel when the call demodulates (a NaN albedo reads as the floor), else 1
AKR_HD float4 dn_divisor(const float4& a, bool demodulate, float albedo_floor) {
    float4 d;
    d.x = demodulate ? (a.x > albedo_floor ? a.x : albedo_floor) : 1.0f;
    d.y = demodulate ? (a.y > albedo_floor ? a.y : albedo_floor) : 1.0f;
    d.z = demodulate ? (a.z > albedo_floor ? a.z : albedo_floor) : 1.0f;
    d.w = 0.0f;
    return d;
}

// resolve, demodulate, validity: the three records of pixel i. DnVariance: plus the two-half estimate r = |xA - xB|^2 (wA wB) / (C.w C.w) of
// `half`, the colour film as it stood after a subset of the samples (its splat plane is not read). DnPlain does not read `half`.
template <class G>
AKR_HD void dn_prepare_pixel(const float* color, float color_scale, const float* half, const float* albedo, float albedo_scale, const float* normal,
                             float normal_scale, uint64_t n, uint64_t i, bool demodulate, float albedo_floor, float4& x, float4& nn, float4& a) {
    const float4 c = dn_resolve(color, n, i, color_scale);
    a = dn_resolve(albedo, n, i, albedo_scale);
    nn = dn_resolve(normal, n, i, normal_scale);
    const float4 d = dn_divisor(a, demodulate, albedo_floor);
    x.x = c.x / d.x;
    x.y = c.y / d.y;
    x.z = c.z / d.z;
    const bool valid = dn_finite(x.x) && dn_finite(x.y) && dn_finite(x.z) && dn_finite(nn.x) && dn_finite(nn.y) && dn_finite(nn.z) && dn_finite(a.x) &&
                       dn_finite(a.y) && dn_finite(a.z);
    x.w = valid ? G::kValidW : G::kInvalidW;
    if constexpr (G::kVariance) {
        const float wc = color[6 * n + i];
        const float wa = half[6 * n + i], wb = wc - wa;
        float4 xa, xb;
        xa.x = (half[3 * i + 0] / wa) / d.x;
        xa.y = (half[3 * i + 1] / wa) / d.y;
        xa.z = (half[3 * i + 2] / wa) / d.z;
        xb.x = ((color[3 * i + 0] - half[3 * i + 0]) / wb) / d.x;
        xb.y = ((color[3 * i + 1] - half[3 * i + 1]) / wb) / d.y;
        xb.z = ((color[3 * i + 2] - half[3 * i + 2]) / wb) / d.z;
        xa.w = xb.w = 0.0f;
        const float f = (wa * wb) / (wc * wc);
        const float r = dn_dist2(xa, xb) * f;
        const bool est = valid && wa > 0.0f && wb > 0.0f && dn_finite(r);
        nn.w = est ? r : -1.0f;
    }
}

// v0 of the valid pixel (px, py) of akr_denoise_variance: the 7 x 7 guide-weighted mean of the estimates r. fetch(dx, dy, nq, aq) -> bool reads
// the n and a records of the in-image pixel (px, py) + (dx, dy) and says whether it carries an estimate (nq.w, then)
template <class Fetch>
AKR_HD float dn_prefilter_pixel(int px, int py, const DenoiseLevel& lv, Fetch&& fetch) {
    float4 np_, ap;
    (void)fetch(0, 0, np_, ap);
    float num = 0.0f, den = 0.0f;
    for (int dy = -3; dy <= 3; dy++) {
        const int qy = py + dy;
        for (int dx = -3; dx <= 3; dx++) {
            const int qx = px + dx;
            if (qx < 0 || qy < 0 || qx >= (int)lv.width || qy >= (int)lv.height) continue;
            float4 nq, aq;
            if (!fetch(dx, dy, nq, aq)) continue;
            const float m = exp_f(-(dn_dist2(np_, nq) * lv.kn + dn_dist2(ap, aq) * lv.ka));
            num = num + m * nq.w;
            den = den + m;
        }
    }
    return den > 0.0f ? num / den : 0.0f;
}

// out = y d
AKR_HD void dn_finish_pixel(const float4& y, const float4& a, bool demodulate, float albedo_floor, float out[3]) {
    const float4 d = dn_divisor(a, demodulate, albedo_floor);
    out[0] = y.x * d.x;
    out[1] = y.y * d.y;
    out[2] = y.z * d.z;
}

}  // namespace akr
