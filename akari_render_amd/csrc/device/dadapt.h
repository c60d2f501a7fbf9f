// dadapt.h -- the error estimate of adaptive sampling, written once for the device (adapt_kernels.hip) and the
// host (host/api_adapt.cpp akr_host_tile_error). Under the AKR-F32 contract: no contraction, IEEE division and square root.
//
// C is a pt film [rgb 3N | splat 3N | weight N], Hf the half film: the same layout, holding the samples of the A-rounds only. The two
// halves of a pixel's samples give its error estimate (Dammertz et al. 2010, the stopping measure); a tile's error is the mean of its
// pixels' estimates, summed through a fixed binary tree so that any implementation of the reduction gives the same bits.
#pragma once
#include "dmath.h"

namespace akr {

constexpr uint32_t kAdaptMaxTilePixels = 4096;  // tile_w * tile_h of an adaptive render (the tree's leaves live in 16 KB of LDS)

// P: the tree's leaf count, the next power of two >= tile_w * tile_h
AKR_HD uint32_t ad_tree_leaves(uint32_t tile_pixels) {
    uint32_t p = 1;
    while (p < tile_pixels) p <<= 1;
    return p;
}

// e of pixel i of an N-pixel frame; has = the pixel has an estimate (wA > 0, wB > 0, e finite). The splat planes are not read.
//   cA = Hf.rgb / wA, cB = (C.rgb - Hf.rgb) / wB, c = C.rgb / C.w
//   d = (|cA_r - cB_r| + |cA_g - cB_g|) + |cA_b - cB_b|,  f = sqrt((wA wB) / (C.w C.w)),  l = (c_r + c_g) + c_b
//   e = (d f) / sqrt(l + 0.01)
AKR_HD float ad_pixel_error(const float* film, const float* half, uint64_t n, uint64_t i, bool& has) {
    const float wc = film[6 * n + i];
    const float wa = half[6 * n + i], wb = wc - wa;
    const float cr = film[3 * i + 0], cg = film[3 * i + 1], cb = film[3 * i + 2];
    const float hr = half[3 * i + 0], hg = half[3 * i + 1], hb = half[3 * i + 2];
    const float ar = hr / wa, ag = hg / wa, ab = hb / wa;
    const float br = (cr - hr) / wb, bg = (cg - hg) / wb, bb = (cb - hb) / wb;
    const float d = (abs_f(ar - br) + abs_f(ag - bg)) + abs_f(ab - bb);
    const float f = sqrt_f((wa * wb) / (wc * wc));
    const float l = (cr / wc + cg / wc) + cb / wc;
    const float e = (d * f) / sqrt_f(l + 0.01f);
    has = wa > 0.0f && wb > 0.0f && is_finite(e);
    return has ? e : 0.0f;
}

// Leaf `slot` of tile (tx, ty): the estimate of pixel (x_in_tile, y_in_tile) = (slot % tile_w, slot / tile_w), +0 for a pixel without
// one, outside the frame, or a slot past the tile's pixels. has as above (false for the padding).
AKR_HD float ad_tile_leaf(const float* film, const float* half, uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t tx, uint32_t ty,
                          uint32_t slot, bool& has) {
    has = false;
    if (slot >= tile_w * tile_h) return 0.0f;
    const uint32_t yt = slot / tile_w, xt = slot - yt * tile_w;
    const uint32_t px = tx * tile_w + xt, py = ty * tile_h + yt;
    if (px >= width || py >= height) return 0.0f;
    return ad_pixel_error(film, half, (uint64_t)width * height, (uint64_t)py * width + px, has);
}

// err of a tile from the tree's root and the count of pixels with an estimate
AKR_HD float ad_tile_error(float root, uint32_t n_est) { return n_est > 0 ? root / (float)n_est : u2f(0x7f800000u); }

// The half film around an A-round: open is Hf <- Hf - C before it, close Hf <- Hf + C after it, on the rgb and weight planes of a pixel;
// (Hf - C_before) + C_after adds the round's samples to Hf, and its rounding is part of the definition.
AKR_HD void ad_half_pixel(const float* film, float* half, uint64_t n, uint64_t i, bool close) {
    for (int k = 0; k < 3; k++) half[3 * i + k] = close ? half[3 * i + k] + film[3 * i + k] : half[3 * i + k] - film[3 * i + k];
    half[6 * n + i] = close ? half[6 * n + i] + film[6 * n + i] : half[6 * n + i] - film[6 * n + i];
}

}  // namespace akr
