// display_kernels.h -- host-callable launchers of display_kernels.hip (akr_display_transform). Host side only.
#pragma once
#include <hip/hip_runtime.h>

#include "device/ddisplay.h"

namespace akr {

// films are accumulators [rgb 3N | splat 3N | weight N]; a bloom level is float4[w * h]
// counts257: 256 bins and the skipped count, device memory, added to (the caller zeroes it)
hipError_t launch_lum_histogram(const float* film, float splat_scale, uint64_t n_pixels, uint32_t* counts257, hipStream_t stream);
// film (w x h) -> level 1 (ceil(w / 2) x ceil(h / 2)): the 2 x 2 box of the bright pass
hipError_t launch_bloom_source(const float* film, float splat_scale, uint32_t w, uint32_t h, float k, float threshold, float4* level1, hipStream_t stream);
// level l (sw x sh) -> level l + 1 (ceil(sw / 2) x ceil(sh / 2))
hipError_t launch_bloom_down(const float4* src, uint32_t sw, uint32_t sh, float4* dst, hipStream_t stream);
// src -> dst, [1 4 6 4 1] / 16 horizontally then vertically. tiled = false: two gathering passes through tmp (w x h records);
// true: one kernel whose horizontal pass stays in LDS (tmp is not touched). dst and tmp differ from src.
hipError_t launch_bloom_blur(const float4* src, float4* tmp, float4* dst, uint32_t w, uint32_t h, bool tiled, hipStream_t stream);
// dst (dw x dh) += up(src (sw x sh))
hipError_t launch_bloom_up(float4* dst, uint32_t dw, uint32_t dh, const float4* src, uint32_t sw, uint32_t sh, hipStream_t stream);
// film -> out film (rgb = the result, splat = 0, weight = 1); u1 = U_1 (lw x lh), read only when p.strength != 0. out may be film.
hipError_t launch_display_apply(const float* film, float splat_scale, uint32_t w, uint32_t h, DisplayParams p, const float4* u1, uint32_t lw, uint32_t lh, float* out,
                                hipStream_t stream);

}  // namespace akr
