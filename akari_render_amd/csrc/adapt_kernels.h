// adapt_kernels.h -- host-callable launchers of adapt_kernels.hip (adaptive sampling). Host side only.
#pragma once
#include <hip/hip_runtime.h>

#include "device/dadapt.h"

namespace akr {

// a frame cut into tiles; films are accumulators [rgb 3N | splat 3N | weight N]
struct AdaptFrame {
    uint32_t width, height, tile_w, tile_h, tiles_x;
};
// err[j] = the error of tile tiles[j] (row-major ids, all below tiles_x * tiles_y), j < n; tiles and err are device arrays
hipError_t launch_tile_error(const AdaptFrame& fr, const float* film, const float* half, const uint32_t* tiles, uint32_t n, float* err, hipStream_t stream);
// half <- half - film (close = false) or half + film (close = true) over the rgb and weight planes of the listed tiles' pixels
hipError_t launch_half_bracket(const AdaptFrame& fr, const float* film, float* half, const uint32_t* tiles, uint32_t n, bool close, hipStream_t stream);

}  // namespace akr
