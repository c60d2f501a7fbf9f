// denoise_kernels.h -- host-callable launchers of denoise_kernels.hip (akr_denoise). Host side only.
#pragma once
#include <hip/hip_runtime.h>

#include "device/ddenoise.h"

namespace akr {

// the three record planes of a frame: float4[N] each
struct DenoiseRecords {
    float4 *x, *n, *a;
};
// films are accumulators [rgb 3N | splat 3N | weight N]; albedo / normal may be nullptr
hipError_t launch_denoise_prepare(const float* color, float color_scale, const float* albedo, float albedo_scale, const float* normal, float normal_scale,
                                  uint64_t n_pixels, uint32_t demodulate, float albedo_floor, DenoiseRecords rec, hipStream_t stream);
// one level: rec.x -> x_out. tiled = false: one thread per pixel gathering from global memory; true: the LDS-tiled kernel
hipError_t launch_denoise_level(const DenoiseLevel& lv, DenoiseRecords rec, float4* x_out, bool tiled, hipStream_t stream);
// akr_denoise_variance: prepare with the half film (records {x, v | -1}, {n, r | -1}, {a, -}), the prefilter that turns the estimates r
// into v0 in place in rec.x (lv.kn, lv.ka and the size are read), and one variance-guided level (lv.kc = kv)
hipError_t launch_denoise_prepare_var(const float* color, float color_scale, const float* half, const float* albedo, float albedo_scale, const float* normal,
                                      float normal_scale, uint64_t n_pixels, uint32_t demodulate, float albedo_floor, DenoiseRecords rec, hipStream_t stream);
hipError_t launch_denoise_variance(const DenoiseLevel& lv, DenoiseRecords rec, hipStream_t stream);
hipError_t launch_denoise_level_var(const DenoiseLevel& lv, DenoiseRecords rec, float4* x_out, bool tiled, hipStream_t stream);
// out film: rgb = x d, splat = 0, weight = 1
hipError_t launch_denoise_finish(const float4* x, const float4* a, uint64_t n_pixels, uint32_t demodulate, float albedo_floor, float* out_film, hipStream_t stream);

}  // namespace akr
