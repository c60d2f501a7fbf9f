// denoise_kernels.h -- host-callable launchers of denoise_kernels.hip (akr_denoise, akr_denoise_variance). Host side only.
#pragma once
#include <hip/hip_runtime.h>

#include "device/ddenoise.h"

namespace akr {

// the three record planes of a frame: float4[N] each
struct DenoiseRecords {
    float4 *x, *n, *a;
};
// films are accumulators [rgb 3N | splat 3N | weight N]; albedo / normal may be nullptr. half = nullptr: akr_denoise's records; else
// akr_denoise_variance's, from the half film (ddenoise.h DnPlain, DnVariance)
hipError_t launch_denoise_prepare(const float* color, float color_scale, const float* half, const float* albedo, float albedo_scale, const float* normal,
                                  float normal_scale, uint64_t n_pixels, uint32_t demodulate, float albedo_floor, DenoiseRecords rec, hipStream_t stream);
// akr_denoise_variance's prefilter: turns the estimates r into v0 in place in rec.x (lv.kn, lv.ka and the size are read)
hipError_t launch_denoise_variance(const DenoiseLevel& lv, DenoiseRecords rec, hipStream_t stream);
// one level: rec.x -> x_out. tiled = false: one thread per pixel gathering from global memory; true: the LDS-tiled kernel.
// variance: the variance-guided level (lv.kc = kv) over akr_denoise_variance's records
hipError_t launch_denoise_level(const DenoiseLevel& lv, DenoiseRecords rec, float4* x_out, bool tiled, bool variance, hipStream_t stream);
// out film: rgb = x d, splat = 0, weight = 1
hipError_t launch_denoise_finish(const float4* x, const float4* a, uint64_t n_pixels, uint32_t demodulate, float albedo_floor, float* out_film, hipStream_t stream);

}  // namespace akr
