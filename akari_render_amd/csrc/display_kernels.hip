// display_kernels.hip -- akr_display_transform: auto-exposure histogram, bloom pyramid and the fused exposure / bloom / tone-curve pass over a
// film. The arithmetic is device/ddisplay.h, shared with the host; the kernels below only decide where a pixel's
// records lie.
#include "display_kernels.h"
#include "launch.h"

namespace akr {

// The log-luminance histogram, grid-stride. Each of the four waves of a workgroup counts into its own LDS histogram (a flat image sends every
// lane to one bin: one histogram per workgroup would serialise all 256 lanes on it), bin 256 counting the skipped pixels. A pitch of 257
// dwords puts one bin of the four histograms into four different banks. After a barrier the four are summed and every non-zero bin is one
// global atomicAdd per workgroup. Integer adds: the counts do not depend on the order.
constexpr int kDpHistPitch = kDpBins + 1;
__global__ void __launch_bounds__(256) k_lum_histogram(const float* __restrict__ film, float splat_scale, uint64_t n, uint32_t* __restrict__ counts) {
    __shared__ uint32_t hist[4 * kDpHistPitch];
    for (int t = (int)threadIdx.x; t < 4 * kDpHistPitch; t += 256) hist[t] = 0u;
    __syncthreads();
    uint32_t* mine = hist + (threadIdx.x >> 6) * kDpHistPitch;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const int b = dp_bin(dp_lum(dp_load(film, n, i, splat_scale)));
        atomicAdd(&mine[b < 0 ? kDpBins : b], 1u);
    }
    __syncthreads();
    for (int t = (int)threadIdx.x; t < kDpHistPitch; t += 256) {
        const uint32_t s = (hist[t] + hist[kDpHistPitch + t]) + (hist[2 * kDpHistPitch + t] + hist[3 * kDpHistPitch + t]);
        if (s) atomicAdd(&counts[t], s);
    }
}

// film -> level 1: one thread per level-1 pixel, the bright pass of its four film pixels (coordinates clamped to the edge) and their box
__global__ void __launch_bounds__(256) k_bloom_source(const float* __restrict__ film, float splat_scale, uint32_t w, uint32_t h, float k, float threshold,
                                                      float4* __restrict__ dst, uint32_t dw, uint32_t dh) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint64_t)dw * dh) return;
    const uint32_t x = (uint32_t)(i % dw), y = (uint32_t)(i / dw);
    const uint32_t x0 = 2 * x, y0 = 2 * y, x1 = x0 + 1 < w ? x0 + 1 : w - 1, y1 = y0 + 1 < h ? y0 + 1 : h - 1;
    const uint64_t n = (uint64_t)w * h;
    auto b = [&](uint32_t px, uint32_t py) { return dp_bright(dp_load(film, n, (uint64_t)py * w + px, splat_scale), k, threshold); };
    dst[i] = dp_box(b(x0, y0), b(x1, y0), b(x0, y1), b(x1, y1));
}

// level l -> level l + 1: one thread per destination pixel
__global__ void __launch_bounds__(256) k_bloom_down(const float4* __restrict__ src, uint32_t sw, uint32_t sh, float4* __restrict__ dst, uint32_t dw, uint32_t dh) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint64_t)dw * dh) return;
    const uint32_t x = (uint32_t)(i % dw), y = (uint32_t)(i / dw);
    const uint32_t x0 = 2 * x, y0 = 2 * y, x1 = x0 + 1 < sw ? x0 + 1 : sw - 1, y1 = y0 + 1 < sh ? y0 + 1 : sh - 1;
    dst[i] = dp_box(src[(size_t)y0 * sw + x0], src[(size_t)y0 * sw + x1], src[(size_t)y1 * sw + x0], src[(size_t)y1 * sw + x1]);
}

// Blur, implementation 0: one gathering pass per axis, one thread per pixel, five 16-byte loads from global memory
template <bool VERTICAL>
__global__ void __launch_bounds__(256) k_bloom_blur_pass(const float4* __restrict__ src, float4* __restrict__ dst, uint32_t w, uint32_t h) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint64_t)w * h) return;
    const int x = (int)(i % w), y = (int)(i / w), W = (int)w, H = (int)h;
    dst[i] = dp_blur5([&](int d) { return VERTICAL ? src[(size_t)dp_clampi(y + d, H - 1) * W + x] : src[(size_t)y * W + dp_clampi(x + d, W - 1)]; });
}

// Blur, implementation 1: both passes in one kernel. A workgroup takes a tile of 16 x 16 pixels; the horizontal pass of the tile's rows and of
// two halo rows above and below it (rows clamped to the image, as the vertical pass clamps its taps) goes to LDS -- 20 x 16 records, 5 120
// bytes --, then a barrier, then the vertical pass reads its five taps from LDS. The same additions on the same operands as implementation 0.
// LDS banks: a tile row is 16 records = 256 bytes = every bank once, and the pitch is one row, so a record's banks depend on its column
// alone; with lane = 16 row + column each of the four 16-lane groups that serve a 16-byte LDS read ({0-3, 12-15, 20-27}, {4-11, 16-19,
// 28-31}, the same + 32) holds 16 different columns: no conflicts (derived from the bank rule, not counted).
constexpr int kDpTile = 16, kDpHalo = 2, kDpRows = kDpTile + 2 * kDpHalo;
__global__ void __launch_bounds__(256) k_bloom_blur_tiled(const float4* __restrict__ src, float4* __restrict__ dst, uint32_t w, uint32_t h, uint32_t tiles_x) {
    __shared__ float4 hp[kDpRows * kDpTile];
    const int W = (int)w, H = (int)h;
    const int x0 = (int)(blockIdx.x % tiles_x) * kDpTile, y0 = (int)(blockIdx.x / tiles_x) * kDpTile;
    for (int t = (int)threadIdx.x; t < kDpRows * kDpTile; t += 256) {
        const int j = t / kDpTile, i = t - j * kDpTile;
        const int X = x0 + i, Y = dp_clampi(y0 + j - kDpHalo, H - 1);
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (X < W) v = dp_blur5([&](int d) { return src[(size_t)Y * W + dp_clampi(X + d, W - 1)]; });
        hp[t] = v;
    }
    __syncthreads();
    const int lx = (int)threadIdx.x & 15, ly = (int)threadIdx.x >> 4;
    const int px = x0 + lx, py = y0 + ly;
    if (px >= W || py >= H) return;
    dst[(size_t)py * W + px] = dp_blur5([&](int d) { return hp[(ly + kDpHalo + d) * kDpTile + lx]; });
}

// dst += up(src): one thread per destination pixel
__global__ void __launch_bounds__(256) k_bloom_up(float4* __restrict__ dst, uint32_t dw, uint32_t dh, const float4* __restrict__ src, uint32_t sw, uint32_t sh) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint64_t)dw * dh) return;
    const int x = (int)(i % dw), y = (int)(i / dw);
    const float4 u = dp_up(x, y, (int)sw, (int)sh, [&](int sx, int sy) { return src[(size_t)sy * sw + sx]; });
    dst[i] = dp_add(dst[i], u);
}

// The full-resolution pass: exposure, the bloom term up(U_1), the curve; writes the three planes of `out` (which may be `film`: a thread reads
// no film pixel but its own)
__global__ void __launch_bounds__(256) k_display_apply(const float* film, float splat_scale, uint32_t w, uint32_t h, DisplayParams p, const float4* __restrict__ u1,
                                                       uint32_t lw, uint32_t lh, float* out) {
    const uint64_t n = (uint64_t)w * h;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 c = dp_load(film, n, i, splat_scale);
    float4 u = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (p.strength != 0.0f) u = dp_up((int)(i % w), (int)(i / w), (int)lw, (int)lh, [&](int sx, int sy) { return u1[(size_t)sy * lw + sx]; });
    float rgb[3];
    dp_apply(c, u, p, rgb);
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        out[3 * i + ch] = rgb[ch];
        out[3 * n + 3 * i + ch] = 0.0f;
    }
    out[6 * n + i] = 1.0f;
}

static uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + 255) / 256); }

hipError_t launch_lum_histogram(const float* film, float splat_scale, uint64_t n, uint32_t* counts257, hipStream_t stream) {
    const uint64_t blocks = (n + 255) / 256;
    launch_kernel(k_lum_histogram, (uint32_t)(blocks < 2048 ? blocks : 2048), 0, stream, film, splat_scale, n, counts257);
    return hipGetLastError();
}
hipError_t launch_bloom_source(const float* film, float splat_scale, uint32_t w, uint32_t h, float k, float threshold, float4* level1, hipStream_t stream) {
    const uint32_t dw = (w + 1) / 2, dh = (h + 1) / 2;
    launch_kernel(k_bloom_source, blocks_of((uint64_t)dw * dh), 0, stream, film, splat_scale, w, h, k, threshold, level1, dw, dh);
    return hipGetLastError();
}
hipError_t launch_bloom_down(const float4* src, uint32_t sw, uint32_t sh, float4* dst, hipStream_t stream) {
    const uint32_t dw = (sw + 1) / 2, dh = (sh + 1) / 2;
    launch_kernel(k_bloom_down, blocks_of((uint64_t)dw * dh), 0, stream, src, sw, sh, dst, dw, dh);
    return hipGetLastError();
}
hipError_t launch_bloom_blur(const float4* src, float4* tmp, float4* dst, uint32_t w, uint32_t h, bool tiled, hipStream_t stream) {
    if (tiled) {
        const uint32_t tiles_x = (w + kDpTile - 1) / kDpTile, tiles_y = (h + kDpTile - 1) / kDpTile;
        launch_kernel(k_bloom_blur_tiled, tiles_x * tiles_y, 0, stream, src, dst, w, h, tiles_x);
    } else {
        launch_kernel(k_bloom_blur_pass<false>, blocks_of((uint64_t)w * h), 0, stream, src, tmp, w, h);
        launch_kernel(k_bloom_blur_pass<true>, blocks_of((uint64_t)w * h), 0, stream, (const float4*)tmp, dst, w, h);
    }
    return hipGetLastError();
}
hipError_t launch_bloom_up(float4* dst, uint32_t dw, uint32_t dh, const float4* src, uint32_t sw, uint32_t sh, hipStream_t stream) {
    launch_kernel(k_bloom_up, blocks_of((uint64_t)dw * dh), 0, stream, dst, dw, dh, src, sw, sh);
    return hipGetLastError();
}
hipError_t launch_display_apply(const float* film, float splat_scale, uint32_t w, uint32_t h, DisplayParams p, const float4* u1, uint32_t lw, uint32_t lh, float* out,
                                hipStream_t stream) {
    launch_kernel(k_display_apply, blocks_of((uint64_t)w * h), 0, stream, film, splat_scale, w, h, p, u1, lw, lh, out);
    return hipGetLastError();
}

}  // namespace akr
