// adapt_kernels.hip -- adaptive sampling's kernels over pt films: a tile's error from the film and its half film,
// and the two elementwise passes that keep the half film around an A-round. The arithmetic is device/dadapt.h, shared with the host; the
// kernels below only decide which lane takes which pixel and how the tree's sums travel.
#include "adapt_kernels.h"
#include "launch.h"

namespace akr {

// One workgroup per listed tile. Lane t takes the leaves t, t + 256, ...: a leaf is a pixel in row-major order of the tile, so a wave reads
// 64 consecutive pixels of a film row (or whole rows of a narrow tile) -- 768 contiguous bytes of the rgb plane, 256 of the weight plane, per film.
// The tree: s[i] += s[i + stride] for stride = P / 2 ... 1. Strides of 64 and more go through LDS with a barrier between two of them (a step
// reads [stride, 2 stride) and writes [0, stride): no hazard inside one); the last six are shuffles inside wave 0, lane i adding lane
// i + stride's value -- the same additions on the same operands, and what the lanes >= stride compute is never read.
__global__ void __launch_bounds__(256) k_tile_error(AdaptFrame fr, const float* __restrict__ film, const float* __restrict__ half, const uint32_t* __restrict__ tiles,
                                                    float* __restrict__ err) {
    __shared__ float s[kAdaptMaxTilePixels];
    __shared__ uint32_t n_est;
    const uint32_t tile = tiles[blockIdx.x];
    const uint32_t ty = tile / fr.tiles_x, tx = tile - ty * fr.tiles_x;
    const uint32_t P = ad_tree_leaves(fr.tile_w * fr.tile_h);  // 64 ... 4096
    if (threadIdx.x == 0) n_est = 0u;
    uint32_t mine = 0;
    for (uint32_t i = threadIdx.x; i < P; i += 256u) {
        bool has;
        s[i] = ad_tile_leaf(film, half, fr.width, fr.height, fr.tile_w, fr.tile_h, tx, ty, i, has);
        mine += has ? 1u : 0u;
    }
    for (int off = 32; off >= 1; off >>= 1) mine += __shfl_down(mine, off, 64);  // (an integer sum: any order)
    __syncthreads();  // the leaves, and n_est = 0
    if ((threadIdx.x & 63u) == 0u && mine != 0u) atomicAdd(&n_est, mine);
    for (uint32_t stride = P >> 1; stride >= 64u; stride >>= 1) {
        for (uint32_t i = threadIdx.x; i < stride; i += 256u) s[i] = s[i] + s[i + stride];
        __syncthreads();
    }
    __syncthreads();  // (P = 64: no step above; the counts in any case)
    if (threadIdx.x < 64u) {
        float v = s[threadIdx.x];
        for (int stride = 32; stride >= 1; stride >>= 1) v = v + __shfl_down(v, stride, 64);
        if (threadIdx.x == 0) err[blockIdx.x] = ad_tile_error(v, n_est);
    }
}

// One workgroup per listed tile, a lane per pixel in row-major order of the tile
template <bool CLOSE>
__global__ void __launch_bounds__(256) k_half_bracket(AdaptFrame fr, const float* __restrict__ film, float* __restrict__ half, const uint32_t* __restrict__ tiles) {
    const uint32_t tile = tiles[blockIdx.x];
    const uint32_t ty = tile / fr.tiles_x, tx = tile - ty * fr.tiles_x;
    const uint64_t n = (uint64_t)fr.width * fr.height;
    for (uint32_t i = threadIdx.x; i < fr.tile_w * fr.tile_h; i += 256u) {
        const uint32_t yt = i / fr.tile_w, xt = i - yt * fr.tile_w;
        const uint32_t px = tx * fr.tile_w + xt, py = ty * fr.tile_h + yt;
        if (px < fr.width && py < fr.height) ad_half_pixel(film, half, n, (uint64_t)py * fr.width + px, CLOSE);
    }
}

hipError_t launch_tile_error(const AdaptFrame& fr, const float* film, const float* half, const uint32_t* tiles, uint32_t n, float* err, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    launch_kernel(k_tile_error, n, 0, stream, fr, film, half, tiles, err);
    return hipGetLastError();
}
hipError_t launch_half_bracket(const AdaptFrame& fr, const float* film, float* half, const uint32_t* tiles, uint32_t n, bool close, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    dispatch_bools([&](auto C) { launch_kernel(k_half_bracket<C()>, n, 0, stream, fr, film, half, tiles); }, close);
    return hipGetLastError();
}

}  // namespace akr
