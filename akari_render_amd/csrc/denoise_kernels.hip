// denoise_kernels.hip -- akr_denoise and akr_denoise_variance: the edge-avoiding a-trous filter over three films.
// The arithmetic is device/ddenoise.h, shared with the host; the kernels below only decide where a pixel's records lie. The kernels that
// the two calls share are templates over ddenoise.h's guide policy G (DnPlain, DnVariance).
#include <type_traits>

#include "denoise_kernels.h"
#include "launch.h"

namespace akr {

// k_denoise_prepare's `half` argument: the half film under DnVariance; under DnPlain, which reads none, an empty object that a launch makes
// of the (null) pointer -- the kernel carries no pointer that it never reads, and its other arguments lie where they do without one
struct DnNoHalf {
    __host__ __device__ DnNoHalf(const float*) {}
    __host__ __device__ operator const float*() const { return nullptr; }
};
template <class G>
using DnHalfArg = std::conditional_t<G::kVariance, const float* __restrict__, DnNoHalf>;

template <class G>
__global__ void __launch_bounds__(256) k_denoise_prepare(const float* __restrict__ color, float color_scale, DnHalfArg<G> half,
                                                         const float* __restrict__ albedo, float albedo_scale, const float* __restrict__ normal,
                                                         float normal_scale, uint64_t n, uint32_t demodulate, float albedo_floor, DenoiseRecords rec) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float4 x, nn, a;
    dn_prepare_pixel<G>(color, color_scale, half, albedo, albedo_scale, normal, normal_scale, n, i, demodulate != 0, albedo_floor, x, nn, a);
    rec.x[i] = x;
    rec.n[i] = nn;
    rec.a[i] = a;
}

// Baseline level kernel: one thread per pixel, a workgroup = 32 x 8 pixels, every tap three 16-byte loads from global memory.
template <class G>
__global__ void __launch_bounds__(256) k_denoise_level(DenoiseLevel lv, const float4* __restrict__ xs, const float4* __restrict__ ns, const float4* __restrict__ as,
                                                       float4* __restrict__ x_out, uint32_t blocks_x) {
    const uint32_t bx = blockIdx.x % blocks_x, by = blockIdx.x / blocks_x;
    const int px = (int)(bx * 32 + (threadIdx.x & 31)), py = (int)(by * 8 + (threadIdx.x >> 5));
    if (px >= (int)lv.width || py >= (int)lv.height) return;
    const int s = (int)lv.step, W = (int)lv.width;
    const float4 y = dn_level_pixel<G>(px, py, lv, [&](int dx, int dy, float4& xq, float4& nq, float4& aq) {
        const size_t q = (size_t)(py + s * dy) * W + (px + s * dx);
        xq = xs[q];
        nq = ns[q];
        aq = as[q];
        return G::valid(xq);
    });
    x_out[(size_t)py * W + px] = y;
}

// The lane-to-pixel mapping of the tiled kernels: column = lane & 15, and the row such that each of the four 16-lane groups the hardware
// serves a 16-byte LDS read in ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32) covers the 16 pixels of ONE tile row: 256
// contiguous bytes, every bank once, whatever the row pitch is. (With lane = 16 row + column the groups straddle two rows and a pitch of
// 20 records makes a quarter of each read 2-way.)
__device__ __forceinline__ void dn_tile_lane(int& lx, int& ly) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, quad = (lane >> 2) & 7;
    lx = lane & 15;
    ly = wave * 4 + ((lane >> 5) << 1) + ((((quad + 1) >> 1) & 1) ^ (quad >> 2));
}

// LDS-tiled level kernel. At step s the pixels of one residue class (x mod s, y mod s) form a dense image of their own, in which the
// level is a plain 5 x 5 convolution (the 3 x 3 taps of DnVariance's g lie inside it): a workgroup takes a 16 x 16 tile of one class,
// loads the tile and its halo of 2 once -- 20 x 20 x 3 records, 19 200 bytes -- and every tap is a 16-byte LDS read at a constant offset,
// lanes laid over the tile by dn_tile_lane. A record outside the image is stored invalid (x.w = G::kInvalidW).
constexpr int kDnTile = 16, kDnHalo = 2, kDnPitch = kDnTile + 2 * kDnHalo;
template <class G>
__global__ void __launch_bounds__(256) k_denoise_level_tiled(DenoiseLevel lv, const float4* __restrict__ xs, const float4* __restrict__ ns,
                                                             const float4* __restrict__ as, float4* __restrict__ x_out, uint32_t tiles_x) {
    __shared__ float4 sx[kDnPitch * kDnPitch], sn[kDnPitch * kDnPitch], sa[kDnPitch * kDnPitch];
    const int s = (int)lv.step, W = (int)lv.width, H = (int)lv.height;
    // the class is the fastest-varying part of the block index: neighbouring blocks read neighbouring 16-byte records of the same lines
    uint32_t b = blockIdx.x;
    const int rx = (int)(b % lv.step);
    b /= lv.step;
    const int ry = (int)(b % lv.step);
    b /= lv.step;
    const int cx0 = (int)(b % tiles_x) * kDnTile, cy0 = (int)(b / tiles_x) * kDnTile;  // the tile's origin in class coordinates
    if (rx + s * cx0 >= W || ry + s * cy0 >= H) return;  // a class with fewer tiles than the widest one (the whole workgroup leaves)
    for (int t = (int)threadIdx.x; t < kDnPitch * kDnPitch; t += 256) {
        const int j = t / kDnPitch, i = t - j * kDnPitch;
        const int X = rx + s * (cx0 + i - kDnHalo), Y = ry + s * (cy0 + j - kDnHalo);
        // outside the image: x invalid, n and a zero. (n is spelled so that each instantiation compiles to the code it had as a kernel of its own)
        float4 x = make_float4(0.0f, 0.0f, 0.0f, G::kInvalidW), n = G::kVariance ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : x, a = n;
        if (X >= 0 && Y >= 0 && X < W && Y < H) {
            const size_t q = (size_t)Y * W + X;
            x = xs[q];
            n = ns[q];
            a = as[q];
        }
        sx[t] = x;
        sn[t] = n;
        sa[t] = a;
    }
    __syncthreads();
    int lx, ly;
    dn_tile_lane(lx, ly);
    const int px = rx + s * (cx0 + lx), py = ry + s * (cy0 + ly);
    if (px >= W || py >= H) return;
    const int centre = (ly + kDnHalo) * kDnPitch + lx + kDnHalo;
    const float4 y = dn_level_pixel<G>(px, py, lv, [&](int dx, int dy, float4& xq, float4& nq, float4& aq) {
        const int q = centre + dy * kDnPitch + dx;
        xq = sx[q];
        nq = sn[q];
        aq = sa[q];
        return G::valid(xq);
    });
    x_out[(size_t)py * W + px] = y;
}

// The prefilter of akr_denoise_variance: v0 = the 7 x 7 guide-weighted mean of the two-half estimates, written into x.w of every valid pixel.
// A workgroup takes 16 x 16 pixels, loads their n and a records and a halo of 3 -- 22 x 22 x 2 records, 15 488 bytes -- and reads every tap
// from LDS, lanes laid over the tile as in k_denoise_level_tiled. A record outside the image is stored without an estimate.
constexpr int kDnVarHalo = 3, kDnVarPitch = kDnTile + 2 * kDnVarHalo;
__global__ void __launch_bounds__(256) k_denoise_variance(DenoiseLevel lv, float4* __restrict__ xs, const float4* __restrict__ ns, const float4* __restrict__ as,
                                                          uint32_t tiles_x) {
    __shared__ float4 sn[kDnVarPitch * kDnVarPitch], sa[kDnVarPitch * kDnVarPitch];
    const int W = (int)lv.width, H = (int)lv.height;
    const int x0 = (int)(blockIdx.x % tiles_x) * kDnTile, y0 = (int)(blockIdx.x / tiles_x) * kDnTile;
    for (int t = (int)threadIdx.x; t < kDnVarPitch * kDnVarPitch; t += 256) {
        const int j = t / kDnVarPitch, i = t - j * kDnVarPitch;
        const int X = x0 + i - kDnVarHalo, Y = y0 + j - kDnVarHalo;
        float4 n = make_float4(0.0f, 0.0f, 0.0f, -1.0f), a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (X >= 0 && Y >= 0 && X < W && Y < H) {
            const size_t q = (size_t)Y * W + X;
            n = ns[q];
            a = as[q];
        }
        sn[t] = n;
        sa[t] = a;
    }
    __syncthreads();
    int lx, ly;
    dn_tile_lane(lx, ly);
    const int px = x0 + lx, py = y0 + ly;
    if (px >= W || py >= H) return;
    const size_t p = (size_t)py * W + px;
    float4 x = xs[p];
    if (!DnVariance::valid(x)) return;
    const int centre = (ly + kDnVarHalo) * kDnVarPitch + lx + kDnVarHalo;
    x.w = dn_prefilter_pixel(px, py, lv, [&](int dx, int dy, float4& nq, float4& aq) {
        const int q = centre + dy * kDnVarPitch + dx;
        nq = sn[q];
        aq = sa[q];
        return !(nq.w < 0.0f);
    });
    xs[p] = x;
}

__global__ void __launch_bounds__(256) k_denoise_finish(const float4* __restrict__ xs, const float4* __restrict__ as, uint64_t n, uint32_t demodulate,
                                                        float albedo_floor, float* __restrict__ film) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float out[3];
    dn_finish_pixel(xs[i], as[i], demodulate != 0, albedo_floor, out);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        film[3 * i + c] = out[c];
        film[3 * n + 3 * i + c] = 0.0f;
    }
    film[6 * n + i] = 1.0f;
}

hipError_t launch_denoise_prepare(const float* color, float color_scale, const float* half, const float* albedo, float albedo_scale, const float* normal,
                                  float normal_scale, uint64_t n, uint32_t demodulate, float albedo_floor, DenoiseRecords rec, hipStream_t stream) {
    auto launch = [&](auto* kernel) {
        launch_kernel(kernel, (uint32_t)((n + 255) / 256), 0, stream, color, color_scale, half, albedo, albedo_scale, normal, normal_scale, n, demodulate, albedo_floor, rec);
    };
    if (half) launch(k_denoise_prepare<DnVariance>);
    else launch(k_denoise_prepare<DnPlain>);
    return hipGetLastError();
}
hipError_t launch_denoise_variance(const DenoiseLevel& lv, DenoiseRecords rec, hipStream_t stream) {
    const uint32_t tiles_x = (lv.width + kDnTile - 1) / kDnTile, tiles_y = (lv.height + kDnTile - 1) / kDnTile;
    launch_kernel(k_denoise_variance, tiles_x * tiles_y, 0, stream, lv, rec.x, (const float4*)rec.n, (const float4*)rec.a, tiles_x);
    return hipGetLastError();
}
hipError_t launch_denoise_level(const DenoiseLevel& lv, DenoiseRecords rec, float4* x_out, bool tiled, bool variance, hipStream_t stream) {
    uint32_t blocks, across;  // the grid, and how many tiles (tiled) or 32 x 8 blocks lie side by side
    if (tiled) {
        const uint32_t cw = (lv.width + lv.step - 1) / lv.step, ch = (lv.height + lv.step - 1) / lv.step;  // the largest class
        across = (cw + kDnTile - 1) / kDnTile;
        blocks = across * ((ch + kDnTile - 1) / kDnTile) * lv.step * lv.step;
    } else {
        across = (lv.width + 31) / 32;
        blocks = across * ((lv.height + 7) / 8);
    }
    const auto kernel = tiled ? (variance ? k_denoise_level_tiled<DnVariance> : k_denoise_level_tiled<DnPlain>)
                              : (variance ? k_denoise_level<DnVariance> : k_denoise_level<DnPlain>);
    launch_kernel(kernel, blocks, 0, stream, lv, (const float4*)rec.x, (const float4*)rec.n, (const float4*)rec.a, x_out, across);
    return hipGetLastError();
}
hipError_t launch_denoise_finish(const float4* x, const float4* a, uint64_t n, uint32_t demodulate, float albedo_floor, float* out_film, hipStream_t stream) {
    launch_kernel(k_denoise_finish, (uint32_t)((n + 255) / 256), 0, stream, x, a, n, demodulate, albedo_floor, out_film);
    return hipGetLastError();
}

}  // namespace akr
