// cost_order_kernels.hip -- the item -> pixel table of a pt session that orders its work items by measured pixel cost
// (DESIGN.md section 4.1). A pixel's samples are sequential and what a pixel costs depends on what it sees; items dealt by position put
// cheap and dear pixels into one wave, which waits for its dearest. The session's first launch records every item's closest-hit rays
// (pt_pass.h, PtParams.item_cost); here its items are sorted by that count, dearest first, so that the 64 lanes of a wave and the
// four waves of a workgroup hold pixels of near-equal cost and the workgroups are dispatched longest first. Once per session, on its stream.
#include <hip/hip_runtime.h>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>

#include "device/dpath.h"

namespace akr {

// One 64-bit key per item: ~cost in the high word, the pixel in the low one, so that ONE ascending sort gives descending cost with ties in
// ascending pixel order, whatever order the items enumerate the pixels in. An item without a pixel (out of frame, padding) is all ones:
// it sorts behind every pixel and its low word is kInvalid.
__global__ __launch_bounds__(256) void k_cost_order_keys(const PtParams p, uint32_t n_padded, uint64_t* __restrict__ keys) {
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    if (item >= n_padded) return;
    uint32_t px = 0, py = 0;
    uint64_t key = ~0ull;
    if (item < p.n_items && item_to_pixel(p, item, px, py)) {
        const uint32_t pix = px + py * p.width;
        key = ((uint64_t)(~p.item_cost[item]) << 32) | pix;
    }
    keys[item] = key;
}
__global__ __launch_bounds__(256) void k_cost_order_table(const uint64_t* __restrict__ keys, uint32_t n_padded, uint32_t* __restrict__ table) {
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    if (item < n_padded) table[item] = (uint32_t)keys[item];
}

// test hook: the costs of p's items (dealt by position) as a map over the frame's pixels; pixels without an item keep what they hold
__global__ __launch_bounds__(256) void k_cost_to_pixels(const PtParams p, const uint32_t* __restrict__ item_cost, uint32_t* __restrict__ pixel_cost) {
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    uint32_t px = 0, py = 0;
    if (item < p.n_items && item_to_pixel(p, item, px, py)) pixel_cost[px + py * p.width] = item_cost[item];
}
hipError_t launch_cost_to_pixels(const PtParams& p, const uint32_t* item_cost, uint32_t* pixel_cost, hipStream_t stream) {
    const uint32_t blocks = (p.n_items + 255u) / 256u;
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_cost_to_pixels, dim3(blocks), dim3(256), 0, stream, p, item_cost, pixel_cost);
    return hipGetLastError();
}

size_t cost_order_temp_bytes(uint32_t n_padded) {
    size_t bytes = 0;
    (void)rocprim::radix_sort_keys(nullptr, bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)n_padded, 0u, 64u, (hipStream_t) nullptr);
    return bytes;
}
hipError_t launch_cost_order(const PtParams& p, uint32_t n_padded, uint64_t* keys, uint64_t* keys_sorted, void* temp, size_t temp_bytes, uint32_t* table, hipStream_t stream) {
    if (n_padded == 0) return hipSuccess;
    if (p.item_cost == nullptr || (n_padded & 255u) != 0 || n_padded < p.n_items) return hipErrorInvalidValue;
    const uint32_t blocks = n_padded / 256u;
    hipLaunchKernelGGL(k_cost_order_keys, dim3(blocks), dim3(256), 0, stream, p, n_padded, keys);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rocprim::radix_sort_keys(temp, temp_bytes, (const uint64_t*)keys, keys_sorted, (size_t)n_padded, 0u, 64u, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cost_order_table, dim3(blocks), dim3(256), 0, stream, (const uint64_t*)keys_sorted, n_padded, table);
    return hipGetLastError();
}

}  // namespace akr
