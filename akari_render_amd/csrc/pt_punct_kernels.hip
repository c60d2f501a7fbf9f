// pt_punct_kernels.hip -- k_pt_pass for flattened scenes with punctual lights (PUNCT = true: device/dpunct.h) without an environment light or a lens,
// in a translation unit of their own: what kernels.h pt_variant_compiled leaves of k_pt_pass with PUNCT on.
#include "pt_launch.h"

namespace akr {

hipError_t pt_pass_entry_punct(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream) { return pt_pass_entry_t<false, false, false, true>(q, v, blocks, lds, stream); }

// ---------------------------------------------------------------------------------------------------- test hook
__global__ void k_probe_light_sample(const AliasPacked* __restrict__ light_alias, const LightRec* __restrict__ lights, const DPunct* __restrict__ punct, uint32_t n_lights, uint32_t n,
                                     const float* __restrict__ rows9, float* __restrict__ out13, uint32_t* __restrict__ light) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    punct_probe_row(light_alias, lights, punct, n_lights, rows9 + 9 * (size_t)i, out13 + 13 * (size_t)i, light + i);
}
hipError_t launch_probe_light_sample(const PtParams& p, uint32_t n, const float* rows9, float* out13, uint32_t* light, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_probe_light_sample, dim3((n + 255) / 256), dim3(256), 0, stream, p.sc.light_alias, p.sc.lights, p.sc.punct, p.sc.n_lights, n, rows9, out13, light);
    return hipGetLastError();
}

__global__ void k_probe_light_tree_sample(const AliasPacked* __restrict__ light_alias, const LightRec* __restrict__ lights, const DPunct* __restrict__ punct, uint32_t punct_tree,
                                          uint32_t n_lights, uint32_t n, const float* __restrict__ rows9, float* __restrict__ out13, uint32_t* __restrict__ light,
                                          uint32_t* __restrict__ record) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    light_tree_probe_row(light_alias, lights, punct, punct_tree, n_lights, rows9 + 9 * (size_t)i, out13 + 13 * (size_t)i, light + i, record + i);
}
hipError_t launch_probe_light_tree_sample(const PtParams& p, uint32_t n, const float* rows9, float* out13, uint32_t* light, uint32_t* record, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_probe_light_tree_sample, dim3((n + 255) / 256), dim3(256), 0, stream, p.sc.light_alias, p.sc.lights, p.sc.punct, p.sc.punct_tree, p.sc.n_lights, n, rows9, out13,
                       light, record);
    return hipGetLastError();
}

}  // namespace akr
