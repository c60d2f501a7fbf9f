// pt_lens_kernels.hip -- k_pt_pass for flattened scenes seen through a thin lens (LENS = true; device/dpath.h generate_ray_lens_from, DESIGN.md
// section 4.9), in a translation unit of their own: what kernels.h pt_variant_compiled leaves of k_pt_pass with LENS on. LENS x ENV is a full
// cross: scenes that also have an environment light run the instantiations of pt_lens_env_kernels.hip. Kept
// scenes run k_pt_pass_inst<.., LENS> (pt_inst_lens_kernels.hip), the wavefront schedule k_wf_init / k_wf_shade<.., LENS> (wf_lens_kernels.hip),
// the aov integrator k_aov<.., LENS> (aov_lens_kernels.hip).
#include "pt_launch.h"

namespace akr {

hipError_t pt_pass_entry_lens(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream) { return pt_pass_entry_t<false, true>(q, v, blocks, lds, stream); }

// ---------------------------------------------------------------------------------------------------- test hook
// the camera ray of n items: pixel (x, y), u_filter.xy, u_lens.xy -> o.xyz, d.xyz; the pinhole's function when the camera has no lens
__global__ void k_probe_camera_rays(const PtParams p, uint32_t n, const uint32_t* __restrict__ pixels, const float* __restrict__ u, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* ui = u + 4 * (size_t)i;
    vec3 o, d;
    if (p.lens_radius > 0.0f) generate_ray_lens_from(p, pixels[2 * (size_t)i], pixels[2 * (size_t)i + 1], mk2(ui[0], ui[1]), mk2(ui[2], ui[3]), o, d);
    else generate_ray_from(p, pixels[2 * (size_t)i], pixels[2 * (size_t)i + 1], mk2(ui[0], ui[1]), o, d);
    float* r = out + 6 * (size_t)i;
    r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = d.x; r[4] = d.y; r[5] = d.z;
}
hipError_t launch_probe_camera_rays(const PtParams& p, uint32_t n, const uint32_t* pixels2, const float* u4, float* out6, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_probe_camera_rays, dim3((n + 255) / 256), dim3(256), 0, stream, p, n, pixels2, u4, out6);
    return hipGetLastError();
}

}  // namespace akr
