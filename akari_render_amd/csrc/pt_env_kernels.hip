// pt_env_kernels.hip -- k_pt_pass for flattened scenes with an environment light (device/denv.h; ENV = true), in a translation unit of
// their own so that the library's build compiles them beside pt_kernels.hip: what kernels.h pt_variant_compiled leaves of k_pt_pass with ENV on.
// Kept scenes run k_pt_pass_inst<.., ENV> (pt_inst_env_kernels.hip), the wavefront schedule k_wf_shade<.., ENV> (wf_env_kernels.hip).
#include "pt_launch.h"

namespace akr {

hipError_t pt_pass_entry_env(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream) { return pt_pass_entry_t<true, false>(q, v, blocks, lds, stream); }

// ---------------------------------------------------------------------------------------------------- test hook
// mode 0: in = u (2 floats / item) -> out = wi.xyz, pdf, valid (5 floats); mode 1: in = direction (3 floats) -> out = pdf, radiance.rgb (4 floats)
__global__ void k_probe_env(const DEnv* __restrict__ env_p, uint32_t color, uint32_t mode, uint32_t n, const float* __restrict__ in, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DEnv& env = *env_p;
    if (mode == 0) {
        vec3 wi;
        float pdf;
        const bool ok = env_sample(env, mk2(in[2 * (size_t)i], in[2 * (size_t)i + 1]), wi, pdf);
        float* o = out + 5 * (size_t)i;
        o[0] = wi.x; o[1] = wi.y; o[2] = wi.z; o[3] = pdf; o[4] = ok ? 1.0f : 0.0f;
    } else {
        const vec3 d = mk3(in[3 * (size_t)i], in[3 * (size_t)i + 1], in[3 * (size_t)i + 2]);
        const vec3 le = env_eval(env, color, d);
        float* o = out + 4 * (size_t)i;
        o[0] = env_pdf(env, d); o[1] = le.x; o[2] = le.y; o[3] = le.z;
    }
}
hipError_t launch_probe_env(const PtParams& p, uint32_t mode, uint32_t n, const float* in, float* out, hipStream_t stream) {
    if (!p.sc.env || mode > 1) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_probe_env, dim3((n + 255) / 256), dim3(256), 0, stream, p.sc.env, p.color, mode, n, in, out);
    return hipGetLastError();
}

}  // namespace akr
