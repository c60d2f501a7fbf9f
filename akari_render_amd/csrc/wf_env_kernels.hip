// wf_env_kernels.hip -- k_wf_shade of scenes with an environment light (ENV = true; device/denv.h): textures x sampler family x kept or
// flattened scene, in a translation unit of their own (wf_path.h). launch_wf_shade (wf_kernels.hip) hands such scenes here.
#include "wf_path.h"

namespace akr {

hipError_t launch_wf_shade_env(const PtParams& p, const WfBuffers& wf, uint32_t q_out, hipStream_t stream) {
    uint32_t blocks = (wf.slot_end - wf.slot_base + 255u) / 256u;
    if (blocks == 0) return hipSuccess;
    const bool tex = p.sc.tex.nodes != nullptr, pmj = p.sampler != 0;
    const bool inst = p.sc.in2.on != 0;
#define AKR_WF_SHADE_ENV(T, S, Q, L)                                                                                          \
    {                                                                                                                       \
        if (inst) hipLaunchKernelGGL((k_wf_shade<T, S, true, true>), dim3(blocks), dim3(256), L, stream, Q, wf, q_out);        \
        else hipLaunchKernelGGL((k_wf_shade<T, S, false, true>), dim3(blocks), dim3(256), L, stream, Q, wf, q_out);            \
    }
    if (tex) {
        size_t lds;
        const PtParams q = with_tex_slots(p, 0, lds);
        if (pmj) AKR_WF_SHADE_ENV(true, true, q, lds) else AKR_WF_SHADE_ENV(true, false, q, lds)
    } else {
        if (pmj) AKR_WF_SHADE_ENV(false, true, p, 0) else AKR_WF_SHADE_ENV(false, false, p, 0)
    }
#undef AKR_WF_SHADE_ENV
    return hipGetLastError();
}

}  // namespace akr
