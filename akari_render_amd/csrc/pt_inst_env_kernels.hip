// pt_inst_env_kernels.hip -- k_pt_pass_inst of kept scenes with an environment light (ENV = true; device/denv.h): force_diffuse x textures x
// sampler family, in a translation unit of their own (pt_inst_kernel.h). launch_pt_pass_inst (pt_inst_kernels.hip) hands such scenes here.
#include "pt_inst_kernel.h"

namespace akr {

hipError_t launch_pt_pass_inst_env(const PtParams& p, hipStream_t stream) {
    size_t lds;
    uint32_t blocks;
    const PtParams q = pt_pass_layout(p, lds, blocks);
    if (blocks == 0) return hipSuccess;
    const bool fd = p.force_diffuse != 0, tex = p.sc.tex.nodes != nullptr, pmj = p.sampler != 0;
#define AKR_LAUNCH_INST_ENV(F, T, S)                                                                                                      \
    {                                                                                                                                   \
        if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)(k_pt_pass_inst<F, T, S, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        hipLaunchKernelGGL((k_pt_pass_inst<F, T, S, true>), dim3(blocks), dim3(256), lds, stream, q);                                      \
    }
    if (fd) {
        if (tex) { if (pmj) AKR_LAUNCH_INST_ENV(true, true, true) else AKR_LAUNCH_INST_ENV(true, true, false) }
        else { if (pmj) AKR_LAUNCH_INST_ENV(true, false, true) else AKR_LAUNCH_INST_ENV(true, false, false) }
    } else {
        if (tex) { if (pmj) AKR_LAUNCH_INST_ENV(false, true, true) else AKR_LAUNCH_INST_ENV(false, true, false) }
        else { if (pmj) AKR_LAUNCH_INST_ENV(false, false, true) else AKR_LAUNCH_INST_ENV(false, false, false) }
    }
#undef AKR_LAUNCH_INST_ENV
    return hipGetLastError();
}

}  // namespace akr
