// pt_inst_kernel.h -- k_pt_pass_inst, the persistent-lane path tracer over a scene kept as meshes + instances, and the entry point of a
// translation unit that instantiates it. A header so that the instantiations of scenes with an environment light (pt_inst_env_kernels.hip,
// ENV = true) are compiled in a translation unit of their own: those of pt_inst_kernels.hip (ENV = false), and their code, are the ones of a
// library without environments. The same for cameras with a thin lens (LENS = true, with and without an environment: pt_inst_lens_kernels.hip).
#pragma once
#include "pt_launch.h"

#ifndef AKR_PT_MIN_WAVES_INST
#define AKR_PT_MIN_WAVES_INST AKR_PT_MIN_WAVES_BVH
#endif
#ifndef AKR_PT_MIN_WAVES_INST_TEX
#define AKR_PT_MIN_WAVES_INST_TEX AKR_PT_MIN_WAVES_BVH_TEX
#endif

namespace akr {

template <bool FD, bool TEX, bool PMJ, bool ENV = false, bool LENS = false>
__global__ __launch_bounds__(256, TEX ? AKR_PT_MIN_WAVES_INST_TEX : AKR_PT_MIN_WAVES_INST) void k_pt_pass_inst(const PtParams p) {
    pt_pass_body<true, FD, TEX, PMJ, false, false, 0u, true, ENV, LENS>(p);
}

// force_diffuse x textures x sampler family: what a kept scene's variant has left (kernels.h pt_variant_compiled)
template <bool ENV, bool LENS>
hipError_t pt_pass_entry_inst_t(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream) {
    if (!v.inst || v.env != ENV || v.lens != LENS || !pt_variant_compiled(v)) return hipErrorInvalidValue;
    dispatch_bools([&](auto F, auto T, auto P) { launch_kernel<true>(k_pt_pass_inst<F(), T(), P(), ENV, LENS>, blocks, lds, stream, q); }, v.fd, v.tex, v.pmj);
    return hipGetLastError();
}

}  // namespace akr
