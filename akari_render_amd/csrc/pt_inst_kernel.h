// pt_inst_kernel.h -- k_pt_pass_inst, the persistent-lane path tracer over a scene kept as meshes + instances (host/scene_inst.cpp; the two-level
// traversal of device/dinst_trav.h), and the entry point of a unit that instantiates it: the four units of kind PT_KIND_INST, one per ENV x LENS
// (kernels.h; pt_unit_kernels.hip).
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
