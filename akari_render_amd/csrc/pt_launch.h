// pt_launch.h -- k_pt_pass and the entry point of a translation unit that instantiates it. Templates and inline functions only: every
// translation unit that includes it gets the instantiations its entry point names, no others. Those are pt_kernels.hip (the AKR-F32 contract:
// the default, and the verifier), pt_kernels_relaxed.hip (the relaxed arithmetic tier, device/dmath.h AKR_ARITH_RELAXED; there everything below
// lives in namespace akr_rx), pt_env_kernels.hip (ENV), pt_lens_kernels.hip / pt_lens_env_kernels.hip (LENS without / with ENV), pt_feat*_kernels.hip (FEAT, with the same four of ENV x LENS),
// pt_punct*_kernels.hip (PUNCT, the same four again), pt_punct_tree*_kernels.hip (PUNCT + LTREE, four more), and through
// pt_inst_kernel.h the three of kept scenes. Which variant a session runs is decided once (kernels.h PtVariant, host/api_pt.cpp), its LDS is
// laid out once (kernels.h pt_lds_layout), and launch_pt_pass (pt_kernels.hip) goes through a table to the unit's entry point: nothing here
// decides either again.
#pragma once
#include "device/pt_pass.h"
#include "launch.h"

namespace akr {

template <bool BVH, bool FD, bool TEX, bool PMJ, bool STAGE, bool DEFER, bool SIMPLE = false, bool ENV = false, bool LENS = false, bool FEAT = false, bool PUNCT = false, bool LTREE = false>
__global__ __launch_bounds__(256, pt_pass_min_waves(BVH, FD, TEX)) void k_pt_pass(const PtParams p) {
    pt_pass_body<BVH, FD, TEX, PMJ, STAGE, DEFER, SIMPLE ? AB_SIMPLE : 0u, false, ENV, LENS, FEAT, PUNCT, LTREE>(p);
}

// What a translation unit exposes: `q` is the parameter block with the layout's offsets filled in, `v` the session's variant with
// (v.inst, v.env, v.lens) the unit's own, `lds` the launch's dynamic LDS in bytes.
using PtPassEntry = hipError_t (*)(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream);
hipError_t pt_pass_entry_env(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream);            // pt_env_kernels.hip
hipError_t pt_pass_entry_lens(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream);           // pt_lens_kernels.hip
hipError_t pt_pass_entry_lens_env(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream);       // pt_lens_env_kernels.hip
hipError_t pt_pass_entry_feat(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream);           // pt_feat_kernels.hip
hipError_t pt_pass_entry_feat_env(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream);       // pt_feat_env_kernels.hip
hipError_t pt_pass_entry_feat_lens(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream);      // pt_feat_lens_kernels.hip
hipError_t pt_pass_entry_feat_lens_env(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream);  // pt_feat_lens_env_kernels.hip
hipError_t pt_pass_entry_punct(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream);          // pt_punct_kernels.hip
hipError_t pt_pass_entry_punct_env(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream);      // pt_punct_env_kernels.hip
hipError_t pt_pass_entry_punct_lens(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream);     // pt_punct_lens_kernels.hip
hipError_t pt_pass_entry_punct_lens_env(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream); // pt_punct_lens_env_kernels.hip
hipError_t pt_pass_entry_punct_tree(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream);          // pt_punct_tree_kernels.hip
hipError_t pt_pass_entry_punct_tree_env(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream);      // pt_punct_tree_env_kernels.hip
hipError_t pt_pass_entry_punct_tree_lens(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream);     // pt_punct_tree_lens_kernels.hip
hipError_t pt_pass_entry_punct_tree_lens_env(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream); // pt_punct_tree_lens_env_kernels.hip
hipError_t pt_pass_entry_inst(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream);           // pt_inst_kernels.hip
hipError_t pt_pass_entry_inst_env(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream);       // pt_inst_env_kernels.hip
hipError_t pt_pass_entry_inst_lens(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream);      // pt_inst_lens_kernels.hip
hipError_t pt_pass_entry_inst_lens_env(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream);  // pt_inst_lens_kernels.hip

// The precompiled k_pt_pass of a flattened scene: the dispatch over the flags a unit with fixed ENV, LENS, FEAT and PUNCT has left. What
// pt_variant_compiled rules out is not compiled, and a variant that asks for it is refused.
template <bool ENV, bool LENS, bool FEAT = false, bool PUNCT = false, bool LTREE = false>
hipError_t pt_pass_entry_t(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream) {
    if (v.inst || v.env != ENV || v.lens != LENS || v.feat != FEAT || v.punct != PUNCT || v.ltree != LTREE || !pt_variant_compiled(v)) return hipErrorInvalidValue;
    if (FEAT && (q.feat_albedo == nullptr || q.feat_normal == nullptr)) return hipErrorInvalidValue;
    if (PUNCT && (q.sc.punct == nullptr || (q.sc.n_punct & ~kPunctSoftBit) == 0)) return hipErrorInvalidValue;
    if (LTREE != (q.sc.punct_tree != 0)) return hipErrorInvalidValue;  // (a tree's entry in the light table and the kernels that walk it go together)
    dispatch_bools([&](auto B, auto F, auto T, auto P, auto S, auto D, auto X) {
        if constexpr (pt_variant_compiled(PtVariant{B(), F(), T(), P(), S(), D(), X(), false, ENV, LENS, FEAT, PUNCT, LTREE}))
            launch_kernel<true>(k_pt_pass<B(), F(), T(), P(), S(), D(), X(), ENV, LENS, FEAT, PUNCT, LTREE>, blocks, lds, stream, q);
    }, v.bvh, v.fd, v.tex, v.pmj, v.stage, v.defer, v.simple);
    return hipGetLastError();
}
}  // namespace akr
