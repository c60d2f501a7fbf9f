// pt_launch.h -- k_pt_pass, the entry point of a flattened scene's units, and the declaration of a unit's entry point. Templates and inline
// functions only: a translation unit that includes it gets the instantiations its entry point names, no others. The units (kernels.h PtKind,
// pt_unit_index) are all compiled from pt_unit_kernels.hip, once per unit (build.py PT_UNITS); the relaxed arithmetic tier
// (pt_kernels_relaxed.hip; device/dmath.h AKR_ARITH_RELAXED) compiles the plain unit's kernels a second time, with everything below in namespace
// akr_rx. Which variant a session runs is decided once (kernels.h PtVariant, host/api_pt.cpp), its LDS is laid out once (kernels.h
// pt_lds_layout), and launch_pt_pass (pt_kernels.hip) goes through the table of units to the entry point: nothing here decides either again.
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
// The entry point of unit UNIT (kernels.h pt_unit_flags). Declared here, defined and explicitly instantiated in pt_unit_kernels.hip alone: the
// router names all kPtUnits of them without compiling a kernel.
template <uint32_t UNIT>
hipError_t pt_pass_entry_unit(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream);

// The variant of a flattened scene, by name: the seven flags a unit dispatches on and the five it fixes.
constexpr PtVariant pt_flat_variant(bool bvh, bool fd, bool tex, bool pmj, bool stage, bool defer, bool simple, bool env, bool lens, bool feat, bool punct, bool ltree) {
    PtVariant v;
    v.bvh = bvh, v.fd = fd, v.tex = tex, v.pmj = pmj, v.stage = stage, v.defer = defer, v.simple = simple;
    v.env = env, v.lens = lens, v.feat = feat, v.punct = punct, v.ltree = ltree;
    return v;
}

// The precompiled k_pt_pass of a flattened scene: the dispatch over the flags a unit with fixed ENV, LENS, FEAT and PUNCT has left. What
// pt_variant_compiled rules out is not compiled, and a variant that asks for it is refused.
template <bool ENV, bool LENS, bool FEAT = false, bool PUNCT = false, bool LTREE = false>
hipError_t pt_pass_entry_t(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream) {
    if (v.inst || v.env != ENV || v.lens != LENS || v.feat != FEAT || v.punct != PUNCT || v.ltree != LTREE || !pt_variant_compiled(v)) return hipErrorInvalidValue;
    if (FEAT && (q.feat_albedo == nullptr || q.feat_normal == nullptr)) return hipErrorInvalidValue;
    if (PUNCT && (q.sc.punct == nullptr || (q.sc.n_punct & ~kPunctSoftBit) == 0)) return hipErrorInvalidValue;
    if (LTREE != (q.sc.punct_tree != 0)) return hipErrorInvalidValue;  // (a tree's entry in the light table and the kernels that walk it go together)
    dispatch_bools([&](auto B, auto F, auto T, auto P, auto S, auto D, auto X) {
        if constexpr (pt_variant_compiled(pt_flat_variant(B(), F(), T(), P(), S(), D(), X(), ENV, LENS, FEAT, PUNCT, LTREE)))
            launch_kernel<true>(k_pt_pass<B(), F(), T(), P(), S(), D(), X(), ENV, LENS, FEAT, PUNCT, LTREE>, blocks, lds, stream, q);
    }, v.bvh, v.fd, v.tex, v.pmj, v.stage, v.defer, v.simple);
    return hipGetLastError();
}
}  // namespace akr
