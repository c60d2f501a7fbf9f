// pt_launch.h -- k_pt_pass, the LDS plan of its launches and the launcher that picks the instantiation. Templates and inline functions
// only: every translation unit that instantiates the kernel includes it and gets the instantiations its launcher names, no others.
// Those are pt_kernels.hip (the AKR-F32 contract: the default, and the verifier), pt_kernels_relaxed.hip (the relaxed arithmetic tier,
// device/dmath.h AKR_ARITH_RELAXED; there everything below lives in namespace akr_rx), pt_env_kernels.hip (ENV = true: scenes with an
// environment light) and pt_lens_kernels.hip / pt_lens_env_kernels.hip (LENS = true: cameras with a thin lens, without / with an environment).
// The kept-scene launchers (pt_inst_kernel.h) share the LDS plan.
#pragma once
#include <algorithm>
#include "device/pt_pass.h"
#include "launch.h"

namespace akr {

template <bool BVH, bool FD, bool TEX, bool PMJ, bool STAGE, bool DEFER, bool SIMPLE = false, bool ENV = false, bool LENS = false>
__global__ __launch_bounds__(256, pt_pass_min_waves(BVH, FD, TEX)) void k_pt_pass(const PtParams p) {
    pt_pass_body<BVH, FD, TEX, PMJ, STAGE, DEFER, SIMPLE ? AB_SIMPLE : 0u, false, ENV, LENS>(p);
}

// Dynamic LDS of a k_pt_pass launch and where its blocks start: [traversal stacks][staged tables][triangle records (exhaustive kernels)][node
// tile][park columns][carry columns][blue-noise columns (pmj02bn)][graph values]. Shared by the precompiled kernels, the per-scene
// kernels and the instanced-scene kernels (pt_inst_kernel.h).
inline PtParams pt_pass_layout(const PtParams& p, size_t& lds, uint32_t& blocks) {
    blocks = (p.n_items + 255u) / 256u;
    const bool fd = p.force_diffuse != 0, tex = p.sc.tex.nodes != nullptr;
    const bool bvh = p.sc.bvh_nodes != nullptr, inst = p.sc.in2.on != 0;
    const PtLdsPlan plan = pt_lds_plan(bvh, fd, tex, p.defer_metal != 0, p.sc.n_tris);
    size_t base = (bvh ? p.sc.bvh_stack_depth * 256 * 4 : 0) + p.stage_total + plan.recs_bytes;
    base = (base + 15) & ~(size_t)15;
    PtParams pp = p;
    pp.tile_offset = (uint32_t)(base / 4);
    pp.sc.bvh_tile_nodes = 0;
    if (plan.tile && !inst) {
        // what is left of the workgroup's share of the CU's LDS after the launch's other blocks
        const size_t other = base + plan.park_bytes + plan.carry_bytes + (tex ? (size_t)p.tex_slots * kTexValStride * sizeof(TexVal) : 0);
        const size_t budget = pt_lds_budget(tex) - 256;
        if (other < budget) pp.sc.bvh_tile_nodes = (uint32_t)std::min<size_t>({(budget - other) / (kBvhNodeWords * 4), (size_t)p.sc.n_nodes, (size_t)1024});
        base += (size_t)pp.sc.bvh_tile_nodes * kBvhNodeWords * 4;
        base = (base + 15) & ~(size_t)15;
    }
    pp.park_offset = (uint32_t)(base / 4);
    base += plan.park_bytes;
    pp.carry_offset = (uint32_t)(base / 4);
    base += inst ? (AKR_PT_STRAGGLERS_INST > 0 ? (size_t)kCarrySlotsInstanced * 256 * 4 : 0) : plan.carry_bytes;
    pp.bn_offset = 0;
    {   // pmj02bn: the lanes' blue-noise columns, if the workgroup's share of the CU's LDS has room for them (exhaustive kernels of
        // small scenes: 24 KB next to ~13 KB of staged tables; the BVH kernels' traversal stacks leave none)
        const size_t slots = tex ? (size_t)p.tex_slots * kTexValStride * sizeof(TexVal) : 0;
        if (p.sampler == 1u && !bvh && p.bluenoise != nullptr && base + slots + kBlueNoiseColumnBytes <= pt_lds_budget(tex)) {
            base = (base + 15) & ~(size_t)15;
            pp.bn_offset = (uint32_t)(base / 4);
            base += kBlueNoiseColumnBytes;
        }
    }
    return with_tex_slots(pp, base, lds);
}
// The precompiled k_pt_pass of a flattened scene, or the session's per-scene kernel. ENV: the scene has an environment light (device/denv.h);
// LENS: the camera has a thin lens (device/dpath.h generate_ray). launch_pt_pass (pt_kernels.hip), launch_pt_pass_env (pt_env_kernels.hip) and the two
// of launch_pt_pass_lens (pt_lens_kernels.hip, pt_lens_env_kernels.hip) are the instantiations, each in its own translation unit.
template <bool ENV, bool LENS = false>
hipError_t launch_pt_pass_t(const PtParams& p, hipStream_t stream, hipFunction_t spec_fn = nullptr) {
    size_t lds;
    uint32_t blocks;
    const PtParams q = pt_pass_layout(p, lds, blocks);
    if (blocks == 0) return hipSuccess;
    if (spec_fn) {  // the scene's own kernel (host/specialise.cpp): same parameter block, same LDS layout (p.tex_slots is 0: no value slots)
        if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)spec_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        void* args[] = {(void*)&q};
        return hipModuleLaunchKernel(spec_fn, blocks, 1, 1, 256, 1, 1, (unsigned)lds, stream, args, nullptr);
    }
    const bool bvh = p.sc.bvh_nodes != nullptr, fd = p.force_diffuse != 0, tex = p.sc.tex.nodes != nullptr, pmj = p.sampler != 0;
    if (ENV && !bvh && p.stage_total == 0) return hipErrorInvalidValue;  // (the exhaustive kernels read their tables from LDS: the host guarantees the fit)
    const bool stage = !bvh || p.stage_total != 0;  // staged tables: the exhaustive kernels always, the BVH kernels where they fit
    // deferred metal vertices: full-graph kernels, of BVH scenes those with textures; the absent-lobe masks of SIMPLE: full-graph kernels
    // of scenes without textures; neither where there is an environment light or a lens
    const bool defer = !ENV && !LENS && p.defer_metal != 0 && !fd && (!bvh || tex);
    const bool simple = !ENV && !LENS && p.simple_scene != 0 && !fd && !tex;
    dispatch_bools([&](auto B, auto F, auto T, auto P, auto S, auto D, auto X) {
        // (what the rules above cannot produce is not compiled)
        if constexpr ((B() || S()) && !(D() && (F() || (B() && !T()))) && !(X() && (F() || T())) && !((ENV || LENS) && (D() || X())))
            launch_kernel<true>(k_pt_pass<B(), F(), T(), P(), S(), D(), X(), ENV, LENS>, blocks, lds, stream, q);
    }, bvh, fd, tex, pmj, stage, defer, simple);
    return hipGetLastError();
}
}  // namespace akr
