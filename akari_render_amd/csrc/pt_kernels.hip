// pt_kernels.hip -- launch_pt_pass, the router of every pt launch (the kernels themselves: pt_unit_kernels.hip, pt_kernels_relaxed.hip), and the kernels around a
// render that belong to no unit: sampler states, film resolve, the GGX table, the shared-plane bits of a kept scene.
#include <algorithm>
#include <array>
#include <utility>
#include "pt_launch.h"

namespace akr {

// init_pcg32_buffer_with_seed's device half (sampler/mod.rs:152-158)
__global__ void k_init_pcg32(const uint64_t* __restrict__ seeds, Pcg32* __restrict__ states, uint64_t n) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) states[i] = pcg_new_seq_offset(i, seeds[i]);
}

// Film resolve: copy_to_rgba_image with hdr = true (film.rs:120-148)
__global__ void k_film_resolve(const float* __restrict__ film, uint64_t n, float splat_scale, float* __restrict__ rgb) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float w = film[6 * n + i];
    float inv = w == 0.0f ? 1.0f : w;
#pragma unroll
    for (int c = 0; c < 3; c++) rgb[3 * i + c] = film[3 * i + c] / inv + film[3 * n + 3 * i + c] * splat_scale;
}

// PreComputedTables::init "ggx_dielectric_s" (svm/surface/precompute.rs:56-94,133-145; mod.rs:1336-1356):
// one thread per table entry, 2^20 sequential samples each (the f32 running sum makes the order part of the value).
__global__ void k_ggx_dielectric_table(const uint64_t* __restrict__ seeds, float* __restrict__ table, uint32_t samples) {
    const uint32_t dim = 16;
    uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= dim * dim * dim) return;
    uint32_t tx = gid % dim, ty = (gid / dim) % dim, tz = gid / (dim * dim);
    Pcg32 rng = pcg_new_seq_offset(gid, seeds[gid]);
    float fx = clamp_f((float)tx / ((float)dim - 1.0f), 1e-4f, 0.9999f);
    float fy = clamp_f((float)ty / ((float)dim - 1.0f), 1e-4f, 0.9999f);
    float fz = clamp_f((float)tz / ((float)dim - 1.0f), 1e-4f, 0.9999f);
    float ior = ior_from_f0(sqr(sqr(fz)));
    vec2 alpha = mk2(max_f(fx * fx, 1e-4f), max_f(fx * fx, 1e-4f));
    Frame frame = frame_from_n(mk3(0, 0, 1));
    vec3 ng = mk3(0, 0, 1);
    vec3 wo = mk3(__builtin_sqrtf(1.0f - sqr(fy)), 0.0f, fy);
    float sum = 0.0f;
    for (uint32_t s = 0; s < samples; s++) {
        float u0 = pcg_next_1d(rng), u1 = pcg_next_1d(rng), u2 = pcg_next_1d(rng);
        (void)u0;
        // SurfaceClosure::sample on MicrofacetReflection{color 1, FresnelDielectric(ior), GGX(roughness)}
        vec3 lo = to_local(frame, wo), wl;
        bool valid = sample_lobe(LOBE_REFLECT, alpha, ior, lo, mk2(u1, u2), wl);
        vec3 wi = to_world(frame, wl);
        valid = valid & check_wo_wi_valid(frame.n, ng, wo, wi);
        float val = 0.0f;
        if (valid) {
            BsdfEval e{mk3(0, 0, 0), 0.0f};
            if (check_wo_wi_valid(frame.n, ng, wo, wi))
                e = eval_reflection<FR_DIELECTRIC>(mk3(1, 1, 1), ior, mk3(0, 0, 0), mk3(0, 0, 0), alpha, to_local(frame, wo), to_local(frame, wi));
            if (e.pdf > 0.0f) val = e.f.x / e.pdf;
        }
        sum += val;
    }
    table[gid] = sum / (float)samples;
}

// One thread per instance-triangle, once per scene: the bit of an odd triangle that takes its even neighbour's plane row (dinst.h
// share_plane_row) -- what the flattening compiler decides per instance-triangle and resolve_pending used to decide at every candidate.
__global__ __launch_bounds__(256) void k_inst_share_bits(const DScene sc, uint32_t* __restrict__ bits, uint32_t* __restrict__ mesh_tri_words) {
    const uint32_t n_inst = sc.in2.n_instances;
    for (uint64_t gid = (uint64_t)blockIdx.x * 256u + threadIdx.x; gid < sc.n_tris; gid += (uint64_t)gridDim.x * 256u) {
        uint32_t lo = 0, hi = n_inst;  // the instance of gid: the last one whose first id is <= gid (inst_tri_offset has n_inst + 1 entries)
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (sc.inst_tri_offset[mid] <= gid) lo = mid; else hi = mid;
        }
        const uint32_t prim = (uint32_t)gid - sc.inst_tri_offset[lo];
        uint32_t pos;
        if ((prim & 1u) && inst_pair_shares(sc, lo, prim, pos)) {
            atomicOr(&bits[gid >> 5], 1u << ((uint32_t)gid & 31u));
            atomicOr(&mesh_tri_words[16ull * pos + 15u], kMeshTriShares);  // (nothing here reads that word)
        }
    }
}

// ---------------------------------------------------------------------------------------------------- launchers
}  // namespace akr
// pt_kernels_relaxed.hip: pt_pass_entry_t<false, false> of the relaxed arithmetic tier (its PtParams is akr's, in another namespace)
extern "C" hipError_t akr_launch_pt_pass_relaxed(const void* params, const PtVariant* v, uint32_t blocks, size_t lds, hipStream_t stream);
namespace akr {
// The entry point of every unit, by unit index (kernels.h pt_unit_index). Only their declaration is visible here (pt_launch.h), so naming them
// compiles no kernel into this object; each is defined by one compilation of pt_unit_kernels.hip. kPtUnits and the units the build
// compiles (build.py PT_UNITS) go together: a unit named here that was not compiled is an undefined symbol, and the library does not load.
template <uint32_t... UNIT>
static constexpr std::array<PtPassEntry, sizeof...(UNIT)> pt_pass_entries(std::integer_sequence<uint32_t, UNIT...>) { return {{pt_pass_entry_unit<UNIT>...}}; }
static constexpr auto kPtPassEntry = pt_pass_entries(std::make_integer_sequence<uint32_t, kPtUnits>{});
hipError_t launch_pt_pass(const PtParams& p, const PtVariant& v, hipStream_t stream, hipFunction_t spec_fn, bool relaxed) {
    const uint32_t blocks = (p.n_items + 255u) / 256u;
    if (blocks == 0) return hipSuccess;
    const PtLdsLayout L = pt_lds_layout(v, pt_lds_sizes(p));
    const PtParams q = pt_params_with_layout(p, L);
    // sessions that collect guides and scenes with punctual lights: precompiled kernels on the contract, nothing else (host/api_pt.cpp
    // akr_pt_begin_features and pt_begin refuse the rest; pt_plan asks for no per-scene kernel)
    if ((v.feat || v.punct) && (spec_fn || relaxed)) return hipErrorInvalidValue;
    if (spec_fn) {  // the scene's own kernel (host/specialise.cpp) wraps the body of whatever the variant is: same parameter block, same LDS layout
        if (L.total_bytes > 64 * 1024) (void)hipFuncSetAttribute((const void*)spec_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.total_bytes);
        void* args[] = {(void*)&q};
        return hipModuleLaunchKernel(spec_fn, blocks, 1, 1, 256, 1, 1, (unsigned)L.total_bytes, stream, args, nullptr);
    }
    if (relaxed) return akr_launch_pt_pass_relaxed(&q, &v, blocks, L.total_bytes, stream);
    return kPtPassEntry[pt_unit_index(v)](q, v, blocks, L.total_bytes, stream);  // (the unit refuses a variant that is not its own, or not compiled)
}
hipError_t launch_init_pcg32(const uint64_t* seeds, void* states, uint64_t n, hipStream_t stream) {
    uint32_t blocks = (uint32_t)((n + 255) / 256);
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_init_pcg32, dim3(blocks), dim3(256), 0, stream, seeds, (Pcg32*)states, n);
    return hipGetLastError();
}
hipError_t launch_film_resolve(const float* film, uint64_t n, float splat_scale, float* rgb, hipStream_t stream) {
    uint32_t blocks = (uint32_t)((n + 255) / 256);
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_film_resolve, dim3(blocks), dim3(256), 0, stream, film, n, splat_scale, rgb);
    return hipGetLastError();
}
hipError_t launch_ggx_table(const uint64_t* seeds, float* table, uint32_t samples, hipStream_t stream) {
    hipLaunchKernelGGL(k_ggx_dielectric_table, dim3(64), dim3(64), 0, stream, seeds, table, samples);
    return hipGetLastError();
}
hipError_t launch_inst_share_bits(const DScene& sc, uint32_t* bits, uint32_t* mesh_tri_words, hipStream_t stream) {
    if (sc.n_tris == 0 || sc.in2.n_instances == 0) return hipSuccess;
    const uint64_t blocks = ((uint64_t)sc.n_tris + 255u) / 256u;
    hipLaunchKernelGGL(k_inst_share_bits, dim3((uint32_t)(blocks < (1u << 20) ? blocks : (1u << 20))), dim3(256), 0, stream, sc, bits, mesh_tri_words);
    return hipGetLastError();
}

}  // namespace akr
