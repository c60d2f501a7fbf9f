// pt_kernels.hip -- hand-written gfx950 kernels of the `pt` integrator. k_pt_pass: device/pt_pass.h, pt_launch.h (ENV = false, LENS = false here); launch_pt_pass, the router of every pt launch.
#include <algorithm>
#include "device/pt_pass.h"
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

// ---------------------------------------------------------------------------------------------------- probes
__global__ void k_probe_math(uint32_t n, const float* __restrict__ x, float* s, float* c, float* l) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float sv, cv;
    sincos_f(x[i], sv, cv);
    s[i] = sv;
    c[i] = cv;
    l[i] = log_f(x[i]);
}
// the rest of the contract's elementary functions for (x, y): out6 = exp_f(x), pow_f(x, y), atan2_f(y, x), sqrt_f(x), rcp_f(x), srgb_to_linear1(x)
__global__ void k_probe_math2(uint32_t n, const float* __restrict__ xy, float* __restrict__ out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = xy[2 * (size_t)i], y = xy[2 * (size_t)i + 1];
    float* o = out + 6 * (size_t)i;
    o[0] = exp_f(x);
    o[1] = pow_f(x, y);
    o[2] = atan2_f(y, x);
    o[3] = sqrt_f(x);
    o[4] = rcp_f(x);
    o[5] = srgb_to_linear1(x);
}
// a / b by the pair walk's division without range scaling (dmath.h div_f_unscaled) and by the contract's
__global__ void k_probe_div(uint32_t n, const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out_fast, float* __restrict__ out_ieee) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out_fast[i] = div_f_unscaled(a[i], b[i]);
    out_ieee[i] = div_f(a[i], b[i]);
}
// the end of a pass of the independent sampler, advance(-dim): by the closed form the kernels use (drng.h pcg_end_pass) and by the loop that defines it
__global__ void k_probe_pcg_end_pass(uint32_t n, const uint64_t* __restrict__ state, const uint64_t* __restrict__ inc, const uint32_t* __restrict__ dim,
                                     uint64_t* __restrict__ out_closed, uint64_t* __restrict__ out_loop) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Pcg32 a{state[i], inc[i]}, b = a;
    pcg_end_pass(a, dim[i]);
    pcg_advance(b, -(int64_t)dim[i]);
    out_closed[i] = a.state;
    out_loop[i] = b.state;
}
__global__ void k_probe_bsdf(const DMaterial* __restrict__ m, const float* __restrict__ table, int mode, vec3 wo, uint32_t n,
                             const float* __restrict__ in, float* __restrict__ out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ShadePoint sp;
    shade_point_init(sp, *m, frame_from_n(mk3(0, 0, 1)), mk3(0, 0, 1), false);
    if (mode == 0) {
        BsdfEval e = shade_evaluate(sp, *m, table, wo, mk3(in[3 * i], in[3 * i + 1], in[3 * i + 2]));
        out[4 * i + 0] = e.f.x;
        out[4 * i + 1] = e.f.y;
        out[4 * i + 2] = e.f.z;
        out[4 * i + 3] = e.pdf;
    } else {
        BsdfSample s = shade_sample(sp, *m, table, wo, in[3 * i], mk2(in[3 * i + 1], in[3 * i + 2]));
        float* o = out + 8 * (size_t)i;
        o[0] = s.wi.x; o[1] = s.wi.y; o[2] = s.wi.z;
        o[3] = s.color.x; o[4] = s.color.y; o[5] = s.color.z;
        o[6] = s.pdf;
        o[7] = s.valid ? 1.0f : 0.0f;
    }
}
template <bool BVH, bool INST = false>
__global__ __launch_bounds__(256) void k_probe_intersect(PtParams p, uint32_t n, const float* __restrict__ rays, uint32_t* __restrict__ out, float* __restrict__ bary) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    TraceCtx tc;
    tc.stack = lds_stack + threadIdx.x;
    tc.cnt = TraceCounters{0, 0, 0};
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool act = i < n;
    const float* r = rays + 8 * (size_t)(act ? i : 0);
    Hit h;
    bool found = INST ? trace_inst<false, false>(p.sc, mk3(r[0], r[1], r[2]), mk3(r[3], r[4], r[5]), r[6], r[7], kInvalid, kInvalid, h, tc.stack, tc.cnt)
                      : trace<BVH, false>(p, tc, mk3(r[0], r[1], r[2]), mk3(r[3], r[4], r[5]), r[6], r[7], kInvalid, kInvalid, h);
    if (!act) return;
    uint32_t inst = 0, prim = 0;
    if (found) {
        inst = INST ? inst_of_gid(p.sc, h.gid) : f2u(p.sc.shade[(size_t)h.gid * SHADE_ROWS + 6].z);
        prim = h.gid - p.sc.inst_tri_offset[inst];
    }
    out[3 * i + 0] = found ? 1u : 0u;
    out[3 * i + 1] = inst;
    out[3 * i + 2] = prim;
    bary[2 * i + 0] = found ? h.u : 0.0f;
    bary[2 * i + 1] = found ? h.v : 0.0f;
}
// trace_pair_exhaustive as pt_pass_body calls it: the records staged in LDS, one closest-hit and one shadow ray per lane (a ray with
// tmax < 0 does not exist). rays: o.xyz d.xyz tmax - | so.xyz sd.xyz stmax - (16 floats), excl: ex0 sex0 sex1 (record ids or kInvalid);
// out: found gid occluded took_ieee_walk, out_tuv: t u v of the hit
__global__ __launch_bounds__(256) void k_probe_intersect_pair(PtParams p, uint32_t n, const float* __restrict__ rays, const uint32_t* __restrict__ excl, uint32_t* __restrict__ out,
                                                              float* __restrict__ out_tuv) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    const uint32_t* g = (const uint32_t*)p.sc.woop;
    for (uint32_t i = threadIdx.x; i < (p.sc.n_tris + 2u) * 12u; i += 256u) lds_stack[i] = g[i];
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = i < n;
    const float* r = rays + 16 * (size_t)(act ? i : 0);
    const uint32_t* e = excl + 3 * (size_t)(act ? i : 0);
    Hit h;
    bool found = false, occluded = false;
    uint32_t redo = 0;
    trace_pair_exhaustive<false>(p.sc, mk3(r[0], r[1], r[2]), mk3(r[3], r[4], r[5]), act ? r[6] : -1.0f, e[0], mk3(r[8], r[9], r[10]), mk3(r[11], r[12], r[13]),
                                 act ? r[14] : -1.0f, e[1], e[2], h, found, occluded, (const float4*)lds_stack, &redo);
    if (!act) return;
    out[4 * i + 0] = found ? 1u : 0u;
    out[4 * i + 1] = h.gid;
    out[4 * i + 2] = occluded ? 1u : 0u;
    out[4 * i + 3] = redo;
    out_tuv[3 * i + 0] = h.t;
    out_tuv[3 * i + 1] = h.u;
    out_tuv[3 * i + 2] = h.v;
}
template <bool INST>
__global__ void k_probe_si(PtParams p, uint32_t n, const uint32_t* __restrict__ inst_prim, const float* __restrict__ bary, float* __restrict__ out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t gid = p.sc.inst_tri_offset[inst_prim[2 * i]] + inst_prim[2 * i + 1];
    SurfacePoint s = surface_interaction_any<INST>(p.sc, gid, mk2(bary[2 * i], bary[2 * i + 1]));
    float* o = out + 19 * (size_t)i;
    o[0] = s.p.x; o[1] = s.p.y; o[2] = s.p.z;
    o[3] = s.ng.x; o[4] = s.ng.y; o[5] = s.ng.z;
    o[6] = s.frame.n.x; o[7] = s.frame.n.y; o[8] = s.frame.n.z;
    o[9] = s.frame.t.x; o[10] = s.frame.t.y; o[11] = s.frame.t.z;
    o[12] = s.frame.s.x; o[13] = s.frame.s.y; o[14] = s.frame.s.z;
    o[15] = s.uv.x;  // uv = interp(uv0, uv1, uv2)
    o[16] = s.uv.y;
    o[17] = s.prim_area;
    o[18] = (float)s.material;
}

// evaluated inputs (26 words = akr_material_desc) of `material` at n uv points
__global__ void k_probe_material(PtParams p, uint32_t material, uint32_t n, const float* __restrict__ uv, uint32_t* __restrict__ out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DMaterial& m = p.sc.materials[material];
    MatInputs in = p.sc.tex.mat_inputs[material];
    if (m.flags & MF_TEXTURED) {
        eval_material_graph(p.sc.tex, m.tex_first_node, m.tex_n_nodes & kTexCountMask, mk2(uv[2 * i], uv[2 * i + 1]), in);
    }
    const uint32_t* w = reinterpret_cast<const uint32_t*>(&in);
    for (uint32_t k = 0; k < 26; k++) out[26 * (size_t)i + k] = w[k];
}

// ---------------------------------------------------------------------------------------------------- launchers
}  // namespace akr
// pt_kernels_relaxed.hip: pt_pass_entry_t<false, false> of the relaxed arithmetic tier (its PtParams is akr's, in another namespace)
extern "C" hipError_t akr_launch_pt_pass_relaxed(const void* params, const PtVariant* v, uint32_t blocks, size_t lds, hipStream_t stream);
namespace akr {
static hipError_t pt_pass_entry_plain(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream) { return pt_pass_entry_t<false, false>(q, v, blocks, lds, stream); }
// the translation unit that holds the kernels of a variant, by [inst][env][lens]; those that collect the denoiser's guides by [env][lens]
static constexpr PtPassEntry kPtPassEntry[2][2][2] = {{{pt_pass_entry_plain, pt_pass_entry_lens}, {pt_pass_entry_env, pt_pass_entry_lens_env}},
                                                      {{pt_pass_entry_inst, pt_pass_entry_inst_lens}, {pt_pass_entry_inst_env, pt_pass_entry_inst_lens_env}}};
static constexpr PtPassEntry kPtPassEntryFeat[2][2] = {{pt_pass_entry_feat, pt_pass_entry_feat_lens}, {pt_pass_entry_feat_env, pt_pass_entry_feat_lens_env}};
// ... those of scenes with punctual lights likewise
static constexpr PtPassEntry kPtPassEntryPunct[2][2] = {{pt_pass_entry_punct, pt_pass_entry_punct_lens}, {pt_pass_entry_punct_env, pt_pass_entry_punct_lens_env}};
// ... and of those with a light tree
static constexpr PtPassEntry kPtPassEntryPunctTree[2][2] = {{pt_pass_entry_punct_tree, pt_pass_entry_punct_tree_lens}, {pt_pass_entry_punct_tree_env, pt_pass_entry_punct_tree_lens_env}};
hipError_t launch_pt_pass(const PtParams& p, const PtVariant& v, hipStream_t stream, hipFunction_t spec_fn, bool relaxed) {
    const uint32_t blocks = (p.n_items + 255u) / 256u;
    if (blocks == 0) return hipSuccess;
    const PtLdsLayout L = pt_lds_layout(v, pt_lds_sizes(p));
    const PtParams q = pt_params_with_layout(p, L);
    if (v.feat) {  // precompiled kernels of flattened scenes on the contract, nothing else (host/api_pt.cpp akr_pt_begin_features refuses the rest)
        if (spec_fn || relaxed || v.inst) return hipErrorInvalidValue;
        return kPtPassEntryFeat[v.env][v.lens](q, v, blocks, L.total_bytes, stream);
    }
    if (v.punct) {  // precompiled kernels of flattened scenes on the contract, nothing else (host/api_pt.cpp pt_begin refuses the rest; pt_plan asks for no per-scene kernel)
        if (spec_fn || relaxed || v.inst) return hipErrorInvalidValue;
        return (v.ltree ? kPtPassEntryPunctTree : kPtPassEntryPunct)[v.env][v.lens](q, v, blocks, L.total_bytes, stream);
    }
    if (spec_fn) {  // the scene's own kernel (host/specialise.cpp) wraps the body of whatever the variant is: same parameter block, same LDS layout
        if (L.total_bytes > 64 * 1024) (void)hipFuncSetAttribute((const void*)spec_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.total_bytes);
        void* args[] = {(void*)&q};
        return hipModuleLaunchKernel(spec_fn, blocks, 1, 1, 256, 1, 1, (unsigned)L.total_bytes, stream, args, nullptr);
    }
    if (relaxed) return akr_launch_pt_pass_relaxed(&q, &v, blocks, L.total_bytes, stream);
    return kPtPassEntry[v.inst][v.env][v.lens](q, v, blocks, L.total_bytes, stream);
}
hipError_t launch_probe_material(const PtParams& p, uint32_t material, uint32_t n, const float* uv, uint32_t* out, hipStream_t stream) {
    size_t lds;
    const PtParams q = with_tex_slots(p, 0, lds);
    hipLaunchKernelGGL(k_probe_material, dim3((n + 127) / 128), dim3(128), lds, stream, q, material, n, uv, out);
    return hipGetLastError();
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
hipError_t launch_probe_math(uint32_t n, const float* x, float* s, float* c, float* l, hipStream_t stream) {
    hipLaunchKernelGGL(k_probe_math, dim3((n + 255) / 256), dim3(256), 0, stream, n, x, s, c, l);
    return hipGetLastError();
}
hipError_t launch_probe_math2(uint32_t n, const float* xy, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(k_probe_math2, dim3((n + 255) / 256), dim3(256), 0, stream, n, xy, out);
    return hipGetLastError();
}
hipError_t launch_probe_div(uint32_t n, const float* a, const float* b, float* out_fast, float* out_ieee, hipStream_t stream) {
    hipLaunchKernelGGL(k_probe_div, dim3((n + 255) / 256), dim3(256), 0, stream, n, a, b, out_fast, out_ieee);
    return hipGetLastError();
}
hipError_t launch_probe_pcg_end_pass(uint32_t n, const uint64_t* state, const uint64_t* inc, const uint32_t* dim, uint64_t* out_closed, uint64_t* out_loop, hipStream_t stream) {
    hipLaunchKernelGGL(k_probe_pcg_end_pass, dim3((n + 255) / 256), dim3(256), 0, stream, n, state, inc, dim, out_closed, out_loop);
    return hipGetLastError();
}
hipError_t launch_probe_intersect_pair(const PtParams& p, uint32_t n, const float* rays, const uint32_t* excl, uint32_t* out, float* out_tuv, hipStream_t stream) {
    launch_kernel(k_probe_intersect_pair, (n + 255) / 256, (p.sc.n_tris + 2u) * 48u, stream, p, n, rays, excl, out, out_tuv);
    return hipGetLastError();
}
hipError_t launch_probe_bsdf(const DMaterial* m, const float* table, int mode, const float* wo, uint32_t n, const float* in, float* out,
                             hipStream_t stream) {
    hipLaunchKernelGGL(k_probe_bsdf, dim3((n + 255) / 256), dim3(256), 0, stream, m, table, mode, mk3(wo[0], wo[1], wo[2]), n, in, out);
    return hipGetLastError();
}
hipError_t launch_probe_intersect(const PtParams& p, uint32_t n, const float* rays, uint32_t* out, float* bary, hipStream_t stream) {
    const bool bvh = p.sc.bvh_nodes != nullptr, inst = p.sc.in2.on != 0;  // (a kept scene: the two-level traversal, whatever bvh_nodes says)
    dispatch_bools([&](auto B, auto I) {
        launch_kernel(k_probe_intersect<B() || I(), I()>, (n + 255) / 256, B() || I() ? p.sc.bvh_stack_depth * 256 * 4 : 0, stream, p, n, rays, out, bary);
    }, bvh, inst);
    return hipGetLastError();
}
hipError_t launch_probe_si(const PtParams& p, uint32_t n, const uint32_t* inst_prim, const float* bary, float* out, hipStream_t stream) {
    dispatch_bools([&](auto I) { launch_kernel(k_probe_si<I()>, (n + 255) / 256, 0, stream, p, n, inst_prim, bary, out); }, p.sc.in2.on != 0);
    return hipGetLastError();
}

}  // namespace akr
