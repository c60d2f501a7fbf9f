// probe_kernels.hip -- the device probes (include/akari_hip_test.h: host/api_probe.cpp): kernels that run one device function of the pt kernels over n
// inputs, and their launchers. None of them is part of a render.
#include "device/pt_pass.h"
#include "launch.h"

namespace akr {

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
hipError_t launch_probe_material(const PtParams& p, uint32_t material, uint32_t n, const float* uv, uint32_t* out, hipStream_t stream) {
    size_t lds;
    const PtParams q = with_tex_slots(p, 0, lds);
    hipLaunchKernelGGL(k_probe_material, dim3((n + 127) / 128), dim3(128), lds, stream, q, material, n, uv, out);
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

// ---------------------------------------------------------------------------------------------------- environment light (device/denv.h)
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

// ---------------------------------------------------------------------------------------------------- camera (device/dpath.h)
// the camera ray of n items: pixel (x, y), u_filter.xy, u_lens.xy -> o.xyz, d.xyz; the pinhole's function when the camera has no lens
__global__ void k_probe_camera_rays(const PtParams p, uint32_t n, const uint32_t* __restrict__ pixels, const float* __restrict__ u, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* ui = u + 4 * (size_t)i;
    vec3 o, d;
    if (camera_runs_lens_kernels(p.lens_radius, p.projection)) generate_ray_lens_from(p, pixels[2 * (size_t)i], pixels[2 * (size_t)i + 1], mk2(ui[0], ui[1]), mk2(ui[2], ui[3]), o, d);
    else generate_ray_from(p, pixels[2 * (size_t)i], pixels[2 * (size_t)i + 1], mk2(ui[0], ui[1]), o, d);
    float* r = out + 6 * (size_t)i;
    r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = d.x; r[4] = d.y; r[5] = d.z;
}
hipError_t launch_probe_camera_rays(const PtParams& p, uint32_t n, const uint32_t* pixels2, const float* u4, float* out6, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_probe_camera_rays, dim3((n + 255) / 256), dim3(256), 0, stream, p, n, pixels2, u4, out6);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------- punctual lights (device/dpunct.h, device/dlighttree.h)
__global__ void k_probe_light_sample(const AliasPacked* __restrict__ light_alias, const LightRec* __restrict__ lights, const DPunct* __restrict__ punct, uint32_t n_lights, uint32_t n,
                                     const float* __restrict__ rows9, float* __restrict__ out13, uint32_t* __restrict__ light) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    punct_probe_row(light_alias, lights, punct, n_lights, rows9 + 9 * (size_t)i, out13 + 13 * (size_t)i, light + i);
}
hipError_t launch_probe_light_sample(const PtParams& p, uint32_t n, const float* rows9, float* out13, uint32_t* light, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_probe_light_sample, dim3((n + 255) / 256), dim3(256), 0, stream, p.sc.light_alias, p.sc.lights, p.sc.punct, p.sc.n_lights, n, rows9, out13, light);
    return hipGetLastError();
}

__global__ void k_probe_light_tree_sample(const AliasPacked* __restrict__ light_alias, const LightRec* __restrict__ lights, const DPunct* __restrict__ punct, uint32_t punct_tree,
                                          uint32_t n_lights, uint32_t n, const float* __restrict__ rows9, float* __restrict__ out13, uint32_t* __restrict__ light,
                                          uint32_t* __restrict__ record) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    light_tree_probe_row(light_alias, lights, punct, punct_tree, n_lights, rows9 + 9 * (size_t)i, out13 + 13 * (size_t)i, light + i, record + i);
}
hipError_t launch_probe_light_tree_sample(const PtParams& p, uint32_t n, const float* rows9, float* out13, uint32_t* light, uint32_t* record, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_probe_light_tree_sample, dim3((n + 255) / 256), dim3(256), 0, stream, p.sc.light_alias, p.sc.lights, p.sc.punct, p.sc.punct_tree, p.sc.n_lights, n, rows9, out13,
                       light, record);
    return hipGetLastError();
}

}  // namespace akr
