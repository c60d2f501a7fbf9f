// wf_path.h -- the path half of the wavefront schedule (wf_kernels.hip): the path state's records in HBM, the ray queues, k_wf_init,
// k_wf_shade and its launcher. A header so that the shade kernels of scenes with an environment light (wf_env_kernels.hip, ENV = true) are
// compiled in a translation unit of their own: the instantiations of wf_kernels.hip (ENV = false) and their code are those of a library
// without environments. The same for cameras with a thin lens (LENS = true: k_wf_init and k_wf_shade, wf_lens_kernels.hip).
#pragma once
#include <algorithm>
#include "device/dpath.h"
#include "launch.h"

namespace akr {

enum : uint32_t {
    WF_ACTIVE = 1u, WF_HAS_RAY = 2u, WF_HAS_SHADOW = 4u, WF_S_ADD = 8u, WF_S_DEPTH1 = 16u, WF_FINALIZE = 32u, WF_LANE_DONE = 64u
};

AKR_D void wf_store(const WfBuffers& wf, uint32_t slot, const PathRegs& r) {
    wf.ray_o[slot] = make_float4(r.ro.x, r.ro.y, r.ro.z, u2f(r.ray_ex0));
    wf.ray_d[slot] = make_float4(r.rd.x, r.rd.y, r.rd.z, 0.0f);
    wf.sh_o[slot] = make_float4(r.s_o.x, r.s_o.y, r.s_o.z, u2f(r.s_ex0));
    wf.sh_d[slot] = make_float4(r.s_d.x, r.s_d.y, r.s_d.z, r.s_tmax);
    wf.sh_c[slot] = make_float4(r.s_contrib.x, r.s_contrib.y, r.s_contrib.z, u2f(r.s_ex1));
    wf.beta[slot] = make_float4(r.beta.x, r.beta.y, r.beta.z, r.prev_bsdf_pdf);
    wf.rad[slot] = make_float4(r.radiance.x, r.radiance.y, r.radiance.z, u2f(r.depth));
    uint32_t fl = (r.active ? WF_ACTIVE : 0u) | (r.has_ray ? WF_HAS_RAY : 0u) | (r.has_shadow ? WF_HAS_SHADOW : 0u) |
                  (r.s_add ? WF_S_ADD : 0u) | (r.s_depth1 ? WF_S_DEPTH1 : 0u) | (r.finalize ? WF_FINALIZE : 0u) |
                  (r.lane_done ? WF_LANE_DONE : 0u);
    wf.base[slot] = make_float4(r.base.x, r.base.y, r.base.z, u2f(fl));
    wf.film[slot] = make_float4(r.film_rgb.x, r.film_rgb.y, r.film_rgb.z, r.film_w);
    wf.rng[slot] = make_uint4((uint32_t)r.smp.pcg.state, (uint32_t)(r.smp.pcg.state >> 32), r.smp.dim, r.samples_done);
    wf.misc[slot] = make_uint4(r.pass_idx, r.cur_spp, (uint32_t)r.smp.pcg.inc, (uint32_t)(r.smp.pcg.inc >> 32));
}
AKR_D void wf_load(const WfBuffers& wf, uint32_t slot, PathRegs& r) {
    float4 a = wf.ray_o[slot], b = wf.ray_d[slot], c = wf.sh_o[slot], d = wf.sh_d[slot], e = wf.sh_c[slot];
    float4 f = wf.beta[slot], g = wf.rad[slot], h = wf.base[slot], fm = wf.film[slot];
    uint4 rg = wf.rng[slot], ms = wf.misc[slot];
    r.ro = xyz(a); r.ray_ex0 = f2u(a.w);
    r.rd = xyz(b);
    r.s_o = xyz(c); r.s_ex0 = f2u(c.w);
    r.s_d = xyz(d); r.s_tmax = d.w;
    r.s_contrib = xyz(e); r.s_ex1 = f2u(e.w);
    r.beta = xyz(f); r.prev_bsdf_pdf = f.w;
    r.radiance = xyz(g); r.depth = f2u(g.w);
    r.base = xyz(h);
    uint32_t fl = f2u(h.w);
    r.active = fl & WF_ACTIVE; r.has_ray = fl & WF_HAS_RAY; r.has_shadow = fl & WF_HAS_SHADOW; r.s_add = fl & WF_S_ADD;
    r.s_depth1 = fl & WF_S_DEPTH1; r.finalize = fl & WF_FINALIZE; r.lane_done = fl & WF_LANE_DONE;
    r.film_rgb = xyz(fm); r.film_w = fm.w;
    r.smp.pcg.state = (uint64_t)rg.x | ((uint64_t)rg.y << 32);
    r.smp.dim = rg.z;
    r.samples_done = rg.w;
    r.pass_idx = ms.x; r.cur_spp = ms.y;
    r.smp.pcg.inc = (uint64_t)ms.z | ((uint64_t)ms.w << 32);
    r.c_samples = r.c_closest = r.c_shadow = r.c_shaded = 0;
}

// Workgroup-wide stream compaction: every lane with a ray gets a distinct index into the queue of its kind; the four waves'
// counts meet in LDS and ONE lane per counter adds the workgroup's total (three atomics per workgroup instead of three per wave:
// queue heads and the active counter are single addresses, and their atomics serialise at the L2). Queue order = slot order
// within the workgroup. Must be called by all 256 threads.
// Sort key of a ray (option wf_sort): 21-bit Morton code of the origin's cell in the scene's box (128 cells per axis), then the
// three sign bits of the direction -- rays that start close together and head the same way end up in the same trace wave.
AKR_D uint32_t wf_spread7(uint32_t x) {  // bit i of the low 7 bits -> bit 3 i
    x &= 0x7fu;
    x = (x | (x << 8)) & 0x0000700fu;
    x = (x | (x << 4)) & 0x000430c3u;
    x = (x | (x << 2)) & 0x00049249u;
    return x;
}
AKR_D uint32_t wf_ray_key(const PtParams& p, vec3 o, vec3 d) {
    auto cell = [](float t) { return (uint32_t)(int)min_f(max_f(t, 0.0f), 127.0f); };  // (NaN -> 0)
    const uint32_t cx = cell((o.x - p.sort_lo[0]) * p.sort_scale[0]), cy = cell((o.y - p.sort_lo[1]) * p.sort_scale[1]), cz = cell((o.z - p.sort_lo[2]) * p.sort_scale[2]);
    const uint32_t oct = (d.x >= 0.0f ? 1u : 0u) | (d.y >= 0.0f ? 2u : 0u) | (d.z >= 0.0f ? 4u : 0u);
    return ((wf_spread7(cx) | (wf_spread7(cy) << 1) | (wf_spread7(cz) << 2)) << 3) | oct;
}
// `resume` != 0: the slot's rays of the last trace launch are not all finished (WfBuffers::pend: bit 0 closest-hit ray, bit 1 shadow ray); the
// unfinished ones go back into the queues marked kWfResume -- the trace kernel continues them from their carry records -- and are not counted again.
constexpr uint32_t kWfResume = 0x80000000u;
AKR_D void wf_enqueue(const PtParams& p, const WfBuffers& wf, uint32_t q, uint32_t slot, PathRegs& r, uint32_t resume = 0u) {
    // closest-hit rays and shadow rays go to separate queues so that waves of the trace kernel are homogeneous
    __shared__ uint32_t sh_cnt[4][3], sh_base[3];
    const bool want_c = r.active && (resume ? (resume & 1u) != 0u : r.has_ray), want_s = r.active && (resume ? (resume & 2u) != 0u : r.has_shadow);
    const uint32_t entry = slot | (resume ? kWfResume : 0u);
    const uint64_t mc = __builtin_amdgcn_ballot_w64(want_c), ms = __builtin_amdgcn_ballot_w64(want_s), ma = __builtin_amdgcn_ballot_w64(r.active);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) {
        sh_cnt[wave][0] = (uint32_t)__builtin_popcountll(mc);
        sh_cnt[wave][1] = (uint32_t)__builtin_popcountll(ms);
        sh_cnt[wave][2] = (uint32_t)__builtin_popcountll(ma);
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const uint32_t tot = sh_cnt[0][threadIdx.x] + sh_cnt[1][threadIdx.x] + sh_cnt[2][threadIdx.x] + sh_cnt[3][threadIdx.x];
        uint32_t* counter = threadIdx.x == 2 ? wf.n_active : &wf.qcount[2 * q + threadIdx.x];
        sh_base[threadIdx.x] = tot ? atomicAdd(counter, tot) : 0u;
    }
    __syncthreads();
    uint32_t bc = sh_base[0], bs = sh_base[1];
    for (uint32_t k = 0; k < wave; k++) { bc += sh_cnt[k][0]; bs += sh_cnt[k][1]; }
    const uint64_t below = (1ull << lane) - 1ull;
    if (want_c) {
        const uint32_t at = bc + (uint32_t)__builtin_popcountll(mc & below);
        wf.queue_closest[q][at] = entry;
        if (p.wf_sort) wf.key_closest[q][at] = wf_ray_key(p, r.ro, r.rd);
        if (!resume) r.c_closest++;
    }
    if (want_s) {
        const uint32_t at = bs + (uint32_t)__builtin_popcountll(ms & below);
        wf.queue_shadow[q][at] = entry;
        if (p.wf_sort) wf.key_shadow[q][at] = wf_ray_key(p, r.s_o, r.s_d);
        if (!resume) r.c_shadow++;
    }
}

template <bool PMJ, bool LENS = false>  // LENS: the camera has a thin lens (device/dpath.h generate_ray)
__global__ __launch_bounds__(256) void k_wf_init(const PtParams p, const WfBuffers wf) {
    const uint32_t slot = wf.slot_base + blockIdx.x * 256u + threadIdx.x;
    uint32_t px = 0, py = 0;
    const bool in_frame = slot < wf.slot_end && item_to_pixel(p, slot, px, py);
    const uint32_t pix = px + py * p.width;
    uint32_t sx, sy;
    shifted_pixel(p, px, py, sx, sy);
    PathRegs r;
    path_regs_init<PMJ, LENS>(r, p, in_frame, pix, sx, sy);
    if (slot < wf.slot_end) {
        wf_store(wf, slot, r);
        if (wf.pend) wf.pend[slot] = 0u;
    }
    wf_enqueue(p, wf, 0, slot, r);
    flush_counters(p, r, TraceCounters{0, 0, 0}, true);
}

#ifndef AKR_WF_SHADE_WAVES
#define AKR_WF_SHADE_WAVES 1  // waves per SIMD the shade kernel's register allocation must leave room for (1 = whatever it needs)
#endif
template <bool TEX, bool PMJ, bool INST = false, bool ENV = false, bool LENS = false>  // ENV: the scene has an environment light (device/denv.h); LENS: a thin lens
__global__ __launch_bounds__(256, TEX ? 1 : AKR_WF_SHADE_WAVES) void k_wf_shade(const PtParams p, const WfBuffers wf, uint32_t q_out) {
    const uint32_t slot = wf.slot_base + blockIdx.x * 256u + threadIdx.x;
    PathRegs r;
    r.active = false; r.has_ray = false; r.has_shadow = false;
    r.c_samples = r.c_closest = r.c_shadow = r.c_shaded = 0;
    bool live = false;
    if (slot < wf.slot_end) live = (f2u(wf.base[slot].w) & WF_ACTIVE) != 0;
    // a slot one of whose rays the trace launch carried over is not shaded this time: its state stays as it is and the unfinished rays are queued again
    uint32_t resume = 0u;
    if (live && wf.pend) resume = wf.pend[slot];
    if (resume) r.active = true;
    if (live && !resume) {
        uint32_t px = 0, py = 0;
        item_to_pixel(p, slot, px, py);
        const uint32_t pix = px + py * p.width;
        uint32_t sx, sy;
        shifted_pixel(p, px, py, sx, sy);
        wf_load(wf, slot, r);
        float4 hv = wf.hit[slot];
        Hit hit;
        hit.gid = f2u(hv.x); hit.u = hv.y; hit.v = hv.z; hit.t = 0.0f;
        bool found = hit.gid != kInvalid, occluded = f2u(hv.w) != 0;
        path_step<-1, TEX, PMJ, 0, 0u, INST, ENV, LENS>(p, r, hit, found, occluded, pix, sx, sy);
        wf_store(wf, slot, r);
    }
    // the queue the trace launch before this one emptied is the next shade launch's to fill: its counts and the queue head back to zero
    // (that launch is complete -- stream order -- and nothing in this one reads them; two hipMemsetAsync per iteration did this until round 6)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        wf.qcount[2u * (1u - q_out)] = 0u;
        wf.qcount[2u * (1u - q_out) + 1u] = 0u;
        *wf.qhead = 0u;
    }
    wf_enqueue(p, wf, q_out, slot, r, resume);
    flush_counters(p, r, TraceCounters{0, 0, 0}, true);
}


// The entry points of the translation units that hold the ENV / LENS instantiations; launch_wf_init and launch_wf_shade (wf_kernels.hip) go
// to them through a table
hipError_t wf_init_entry_lens(const PtParams& p, const WfBuffers& wf, hipStream_t stream);                         // wf_lens_kernels.hip
hipError_t wf_shade_entry_env(const PtParams& p, const WfBuffers& wf, uint32_t q_out, hipStream_t stream);       // wf_env_kernels.hip
hipError_t wf_shade_entry_lens(const PtParams& p, const WfBuffers& wf, uint32_t q_out, hipStream_t stream);      // wf_lens_kernels.hip
hipError_t wf_shade_entry_lens_env(const PtParams& p, const WfBuffers& wf, uint32_t q_out, hipStream_t stream);  // wf_lens_kernels.hip

// textures x sampler family x kept or flattened scene
template <bool ENV, bool LENS>
hipError_t launch_wf_shade_t(const PtParams& p, const WfBuffers& wf, uint32_t q_out, hipStream_t stream) {
    const uint32_t blocks = (wf.slot_end - wf.slot_base + 255u) / 256u;
    if (blocks == 0) return hipSuccess;
    const bool tex = p.sc.tex.nodes != nullptr;
    size_t lds = 0;
    const PtParams q = tex ? with_tex_slots(p, 0, lds) : p;
    dispatch_bools([&](auto T, auto P, auto I) { launch_kernel(k_wf_shade<T(), P(), I(), ENV, LENS>, blocks, lds, stream, q, wf, q_out); },
                   tex, p.sampler != 0, p.sc.in2.on != 0);
    return hipGetLastError();
}

// sampler family
template <bool LENS>
hipError_t launch_wf_init_t(const PtParams& p, const WfBuffers& wf, hipStream_t stream) {
    const uint32_t blocks = (wf.slot_end - wf.slot_base + 255u) / 256u;
    if (blocks == 0) return hipSuccess;
    dispatch_bools([&](auto P) { launch_kernel(k_wf_init<P(), LENS>, blocks, 0, stream, p, wf); }, p.sampler != 0);
    return hipGetLastError();
}

}  // namespace akr
