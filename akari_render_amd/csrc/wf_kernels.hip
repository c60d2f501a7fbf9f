// wf_kernels.hip -- wavefront schedule of the same path tracer, for scenes whose intersection cost is dominated by
// BVH traversal (BASELINE configs[3], 10 M triangles).
//
// The megakernel (pt_kernels.hip) keeps a whole path in one lane's registers; with a BVH that means ~120 live
// registers around a divergent traversal loop (4 waves/SIMD, 26 % VALU lane utilisation, 69 % of wave cycles waiting
// on memory on the 10 M-triangle hall). Here the two halves are separate kernels and the path state streams through
// HBM between them (structure-of-arrays, 16-byte records, one slot per pixel):
//   k_wf_trace  persistent waves pull ray ids from a queue: when a lane's ray ends it takes the next id immediately
//               (wave64 __ballot + popcount prefix + one atomicAdd per wave) instead of idling until the slowest
//               lane of its wave is done; only ray + traversal registers are live, so 7-8 waves/SIMD hide latency;
//   k_wf_shade  one thread per path slot: path_step() of device/dpath.h (identical arithmetic to the megakernel),
//               then stream compaction of the rays it produced into the next queue (ballot/prefix-sum again).
// The reference's author sketched the same decomposition in crates/akari_integrator/src/wfpt.rs:59-225,315-494
// (PathState SoA, KernelWorkQueue, raygen / intersect / shade / test_shadow); that file never runs there.
#include <algorithm>
#include "wf_path.h"

namespace akr {

template <bool INST> struct TravOf { typedef Trav type; };
template <> struct TravOf<true> { typedef TravI type; };
template <bool INST, class T>
AKR_D void wf_trav_begin(T& s, vec3 o, vec3 d, float tmin, float tmax, uint32_t ex0, uint32_t ex1) {
    if constexpr (INST) trav_begin_inst(s, o, d, tmin, tmax, ex0, ex1);
    else trav_begin(s, o, d, tmin, tmax, ex0, ex1);
}
// Carried rays. A trace launch used to end with its slowest rays -- a hundred dependent fetches deep, in waves with a handful of lanes left -- while
// the rest of the chip idled: 19 of 73 ms per 8 spp on the kept 1080p forest, 69 of 144 ms with 100 k-triangle meshes (HISTORY R6.6). Now a wave that
// has found the queue empty, is down to WfBuffers::carry_lanes (16) lanes and has given each of them carry_steps (48) steps since it started or resumed (progress
// is guaranteed) writes those lanes' traversals -- best hit, position in the tree, the stack -- into the rays' carry records, marks the slots
// (WfBuffers::pend) and ends. k_wf_shade leaves a marked slot alone and queues its unfinished rays again (kWfResume); the next trace launch
// picks them up with everything else. Launches with fewer than WfBuffers::carry_queue rays (65 536) trace to the end as before (the last iterations of a launch
// group must drain, and a launch of its own per fifty steps would cost more than the tail). Nothing a path computes changes -- the iteration in
// which a vertex is shaded does, as with the megakernel's stragglers (pt_pass.h). Measured with 8 / 16 / 32 / 48 lanes and 16 / 48 / 128 steps: all
// within 2 % of each other (1080p forest x 100 k: 172 -- 177 Msamples/s against 124 without).
// A record is the carried traversal of disect.h / dinst_trav.h (carry_best | carry_place | carry_inst: the fields and order of kernels.h CY_*) as
// 16-byte groups, then the stack.
template <bool INST, class T>
AKR_D void wf_carry_save(const WfBuffers& wf, const T& s, const uint32_t* __restrict__ stack, uint32_t slot, bool any) {
    uint32_t* c = wf.carry + ((size_t)(any ? wf.n_slots : 0u) + slot) * wf.carry_words;  // (carry_words is a multiple of 4: 16-byte aligned records)
    ((uint4*)c)[0] = carry_best(s);
    ((uint4*)c)[1] = carry_place(s);
    if constexpr (INST) ((uint4*)c)[2] = carry_inst(s);
    for (uint32_t k = 0; k < s.sp; k++) c[12u + k] = stack[k * 256u];
}
template <bool INST, class T>
AKR_D void wf_carry_restore(const DScene& sc, const WfBuffers& wf, T& s, uint32_t* __restrict__ stack, uint32_t slot, bool any) {  // (after wf_trav_begin on the slot's ray)
    const uint32_t* c = wf.carry + ((size_t)(any ? wf.n_slots : 0u) + slot) * wf.carry_words;
    const uint4 a = ((const uint4*)c)[0], b = ((const uint4*)c)[1];
    for (uint32_t k = 0; k < b.w; k++) stack[k * 256u] = c[12u + k];
    if constexpr (INST) trav_resume(sc, s, a, b, ((const uint4*)c)[2]);
    else trav_resume(sc, s, a, b);
}

// Persistent traversal kernel. Ray id = slot; ids [0, n_closest) come from the closest-hit queue, the rest from the
// shadow queue. A lane that finishes its ray writes the result and becomes idle; when enough lanes of the wave are
// idle (or all), the wave refills them from the queue head.
#ifndef AKR_WF_REFILL_IDLE
#define AKR_WF_REFILL_IDLE 20  // refill when at least this many of the 64 lanes are idle
#endif
#ifndef AKR_WF_REFILL_IDLE_INST
#define AKR_WF_REFILL_IDLE_INST 8  // ... on a scene kept as meshes + instances (an iteration of its loop costs more: 1 / 4 / 8 / 20 / 32 idle lanes: 232 / 243 / 245 / 241 / 230 Msamples/s, 1080p forest)
#endif
// INST (round 6): the scene is kept as meshes + instances -- the two-level traversal of dinst_trav.h: a lane's candidates wait in its
// pending slot and the wave takes the exact test in batches, as trace_inst does.
#ifndef AKR_WF_TRACE_INST_WAVES
#define AKR_WF_TRACE_INST_WAVES 1  // waves per SIMD the kept-scene trace kernel's register allocation must leave room for (1 = whatever it needs: 128 VGPRs, 4 waves)
#endif
template <bool TEX, bool INST = false>
__global__ __launch_bounds__(256, INST ? AKR_WF_TRACE_INST_WAVES : 1) void k_wf_trace(const PtParams p, const WfBuffers wf, uint32_t q_in) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    uint32_t* stack = lds_stack + threadIdx.x;
    const DScene& sc = p.sc;
    const uint32_t n_closest = wf.qcount[2 * q_in + 0], n_total = n_closest + wf.qcount[2 * q_in + 1];
    const uint32_t lane = threadIdx.x & 63u;
    if (blockIdx.x == 0 && threadIdx.x == 0) *wf.n_active = 0u;  // (the shade launch after this one counts the slots still active; the host reads it after that)
    TraceCounters cnt{0, 0, 0};
    bool has = false, exhausted = false, any = false, resumed = false;
    uint32_t slot = 0, steps = 0, n_carried = 0;
    const bool carry = wf.carry != nullptr && n_total >= wf.carry_queue;
    // 128 ray ids per claim. (ADVICE round 3 suggested 64 -- one wave-fill -- so that near the end of a queue no wave sits on ids that
    // idle waves could have traced; measured in round 4: twice the atomics on the queue head cost more than the shorter tail gains,
    // cbox with a forced BVH 398 against 576 Msamples/s, 10 M-triangle hall 211 against 219.)
    constexpr uint32_t kWfChunk = 128;
    uint32_t c_next = 0, c_end = 0;  // the wave's claimed range of ray ids
    typename TravOf<INST>::type s;
    wf_trav_begin<INST>(s, mk3(0, 0, 0), mk3(0, 0, 1), 0.0f, -1.0f, kInvalid, kInvalid);  // idle: tmax < tmin
    uint32_t waited = 0;
    bool blocked = false;
    for (;;) {
        // Refill idle lanes from the queue. A wave claims kWfChunk consecutive ray ids with ONE atomic and hands them to its idle
        // lanes by ballot + prefix count until the chunk is used up (one atomic per refill -- 150 k of them on one address per
        // launch -- kept the L2's atomic unit busier than the traversal kept the CUs).
        for (int attempt = 0; attempt < 2 && !exhausted; attempt++) {
            const uint64_t idle = __builtin_amdgcn_ballot_w64(!has);
            if (idle == 0) break;
            if (c_next >= c_end) {  // (wave-uniform)
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(wf.qhead, kWfChunk);
                base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                c_next = base;
                c_end = base + kWfChunk < n_total ? base + kWfChunk : n_total;
                if (base >= n_total) { exhausted = true; break; }
            }
            const uint32_t my = c_next + (uint32_t)__builtin_popcountll(idle & ((1ull << lane) - 1ull));
            if (!has && my < c_end) {
                any = my >= n_closest;
                const uint32_t entry = any ? wf.queue_shadow[q_in][my - n_closest] : wf.queue_closest[q_in][my];
                slot = entry & ~kWfResume;
                resumed = (entry & kWfResume) != 0u;
                float4 a = any ? wf.sh_o[slot] : wf.ray_o[slot];
                float4 b = any ? wf.sh_d[slot] : wf.ray_d[slot];
                wf_trav_begin<INST>(s, xyz(a), xyz(b), 0.0f, any ? b.w : 1e20f, f2u(a.w), any ? f2u(wf.sh_c[slot].w) : kInvalid);
                if (resumed) wf_carry_restore<INST>(sc, wf, s, stack, slot, any);
                has = true;
                blocked = false;
                steps = 0;
            }
            const uint32_t n = (uint32_t)__builtin_popcountll(idle);
            c_next = c_next + n < c_end ? c_next + n : c_end;
        }
        if (__builtin_amdgcn_ballot_w64(has) == 0) break;
        for (;;) {
            bool finished;
            if constexpr (INST) {
                bool pending = false, wait = false;
                if (has) {
                    if (s.pend_rec == kInvalid) blocked = false;
                    steps++;
                    if (s.active & !blocked) blocked = trav_step_inst<TEX>(sc, s, stack, cnt);
                    pending = s.pend_rec != kInvalid;
                    wait = pending & (blocked | !s.active);  // cannot go on without the verdict
                }
                if (__builtin_amdgcn_ballot_w64(wait) != 0) {
                    waited++;
                    if (waited >= AKR_INST_PATIENCE || __builtin_amdgcn_ballot_w64(has & s.active & !wait) == 0 ||
                        __builtin_popcountll(__builtin_amdgcn_ballot_w64(pending)) >= AKR_INST_QUORUM) {
                        waited = 0;
                        if (pending) resolve_pending<TEX>(sc, s, any);
#if defined(AKR_INST_PRETEST_CHECK)
                        if (s.check_t == -2.0f) cnt.overflow = 1;
#endif
                    }
                }
                finished = has && !s.active && s.pend_rec == kInvalid;
            } else {
                if (has && s.active) { steps++; trav_step<2, TEX>(sc, s, stack, cnt, any); }
                finished = has && !s.active;
            }
            if (finished) {  // ray finished: publish the result for k_wf_shade
                float* hp = (float*)&wf.hit[slot];
                if (any) {
                    hp[3] = u2f(s.best != kInvalid ? 1u : 0u);
                } else {
                    hp[0] = u2f(s.best); hp[1] = s.best_u; hp[2] = s.best_v;
                }
                if (resumed) atomicAnd(&wf.pend[slot], any ? ~2u : ~1u);
                has = false;
            }
            const uint32_t n_idle = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(!has));
            if (n_idle == 64u) break;
            if (carry && exhausted && n_idle >= 64u - wf.carry_lanes && __builtin_amdgcn_ballot_w64(has && steps < wf.carry_steps) == 0) {
                if (has) {  // the wave's last rays go on in the next launch
                    wf_carry_save<INST>(wf, s, stack, slot, any);
                    atomicOr(&wf.pend[slot], any ? 2u : 1u);
                    has = false;
                    n_carried++;
                }
                break;
            }
            if (!exhausted && n_idle >= (INST ? AKR_WF_REFILL_IDLE_INST : AKR_WF_REFILL_IDLE)) break;
        }
    }
    // traversal counters
    if (p.counters != nullptr) {
        uint64_t* const ctr = p.counters + 8u * (blockIdx.x % kStatStripes);
        uint32_t nn = wave_sum_u32(cnt.nodes), nt = wave_sum_u32(cnt.tris), ov = wave_sum_u32(cnt.overflow);
        if (lane == 0) {
            if (nn) atomicAdd((unsigned long long*)&ctr[4], (unsigned long long)nn);
            if (nt) atomicAdd((unsigned long long*)&ctr[5], (unsigned long long)nt);
            if (ov) atomicAdd((unsigned long long*)&ctr[6], (unsigned long long)ov);
        }
        if (carry) {
            const uint32_t nc = wave_sum_u32(n_carried);
            if (lane == 0 && nc) atomicAdd((unsigned long long*)&ctr[7], (unsigned long long)nc);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- launchers
// the translation unit that holds a session's kernels: k_wf_init by [lens], k_wf_shade by [env][lens]
hipError_t launch_wf_init(const PtParams& p, const WfBuffers& wf, hipStream_t stream) {
    static constexpr hipError_t (*kEntry[2])(const PtParams&, const WfBuffers&, hipStream_t) = {launch_wf_init_t<false>, wf_init_entry_lens};
    return kEntry[camera_runs_lens_kernels(p.lens_radius, p.projection)](p, wf, stream);
}
hipError_t launch_wf_shade(const PtParams& p, const WfBuffers& wf, uint32_t q_out, hipStream_t stream) {
    static constexpr hipError_t (*kEntry[2][2])(const PtParams&, const WfBuffers&, uint32_t, hipStream_t) = {{launch_wf_shade_t<false, false>, wf_shade_entry_lens},
                                                                                                         {wf_shade_entry_env, wf_shade_entry_lens_env}};
    return kEntry[p.sc.env != nullptr][camera_runs_lens_kernels(p.lens_radius, p.projection)](p, wf, q_out, stream);
}
// The trace launch of a scene: its kernel (textures x kept or flattened), its parameter block and its dynamic LDS -- the traversal stacks, then
// the graph-value slots of a scene with textures. One place, so that the occupancy query and the launch cannot name different kernels.
struct WfTraceLaunch {
    void (*kernel)(const PtParams, const WfBuffers, uint32_t);
    PtParams q;
    size_t lds;
};
static WfTraceLaunch wf_trace_launch(const PtParams& p) {
    const bool tex = p.sc.tex.nodes != nullptr;
    WfTraceLaunch l{nullptr, p, (size_t)p.sc.bvh_stack_depth * 256 * 4};
    if (tex) l.q = with_tex_slots(p, l.lds, l.lds);
    dispatch_bools([&](auto T, auto I) { l.kernel = k_wf_trace<T(), I()>; }, tex, p.sc.in2.on != 0);
    return l;
}
// Workgroups of the persistent trace kernel one CU holds at once (registers and the LDS stacks of this scene's tree decide).
uint32_t wf_trace_blocks_per_cu(const PtParams& p) {
    const WfTraceLaunch l = wf_trace_launch(p);
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, l.kernel, 256, l.lds) != hipSuccess || n < 1) n = 4;
    return (uint32_t)std::min(n, 8);
}
hipError_t launch_wf_trace(const PtParams& p, const WfBuffers& wf, uint32_t q_in, uint32_t n_blocks, hipStream_t stream) {
    const WfTraceLaunch l = wf_trace_launch(p);
    launch_kernel(l.kernel, n_blocks, l.lds, stream, l.q, wf, q_in);
    return hipGetLastError();
}

}  // namespace akr
