// wf_schedule.cpp -- the host half of the wavefront schedule (wf_kernels.hip): its buffers and slot groups and one launch group (declarations:
// api_internal.h, next to WavefrontState; which sessions it renders, and which may time it against the megakernel: pt_plan.cpp pt_route). Every
// option read is of the session's snapshot (RenderBase::opt).
#include "api_internal.h"

// The groups' shares of the slots [0, n_active): the session's slots, or the shorter range of an active-tile list (akr_pt_set_active_tiles;
// the buffers stay as they were allocated, for the session's own n_items)
void akr_api::wf_set_range(WavefrontState& ws, uint32_t n_active) {
    const uint32_t groups = (uint32_t)ws.group.size();
    const WfBuffers& w = ws.buf;
    for (uint32_t g = 0; g < groups; g++) {
        WfBuffers& wg = ws.group[g];
        // boundaries on whole 1024-slot tiles
        auto bound = [&](uint32_t k) { return k >= groups ? n_active : (uint32_t)(((uint64_t)n_active * k / groups) & ~1023ull); };
        wg.slot_base = bound(g);
        wg.slot_end = bound(g + 1);
        for (int k = 0; k < 2; k++) {  // a group's queues: its share of the session's
            wg.queue_closest[k] = w.queue_closest[k] + wg.slot_base;
            wg.queue_shadow[k] = w.queue_shadow[k] + wg.slot_base;
        }
    }
}

// The wavefront schedule's buffers for the session: a slot per item of the session's parameter block
std::unique_ptr<WavefrontState> akr_api::wf_allocate(const akr_pt_session* se, bool sort) {
    auto ws = std::make_unique<WavefrontState>();
    const uint32_t n_slots = se->params.n_items;
    ws->slots = n_slots;
    ws->sort = sort;
    const size_t n = n_slots ? n_slots : 1;
    ws->state.alloc(12 * n * 16);  // 10 float4 + 2 uint4 arrays
    char* base = (char*)ws->state.p;
    auto take = [&](size_t k) { void* p = base + k * n * 16; return p; };
    WfBuffers& w = ws->buf;
    w.ray_o = (float4*)take(0); w.ray_d = (float4*)take(1); w.sh_o = (float4*)take(2); w.sh_d = (float4*)take(3);
    w.sh_c = (float4*)take(4); w.hit = (float4*)take(5); w.beta = (float4*)take(6); w.rad = (float4*)take(7);
    w.base = (float4*)take(8); w.film = (float4*)take(9); w.rng = (uint4*)take(10); w.misc = (uint4*)take(11);
    ws->queues.alloc(4 * n * sizeof(uint32_t));
    uint32_t* q = (uint32_t*)ws->queues.p;
    w.queue_closest[0] = q; w.queue_closest[1] = q + n; w.queue_shadow[0] = q + 2 * n; w.queue_shadow[1] = q + 3 * n;
    w.key_closest[0] = w.key_closest[1] = w.key_shadow[0] = w.key_shadow[1] = nullptr;
    // carried rays (wf_kernels.hip): a record per (kind, slot) = 12 words + this scene's traversal stack. Not with option wf_sort (a carried ray has no key).
    w.pend = nullptr; w.carry = nullptr; w.carry_words = 0; w.n_slots = n_slots;
    // (option values above 1 = test hook: that launch size, and waves hand over early and nearly whole -- small frames carry thousands of rays)
    const bool carry_test = se->opt.wf_carry > 1;
    w.carry_queue = carry_test ? (uint32_t)se->opt.wf_carry : 65536u;
    w.carry_lanes = carry_test ? 56u : 16u;
    w.carry_steps = carry_test ? 4u : 48u;
    if (se->opt.wf_carry != 0 && !sort && n_slots > 0) {
        w.carry_words = (12u + se->params.sc.bvh_stack_depth + 3u) & ~3u;  // (16-byte aligned records)
        ws->pend.alloc(n * sizeof(uint32_t));
        ws->carry.alloc(2 * n * (size_t)w.carry_words * sizeof(uint32_t));
        w.pend = (uint32_t*)ws->pend.p;
        w.carry = (uint32_t*)ws->carry.p;
    }
    if (sort) {
        ws->keys.alloc(4 * n * sizeof(uint32_t));
        uint32_t* k = (uint32_t*)ws->keys.p;
        w.key_closest[0] = k; w.key_closest[1] = k + n; w.key_shadow[0] = k + 2 * n; w.key_shadow[1] = k + 3 * n;
        ws->sorted.alloc(3 * n * sizeof(uint32_t));
        ws->sorted_closest = (uint32_t*)ws->sorted.p;
        ws->sorted_shadow = ws->sorted_closest + n;
        ws->sorted_keys = ws->sorted_closest + 2 * n;
        ws->sort_tmp.alloc(wf_sort_temp_bytes((uint32_t)n));
    }
    // ---- slot groups. A trace launch ends with its slowest rays, a hundred dependent fetches deep, while the rest of the chip idles, and a
    // launch group is a hundred such launches (the slots with the longest paths decide): measured on the kept 1080p forest that tail is
    // 19 ms of 73 ms (1000 x 10 k triangles) and 69 ms of 144 ms (x 100 k) per 8 spp -- tools/kept_schedules.py at four frame sizes,
    // HISTORY R6.6. The slots are therefore divided into groups that run the same init / trace / shade chain on streams of their own:
    // one group's kernels fill the CUs another's tail leaves idle. Nothing a slot computes depends on which group it is in.
    // Measured (profiles/r6_kept_schedules.txt, 1080p): two groups 113 -> 136 Msamples/s on the kept forest of 100 k-triangle meshes (its trace
    // launches wait on memory -- the meshes do not fit the L2s -- and the other group's shade launch streams meanwhile), 228 -> 221 on the
    // 10 k-triangle one, 208 -> 213 on the flattened hall; four groups and more lose everywhere (each group's launches are shorter and their
    // ends no better filled). Option wf_groups: 0 = the library decides (two for a kept scene whose meshes exceed the L2s, else one).
    const akr_scene* sc = se->scene;
    const size_t mesh_bytes = sc->cs.instanced.on ? (sc->cs.instanced.nodes.size() + sc->cs.instanced.mesh_tris.size()) * 4 : 0;
    const int opt_groups = se->opt.wf_groups;
    // With carried rays (option wf_carry, the default since the end of round 6) a launch has no such tail and one group wins at every size measured
    // (1080p, x 100 k: 175 against 158 with two; 4K: 220 against 203): the automatic choice is two groups only without them.
    uint32_t groups = sort ? 1u : (opt_groups > 0 ? (uint32_t)opt_groups : (mesh_bytes > (16u << 20) && w.carry == nullptr ? 2u : 1u));
    groups = std::min(groups, std::max(1u, n_slots / 65536u));  // (small frames: a group should still be a few waves per CU)
    ws->ctrl.alloc((size_t)groups * 8 * sizeof(uint32_t));  // per group: qcount[4], qhead, n_active
    for (uint32_t g = 0; g < groups; g++) {
        WfBuffers wg = w;
        uint32_t* c = (uint32_t*)ws->ctrl.p + 8 * g;
        wg.qcount = c; wg.qhead = c + 4; wg.n_active = c + 5;
        ws->group.push_back(wg);
    }
    wf_set_range(*ws, n_slots);
    if (groups > 1) {
        for (uint32_t g = 0; g < groups; g++) {
            hipStream_t st = nullptr;
            HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            ws->streams.push_back(st);
            hipEvent_t ev = nullptr;
            HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            ws->join.push_back(ev);
        }
        HIP_CHECK(hipEventCreateWithFlags(&ws->fork, hipEventDisableTiming));
    }
    // persistent trace kernel: as many workgroups as the CUs hold at once (occupancy API: registers + this tree's LDS stacks)
    // ... but no more than the scene's data can feed: every resident wave is 64 more rays gathering from the tree, and past the L2s and the
    // 256 MB infinity cache more rays in flight only evict each other's nodes (the trace kernel of a flattened scene fits six waves per SIMD,
    // the megakernel runs four). Measured, workgroups per CU 4 / 5 / 6: hall of 0.1 M triangles (21 MB on the device) 337 / 353 / 356 Msamples/s,
    // 1 M (214 MB) 300 / 310 / 307, 3 M (642 MB) 273 / 281 / 265, 10 M (2.1 GB) 253 / 247 / 228, flattened forest of 10 M (2.6 GB) 370 / 366 / 351.
    uint32_t per_cu = wf_trace_blocks_per_cu(se->params);
    const uint64_t scene_bytes = sc->device_bytes;
    per_cu = std::min(per_cu, scene_bytes > (1200ull << 20) ? 4u : (scene_bytes > (400ull << 20) ? 5u : 8u));
    if (const char* e = std::getenv("AKR_WF_TRACE_BLOCKS_PER_CU")) per_cu = (uint32_t)std::max(1, std::min(8, std::atoi(e)));  // (measurement hook)
    ws->trace_blocks = (uint32_t)se->ctx->props.multiProcessorCount * per_cu;
    return ws;
}

// One launch group of the wavefront schedule = `fused` passes for every slot: init, then trace/shade iterations until
// no slot is active. The host only looks at the device every 16 iterations (every 4 once few slots are left).
void akr_api::wf_run(akr_pt_session* se) {
    hipStream_t main_st = se->ctx->stream;
    const PtParams& p = se->params;
    WavefrontState& ws = *se->wf;
    const uint32_t groups = (uint32_t)ws.group.size();
    HIP_CHECK(hipMemsetAsync(ws.ctrl.p, 0, ws.ctrl.bytes, main_st));
    std::vector<hipStream_t> streams(groups, main_st);
    if (groups > 1) {  // the groups' streams start after everything the session's stream holds so far ...
        HIP_CHECK(hipEventRecord(ws.fork, main_st));
        for (uint32_t g = 0; g < groups; g++) {
            streams[g] = ws.streams[g];
            HIP_CHECK(hipStreamWaitEvent(streams[g], ws.fork, 0));
        }
    }
    struct Join {  // ... and the session's stream goes on after all of them, also when this function is left by an exception
        WavefrontState& ws; std::vector<hipStream_t>& st; hipStream_t main_st;
        ~Join() {
            if (st.size() < 2) return;
            for (size_t g = 0; g < st.size(); g++) {
                (void)hipEventRecord(ws.join[g], st[g]);
                (void)hipStreamWaitEvent(main_st, ws.join[g], 0);
            }
        }
    } join{ws, streams, main_st};
    for (uint32_t g = 0; g < groups; g++) HIP_CHECK(launch_wf_init(p, ws.group[g], streams[g]));
    int check_every = 16, since_check = 0;  // iterations between two looks at the device (every look drains the stream)
    uint32_t q = 0;
    std::vector<uint8_t> done(groups, 0);
    for (uint64_t iter = 0;; iter++) {
        // option wf_sort (one group): the sizes of the queue this iteration traces (rocPRIM wants the element count on the host): one small
        // read-back per iteration, before the counters are reset -- it also ends the loop the moment the last path has finished
        uint32_t nc = 0, ns = 0;
        const bool sort_now = ws.sort && iter > 0;  // (the first iteration's camera rays are in pixel order: coherent as they are)
        if (sort_now) {
            uint32_t counts[6];
            HIP_CHECK(hipMemcpyAsync(counts, ws.ctrl.p, sizeof counts, hipMemcpyDeviceToHost, main_st));
            HIP_CHECK(hipStreamSynchronize(main_st));
            if (counts[5] == 0) break;  // n_active after the last shade
            nc = counts[2 * q];
            ns = counts[2 * q + 1];
        }
        for (uint32_t g = 0; g < groups; g++) {
            if (done[g]) continue;
            const WfBuffers& wg = ws.group[g];
            hipStream_t st = streams[g];
            // queue q holds the rays to trace. (The head, the other queue's counts and the active counter are reset by the kernels themselves:
            // k_wf_trace zeroes n_active, k_wf_shade the counts of the queue just traced and the head.)
            if (sort_now) {
                WfBuffers sorted = wg;
                HIP_CHECK(wf_sort_pairs(ws.sort_tmp.p, ws.sort_tmp.bytes, wg.key_closest[q], ws.sorted_keys, wg.queue_closest[q], ws.sorted_closest, nc, st));
                HIP_CHECK(wf_sort_pairs(ws.sort_tmp.p, ws.sort_tmp.bytes, wg.key_shadow[q], ws.sorted_keys, wg.queue_shadow[q], ws.sorted_shadow, ns, st));
                sorted.queue_closest[q] = ws.sorted_closest;
                sorted.queue_shadow[q] = ws.sorted_shadow;
                HIP_CHECK(launch_wf_trace(p, sorted, q, ws.trace_blocks, st));
            } else {
                HIP_CHECK(launch_wf_trace(p, wg, q, ws.trace_blocks, st));
            }
            HIP_CHECK(launch_wf_shade(p, wg, 1 - q, st));
        }
        q = 1 - q;
        if (!ws.sort && ++since_check >= check_every) {
            since_check = 0;
            std::vector<uint32_t> n_active(groups, 0);
            for (uint32_t g = 0; g < groups; g++)
                if (!done[g]) HIP_CHECK(hipMemcpyAsync(&n_active[g], ws.group[g].n_active, sizeof(uint32_t), hipMemcpyDeviceToHost, streams[g]));
            bool all = true;
            for (uint32_t g = 0; g < groups; g++) {
                if (done[g]) continue;
                HIP_CHECK(hipStreamSynchronize(streams[g]));
                if (n_active[g] == 0) done[g] = 1; else all = false;
            }
            if (all) break;
            // the last slots' paths: launches with next to nothing to do -- look more often, so that fewer of them run for nothing
            uint64_t left = 0;
            for (uint32_t g = 0; g < groups; g++) left += n_active[g];
            check_every = left * 64 < ws.slots ? 4 : 16;
        }
        if (iter > (1ull << 26)) throw RenderError("wavefront schedule did not terminate");
    }
}
