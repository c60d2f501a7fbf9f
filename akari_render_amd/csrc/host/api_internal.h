// api_internal.h -- what the translation units of the C ABI share (api_common.cpp: errors, options, contexts, films; api_scene.cpp;
// api_pt.cpp: the `pt` sessions; api_aux.cpp: aov / gpt / mcmc_opt; api_task.cpp: akr_render_task; api_probe.cpp: test hooks).
// Every entry point catches C++ exceptions and HIP errors and turns them into an akr_status plus a thread-local message; nothing
// throws or aborts across the boundary.
#pragma once
#include <atomic>
#include <mutex>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstdio>
#include <chrono>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "scene_build.h"
#include "specialise.h"
#include "stdrng.h"


namespace akr_api {
using namespace akr;


extern thread_local std::string g_last_error;  // api_common.cpp

struct HipError : std::runtime_error {
    explicit HipError(const std::string& s) : std::runtime_error(s) {}
};
struct Unsupported : std::runtime_error {
    explicit Unsupported(const std::string& s) : std::runtime_error(s) {}
};
struct IoError : std::runtime_error {
    explicit IoError(const std::string& s) : std::runtime_error(s) {}
};
struct RenderError : std::runtime_error {  // the device ran, but the result is not a valid render (not an input-file problem)
    explicit RenderError(const std::string& s) : std::runtime_error(s) {}
};

#define HIP_CHECK(expr)                                                                                         \
    do {                                                                                                        \
        hipError_t _e = (expr);                                                                                 \
        if (_e != hipSuccess) throw HipError(std::string(#expr) + ": " + hipGetErrorString(_e));                \
    } while (0)

inline int32_t fail(int32_t code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

template <typename F>
int32_t guarded(F&& f) {
    try {
        g_last_error.clear();
        f();
        return AKR_OK;
    } catch (const HipError& e) {
        return fail(AKR_ERR_HIP, e.what());
    } catch (const Unsupported& e) {
        return fail(AKR_ERR_UNSUPPORTED, e.what());
    } catch (const IoError& e) {
        return fail(AKR_ERR_IO, e.what());
    } catch (const RenderError& e) {
        return fail(AKR_ERR_RENDER, e.what());
    } catch (const std::invalid_argument& e) {
        return fail(AKR_ERR_INVALID_ARGUMENT, e.what());
    } catch (const std::bad_alloc&) {
        return fail(AKR_ERR_OUT_OF_MEMORY, "out of host memory");
    } catch (const std::exception& e) {
        std::string w = e.what();
        if (w.rfind("unsupported", 0) == 0 || w.find("unsupported:") != std::string::npos) return fail(AKR_ERR_UNSUPPORTED, w);
        if (w.rfind("cannot open", 0) == 0) return fail(AKR_ERR_IO, w);
        return fail(AKR_ERR_PARSE, w);
    } catch (...) {
        return fail(AKR_ERR_INVALID_ARGUMENT, "unknown error");
    }
}

// RAII device buffer
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    void alloc(size_t n) {
        release();
        if (n == 0) return;
        HIP_CHECK(hipMalloc(&p, n));
        bytes = n;
    }
    void upload(const void* src, size_t n) {
        alloc(n);
        if (n) HIP_CHECK(hipMemcpy(p, src, n, hipMemcpyHostToDevice));
    }
    template <typename T>
    void upload(const std::vector<T>& v) { upload(v.data(), v.size() * sizeof(T)); }
    template <typename T>
    T* as() const { return (T*)p; }
};

// The timing events of a call's stages on one stream (the *_times test hooks): mark() records the next one, ms(a, b) is the time from
// mark a to mark b once the stream is synchronised. Not enabled (the entry points that time nothing): mark() does nothing, no event is made.
struct StreamMarks {
    hipStream_t stream;
    bool enabled;
    std::vector<hipEvent_t> ev;
    StreamMarks(hipStream_t stream, bool enabled) : stream(stream), enabled(enabled) {}
    StreamMarks(const StreamMarks&) = delete;
    StreamMarks& operator=(const StreamMarks&) = delete;
    ~StreamMarks() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    void mark() {
        if (!enabled) return;
        hipEvent_t e;
        HIP_CHECK(hipEventCreate(&e));
        ev.push_back(e);
        HIP_CHECK(hipEventRecord(e, stream));
    }
    float ms(size_t a, size_t b) const {
        float t = 0.0f;
        HIP_CHECK(hipEventElapsedTime(&t, ev[a], ev[b]));
        return t;
    }
};

// A frame cut into tiles (0 = the default size, 32) and the pixels of the tiles rank `rank` of `count` owns, whole tiles counted
struct TileGrid {
    uint32_t tile_w = 32, tile_h = 32, tiles_x = 0, tiles_y = 0, n_items = 0;
};
inline TileGrid tile_grid(uint32_t tile_w, uint32_t tile_h, uint32_t width, uint32_t height, uint32_t rank, uint32_t count) {
    TileGrid g;
    auto or_default = [](uint32_t t) { return t ? t : 32u; };
    g.tile_w = or_default(tile_w);
    g.tile_h = or_default(tile_h);
    g.tiles_x = (width + g.tile_w - 1) / g.tile_w;
    g.tiles_y = (height + g.tile_h - 1) / g.tile_h;
    uint32_t n = g.tiles_x * g.tiles_y;
    if (count > 1) {
        n = 0;
        for (uint32_t ty = 0; ty < g.tiles_y; ty++)
            for (uint32_t tx = 0; tx < g.tiles_x; tx++) n += tile_owner(tx, ty, count) == rank ? 1u : 0u;
    }
    g.n_items = n * g.tile_w * g.tile_h;
    return g;
}

}  // namespace akr_api
using namespace akr_api;


struct akr_context {
    int device = 0;
    hipStream_t stream = nullptr;
    hipDeviceProp_t props;
    void bind() const { HIP_CHECK(hipSetDevice(device)); }
    SpecCache spec_cache;  // per-scene kernels loaded on this device (host/specialise.cpp)
    // PreComputedTables (svm/surface/precompute.rs:133-145) as this context's first scene that needed it computed it: the table is
    // a constant of the algorithm (fixed seed stream, 2^20 samples per entry: 1.8 s on an MI355X), not of the scene
    std::mutex ggx_mutex;
    std::vector<float> ggx_cache;
    // tables of the pmj02bn sampler, uploaded when the first session asks for it
    DevBuf pmj_sets, bluenoise;
    void ensure_pmj_tables() {
        if (pmj_sets.p && bluenoise.p) return;
        std::vector<uint32_t> sets;
        std::vector<uint16_t> bn;
        make_pmj02_sets(sets);
        load_bluenoise(bn);
        pmj_sets.upload(sets);
        bluenoise.upload(bn);
    }
};

struct akr_scene {
    akr_context* ctx = nullptr;
    FlatScene flat;
    CompiledScene cs;
    // the device tables: one row of api_scene.cpp kSceneTables per member (what it holds, when it exists, which pointer of DScene finds it) ...
    DevBuf woop, tri_gid, shade, normals, inst, materials, area_entries, area_pdf, inst_tri_offset, bvh_nodes;
    DevBuf in2_tlas_leaves, in2_mesh_tris, in2_mesh_pos, in2_mesh_meta, in2_mesh_normals, in2_inst_mats;
    DevBuf tex_nodes, tex_images, tex_texels, tex_mat_inputs;
    DevBuf light_entries, light_pdf, light_inst, light_tri_offset, light_n_tris, punct, light_alias, area_alias, lights, env_texels, env_marginal, env_conditional, env_rec;
    DevBuf ggx_table, in2_share_bits;  // ... but these two, which the device fills (api_scene.cpp ensure_ggx_table, scene_finish)
    std::atomic<int> sessions{0};  // pt / aov / gpt / mcmc_opt sessions that hold the scene (akr_scene_set_environment and the punctual lights' setters are refused meanwhile)
    std::vector<float> ggx_host;
    // materials / node lists / raw inputs re-compiled for a non-default colour pipeline (akr_pt_config.color), by pipeline (api_pt.cpp color_set makes them)
    struct ColorSet {
        DevBuf materials, tex_nodes, mat_inputs;
        DevBuf punct;  // the punctual lights' records: their colour goes through the pipeline on the host, as an Emission material's
        void apply(const CompiledScene& cs, DScene& d) const {  // the tables of a parameter block's scene that this pipeline replaces
            d.materials = materials.as<DMaterial>();
            if (cs.has_textures) d.tex.nodes = tex_nodes.as<DNode>(), d.tex.mat_inputs = mat_inputs.as<MatInputs>();
            if (!cs.punct.empty()) d.punct = punct.as<DPunct>();
        }
    };
    std::map<uint32_t, std::unique_ptr<ColorSet>> color_sets;
    std::mutex color_sets_mutex;  // sessions of several host threads may begin on one scene; entries are never removed before the scene dies
    // the scene's shader kinds as kernel text (host/specialise.cpp), made when the first session asks for a per-scene kernel
    std::string spec_header;
    bool spec_header_made = false;
    std::mutex spec_mutex;
    DScene dscene;
    float r2c[16], c2w[16];
    uint32_t c2w_identity = 0;
    uint64_t device_bytes = 0;
};

struct akr_film {
    akr_context* ctx = nullptr;
    uint32_t width = 0, height = 0;
    DevBuf own;
    float* data = nullptr;  // 7 * W * H floats
    float splat_scale = 1.0f;  // Film.splat_scale, film.rs:73,117
    size_t n_floats() const { return 7ull * width * height; }
};

// What every integrator's session holds (pt, aov, gpt, mcmc_opt): made by base_begin, ended by base_end (api_pt.cpp).
struct RenderBase {
    akr_context* ctx = nullptr;
    akr_scene* scene = nullptr;
    akr_film* film = nullptr;
    akr_pt_config cfg;
    DevBuf states, counters;
    TileGrid grid;             // the frame's tiles and this rank's share of them
    DevBuf owned_tiles;        // shard_count > 1: PtParams.owned_tiles
    uint32_t spp_done = 0, n_launches = 0;
    uint32_t pmj_spp = 1;  // the spp the pmj02bn sampler stratifies for (the method's total spp)
    const akr_scene::ColorSet* color_set = nullptr;  // the scene's tables for cfg.color != 0 (api_pt.cpp color_set, under the scene's lock)
    // the process-wide tuning options as they were when the session began (base_begin; akr_pt_begin_features: before its refusals): the one
    // state every decision of the session's life is made from -- an akr_option_set on another thread cannot give a session two
    TuningOptions opt;
    // timed regions on the context's stream: pairs still in flight, and the elapsed time of the completed ones (folded in and
    // destroyed as they complete, so a long progressive session holds a bounded number of events)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double kernel_ms = 0.0;
    PtVariant variant{};  // which instantiation of the pt kernel the session runs (session_params; kernels.h)
    PtParams params;  // the session's constant block (session_params); a launch sets n_passes / last_pass_spp (set_launch_passes)
    bool holds_scene = false;  // counted in scene->sessions (base_begin)
    // a pt session begun by akr_pt_begin_features: the two guide films its FEAT kernels accumulate into; else null
    akr_film *feat_albedo = nullptr, *feat_normal = nullptr;
    void fold_events(bool all) {  // all: the stream has been synchronised
        size_t keep = 0;
        for (size_t i = 0; i < pending.size(); i++) {
            auto& ev = pending[i];
            if (all || hipEventQuery(ev.second) == hipSuccess) {
                float t = 0.0f;
                if (hipEventElapsedTime(&t, ev.first, ev.second) == hipSuccess) kernel_ms += t;
                (void)hipEventDestroy(ev.first);
                (void)hipEventDestroy(ev.second);
            } else {
                pending[keep++] = ev;
            }
        }
        pending.resize(keep);
    }
    virtual ~RenderBase() {
        if (holds_scene) scene->sessions--;
        for (auto& ev : pending) {
            (void)hipEventDestroy(ev.first);
            (void)hipEventDestroy(ev.second);
        }
    }
};

// Which kernel a pt session of (scene, config) runs and which tables it stages in LDS: the ONE place that decides it (pt_plan.cpp pt_plan), from the
// compiled scene, the config and the options a session snapshots -- never from device pointers, so it answers for a host-only scene too.
struct PtPlan {
    PtVariant v;
    uint32_t simple_scene, defer_metal, defer_flags;  // PtParams' fields of these names
    uint32_t stage_bytes[ST_COUNT], stage_total, tex_slots;
    bool cost_order;  // the session's megakernel launches may deal their items by measured pixel cost (PtRoute::record_costs)
};
// What kind of session akr_pt_begin / akr_pt_begin_features make of (scene, config, options): the ONE place that decides it (pt_plan.cpp pt_route).
struct PtRoute {
    std::string refusal;  // not empty: no session; this message with AKR_ERR_UNSUPPORTED, and nothing below is filled in
    bool wavefront = false;  // the wavefront schedule renders the session from its beginning ...
    bool wf_sort = false;    // ... with sorted queues (option wf_sort): PtParams.wf_sort, the queues' keys
    bool relaxed = false;    // option arith = 1 and the session is one the relaxed tier covers: launches go to pt_kernels_relaxed.hip
    // per-scene kernel (host/specialise.cpp): asked for -- which also shapes the plan --, for spec_waves waves per SIMD, compiled on a cache miss only if may_compile
    bool spec = false, may_compile = false;
    int spec_waves = 3;
    std::string status;  // akr_pt_kernel_info's text, until a per-scene kernel's own status or a timed trial's result takes its place
    bool sched_trial = false;   // the first blocking akr_pt_passes call may time both schedules and keep the faster (option sched_trial)
    bool record_costs = false;  // its megakernel launches record item costs and then deal items by them (CostOrder)
    PtPlan plan{};  // for those choices
};

// wavefront schedule (wf_kernels.hip): path state SoA + ray queues. A pt session holds one only while that schedule renders it.
struct WavefrontState {
    DevBuf state, queues, ctrl, pend, carry;
    // option wf_sort: keys of the queue entries, the sorted copies the trace kernel reads, rocPRIM's scratch
    bool sort = false;
    DevBuf keys, sorted, sort_tmp;
    uint32_t *sorted_closest = nullptr, *sorted_shadow = nullptr, *sorted_keys = nullptr;
    WfBuffers buf;
    uint32_t slots = 0, trace_blocks = 0;
    // slot groups (option wf_groups; wf_schedule.cpp wf_run): each with its own queues, counters and stream
    std::vector<WfBuffers> group;
    std::vector<hipStream_t> streams;
    std::vector<hipEvent_t> join;
    hipEvent_t fork = nullptr;
    ~WavefrontState() {
        for (hipStream_t st : streams) (void)hipStreamDestroy(st);
        for (hipEvent_t ev : join) (void)hipEventDestroy(ev);
        if (fork) (void)hipEventDestroy(fork);
    }
};

// Work items ordered by measured pixel cost, where the route records costs. State 1: a megakernel launch stores every item's closest-hit
// rays in item_cost (params.item_cost); the first launch after one that recorded sorts the items by it into item_pixels (params.item_pixels), on the stream;
// then 2: recording stops, later launches deal from the table. 0: off -- not routed so, another schedule took the session over, or an active-tile list.
struct CostOrder {
    int state = 0;
    bool recorded = false;  // a launch has written item_cost
    DevBuf item_cost, item_pixels, keys, keys_sorted, sort_tmp;  // (the last three: the sort's scratch, released once it has run)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // around the sort (test hook: its one-time cost)
    float sort_ms = 0.0f;
    ~CostOrder() {  // (not copyable: its DevBufs are not)
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

// The pt integrator's session: the base plus what only k_pt_pass and the wavefront schedule need. The other integrators hold a plain
// RenderBase, so a per-scene kernel's parameter block (no graph value slots in LDS) cannot reach their kernels.
struct akr_pt_session : RenderBase {
    PtRoute route;  // what akr_pt_begin decided (pt_route); route.spec: the per-scene kernel compiled and `spec` launches
    std::unique_ptr<WavefrontState> wf;  // set = the wavefront schedule renders the session
    int sched_trial = 0;  // 1 = route.sched_trial and still to run: the first blocking akr_pt_passes call times both schedules and keeps the faster (api_pt.cpp), 2 = done
    uint64_t passes_launched = 0;  // passes of all akr_pt_passes launches so far (kernel_ms / passes_launched = what a pass costs)
    std::shared_ptr<SpecKernel> spec;
    std::string spec_status = "not requested";
    // akr_pt_set_active_tiles: the list the passes render instead of the session's own tiles (params.owned_tiles points at it, params.shard_count
    // is at least 2 so that item_to_pixel reads it, params.n_items counts its pixels); room for every tile of the grid, allocated at the first call
    DevBuf active_tiles;
    bool active_set = false;
    CostOrder cost;
};

namespace akr_api {
// wf_schedule.cpp: the wavefront schedule's host half. Every option it reads is of se->opt.
std::unique_ptr<WavefrontState> wf_allocate(const akr_pt_session* se, bool sort);  // the buffers: a slot per item of the session's parameter block
void wf_set_range(WavefrontState& ws, uint32_t n_active);  // the groups' shares of the slots [0, n_active)
void wf_run(akr_pt_session* se);  // one launch group: the passes set_launch_passes set, for every slot
// One timed region on a session's stream. The event pair is handed to the session by stop(); if the region is left by an
// exception the pair is destroyed here.
struct LaunchTimer {
    RenderBase* se;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    explicit LaunchTimer(RenderBase* s) : se(s) {
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        HIP_CHECK(hipEventRecord(e0, se->ctx->stream));
    }
    LaunchTimer(const LaunchTimer&) = delete;
    LaunchTimer& operator=(const LaunchTimer&) = delete;
    void stop() {
        HIP_CHECK(hipEventRecord(e1, se->ctx->stream));
        se->pending.emplace_back(e0, e1);
        e0 = e1 = nullptr;
        if (se->pending.size() > 16) se->fold_events(false);
    }
    ~LaunchTimer() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

// api_pt.cpp
// What all four integrators begin with: the config validated, the film's size checked, the colour set, sampler states, counters, the
// owned-tile list, the scene reference. Throws; the caller then computes the session's parameter block (session_params).
// opt: the snapshot the caller has already taken and decided from (akr_pt_begin_features); null = taken here.
void base_begin(RenderBase* se, akr_context* ctx, akr_scene* scene, const akr_pt_config* cfg, akr_film* film, const TuningOptions* opt = nullptr);
// base_begin + the block every integrator but pt renders with, behind the C ABI's error boundary (aov, gpt, mcmc_opt)
int32_t render_begin(akr_context* ctx, akr_scene* scene, const akr_pt_config* cfg, akr_film* film, RenderBase** out);
int32_t base_end(RenderBase* se, akr_pt_stats* stats);  // the stats read back, the session deleted (the scene released)
// The session's kernel parameter block, computed once: everything but the two fields of set_launch_passes is constant while the
// session lives (n_passes = 1 full pass until a launch says otherwise). plan: a pt session's (its route's); null = the plan of a session without
// per-scene kernel, guides and cost order, which is every other integrator's.
void session_params(RenderBase* se, const PtPlan* plan = nullptr);
inline void set_launch_passes(RenderBase* se, uint32_t n_passes, uint32_t last_pass_spp) {
    se->params.n_passes = n_passes;
    se->params.last_pass_spp = last_pass_spp;
}
// pt_plan.cpp
// feat: the session collects the denoiser's guides (akr_pt_begin_features): the FEAT kernels, which exclude DEFER and SIMPLE as ENV and LENS do.
// opt: defer_metal, simple_kernels, defer_on. cost_order: the mode below.
PtPlan pt_plan(const akr_scene* s, const akr_pt_config& c, const TuningOptions& opt, bool spec_active, int spec_waves, bool feat = false, int cost_order = 1);
// Whether pt sessions order their work items by measured pixel cost: 0 never, 1 where pt_plan's rule says it pays (the library's behaviour),
// 2 every megakernel session. Process-wide, read once per session by akr_pt_begin. It is not a row of the option table (host/options.cpp): results do
// not depend on it, and only the test hook akr_probe_pt_cost_order_mode sets it, for tests and measurements.
int cost_order_mode();
int cost_order_mode_set(int mode);  // returns the previous mode; values outside 0..2 are ignored
// the part of the variant that is a fact of the scene and the config: bvh, fd, tex, pmj, inst, env, lens, punct
PtVariant pt_scene_facts(const akr_scene* s, const akr_pt_config& c);
// The route of a pt session: t = its snapshot of the options, grid = its tiles, feat = it collects guides, cost_order = the mode above, spec_possible =
// false once the per-scene kernel asked for has failed to compile. Reads no device pointer; an unvalidated config does no harm (the test hooks).
PtRoute pt_route(const akr_scene* s, const akr_pt_config& c, const TuningOptions& t, const TileGrid& grid, bool feat, int cost_order, bool spec_possible = true);
// pt_route's refusals that are facts of scene and options alone ("" = none): punctual lights, guides. akr_pt_begin reports them before it has looked at its
// other arguments, so it asks ahead of the route (whose refusal they also are); the relaxed tier's two come with the route, after those checks.
std::string pt_route_refusal(const akr_scene* s, const TuningOptions& t, bool feat);
// DScene.bvh_stack_depth / n_nodes of a compiled scene (scene_finish fills them in; a host-only scene has no DScene)
inline uint32_t scene_stack_depth(const CompiledScene& cs) {
    // one pending group per tree level at most (disect.h); a kept scene: two levels + the three words that remember the TLAS position
    // (dinst_trav.h; scene_inst.cpp checked the bound)
    return cs.instanced.on ? cs.bvh_depth : std::max(1u, std::min(cs.bvh_depth, kBvhStackDepth));
}
inline uint32_t scene_n_nodes(const CompiledScene& cs) { return (uint32_t)((cs.instanced.on ? cs.instanced.nodes.size() : cs.bvh_nodes.size()) / kBvhNodeWords); }
// the camera part of a parameter block: r2c, c2w, c2w_identity, width, height, filter, lens
void camera_params(PtParams& p, const akr_scene* s, uint32_t filter_type, float filter_radius);
// Ends a session after `rc`, the status of what ran in it: the first error and its message are what the caller sees.
template <typename End>
int32_t end_keeping_first_error(int32_t rc, End&& end) {
    const std::string err = g_last_error;
    const int32_t rc2 = end();
    if (rc == AKR_OK) return rc2;
    g_last_error = err;
    return rc;
}
uint32_t session_samples(const akr_pt_config& c);
// the tiles (row-major ids) rank `rank` of `count` owns, in Morton order (kernels.h tile_owner)
std::vector<uint32_t> owned_tiles(uint32_t tiles_x, uint32_t tiles_y, uint32_t rank, uint32_t count);
// api_scene.cpp
void scene_finish(akr_scene* s, const TuningOptions& opt);  // opt: the snapshot akr_scene_create / akr_scene_load took
// the light tables packed as the kernels read them (dgeom.h AliasPacked, dscene.h LightRec): what upload_lights uploads and akr_host_light_sample samples
void packed_light_tables(const CompiledScene& cs, std::vector<AliasPacked>& light_alias, std::vector<AliasPacked>& area_alias, std::vector<LightRec>& lights);
// api_aux.cpp: shard_count > 1 = this rank's share (akr_mcmc_render_shard); on_pass: akr_render_task's progress hook
int32_t mcmc_render_impl(akr_context* ctx, akr_scene* scene, const akr_mcmc_config* cfg, akr_film* film, akr_mcmc_result* result, uint32_t* chain_states,
                         akr_pt_stats* stats, const std::function<void(uint32_t, double)>& on_pass, uint32_t shard_rank = 0, uint32_t shard_count = 1,
                         akr_mcmc_partial* partial = nullptr);
}  // namespace akr_api
