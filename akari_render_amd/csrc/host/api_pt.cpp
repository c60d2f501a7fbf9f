// api_pt.cpp -- the `pt` integrator: kernel parameters, the base session, the pt sessions and their per-scene kernels (C ABI of libakari_hip.so,
// include/akari_hip.h; shared internals: api_internal.h; what a session is routed to and what its launches run: pt_plan.cpp; the wavefront
// schedule's host half: wf_schedule.cpp)
#include "api_internal.h"

void akr_api::camera_params(PtParams& p, const akr_scene* s, uint32_t filter_type, float filter_radius) {
    std::memcpy(p.r2c, s->r2c, 64);
    std::memcpy(p.c2w, s->c2w, 64);
    p.c2w_identity = s->c2w_identity;
    p.width = s->flat.camera.width;
    p.height = s->flat.camera.height;
    p.filter_type = filter_type;
    p.filter_radius = filter_radius;
    p.lens_radius = s->flat.lens.radius;  // > 0: the LENS kernels (device/dpath.h generate_ray_lens_from)
    p.lens_focal = s->flat.lens.focal_distance;
    // the projection: anything but perspective runs the LENS kernels too; the panorama's window folded, each value rounded once
    const HostProjection& pr = s->flat.projection;
    p.projection = pr.type;
    p.pano_lon0 = pr.lon_min;
    p.pano_dlon = pr.lon_max - pr.lon_min;
    p.pano_lat1 = pr.lat_max;
    p.pano_dlat = pr.lat_max - pr.lat_min;
    p.pano_inv_w = 1.0f / (float)s->flat.camera.width;
    p.pano_inv_h = 1.0f / (float)s->flat.camera.height;
}
void akr_api::session_params(RenderBase* se, const PtPlan* pt) {
    PtParams& p = se->params;
    const akr_scene* s = se->scene;
    const akr_pt_config& c = se->cfg;
    std::memset(&p, 0, sizeof p);
    p.sc = s->dscene;
    camera_params(p, s, c.filter_type, c.filter_radius);
    p.max_depth = c.max_depth;
    p.rr_depth = c.rr_depth;
    p.use_nee = c.use_nee;
    p.indirect_only = c.indirect_only;
    p.force_diffuse = c.force_diffuse;
    p.debug_depth = c.debug_depth;
    p.pixel_offset[0] = c.pixel_offset[0];
    p.pixel_offset[1] = c.pixel_offset[1];
    p.pass_spp = c.spp_per_pass;
    set_launch_passes(se, 1, c.spp_per_pass);
    p.start = pcg_start_constants();
    p.states = se->states.as<Pcg32>();
    p.film = se->film->data;
    p.counters = se->counters.as<uint64_t>();
    p.color = c.color;
    p.sc.tex.color = c.color;
    if (c.color != 0) se->color_set->apply(s->cs, p.sc);  // the tables of this pipeline (color_set)
    p.sampler = c.sampler_type;
    if (c.sampler_type == AKR_SAMPLER_PMJ02BN || c.sampler_type == AKR_SAMPLER_SOBOL) {  // Pmj02BnSamplerCreator::new (sampler/mod.rs:376-395)
        p.smp_seed = (uint32_t)c.sampler_seed;
        p.smp_spp = se->pmj_spp;
        uint32_t w = se->pmj_spp - 1;
        w |= w >> 1; w |= w >> 2; w |= w >> 4; w |= w >> 8; w |= w >> 16;
        p.smp_w = w;
        p.smp_mod_magic = fastmod_magic(se->pmj_spp);
        if (c.sampler_type == AKR_SAMPLER_PMJ02BN) {  // the sobol sampler computes its points, no tables
            p.pmj_sets = se->ctx->pmj_sets.as<uint32_t>();
            p.bluenoise = se->ctx->bluenoise.as<uint16_t>();
        }
    }
    {   // which kernel, which tables staged in LDS: decided from the scene and the config (pt_plan), kept with the session
        const PtPlan plan = pt ? *pt : pt_plan(s, c, se->opt, false, 3, false, /*cost_order=*/0);
        se->variant = plan.v;
        std::memcpy(p.stage_bytes, plan.stage_bytes, sizeof p.stage_bytes);
        p.stage_total = plan.stage_total;
        p.tex_slots = plan.tex_slots;
        p.simple_scene = plan.simple_scene;
        p.defer_metal = plan.defer_metal;
        p.defer_flags = plan.defer_flags;
    }
    for (int a = 0; a < 3; a++) {  // the sort key's grid (PtParams.wf_sort itself: akr_pt_begin): 128 cells per axis over the scene's box
        const float lo = s->cs.scene_lo[a], ext = s->cs.scene_hi[a] - s->cs.scene_lo[a];
        p.sort_lo[a] = lo;
        p.sort_scale[a] = ext > 0.0f ? 128.0f / ext : 0.0f;
    }
    p.shard_rank = c.shard_count > 1 ? c.shard_rank : 0;
    p.shard_count = c.shard_count > 1 ? c.shard_count : 1;
    p.tile_w = se->grid.tile_w;
    p.tile_h = se->grid.tile_h;
    p.tiles_x = se->grid.tiles_x;
    p.tiles_y = se->grid.tiles_y;
    p.owned_tiles = se->owned_tiles.as<uint32_t>();  // (null unless shard_count > 1: base_begin)
    p.n_items = se->grid.n_items;
    p.feat_albedo = se->feat_albedo ? se->feat_albedo->data : nullptr;
    p.feat_normal = se->feat_normal ? se->feat_normal->data : nullptr;
}
std::vector<uint32_t> akr_api::owned_tiles(uint32_t tiles_x, uint32_t tiles_y, uint32_t rank, uint32_t count) {
    std::vector<std::pair<uint32_t, uint32_t>> mine;  // (Morton code, tile)
    for (uint32_t ty = 0; ty < tiles_y; ty++)
        for (uint32_t tx = 0; tx < tiles_x; tx++)
            if (tile_owner(tx, ty, count) == rank) mine.emplace_back(tile_morton(tx, ty), ty * tiles_x + tx);
    std::sort(mine.begin(), mine.end());
    std::vector<uint32_t> out;
    out.reserve(mine.size());
    for (const auto& m : mine) out.push_back(m.second);
    return out;
}

static void read_stats(RenderBase* se, akr_pt_stats* stats);

// A session's items dealt by position from now on: another schedule took it over, or it renders an active-tile list.
static void cost_order_drop(akr_pt_session* se) {
    se->cost.state = 0;
    se->params.item_cost = nullptr;
    se->params.item_pixels = nullptr;
}
// Before a megakernel launch of a session in state 1 whose earlier launch recorded: the table from the costs so far, on the stream (no
// host synchronisation: the launch before wrote item_cost, the launches after read item_pixels, all in stream order).
static void cost_order_build(akr_pt_session* se) {
    PtParams& p = se->params;
    CostOrder& co = se->cost;
    const uint32_t n_padded = (p.n_items + 255u) & ~255u;
    co.item_pixels.alloc((size_t)n_padded * sizeof(uint32_t));
    co.keys.alloc((size_t)n_padded * sizeof(uint64_t));
    co.keys_sorted.alloc((size_t)n_padded * sizeof(uint64_t));
    co.sort_tmp.alloc(std::max<size_t>(16, cost_order_temp_bytes(n_padded)));
    HIP_CHECK(hipEventCreate(&co.ev0));
    HIP_CHECK(hipEventCreate(&co.ev1));
    HIP_CHECK(hipEventRecord(co.ev0, se->ctx->stream));
    HIP_CHECK(launch_cost_order(p, n_padded, co.keys.as<uint64_t>(), co.keys_sorted.as<uint64_t>(), co.sort_tmp.p, co.sort_tmp.bytes, co.item_pixels.as<uint32_t>(), se->ctx->stream));
    HIP_CHECK(hipEventRecord(co.ev1, se->ctx->stream));
    p.item_pixels = co.item_pixels.as<uint32_t>();
    p.item_cost = nullptr;  // one sort per session: nothing reads later costs
    co.state = 2;
}

static void validate_config(const akr_pt_config& c, const TileGrid& grid) {
    if (c.spp_per_pass == 0) throw std::invalid_argument("akr_pt_config: spp_per_pass must be > 0");
    if (c.filter_type > AKR_FILTER_GAUSSIAN) throw std::invalid_argument("akr_pt_config: unknown filter_type");
    if (c.sampler_type > AKR_SAMPLER_SOBOL) throw std::invalid_argument("akr_pt_config: unknown sampler_type");
    if (c.color > (AKR_COLOR_REPR_ACESCG | AKR_COLOR_RGB_ACESCG)) throw std::invalid_argument("akr_pt_config: unknown colour pipeline bits");
    if (c.sampler_type == AKR_SAMPLER_PMJ02BN && c.spp > 65536u)
        throw std::invalid_argument("Pmj02BnSampler supports up to 65536 spp (sampler/mod.rs:381-387)");
    if ((grid.tile_w % 8) || (grid.tile_h % 8)) throw std::invalid_argument("akr_pt_config: tile_w and tile_h must be multiples of 8");
    if (c.shard_count > 1 && c.shard_rank >= c.shard_count) throw std::invalid_argument("akr_pt_config: shard_rank >= shard_count");
    if (c.sample_begin != 0 || c.sample_count != 0) {  // sample-range split (akari_hip.h)
        if (c.sampler_type != AKR_SAMPLER_PMJ02BN && c.sampler_type != AKR_SAMPLER_SOBOL)
            throw Unsupported("akr_pt_config: a sample range needs an index-based sampler (pmj02bn, sobol): the independent sampler's start() advances the pixel's "
                              "PCG stream from wherever the previous sample stopped (sampler/mod.rs:115-131,192-203), sample s cannot be drawn without samples 0 .. s-1");
        if (c.sample_count == 0) throw std::invalid_argument("akr_pt_config: sample_begin without sample_count");
        if ((uint64_t)c.sample_begin + c.sample_count > c.spp) throw std::invalid_argument("akr_pt_config: sample range exceeds spp");
    }
}
// samples the session renders: the configured range, or all spp of the render
uint32_t akr_api::session_samples(const akr_pt_config& c) { return c.sample_count ? c.sample_count : c.spp; }

extern "C" {

AKR_API int32_t akr_pt_config_default(akr_pt_config* c) {
    if (!c) return fail(AKR_ERR_INVALID_ARGUMENT, "config is NULL");
    std::memset(c, 0, sizeof *c);
    c->spp = 256; c->max_depth = 7; c->rr_depth = 5; c->spp_per_pass = 64;  // pt.rs:930-944
    c->use_nee = 1; c->indirect_only = 0; c->force_diffuse = 0;
    c->debug_depth = -1;
    c->filter_type = AKR_FILTER_GAUSSIAN; c->filter_radius = 1.5f;          // film.rs:50-54
    c->sampler_type = AKR_SAMPLER_INDEPENDENT; c->sampler_seed = 0;         // sampler/mod.rs:290-294
    c->shard_rank = 0; c->shard_count = 1; c->tile_w = 32; c->tile_h = 32;
    return AKR_OK;
}
AKR_API int32_t akr_pt_config_from_json(const char* text, akr_pt_config* cfg, char* film_out, uint32_t film_out_len) {
    if (!text || !cfg) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_pt_config_from_json: NULL argument");
    return guarded([&] {
        std::string out;
        parse_method_json(text, cfg, &out);
        if (film_out && film_out_len) std::snprintf(film_out, film_out_len, "%s", out.c_str());
    });
}

}  // extern "C"
// The scene's tables under the colour pipeline `color` != 0 (akr_scene::ColorSet), under the scene's lock from the lookup to the answer: made by the first
// session of that pipeline, the punctual lights' records again after the lights changed (api_scene.cpp punctual_lights_changed drops them). The pointer is
// stable: the map owns the set through a unique_ptr and never removes it.
static const akr_scene::ColorSet* color_set(akr_scene* scene, uint32_t color) {
    std::lock_guard<std::mutex> lock(scene->color_sets_mutex);
    auto it = scene->color_sets.find(color);
    if (it == scene->color_sets.end()) {
        // ColorPipeline other than sRGB / sRGB: the scene's constants were folded for the default pipeline; fold them again
        // for this one (svm/texture/mod.rs:9-43 at every Rgb / spectral_uplift node)
        CompiledScene tmp;
        tmp.images = scene->cs.images;
        std::vector<akr_material_desc> descs;
        compile_materials(scene->flat, color, tmp, descs);
        auto set = std::make_unique<akr_scene::ColorSet>();
        set->materials.upload(tmp.materials);
        if (tmp.has_textures) {
            set->tex_nodes.upload(tmp.tex_nodes);
            set->mat_inputs.upload(tmp.mat_inputs);
        }
        it = scene->color_sets.emplace(color, std::move(set)).first;
    }
    akr_scene::ColorSet& set = *it->second;
    if (!scene->cs.punct.empty() && !set.punct.p) {
        std::vector<DPunct> recs;
        for (const akr_punctual_light_desc& d : scene->flat.punct) recs.push_back(fold_punctual(d, color));
        set.punct.upload(punctual_device_records(recs, scene->cs.punct_tree));  // (the tree's nodes are the same in every set)
    }
    return &set;
}
// The aov / gpt / mcmc_opt integrators begin here as well, for sampler states, counters and the kernel parameter block, but launch their own
// kernels, which interpret shader graphs. They hold a RenderBase and not a pt session, so a per-scene kernel's block cannot reach them.
void akr_api::base_begin(RenderBase* se, akr_context* ctx, akr_scene* scene, const akr_pt_config* cfg, akr_film* film, const TuningOptions* opt) {
    if (!ctx || !scene || !cfg || !film) throw std::invalid_argument("akr_pt_begin: NULL argument");
    if (scene->ctx != ctx) throw std::invalid_argument("akr_pt_begin: the scene was not created on this context (host-only scenes cannot render)");
    se->grid = tile_grid(cfg->tile_w, cfg->tile_h, scene->flat.camera.width, scene->flat.camera.height, cfg->shard_rank, cfg->shard_count);
    validate_config(*cfg, se->grid);
    if (film->width != scene->flat.camera.width || film->height != scene->flat.camera.height)
        throw std::invalid_argument("film resolution does not match the scene camera (pt.rs:1072-1073)");
    ctx->bind();
    se->ctx = ctx;
    se->scene = scene;
    se->film = film;
    se->cfg = *cfg;
    if (cfg->color != 0) se->color_set = color_set(scene, cfg->color);
    const uint64_t n = (uint64_t)film->width * film->height;
    // init_pcg32_buffer_with_seed (sampler/mod.rs:148-160): host StdRng(seed) u64 per pixel, device new_seq_offset
    if (cfg->sampler_type == AKR_SAMPLER_PMJ02BN || cfg->sampler_type == AKR_SAMPLER_SOBOL) {
        // Pmj02BnState per pixel (sampler/mod.rs:451-466): sample_index = u32::MAX, pixel = (x, y), kept in a Pcg32 slot
        if (cfg->sampler_type == AKR_SAMPLER_PMJ02BN) ctx->ensure_pmj_tables();
        se->pmj_spp = cfg->spp ? cfg->spp : 1;
        std::vector<Pcg32> init(n);
        // a sample range [b, ..) starts with sample_index = b - 1: the next start() makes it b (sampler/mod.rs:650-663)
        const uint64_t first = cfg->sample_begin ? (uint64_t)(cfg->sample_begin - 1u) : 0xffffffffull;
        for (uint64_t i = 0; i < n; i++) init[i] = Pcg32{first, (i % film->width) | ((i / film->width) << 32)};
        se->states.upload(init);
    } else {
        std::vector<uint64_t> seeds(n);
        StdRng rng(cfg->sampler_seed);
        for (auto& v : seeds) v = rng.next_u64();
        DevBuf dseeds;
        dseeds.upload(seeds);
        se->states.alloc(n * sizeof(Pcg32));
        HIP_CHECK(launch_init_pcg32(dseeds.as<uint64_t>(), se->states.p, n, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));  // dseeds goes out of scope
    }
    se->counters.alloc(8 * kStatStripes * sizeof(uint64_t));
    HIP_CHECK(hipMemsetAsync(se->counters.p, 0, se->counters.bytes, ctx->stream));
    if (cfg->shard_count > 1) se->owned_tiles.upload(owned_tiles(se->grid.tiles_x, se->grid.tiles_y, cfg->shard_rank, cfg->shard_count));
    se->opt = opt ? *opt : tuning();  // the session's one look at the options
    scene->sessions++;
    se->holds_scene = true;
}
int32_t akr_api::render_begin(akr_context* ctx, akr_scene* scene, const akr_pt_config* cfg, akr_film* film, RenderBase** out) {
    *out = nullptr;
    return guarded([&] {
        auto se = std::make_unique<RenderBase>();
        base_begin(se.get(), ctx, scene, cfg, film);
        session_params(se.get());
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        *out = se.release();
    });
}
// akr_pt_begin, and with the two guide films akr_pt_begin_features: the session is routed (pt_route), refused if the route refuses, and the route carried out
static int32_t pt_begin(akr_context* ctx, akr_scene* scene, const akr_pt_config* cfg, akr_film* film, akr_film* albedo, akr_film* normal, const TuningOptions& t, akr_pt_session** out) {
    *out = nullptr;
    return guarded([&] {
        auto se = std::make_unique<akr_pt_session>();
        const bool features = albedo != nullptr;
        if (scene) {  // what the scene or the guides cannot do under these options, before a byte is allocated ...
            const std::string why = pt_route_refusal(scene, t, features);
            if (!why.empty()) throw Unsupported(why);
        }
        base_begin(se.get(), ctx, scene, cfg, film, &t);
        se->feat_albedo = albedo;
        se->feat_normal = normal;
        const int cost_mode = cost_order_mode();
        PtRoute& r = se->route = pt_route(scene, *cfg, t, se->grid, features, cost_mode);
        if (!r.refusal.empty()) throw Unsupported(r.refusal);  // ... and what the relaxed tier cannot, once the arguments have been checked
        if (r.spec) {  // the route's variant, compiled with the scene's graphs
            std::unique_lock<std::mutex> lock(scene->spec_mutex);
            if (!scene->spec_header_made) scene->spec_header = generate_scene_spec(scene->cs);
            scene->spec_header_made = true;
            lock.unlock();
            se->spec = ctx->spec_cache.get(scene->spec_header, r.plan.v, r.spec_waves, ctx->props.gcnArchName, r.may_compile);
            if (!se->spec->fn) r = pt_route(scene, *cfg, t, se->grid, features, cost_mode, /*spec_possible=*/false);  // the interpreter kernel renders the same film: value slots in LDS, its own LDS budget
        }
        se->spec_status = se->spec ? se->spec->status : r.status;
        session_params(se.get(), &r.plan);
        se->params.wf_sort = r.wf_sort ? 1u : 0u;
        if (r.wavefront) se->wf = wf_allocate(se.get(), r.wf_sort);
        if (r.record_costs) {
            se->cost.item_cost.alloc((size_t)((se->grid.n_items + 255u) & ~255u) * sizeof(uint32_t));  // (a launch's whole grid writes)
            if (se->cost.item_cost.p) HIP_CHECK(hipMemsetAsync(se->cost.item_cost.p, 0, se->cost.item_cost.bytes, ctx->stream));
            se->params.item_cost = se->cost.item_cost.as<uint32_t>();
            se->cost.state = 1;
        }
        se->sched_trial = r.sched_trial ? 1 : 0;
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        *out = se.release();
    });
}
extern "C" {
AKR_API int32_t akr_pt_begin(akr_context* ctx, akr_scene* scene, const akr_pt_config* cfg, akr_film* film, akr_pt_session** out) {
    if (!out) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_pt_begin: NULL argument");
    return pt_begin(ctx, scene, cfg, film, nullptr, nullptr, tuning(), out);
}
// A pt session whose kernels also accumulate the denoiser's guides (include/akari_hip.h). Everything it cannot do is refused
// here or at the head of pt_begin, before a byte is allocated or written.
AKR_API int32_t akr_pt_begin_features(akr_context* ctx, akr_scene* scene, const akr_pt_config* cfg, akr_film* film, akr_film* albedo, akr_film* normal, akr_pt_session** out) {
    if (!out) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_pt_begin_features: NULL argument");
    *out = nullptr;
    if (!ctx || (scene && !scene->ctx))
        return fail(AKR_ERR_UNSUPPORTED, "unsupported: akr_pt_begin_features: guides are collected by GPU kernels; a host-only scene (no device context) cannot render them");
    if (!scene || !cfg || !film) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_pt_begin_features: NULL argument");
    if (!albedo || !normal) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_pt_begin_features: both guide films are required (albedo and normal)");
    if (albedo == normal || albedo == film || normal == film) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_pt_begin_features: film, albedo and normal must be three different films");
    for (const akr_film* g : {albedo, normal}) {
        if (g->ctx != ctx) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_pt_begin_features: a guide film belongs to another context");
        if (g->width != scene->flat.camera.width || g->height != scene->flat.camera.height)
            return fail(AKR_ERR_INVALID_ARGUMENT, "akr_pt_begin_features: a guide film's resolution does not match the scene camera");
    }
    return pt_begin(ctx, scene, cfg, film, albedo, normal, tuning(), out);
}
AKR_API int32_t akr_pt_passes(akr_pt_session* se, uint32_t n_passes, int32_t blocking, uint32_t* spp_done) {
    if (!se) return fail(AKR_ERR_INVALID_ARGUMENT, "session is NULL");
    return guarded([&] {
        se->ctx->bind();
        // the passes requested (each min(spp - cnt, spp_per_pass) samples, pt.rs:1127) are fused into launches
        // of at most kMaxFusedPasses passes: 16, or -- once the session knows what a pass costs, i.e. when every earlier launch has
        // completed (a progressive render, a warm-up) -- as many as fit in about three seconds of kernel time, up to 64. The waves of
        // a launch do not finish together; fewer, longer launches spend less of a render in those tails (C2: +1.2 % at 64 passes,
        // profiles/r4_ab_walk.txt). The bound keeps a launch on a heavy scene from running for minutes.
        uint32_t kMaxFusedPasses = 16;
        se->fold_events(false);
        if (se->cost.state == 2 && se->cost.keys.p && se->pending.empty()) {  // the sort has run: its scratch goes
            se->cost.keys.release();
            se->cost.keys_sorted.release();
            se->cost.sort_tmp.release();
        }
        if (se->opt.max_fused_passes > 0) {
            kMaxFusedPasses = (uint32_t)se->opt.max_fused_passes;  // option max_fused_passes: a fixed bound (deterministic launch counts)
        } else if (blocking && se->pending.empty() && se->passes_launched > 0 && se->kernel_ms > 0.0) {
            // (blocking calls only: a progressive caller that polls between non-blocking calls is not put behind multi-second launches)
            const double per_pass_ms = se->kernel_ms / (double)se->passes_launched;
            const double fit = 3000.0 / per_pass_ms;
            kMaxFusedPasses = fit >= 64.0 ? 64u : (fit <= 16.0 ? 16u : (uint32_t)fit);
        }
        uint32_t left = n_passes;
        const uint32_t total = session_samples(se->cfg);
        auto launch = [&](uint32_t max_fused) {  // one launch (group) of up to max_fused of the passes left
            uint32_t fused = 0, last = 0, done = se->spp_done;
            while (fused < max_fused && fused < left && done < total) {
                last = std::min(total - done, se->cfg.spp_per_pass);
                done += last;
                fused++;
            }
            set_launch_passes(se, fused, last);
            LaunchTimer timer(se);
            if (se->active_set && se->params.n_items == 0) {}  // an empty active-tile list: the passes are counted, nothing runs
            else if (se->wf) {
                if (se->cost.state) cost_order_drop(se);  // (a timed trial handed the session to the other schedule)
                wf_run(se);
            } else {
                if (se->cost.state == 1 && se->cost.recorded && se->params.n_items > 0) cost_order_build(se);
                se->cost.recorded = se->cost.recorded || se->cost.state == 1;
                HIP_CHECK(launch_pt_pass(se->params, se->variant, se->ctx->stream, se->route.spec ? se->spec->fn : nullptr, se->route.relaxed));
            }
            timer.stop();
            se->spp_done = done;
            se->n_launches++;
            se->passes_launched += fused;
            left -= fused;
        };
        if (se->sched_trial == 1 && blocking && left >= 4 && total - se->spp_done >= 4 * se->cfg.spp_per_pass) {  // (pt_route)
            se->sched_trial = 2;
            auto timed = [&](double& ms_per_sample, double& shaded_per_closest) {  // two passes under the current schedule
                HIP_CHECK(hipStreamSynchronize(se->ctx->stream));
                akr_pt_stats a, b;
                read_stats(se, &a);
                launch(2);
                read_stats(se, &b);
                ms_per_sample = (b.kernel_ms - a.kernel_ms) / (double)std::max<uint64_t>(1, b.n_samples - a.n_samples);
                shaded_per_closest = (double)(b.n_shaded - a.n_shaded) / (double)std::max<uint64_t>(1, b.n_closest - a.n_closest);
            };
            double mk = 0.0, wf = 0.0, ratio = 0.0, unused = 0.0;
            timed(mk, ratio);
            char msg[200];
            if (ratio >= 0.97 && se->opt.sched_trial != 1) {
                std::snprintf(msg, sizeof msg, "megakernel (no trial of the other schedule: %.3f shaded vertices per closest-hit ray, a closed scene)", ratio);
            } else {
                se->wf = wf_allocate(se, /*sort=*/false);
                timed(wf, unused);
                const bool keep = wf < 0.95 * mk;
                // (a session on the megakernel never says "wavefront": callers tell the schedule by that word)
                std::snprintf(msg, sizeof msg, keep ? "wavefront schedule (timed trial, 2 passes each: %.3g ns per sample against the megakernel's %.3g)"
                                                    : "megakernel (timed trial, 2 passes each: %.3g ns per sample against the other schedule's %.3g)",
                              (keep ? wf : mk) * 1e6, (keep ? mk : wf) * 1e6);
                if (!keep) se->wf.reset();
            }
            se->spec_status = msg;
        }
        while (left > 0 && se->spp_done < total) launch(kMaxFusedPasses);
        if (blocking) HIP_CHECK(hipStreamSynchronize(se->ctx->stream));
        if (spp_done) *spp_done = se->spp_done;
    });
}
// The tiles the session's passes render from now on (include/akari_hip.h). Host only: the kernels already map items through PtParams.owned_tiles
// whenever shard_count > 1 (device/dpath.h item_to_pixel) and read shard_count nowhere else, and film and sampler state are per pixel.
AKR_API int32_t akr_pt_set_active_tiles(akr_pt_session* se, const uint32_t* tiles, uint32_t n) {
    if (!se) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_pt_set_active_tiles: session is NULL");
    return guarded([&] {
        se->ctx->bind();
        PtParams& p = se->params;
        const akr_pt_config& c = se->cfg;
        const uint32_t n_tiles = se->grid.tiles_x * se->grid.tiles_y, tile_px = se->grid.tile_w * se->grid.tile_h;
        const uint32_t count = c.shard_count > 1 ? c.shard_count : 1, rank = c.shard_count > 1 ? c.shard_rank : 0;
        if (tiles) {
            std::vector<uint8_t> seen(n_tiles, 0);
            for (uint32_t j = 0; j < n; j++) {
                const uint32_t t = tiles[j];
                if (t >= n_tiles) throw std::invalid_argument("akr_pt_set_active_tiles: tile " + std::to_string(t) + " is out of range (the grid has " + std::to_string(n_tiles) + " tiles)");
                if (tile_owner(t % se->grid.tiles_x, t / se->grid.tiles_x, count) != rank)
                    throw std::invalid_argument("akr_pt_set_active_tiles: tile " + std::to_string(t) + " is not owned by this session (shard " + std::to_string(rank) + " of " + std::to_string(count) + ")");
                if (seen[t]) throw std::invalid_argument("akr_pt_set_active_tiles: duplicate tile " + std::to_string(t));
                seen[t] = 1;
            }
        }
        HIP_CHECK(hipStreamSynchronize(se->ctx->stream));  // launches in flight read the list
        se->sched_trial = se->sched_trial == 1 ? 0 : se->sched_trial;  // no timed schedule trial for a session that ever set a list
        if (se->cost.state) cost_order_drop(se);  // ... and no cost order: its table is of the session's own tiles, and a list's tiles are few and alike
        if (!tiles) {
            se->active_set = false;
            p.shard_count = count;
            p.owned_tiles = se->owned_tiles.as<uint32_t>();
            p.n_items = se->grid.n_items;
        } else {
            if (!se->active_tiles.p) se->active_tiles.alloc((size_t)std::max(1u, n_tiles) * sizeof(uint32_t));
            if (n) HIP_CHECK(hipMemcpy(se->active_tiles.p, tiles, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
            se->active_set = true;
            p.shard_count = std::max(2u, count);  // item_to_pixel's list branch
            p.owned_tiles = se->active_tiles.as<uint32_t>();
            p.n_items = n * tile_px;
        }
        if (se->wf) wf_set_range(*se->wf, p.n_items);  // (never more than the slots allocated: a subset of the session's tiles)
    });
}
AKR_API int32_t akr_pt_read_sampler_states(akr_pt_session* se, uint64_t* dst) {
    if (!se || !dst) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_pt_read_sampler_states: NULL argument");
    return guarded([&] {
        se->ctx->bind();
        HIP_CHECK(hipStreamSynchronize(se->ctx->stream));
        HIP_CHECK(hipMemcpy(dst, se->states.p, se->states.bytes, hipMemcpyDeviceToHost));
    });
}
// the session's eight counters, summed over their stripes, once everything on its stream has run
static std::array<uint64_t, 8> read_counters(RenderBase* se) {
    se->ctx->bind();
    HIP_CHECK(hipStreamSynchronize(se->ctx->stream));
    std::vector<uint64_t> stripes(8 * kStatStripes);
    HIP_CHECK(hipMemcpy(stripes.data(), se->counters.p, stripes.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    std::array<uint64_t, 8> c{};
    for (uint32_t k = 0; k < kStatStripes; k++)
        for (int i = 0; i < 8; i++) c[i] += stripes[8 * k + i];
    return c;
}
static void read_stats(RenderBase* se, akr_pt_stats* stats) {
    const std::array<uint64_t, 8> c = read_counters(se);
    se->fold_events(true);
    const double ms = se->kernel_ms;
    if (stats) {
        stats->n_samples = c[0];
        stats->n_closest = c[1];
        stats->n_shadow = c[2];
        stats->n_shaded = c[3];
        stats->n_node_visits = c[4];
        stats->n_tri_tests = c[5];
        stats->kernel_ms = ms;
        stats->n_launches = se->n_launches;
        stats->_pad = (uint32_t)c[6];  // non-zero = a traversal stack overflowed (results invalid)
    }
    if (c[6] != 0) throw RenderError("BVH traversal stack overflow: the render is incomplete");
}
AKR_API int32_t akr_pt_get_stats(akr_pt_session* se, akr_pt_stats* stats) {
    if (!se || !stats) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_pt_get_stats: NULL argument");
    return guarded([&] { read_stats(se, stats); });
}
AKR_API int32_t akr_pt_kernel_info(akr_pt_session* se, akr_kernel_info* info) {
    if (!se || !info) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_pt_kernel_info: NULL argument");
    if (info->struct_size < sizeof(akr_kernel_info)) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_pt_kernel_info: struct_size is smaller than this library's akr_kernel_info (set it to sizeof)");
    return guarded([&] {
        const uint32_t size = info->struct_size;
        std::memset(info, 0, sizeof *info);
        info->struct_size = size;
        info->specialised = se->route.spec ? 1u : 0u;
        info->n_shader_kinds = (uint32_t)se->scene->cs.shader_kinds.size();
        const PtVariant& v = se->variant;  // (bit 0: the flattened scene's tree; a kept scene's two-level traversal does not set it)
        info->kernel_flags = (v.bvh && !v.inst ? 1u : 0u) | (v.pmj ? 2u : 0u) | (v.stage ? 4u : 0u) | (v.defer ? 8u : 0u) | (se->route.relaxed ? 16u : 0u) | (v.lens ? 32u : 0u) | (v.feat ? 64u : 0u) | (v.punct ? 128u : 0u) |
                             (v.ltree ? 256u : 0u);
        info->absent_mask = se->scene->cs.absent;
        if (se->spec) {
            info->cache_hit = se->spec->cache_hit ? 1u : 0u;
            info->min_waves = (uint32_t)se->route.spec_waves;
            info->vgprs = (uint32_t)se->spec->vgprs;
            info->scratch_bytes = (uint32_t)se->spec->scratch_bytes;
            info->compile_ms = se->spec->compile_ms;
            info->load_ms = se->spec->load_ms;
        }
        // (a session whose items are dealt by position says nothing: callers compare the status of such sessions with fixed strings)
        const char* order = se->cost.state == 2 ? "; cost order: in use" : (se->cost.state == 1 ? "; cost order: recording" : "");
        std::snprintf(info->status, sizeof info->status, "%s%s", se->spec_status.c_str(), order);
        if (se->wf && se->wf->buf.carry != nullptr && se->counters.p) {  // what the launches so far carried over (wf_kernels.hip; counter 7)
            const uint64_t carried = read_counters(se)[7];
            std::snprintf(info->status, sizeof info->status, "%s; %llu rays carried into a later trace launch", se->spec_status.c_str(), (unsigned long long)carried);
        }
    });
}
AKR_API int32_t akr_pt_end(akr_pt_session* se, akr_pt_stats* stats) { return base_end(se, stats); }
// every pass of the session begun with status rc_begin, then its end: what akr_pt_render and akr_pt_render_features do with their session
static int32_t render_and_end(int32_t rc_begin, akr_pt_session* se, const akr_pt_config* cfg, akr_pt_stats* stats) {
    if (rc_begin != AKR_OK) return rc_begin;
    const uint32_t n_passes = (session_samples(*cfg) + cfg->spp_per_pass - 1) / cfg->spp_per_pass;
    const int32_t rc = akr_pt_passes(se, n_passes, 1, nullptr);
    return end_keeping_first_error(rc, [&] { return akr_pt_end(se, stats); });
}
AKR_API int32_t akr_pt_render(akr_context* ctx, akr_scene* scene, const akr_pt_config* cfg, akr_film* film, akr_pt_stats* stats) {
    akr_pt_session* se = nullptr;
    return render_and_end(akr_pt_begin(ctx, scene, cfg, film, &se), se, cfg, stats);
}
AKR_API int32_t akr_pt_render_features(akr_context* ctx, akr_scene* scene, const akr_pt_config* cfg, akr_film* film, akr_film* albedo, akr_film* normal, akr_pt_stats* stats) {
    akr_pt_session* se = nullptr;
    return render_and_end(akr_pt_begin_features(ctx, scene, cfg, film, albedo, normal, &se), se, cfg, stats);
}

}  // extern "C"
int32_t akr_api::base_end(RenderBase* se, akr_pt_stats* stats) {
    if (!se) return AKR_OK;
    int32_t rc = guarded([&] { read_stats(se, stats); });
    (void)hipSetDevice(se->ctx->device);
    delete se;
    return rc;
}
