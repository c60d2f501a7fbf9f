// api_pt.cpp -- the `pt` integrator: the plan, kernel parameters, the base session, the pt sessions and their per-scene kernels (C ABI of libakari_hip.so,
// include/akari_hip.h; shared internals: api_internal.h; the wavefront schedule's host half: wf_schedule.cpp)
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
}
PtVariant akr_api::pt_scene_facts(const akr_scene* s, const akr_pt_config& c) {
    const CompiledScene& cs = s->cs;  // (stage, defer, simple: pt_plan)
    PtVariant v;
    v.bvh = cs.has_tree();
    v.fd = c.force_diffuse != 0;
    v.tex = cs.has_textures;
    v.pmj = c.sampler_type != AKR_SAMPLER_INDEPENDENT;
    v.inst = cs.instanced.on;
    v.env = cs.env.on;
    v.lens = s->flat.lens.radius > 0.0f;
    v.punct = !cs.punct.empty();
    v.ltree = !cs.punct_tree.empty();
    return v;
}
std::string akr_api::pt_punctual_refusal(const akr_scene* s, const TuningOptions& t) {
    if (s->cs.punct.empty()) return "";
    const std::string who = "a " + punctual_light_name(s->cs);
    if (t.wavefront == 1) return "unsupported: the scene has " + who + " and the wavefront schedule is forced (option wavefront = 1); only the megakernel samples punctual lights";
    if (t.arith == 1) return "unsupported: the scene has " + who + "; the relaxed arithmetic tier (option arith = 1) has no kernels that sample punctual lights";
    return "";
}
std::string akr_api::pt_features_refusal(const akr_scene* s, const TuningOptions& t) {
    if (s->cs.instanced.on)
        return "unsupported: akr_pt_begin_features: the scene is kept as meshes + instances (option instancing); its kernels collect no guides -- render them with akr_aov_render";
    if (t.wavefront == 1) return "unsupported: akr_pt_begin_features: the wavefront schedule is forced (option wavefront = 1); only the megakernel collects guides";
    if (t.arith == 1) return "unsupported: akr_pt_begin_features: the relaxed arithmetic tier (option arith = 1) has no kernels that collect guides";
    if (!s->cs.punct.empty())
        return "unsupported: akr_pt_begin_features: the scene has a " + punctual_light_name(s->cs) + "; the kernels that sample punctual lights collect no guides -- render them with akr_aov_render";
    return "";
}
static std::atomic<int> g_cost_order_mode{1};
int akr_api::cost_order_mode() { return g_cost_order_mode.load(); }
int akr_api::cost_order_mode_set(int mode) { return mode >= 0 && mode <= 2 ? g_cost_order_mode.exchange(mode) : g_cost_order_mode.load(); }
PtPlan akr_api::pt_plan(const akr_scene* s, const akr_pt_config& c, const TuningOptions& opt, bool spec_active, int spec_waves, bool feat, int cost_order) {
    const CompiledScene& cs = s->cs;
    PtPlan pl{};
    PtVariant& v = pl.v = pt_scene_facts(s, c);
    v.feat = feat;
    // The exclusion rules, applied here and nowhere else (kernels.h pt_variant_compiled states them): no DEFER and no SIMPLE kernels with an
    // environment light, a lens, collected guides or punctual lights; a kept scene has neither, and its kernels stage no tables.
    const bool plain = !v.env && !v.lens && !v.feat && !v.punct;
    {   // SIMPLE instantiations (dbsdf.h principled_eval): the reference traces its kernel from the scene's shader graphs, so a scene
        // without coat / transmission / normal map / glass runs a kernel without that code there too. The conditions are on the
        // folded VALUES (coat_weight and transmission exactly 0), which is what makes dropping the branches exact.
        bool simple = !cs.has_textures;
        for (const DMaterial& m : cs.materials) {
            if (m.kind == MAT_GLASS) simple = false;
            if (m.kind == MAT_PRINCIPLED && ((m.flags & (MF_COAT | MF_EVAL_DIEL | MF_NORMAL_MAP)) != 0 || m.transmission != 0.0f || m.coat_weight != 0.0f)) simple = false;
        }
        pl.simple_scene = (simple && opt.simple_kernels && plain) ? 1u : 0u;
        v.simple = pl.simple_scene != 0 && !v.fd && !v.tex && !v.inst;  // (full-graph kernels of scenes without textures)
    }
    {   // hits on "expensive" materials on even iterations only (device/pt_pass.h: DEFER): pays when SOME materials are expensive and
        // most hits are not. Expensive = the conductor lobe; in the BVH kernels of scenes with textures (option defer_on) also /
        // instead a shader graph to evaluate at the hit.
        uint32_t flags = MF_EVAL_METAL;
        // (measured on the textured room, BVH kernel: conductor hits deferred 591 Msamples/s, textured hits 573, both 573, none 544)
        if (v.bvh && v.tex) flags = opt.defer_on == 2 ? MF_TEXTURED : (opt.defer_on == 3 ? (MF_EVAL_METAL | MF_TEXTURED) : MF_EVAL_METAL);
        size_t n_dear = 0, n_surface = 0;
        for (const DMaterial& m : cs.materials) {
            if (m.kind == MAT_EMISSION) continue;
            n_surface++;
            if (m.flags & flags) n_dear++;  // the kernel's own test (pt_pass.h: DEFER), whatever the material's kind
        }
        bool want = n_dear > 0 && 2 * n_dear <= n_surface;
        uint32_t mask = 1u;  // iterations with (iteration & mask) != 0 put those hits off
        if (opt.defer_metal >= 0) { mask = (uint32_t)opt.defer_metal; want = mask != 0; }  // akr_option_set("defer_metal"): measurements / tests
        // (full-graph kernels, of BVH scenes those with textures)
        pl.defer_metal = (want && (!v.bvh || v.tex) && !v.fd && !v.inst && plain) ? mask : 0u;
        pl.defer_flags = flags;
        v.defer = pl.defer_metal != 0;
    }
    {   // LDS staging of the tables the shading phase gathers from (device/pt_pass.h: STAGE)
        // exhaustive path: everything, per-triangle records included (scene_build.cpp guarantees the fit);
        // BVH path: the per-scene tables only, if the launch still fits its share of the CU's LDS with them (kernels.h pt_lds_layout)
        const bool bvh = v.bvh;
        size_t bytes[13] = {bvh ? 0 : cs.shade.size() * 4, bvh ? 0 : cs.normals.size() * 4, cs.inst.size() * 4, cs.materials.size() * sizeof(DMaterial),
                            (size_t)cs.n_lights * sizeof(AliasPacked), cs.area_entries.size() * sizeof(AliasPacked), (size_t)cs.n_lights * sizeof(LightRec),
                            cs.light_pdf.size() * 4, cs.area_pdf.size() * 4, 0, 0, 0, 0};
        if (cs.has_textures) {  // the node lists have the same size in every colour pipeline
            bytes[9] = cs.tex_nodes.size() * sizeof(DNode);
            bytes[10] = cs.images.size() * sizeof(DImage);
            bytes[11] = cs.mat_inputs.size() * sizeof(MatInputs);
        }
        size_t total = 0;
        for (int i = 0; i < 12; i++) total += (bytes[i] + 15) & ~(size_t)15;
        pl.tex_slots = (cs.has_textures && !spec_active) ? cs.tex_slots : 0;  // a per-scene kernel keeps node values in registers
        // the workgroup's share: a per-scene kernel built for four waves per SIMD has a quarter of the CU's LDS whatever the scene
        const size_t budget = pt_lds_budget(v.tex && !(spec_active && spec_waves >= 4));
        auto fits = [&](size_t staged) {  // (the blue-noise columns and the node tile only take what is left: not part of the question)
            const PtLdsSizes sizes{scene_stack_depth(cs), cs.n_tris, scene_n_nodes(cs), pl.tex_slots, (uint32_t)staged, false};
            return pt_lds_layout(v, sizes, /*plan_larger_park=*/true).required_bytes <= budget;
        };
        // all of it or nothing (a TEX kernel reads its tables through LDS addresses); the kept-scene kernels do not stage
        const bool may = !v.inst && total <= (bvh ? kStageMaxBytesBvh : kStageMaxBytes);
        // the albedo table as well for the full-graph exhaustive kernel of a textured scene (stage_scene_tables: GGX), if three
        // workgroups per CU still fit (AKR_PT_MIN_WAVES_TEX = 3: 160 KB / 3)
        const size_t ggx_bytes = 4096 * sizeof(float);
        if (may && !bvh && v.tex && !v.fd && fits(total + ggx_bytes)) {
            bytes[12] = ggx_bytes;
            total += ggx_bytes;
            v.stage = true;
        } else {
            v.stage = may && (!bvh || fits(total));
        }
        if (v.stage) {
            for (int i = 0; i < 13; i++) pl.stage_bytes[i] = (uint32_t)bytes[i];
            pl.stage_total = (uint32_t)std::max<size_t>(total, 16);
        }
    }
    // Work items ordered by measured pixel cost: on where a wave's spatial coherence buys nothing -- the exhaustive walk reads
    // every record for every lane, and a scene without textures gathers from tables in LDS. Off for the BVH kernels and kept scenes (a wave's
    // rays share nodes), textured scenes (its lanes share texels) and sessions that collect guides (not measured). 2: all of them, to measure.
    pl.cost_order = cost_order == 2 || (cost_order == 1 && !v.bvh && !v.tex && !v.inst && !v.feat);
    if (!pt_variant_compiled(v)) throw RenderError("pt_plan: no kernel for the variant decided");  // (cannot happen: the rules above are pt_variant_compiled's)
    return pl;
}
void akr_api::session_params(RenderBase* se, bool spec_active, int spec_waves) {
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
    if (c.color != 0) {  // the material tables of this pipeline (created by akr_pt_begin)
        const auto& set = *se->color_set;
        p.sc.materials = set.materials.as<DMaterial>();
        if (s->cs.has_textures) {
            p.sc.tex.nodes = set.tex_nodes.as<DNode>();
            p.sc.tex.mat_inputs = set.mat_inputs.as<MatInputs>();
        }
        if (!s->cs.punct.empty()) p.sc.punct = set.punct.as<DPunct>();
    }
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
        const PtPlan plan = pt_plan(s, c, se->opt, spec_active, spec_waves, se->feat_albedo != nullptr, se->cost_order_mode);
        se->variant = plan.v;
        se->plan_cost_order = plan.cost_order;
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
    se->cost_order = 0;
    se->params.item_cost = nullptr;
    se->params.item_pixels = nullptr;
}
// Before a megakernel launch of a session in state 1 whose earlier launch recorded: the table from the costs so far, on the stream (no
// host synchronisation: the launch before wrote item_cost, the launches after read item_pixels, all in stream order).
static void cost_order_build(akr_pt_session* se) {
    PtParams& p = se->params;
    const uint32_t n_padded = (p.n_items + 255u) & ~255u;
    se->item_pixels.alloc((size_t)n_padded * sizeof(uint32_t));
    se->cost_keys.alloc((size_t)n_padded * sizeof(uint64_t));
    se->cost_keys_sorted.alloc((size_t)n_padded * sizeof(uint64_t));
    se->cost_sort_tmp.alloc(std::max<size_t>(16, cost_order_temp_bytes(n_padded)));
    HIP_CHECK(hipEventCreate(&se->cost_ev0));
    HIP_CHECK(hipEventCreate(&se->cost_ev1));
    HIP_CHECK(hipEventRecord(se->cost_ev0, se->ctx->stream));
    HIP_CHECK(launch_cost_order(p, n_padded, se->cost_keys.as<uint64_t>(), se->cost_keys_sorted.as<uint64_t>(), se->cost_sort_tmp.p, se->cost_sort_tmp.bytes,
                                se->item_pixels.as<uint32_t>(), se->ctx->stream));
    HIP_CHECK(hipEventRecord(se->cost_ev1, se->ctx->stream));
    p.item_pixels = se->item_pixels.as<uint32_t>();
    p.item_cost = nullptr;  // one sort per session: nothing reads later costs
    se->cost_order = 2;
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
    std::unique_lock<std::mutex> color_lock(scene->color_sets_mutex);
    if (cfg->color != 0 && !scene->color_sets.count(cfg->color)) {
        // ColorPipeline other than sRGB / sRGB: the scene's constants were folded for the default pipeline; fold them again
        // for this one (svm/texture/mod.rs:9-43 at every Rgb / spectral_uplift node) and keep the tables with the scene
        CompiledScene tmp;
        tmp.images = scene->cs.images;
        std::vector<akr_material_desc> descs;
        compile_materials(scene->flat, cfg->color, tmp, descs);
        auto set = std::make_unique<akr_scene::ColorSet>();
        set->materials.upload(tmp.materials);
        if (tmp.has_textures) {
            set->tex_nodes.upload(tmp.tex_nodes);
            set->mat_inputs.upload(tmp.mat_inputs);
        }
        scene->color_sets[cfg->color] = std::move(set);
    }
    if (cfg->color != 0 && !scene->cs.punct.empty() && !scene->color_sets.at(cfg->color)->punct.p) {  // (dropped when the lights change: api_scene.cpp)
        std::vector<DPunct> recs;
        for (const akr_punctual_light_desc& d : scene->flat.punct) recs.push_back(fold_punctual(d, cfg->color));
        scene->color_sets.at(cfg->color)->punct.upload(punctual_device_records(recs, scene->cs.punct_tree));  // (the tree's nodes are the same in every set)
    }
    if (cfg->color != 0) se->color_set = scene->color_sets.at(cfg->color).get();  // stable: the map owns it through a unique_ptr
    color_lock.unlock();
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
    se->cost_order_mode = cost_order_mode();
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
// akr_pt_begin, and with the two guide films akr_pt_begin_features (whose refusals the caller has already made, from the same snapshot `t`)
static int32_t pt_begin(akr_context* ctx, akr_scene* scene, const akr_pt_config* cfg, akr_film* film, akr_film* albedo, akr_film* normal, const TuningOptions& t, akr_pt_session** out) {
    *out = nullptr;
    return guarded([&] {
        auto se = std::make_unique<akr_pt_session>();
        if (scene) {  // what a scene with punctual lights cannot do, before a byte is allocated
            const std::string why = pt_punctual_refusal(scene, t);
            if (!why.empty()) throw Unsupported(why);
        }
        base_begin(se.get(), ctx, scene, cfg, film, &t);
        se->feat_albedo = albedo;
        se->feat_normal = normal;
        const bool features = albedo != nullptr;
        const bool wavefront = !features && choose_wavefront(se.get());
        se->wf_sort = wavefront && t.wf_sort != 0;
        {
            // A per-scene kernel (host/specialise.cpp) for the megakernel of a scene with texture-fed materials: always / never by
            // option, else when the render is long enough for a first-use compile to pay.
            const uint64_t samples = (uint64_t)film->width * film->height * (uint64_t)session_samples(*cfg);
            // (automatic: a kernel that is already cached is used whatever the render's size; a compile -- about a second -- only
            // when the render is long enough to win it back)
            const bool may_compile = t.specialise == 1 || samples >= kSpecAutoSamples;
            // The relaxed arithmetic tier (pt_kernels_relaxed.hip): the precompiled megakernels of flattened scenes. Everything else --
            // kept scenes, the wavefront schedule, aov / gpt / mcmc_opt -- stays on the contract whatever the option says.
            // Which sessions it takes is decided here and nowhere else: its translation unit holds the variants without inst, env and lens.
            const PtVariant facts = pt_scene_facts(scene, *cfg);
            se->arith_relaxed = t.arith == 1 && !facts.inst && !wavefront && !features;
            if (se->arith_relaxed && facts.env)
                throw Unsupported("unsupported: the relaxed arithmetic tier (option arith = 1) does not render scenes with an environment light");
            if (se->arith_relaxed && facts.lens)
                throw Unsupported("unsupported: the relaxed arithmetic tier (option arith = 1) does not render through a lens (akr_scene_set_lens)");
            if (se->arith_relaxed) se->spec_status = "relaxed arithmetic tier: precompiled kernels";
            else if (wavefront) se->spec_status = "wavefront schedule";
            else if (features) se->spec_status = scene->cs.has_textures && t.specialise == 1 ? "guides are collected by the interpreter kernels: no per-scene kernel (option specialise ignored)"
                                                                                            : "guides are collected by the precompiled kernels";
            else if (!scene->cs.has_textures) se->spec_status = "the scene has no texture-fed material";
            else if (facts.punct) se->spec_status = "punctual lights are sampled by the interpreter kernels: no per-scene kernel (option specialise ignored)";
            else if (t.specialise == 0) se->spec_status = "option specialise = 0";
            else if (cfg->force_diffuse) se->spec_status = "force_diffuse kernels evaluate no surface graphs";
            else {
                {
                    std::lock_guard<std::mutex> lock(scene->spec_mutex);
                    if (!scene->spec_header_made) {
                        scene->spec_header = generate_scene_spec(scene->cs);
                        scene->spec_header_made = true;
                    }
                }
                se->spec_waves = t.specialise_waves ? t.specialise_waves : 3;
                se->spec_active = true;
            }
            session_params(se.get(), se->spec_active, se->spec_waves);
            if (se->spec_active) {  // the session's variant, compiled with the scene's graphs
                se->spec = ctx->spec_cache.get(scene->spec_header, se->variant, se->spec_waves, ctx->props.gcnArchName, may_compile);
                se->spec_status = se->spec->status;
                if (!se->spec->fn) {  // the interpreter kernel renders the same film: with graph value slots in LDS and its own LDS budget
                    se->spec_active = false;
                    session_params(se.get(), false, se->spec_waves);
                }
            }
            se->params.wf_sort = se->wf_sort ? 1u : 0u;
        }
        if (wavefront) se->wf = wf_allocate(se.get(), se->wf_sort);
        if (se->plan_cost_order && !wavefront && !se->arith_relaxed) {  // (the relaxed tier and the other schedule deal by position)
            se->item_cost.alloc((size_t)((se->grid.n_items + 255u) & ~255u) * sizeof(uint32_t));  // (a launch's whole grid writes)
            if (se->item_cost.p) HIP_CHECK(hipMemsetAsync(se->item_cost.p, 0, se->item_cost.bytes, ctx->stream));
            se->params.item_cost = se->item_cost.as<uint32_t>();
            se->cost_order = 1;
        }
        se->sched_trial = schedule_trial_eligible(se.get()) ? 1 : 0;
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
// here, before a byte is allocated or written.
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
    const TuningOptions t = tuning();  // the refusal and the session see the same options
    const std::string why = pt_features_refusal(scene, t);
    if (!why.empty()) return fail(AKR_ERR_UNSUPPORTED, why);
    return pt_begin(ctx, scene, cfg, film, albedo, normal, t, out);
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
        if (se->cost_order == 2 && se->cost_keys.p && se->pending.empty()) {  // the sort has run: its scratch goes
            se->cost_keys.release();
            se->cost_keys_sorted.release();
            se->cost_sort_tmp.release();
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
                if (se->cost_order) cost_order_drop(se);  // (a timed trial handed the session to the other schedule)
                wf_run(se);
            } else {
                if (se->cost_order == 1 && se->cost_recorded && se->params.n_items > 0) cost_order_build(se);
                se->cost_recorded = se->cost_recorded || se->cost_order == 1;
                HIP_CHECK(launch_pt_pass(se->params, se->variant, se->ctx->stream, se->spec_active ? se->spec->fn : nullptr, se->arith_relaxed));
            }
            timer.stop();
            se->spp_done = done;
            se->n_launches++;
            se->passes_launched += fused;
            left -= fused;
        };
        if (se->sched_trial == 1 && blocking && left >= 4 && total - se->spp_done >= 4 * se->cfg.spp_per_pass) {  // (schedule_trial_eligible)
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
        if (se->cost_order) cost_order_drop(se);  // ... and no cost order: its table is of the session's own tiles, and a list's tiles are few and alike
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
        info->specialised = se->spec_active ? 1u : 0u;
        info->n_shader_kinds = (uint32_t)se->scene->cs.shader_kinds.size();
        const PtVariant& v = se->variant;  // (bit 0: the flattened scene's tree; a kept scene's two-level traversal does not set it)
        info->kernel_flags = (v.bvh && !v.inst ? 1u : 0u) | (v.pmj ? 2u : 0u) | (v.stage ? 4u : 0u) | (v.defer ? 8u : 0u) | (se->arith_relaxed ? 16u : 0u) | (v.lens ? 32u : 0u) | (v.feat ? 64u : 0u) | (v.punct ? 128u : 0u) |
                             (v.ltree ? 256u : 0u);
        info->absent_mask = se->scene->cs.absent;
        if (se->spec) {
            info->cache_hit = se->spec->cache_hit ? 1u : 0u;
            info->min_waves = (uint32_t)se->spec_waves;
            info->vgprs = (uint32_t)se->spec->vgprs;
            info->scratch_bytes = (uint32_t)se->spec->scratch_bytes;
            info->compile_ms = se->spec->compile_ms;
            info->load_ms = se->spec->load_ms;
        }
        // (a session whose items are dealt by position says nothing: callers compare the status of such sessions with fixed strings)
        const char* order = se->cost_order == 2 ? "; cost order: in use" : (se->cost_order == 1 ? "; cost order: recording" : "");
        std::snprintf(info->status, sizeof info->status, "%s%s", se->spec_status.c_str(), order);
        if (se->wf && se->wf->buf.carry != nullptr && se->counters.p) {  // what the launches so far carried over (wf_kernels.hip; counter 7)
            const uint64_t carried = read_counters(se)[7];
            std::snprintf(info->status, sizeof info->status, "%s; %llu rays carried into a later trace launch", se->spec_status.c_str(), (unsigned long long)carried);
        }
    });
}
AKR_API int32_t akr_pt_end(akr_pt_session* se, akr_pt_stats* stats) { return base_end(se, stats); }
AKR_API int32_t akr_pt_render(akr_context* ctx, akr_scene* scene, const akr_pt_config* cfg, akr_film* film, akr_pt_stats* stats) {
    akr_pt_session* se = nullptr;
    int32_t rc = akr_pt_begin(ctx, scene, cfg, film, &se);
    if (rc != AKR_OK) return rc;
    uint32_t n_passes = (session_samples(*cfg) + cfg->spp_per_pass - 1) / cfg->spp_per_pass;
    rc = akr_pt_passes(se, n_passes, 1, nullptr);
    return end_keeping_first_error(rc, [&] { return akr_pt_end(se, stats); });
}
AKR_API int32_t akr_pt_render_features(akr_context* ctx, akr_scene* scene, const akr_pt_config* cfg, akr_film* film, akr_film* albedo, akr_film* normal, akr_pt_stats* stats) {
    akr_pt_session* se = nullptr;
    int32_t rc = akr_pt_begin_features(ctx, scene, cfg, film, albedo, normal, &se);
    if (rc != AKR_OK) return rc;
    uint32_t n_passes = (session_samples(*cfg) + cfg->spp_per_pass - 1) / cfg->spp_per_pass;
    rc = akr_pt_passes(se, n_passes, 1, nullptr);
    return end_keeping_first_error(rc, [&] { return akr_pt_end(se, stats); });
}

}  // extern "C"
int32_t akr_api::base_end(RenderBase* se, akr_pt_stats* stats) {
    if (!se) return AKR_OK;
    int32_t rc = guarded([&] { read_stats(se, stats); });
    (void)hipSetDevice(se->ctx->device);
    delete se;
    return rc;
}
