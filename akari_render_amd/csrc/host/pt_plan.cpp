// pt_plan.cpp -- what the pt integrator decides from (scene, config, options) and no device pointer: the route of a session (pt_route: schedule,
// arithmetic tier, per-scene kernel, refusal, status) and the plan of its launches (pt_plan: kernel variant, staged tables). Declarations:
// api_internal.h. api_pt.cpp carries the decisions out; the test hooks (api_probe.cpp) ask the same functions for host-only scenes.
#include "api_internal.h"

PtVariant akr_api::pt_scene_facts(const akr_scene* s, const akr_pt_config& c) {
    const CompiledScene& cs = s->cs;  // (stage, defer, simple: pt_plan)
    PtVariant v;
    v.bvh = cs.has_tree();
    v.fd = c.force_diffuse != 0;
    v.tex = cs.has_textures;
    v.pmj = c.sampler_type != AKR_SAMPLER_INDEPENDENT;
    v.inst = cs.instanced.on;
    v.env = cs.env.on;
    v.lens = camera_runs_lens_kernels(s->flat.lens.radius, s->flat.projection.type);  // (a lens, or a projection other than the perspective one: DESIGN.md 4.17)
    v.punct = !cs.punct.empty();
    v.ltree = !cs.punct_tree.empty();
    return v;
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
        size_t bytes[ST_COUNT], total = 0;
        stage_table_bytes(cs, cs.n_lights, bytes);  // (the node lists have the same size in every colour pipeline)
        if (bvh) bytes[ST_SHADE] = bytes[ST_NORMALS] = 0;
        // the one term that is not scene_build.cpp's: image headers no material reads stay in HBM here and count against the exhaustive budget there
        if (!cs.has_textures) bytes[ST_TEX_IMAGES] = 0;
        for (size_t b : bytes) total += (b + 15) & ~(size_t)15;
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
            bytes[ST_GGX] = ggx_bytes;
            total += ggx_bytes;
            v.stage = true;
        } else {
            v.stage = may && (!bvh || fits(total));
        }
        if (v.stage) {
            for (int i = 0; i < ST_COUNT; i++) pl.stage_bytes[i] = (uint32_t)bytes[i];
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

// Which schedule renders this session: the persistent-lane megakernel (pt_unit_kernels.hip) or the wavefront schedule --
// trace / shade kernels with the path state in HBM (wf_kernels.hip; needs a scene with a tree). Option wavefront: 1 = wherever it can run,
// 0 = never, -1 (default) = the library decides:
//   * flattened scenes: the megakernel, which measured faster on every one (on the 10 M-triangle hall both schedules
//     are bound by the memory system's rate for random 64-byte records, and the wavefront schedule pays for streaming the path state on top);
//   * scenes kept as meshes + instances: the WAVEFRONT schedule for pt sessions of at least wf_auto_items() pixels (round 6). The two-level
//     traversal with its exact test spills 172 registers inside the megakernel (one lane = one whole path) and none in k_wf_trace, and the
//     trace kernel refills a wave's idle lanes where the megakernel's wait: 1080p forest 1000 x 10 k triangles 163 -> 228 Msamples/s, 4K
//     177 -> 282 (x 100 k: 113 -> 136 with two slot groups, 4K 125 -> 179). Below that size the persistent trace kernel's 262 k lanes
//     are not filled and the megakernel wins (1024 x 1024, x 100 k: 124 against 85) -- profiles/r6_kept_schedules.txt. Kept scenes with
//     texture-fed materials as well: k_wf_shade interprets the shader graphs where the megakernel has its per-scene kernels, and still
//     the same forest with image-textured leaves and bark renders at 193 against 157 Msamples/s (x 100 k: 123 against 100).
// A scene without a tree (64 triangles or fewer, no force_bvh) has no wavefront kernels and renders with the megakernel whatever the option says.
// How large: the persistent trace kernel wants its 262 k lanes refilled many times over, and the larger the meshes the longer a launch's last
// rays take. Measured crossovers (tools/kept_schedules.py at seven frame sizes, profiles/r6_kept_schedules.txt), with a launch's last rays carried
// into the next one (option wf_carry, the default): 0.5 M pixels for the forest of 10 k-triangle meshes (1.7 MB of per-mesh data; 800 x 600: 145 vs
// 147, 1024 x 768: 167 -> 189), 0.8 M for 100 k-triangle ones (17 MB; 1024 x 768: 118 vs 122, 1024 x 1024: 138 -> 150). Without carried rays: 0.7 M
// and 1.45 M. 2 M, the constant of the first version, beyond what was measured.
static uint32_t wf_auto_items(const akr_scene* scene, const TuningOptions& opt) {
    const uint64_t mesh_bytes = ((uint64_t)scene->cs.instanced.nodes.size() + scene->cs.instanced.mesh_tris.size()) * 4u;
    const bool carry = opt.wf_carry != 0 && opt.wf_sort == 0;
    return (uint32_t)std::min<uint64_t>(2000000u, carry ? 500000u + mesh_bytes / 55u : 700000u + mesh_bytes / 18u);
}
static bool choose_wavefront(const akr_scene* scene, const TuningOptions& t, uint32_t n_items) {
    if (t.wavefront == 0 || !scene->cs.has_tree()) return false;
    if (t.wavefront > 0) return true;
    return scene->cs.instanced.on && n_items >= wf_auto_items(scene, t);
}

std::string akr_api::pt_route_refusal(const akr_scene* s, const TuningOptions& t, bool feat) {
    const CompiledScene& cs = s->cs;
    if (feat) {  // only the megakernels of flattened scenes without punctual lights collect guides
        const std::string head = "unsupported: akr_pt_begin_features: ";
        if (cs.instanced.on) return head + "the scene is kept as meshes + instances (option instancing); its kernels collect no guides -- render them with akr_aov_render";
        if (t.wavefront == 1) return head + "the wavefront schedule is forced (option wavefront = 1); only the megakernel collects guides";
        if (t.arith == 1) return head + "the relaxed arithmetic tier (option arith = 1) has no kernels that collect guides";
        if (!cs.punct.empty()) return head + "the scene has a " + punctual_light_name(cs) + "; the kernels that sample punctual lights collect no guides -- render them with akr_aov_render";
        return "";
    }
    if (cs.punct.empty()) return "";  // only the contract's megakernels sample punctual lights (kept scenes are refused when the scene is compiled)
    const std::string who = "unsupported: the scene has a " + punctual_light_name(cs);
    if (t.wavefront == 1) return who + " and the wavefront schedule is forced (option wavefront = 1); only the megakernel samples punctual lights";
    if (t.arith == 1) return who + "; the relaxed arithmetic tier (option arith = 1) has no kernels that sample punctual lights";
    return "";
}

// The route of a session (api_internal.h PtRoute). Its timed schedule trial: flattened scenes under option wavefront = -1. Which schedule is faster there depends on the scene -- 1080p, 10 M triangles: the closed hall 308
// (megakernel) against 252 Msamples/s (wavefront), the open forest 309 against 369 -- through how much the lengths of a wave's traversals differ, which
// no number the compiler has predicts. So a render that can pay for it MEASURES: the first blocking akr_pt_passes call runs two passes under the
// megakernel, two under the wavefront schedule (HIP-event time per sample of each), and the session goes on with the faster one. Films are the same
// bit for bit under either schedule and under any sequence of them (both start a launch from, and leave behind, the session's sampler states and
// film). "Can pay": a pt session without textures / relaxed tier / ray sort on a scene with a tree of >= 256 MB (small scenes: the megakernel wins
// by up to 2 x), >= 1 M pixels (the persistent trace kernel wants its lanes refilled), >= 16 passes to render; a scene whose paths practically
// never end at a light or in the open (shaded vertices per closest-hit ray >= 0.97 in the megakernel's two passes: the hall 0.999) skips the
// wavefront half -- it has measured slower on every such scene. Option sched_trial: 0 = never, 1 = every session on a scene with a tree (tests).
PtRoute akr_api::pt_route(const akr_scene* s, const akr_pt_config& c, const TuningOptions& t, const TileGrid& grid, bool feat, int cost_order, bool spec_possible) {
    PtRoute r;
    if (!(r.refusal = pt_route_refusal(s, t, feat)).empty()) return r;
    const CompiledScene& cs = s->cs;
    const PtVariant facts = pt_scene_facts(s, c);
    r.wavefront = !feat && choose_wavefront(s, t, grid.n_items);
    r.wf_sort = r.wavefront && t.wf_sort != 0;
    // The relaxed arithmetic tier (pt_kernels_relaxed.hip): the precompiled megakernels of flattened scenes, without inst, env and lens. Everything
    // else -- kept scenes, the wavefront schedule, aov / gpt / mcmc_opt -- stays on the contract whatever the option says.
    r.relaxed = t.arith == 1 && !facts.inst && !r.wavefront && !feat;
    if (r.relaxed && facts.env) r.refusal = "unsupported: the relaxed arithmetic tier (option arith = 1) does not render scenes with an environment light";
    else if (r.relaxed && s->flat.projection.type != AKR_PROJECTION_PERSPECTIVE)
        r.refusal = std::string("unsupported: the relaxed arithmetic tier (option arith = 1) does not render through ") + projection_name(s->flat.projection.type) + " projection (akr_scene_set_projection)";
    else if (r.relaxed && facts.lens) r.refusal = "unsupported: the relaxed arithmetic tier (option arith = 1) does not render through a lens (akr_scene_set_lens)";
    if (!r.refusal.empty()) return r;
    // A per-scene kernel (host/specialise.cpp) for the megakernel of a scene with texture-fed materials: always / never by option, else a cached
    // one whatever the render's size, and a compile -- about a second -- only when the render is long enough to win it back.
    r.spec_waves = t.specialise_waves ? t.specialise_waves : 3;
    r.may_compile = t.specialise == 1 || (uint64_t)s->flat.camera.width * s->flat.camera.height * (uint64_t)session_samples(c) >= kSpecAutoSamples;
    if (r.relaxed) r.status = "relaxed arithmetic tier: precompiled kernels";
    else if (r.wavefront) r.status = "wavefront schedule";
    else if (feat) r.status = cs.has_textures && t.specialise == 1 ? "guides are collected by the interpreter kernels: no per-scene kernel (option specialise ignored)"
                                                                    : "guides are collected by the precompiled kernels";
    else if (!cs.has_textures) r.status = "the scene has no texture-fed material";
    else if (facts.punct) r.status = "punctual lights are sampled by the interpreter kernels: no per-scene kernel (option specialise ignored)";
    else if (t.specialise == 0) r.status = "option specialise = 0";
    else if (c.force_diffuse) r.status = "force_diffuse kernels evaluate no surface graphs";
    else r.spec = spec_possible;  // (its status is the kernel's own, SpecKernel::status: also when the compile failed and the session was routed again without)
    r.plan = pt_plan(s, c, t, r.spec, r.spec_waves, feat, cost_order);
    const bool contract_megakernel = !r.wavefront && !r.relaxed;  // (the relaxed tier and the other schedule deal their items by position)
    r.record_costs = r.plan.cost_order && contract_megakernel;
    // the timed trial of both schedules (above): sessions the megakernel of the contract renders, on flattened scenes with a tree
    r.sched_trial = t.wavefront == -1 && t.sched_trial != 0 && t.wf_sort == 0 && contract_megakernel && !r.spec && !feat && !facts.punct && !facts.inst && cs.has_tree();
    if (r.sched_trial && t.sched_trial != 1) {
        const uint64_t passes = (session_samples(c) + c.spp_per_pass - 1) / std::max(1u, c.spp_per_pass);  // (a hook's config has not been validated)
        r.sched_trial = !cs.has_textures && s->device_bytes >= (256ull << 20) && passes >= 16 && grid.n_items >= 1000000u;
    }
    return r;
}
