// api_scene.cpp -- scenes: compile + upload, inspection, per-scene kernel text (C ABI of libakari_hip.so, include/akari_hip.h; shared internals: api_internal.h)
#include "api_internal.h"

static void ensure_ggx_table(akr_scene* s) {
    akr_context* ctx = s->ctx;
    if (!s->flat.ggx_table.empty()) {
        s->ggx_host = s->flat.ggx_table;
    } else if (s->cs.needs_ggx_table) {
        std::lock_guard<std::mutex> lock(ctx->ggx_mutex);
        if (!ctx->ggx_cache.empty()) {  // computed for an earlier scene of this context
            s->ggx_host = ctx->ggx_cache;
            s->ggx_table.upload(s->ggx_host);
            return;
        }
        // PreComputedTables::init (svm/surface/precompute.rs:133-145): seeds = StdRng(0) stream, one per entry
        std::vector<uint64_t> seeds(4096);
        StdRng rng(0);
        for (auto& v : seeds) v = rng.next_u64();
        DevBuf dseeds;
        dseeds.upload(seeds);
        s->ggx_table.alloc(4096 * sizeof(float));
        HIP_CHECK(launch_ggx_table(dseeds.as<uint64_t>(), s->ggx_table.as<float>(), 1u << 20, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        s->ggx_host.resize(4096);
        HIP_CHECK(hipMemcpy(s->ggx_host.data(), s->ggx_table.p, 4096 * sizeof(float), hipMemcpyDeviceToHost));
        ctx->ggx_cache = s->ggx_host;
        return;
    } else {
        s->ggx_host.assign(4096, 0.0f);  // never read with a non-zero weight
    }
    s->ggx_table.upload(s->ggx_host);
}

static void pack_alias(const std::vector<AliasEntry>& e, const std::vector<float>& pdf, size_t first, size_t n, std::vector<AliasPacked>& out) {
    for (size_t i = 0; i < n; i++) out.push_back(AliasPacked{e[first + i].j, e[first + i].t, pdf[first + i], pdf[first + e[first + i].j]});
}
void akr_api::packed_light_tables(const CompiledScene& cs, std::vector<AliasPacked>& la, std::vector<AliasPacked>& aa, std::vector<LightRec>& lr) {
    pack_alias(cs.light_entries, cs.light_pdf, 0, cs.n_lights, la);
    // a punctual light's own entry says where its record is: the next one, or with a light tree (only the suns have entries of their own then) the next sun's
    uint32_t n_punct = 0;
    auto next_record = [&] {
        if (!cs.punct_tree.empty())
            while (n_punct < cs.punct.size() && cs.punct[n_punct].kind != PUNCT_SUN) n_punct++;
        return n_punct++;
    };
    for (uint32_t l = 0; l < cs.n_lights; l++) {
        if (cs.light_inst[l] == 0xffffffffu) {  // the environment (no triangles)
            lr.push_back(LightRec{cs.light_tri_offset[l], 0u, 0u, 0xffffffffu});
            continue;
        }
        if (cs.light_inst[l] == kPunctInst) {  // a punctual light (no triangles): first_gid = its record in DScene.punct
            lr.push_back(LightRec{cs.light_tri_offset[l], 0u, next_record(), kPunctInst});
            continue;
        }
        if (cs.light_inst[l] == kPunctTreeInst) {  // all point and spot lights: the walk finds the record
            lr.push_back(LightRec{cs.light_tri_offset[l], 0u, 0u, kPunctTreeInst});
            continue;
        }
        pack_alias(cs.area_entries, cs.area_pdf, cs.light_tri_offset[l], cs.light_n_tris[l], aa);
        lr.push_back(LightRec{cs.light_tri_offset[l], cs.light_n_tris[l], cs.inst_tri_offset[cs.light_inst[l]], cs.light_inst[l]});
    }
}
// the light tables (and the environment's record and tables, and the punctual lights' records) on the device, and their pointers in s->dscene: at scene
// creation and after akr_scene_set_environment / akr_scene_add_punctual_light / akr_scene_clear_punctual_lights
static void upload_lights(akr_scene* s) {
    const CompiledScene& cs = s->cs;
    s->light_entries.upload(cs.light_entries);
    s->light_pdf.upload(cs.light_pdf);
    s->light_inst.upload(cs.light_inst);
    s->light_tri_offset.upload(cs.light_tri_offset);
    s->light_n_tris.upload(cs.light_n_tris);
    s->punct.upload(punctual_device_records(cs.punct, cs.punct_tree));
    {  // the light tables once more, packed so that each level of light sampling is ONE gather (device/dgeom.h, dscene.h)
        auto pack = pack_alias;
        std::vector<AliasPacked> la, aa;
        std::vector<LightRec> lr;
        packed_light_tables(cs, la, aa, lr);
        s->light_alias.upload(la);
        s->area_alias.upload(aa);
        s->lights.upload(lr);
        if (cs.env.on) {
            std::vector<AliasPacked> marg, cond;
            pack(cs.env.marginal_entries, cs.env.marginal_pdf, 0, cs.env.h, marg);
            for (uint32_t y = 0; y < cs.env.h; y++) {
                const size_t first = (size_t)y * cs.env.w;
                for (uint32_t x = 0; x < cs.env.w; x++) {  // j is relative to the row
                    const AliasEntry& e = cs.env.conditional_entries[first + x];
                    cond.push_back(AliasPacked{e.j, e.t, cs.env.conditional_pdf[first + x], cs.env.conditional_pdf[first + e.j]});
                }
            }
            s->env_texels.upload(cs.env.texels);
            s->env_marginal.upload(marg);
            s->env_conditional.upload(cond);
            DEnv rec;
            std::memset(&rec, 0, sizeof rec);
            rec.texels = s->env_texels.as<float4>();
            rec.marginal = s->env_marginal.as<AliasPacked>();
            rec.conditional = s->env_conditional.as<AliasPacked>();
            for (int k = 0; k < 9; k++) rec.rot[k] = cs.env.rot_t[k];
            rec.w = cs.env.w;
            rec.h = cs.env.h;
            rec.filter = cs.env.filter;
            rec.light = cs.n_lights - 1;
            s->env_rec.alloc(sizeof rec);
            HIP_CHECK(hipMemcpy(s->env_rec.p, &rec, sizeof rec, hipMemcpyHostToDevice));
        } else {
            s->env_texels.release();
            s->env_marginal.release();
            s->env_conditional.release();
            s->env_rec.release();
        }
    }
    DScene& d = s->dscene;
    d.light_entries = s->light_entries.as<AliasEntry>();
    d.light_pdf = s->light_pdf.as<float>();
    d.light_inst = s->light_inst.as<uint32_t>();
    d.light_tri_offset = s->light_tri_offset.as<uint32_t>();
    d.light_alias = s->light_alias.as<AliasPacked>();
    d.area_alias = s->area_alias.as<AliasPacked>();
    d.lights = s->lights.as<LightRec>();
    d.n_lights = cs.n_lights;
    d.env = cs.env.on ? s->env_rec.as<DEnv>() : nullptr;
    d.punct = s->punct.as<DPunct>();
    d.n_punct = (uint32_t)cs.punct.size();
    for (const DPunct& r : cs.punct)  // (the size is not a matter of the colour pipeline: the colour sets' records have it where these do)
        if (r.radius != 0.0f || r.cos_max != 0.0f) d.n_punct |= kPunctSoftBit;
    d.punct_tree = cs.punct_tree.empty() ? 0u : (uint32_t)cs.punct.size();
}
static void count_device_bytes(akr_scene* s) {
    s->device_bytes = 0;
    for (const DevBuf* b : {&s->woop, &s->tri_gid, &s->shade, &s->normals, &s->inst, &s->materials, &s->ggx_table, &s->light_entries,
                            &s->light_pdf, &s->light_inst, &s->light_tri_offset, &s->light_n_tris, &s->area_entries, &s->area_pdf,
                            &s->inst_tri_offset, &s->light_alias, &s->area_alias, &s->lights, &s->bvh_nodes, &s->tex_nodes, &s->tex_images, &s->tex_texels, &s->tex_mat_inputs,
                            &s->in2_tlas_leaves, &s->in2_mesh_tris, &s->in2_mesh_pos, &s->in2_mesh_meta, &s->in2_mesh_normals, &s->in2_inst_mats, &s->in2_share_bits,
                            &s->env_texels, &s->env_marginal, &s->env_conditional, &s->env_rec, &s->punct})
        s->device_bytes += b->bytes;
}

// The pair walk's origin bound (dscene.h walk_bound_word): the largest power of two B <= 2^40 such that a ray with |o| <= B and |d| <= 2 per component gives, on every plane row
// (x, y, z, w) of the n records, |oz| = |x o.x + y o.y + z o.z + w| < 2^46 and |dz| = |x d.x + y d.y + z d.z| < 2^46 -- what the pair walk's
// division without range scaling assumes of its operands (device/disect.h UNSCALED_DIV). Bounded here in double by the triangle
// inequality against 2^45: the factor of two covers the rounding of the f32 fma chains (a few parts in 2^24) many times over.
// -1: a row is not finite or too large for any such B; the scene's walks then keep the compiler's division.
static float walk_origin_bound(const std::vector<float>& woop, uint32_t n) {
    double s_max = 0.0, w_max = 0.0;
    for (uint32_t k = 0; k < n; k++) {
        const float* r = &woop[12ull * k + 8];
        if (!(std::isfinite(r[0]) && std::isfinite(r[1]) && std::isfinite(r[2]) && std::isfinite(r[3]))) return -1.0f;
        s_max = std::max(s_max, std::fabs((double)r[0]) + std::fabs((double)r[1]) + std::fabs((double)r[2]));
        w_max = std::max(w_max, std::fabs((double)r[3]));
    }
    const double limit = 0x1p45;
    if (!(2.0 * s_max <= limit && w_max < limit)) return -1.0f;
    double b = 0x1p40;
    while (b >= 0x1p-40 && s_max * b + w_max > limit) b *= 0.5;
    return b >= 0x1p-40 ? (float)b : -1.0f;
}

// A lens moves the ray origins off the camera's position, and so does an orthographic projection, whose origins cover the film rectangle in the camera's
// x / y plane. The padding of the scene's boxes was sized from the largest coordinate magnitude an
// origin can have (scene_build.cpp, scene_inst.cpp: the camera's translation against the scene's box). The trees of a scene
// are the ones of its lens-less perspective compile, so a lens and a film are accepted only where every origin on them stays inside that magnitude.
// A panorama's origins are the pinhole's.
static void check_lens_reach(const akr_scene* s, const HostLens& lens, const HostProjection& proj, uint32_t width, uint32_t height) {
    const CompiledScene& cs = s->cs;
    const bool ortho = proj.type == AKR_PROJECTION_ORTHOGRAPHIC;
    if ((lens.radius == 0.0f && !ortho) || (cs.bvh_nodes.empty() && !cs.instanced.on)) return;  // (the exhaustive walk has no boxes)
    const float* c2w = s->flat.camera.c2w;
    float bound[3], moved[16], half_x = 0.0f, half_y = 0.0f;
    if (ortho) ortho_film_half_extents(proj.ortho_scale, width, height, &half_x, &half_y);
    lens_origin_bound(c2w, lens.radius, half_x, half_y, bound);
    std::memcpy(moved, c2w, sizeof moved);
    bool inside = true;
    for (int a = 0; a < 3; a++) {
        const float m = std::max(std::max(std::fabs(cs.scene_lo[a]), std::fabs(cs.scene_hi[a])), std::fabs(c2w[12 + a]));
        if (bound[a] > m) inside = false;
        moved[12 + a] = bound[a];
    }
    // flattened scenes: the padding looks at max(diagonal, reach) only -- unchanged is enough; kept scenes also use the per-axis magnitudes
    if (inside || (!cs.instanced.on && bvh_box_padding(cs.scene_lo, cs.scene_hi, moved) == bvh_box_padding(cs.scene_lo, cs.scene_hi, c2w))) return;
    char msg[400];
    if (ortho)
        std::snprintf(msg, sizeof msg, "projection: an orthographic film of scale %g%s puts ray origins at coordinates up to (%g, %g, %g), beyond the magnitude the scene's "
                      "acceleration structure was padded for (its box and the camera position); use a smaller ortho_scale", proj.ortho_scale,
                      lens.radius > 0.0f ? " with its lens" : "", bound[0], bound[1], bound[2]);
    else
        std::snprintf(msg, sizeof msg, "lens: a lens of radius %g puts ray origins at coordinates up to (%g, %g, %g), beyond the magnitude the scene's acceleration "
                      "structure was padded for (its box and the camera position); use a smaller radius", lens.radius, bound[0], bound[1], bound[2]);
    throw std::invalid_argument(msg);
}
static void check_lens_reach(const akr_scene* s, const HostLens& lens, const HostProjection& proj) { check_lens_reach(s, lens, proj, s->flat.camera.width, s->flat.camera.height); }
static void refuse_lens_on_panorama(const HostLens& lens, const HostProjection& proj, const char* who) {
    if (lens.radius > 0.0f && proj.type == AKR_PROJECTION_PANORAMA)
        throw std::invalid_argument(std::string(who) + ": a panorama camera has no lens (remove the lens, or choose another projection)");
}

void akr_api::scene_finish(akr_scene* s, const TuningOptions& opt) {
    akr_context* ctx = s->ctx;
    compile_scene(s->flat, opt, s->cs);
    compile_punctual(s->flat, s->cs);
    compile_environment(s->flat, s->cs);
    refuse_lens_on_panorama(s->flat.lens, s->flat.projection, "scene");
    check_lens_reach(s, s->flat.lens, s->flat.projection);  // (a lens from the file, option `lens`; an orthographic camera of the file)
    CompiledScene& cs = s->cs;
    camera_matrices(s->flat.camera, s->r2c, s->c2w, &s->c2w_identity, &s->flat.projection);
    if (!ctx) {  // host-only scene: inspectable, not renderable
        s->ggx_host = s->flat.ggx_table.empty() ? std::vector<float>(4096, 0.0f) : s->flat.ggx_table;
        std::memset(&s->dscene, 0, sizeof s->dscene);
        return;
    }
    ctx->bind();
    if (cs.bvh_nodes.empty() && !cs.instanced.on && cs.woop.size() > walk_bound_word(cs.n_tris))  // exhaustive path: the pair walk's origin bound, in the records' padding
        cs.woop[walk_bound_word(cs.n_tris)] = walk_origin_bound(cs.woop, cs.n_tris);
    s->woop.upload(cs.woop);
    s->tri_gid.upload(cs.tri_gid);
    s->shade.upload(cs.shade);
    s->normals.upload(cs.normals);
    s->inst.upload(cs.inst);
    s->materials.upload(cs.materials);
    s->area_entries.upload(cs.area_entries);
    s->area_pdf.upload(cs.area_pdf);
    s->inst_tri_offset.upload(cs.inst_tri_offset);
    s->bvh_nodes.upload(cs.instanced.on ? cs.instanced.nodes : cs.bvh_nodes);
    if (cs.instanced.on) {
        s->in2_tlas_leaves.upload(cs.instanced.tlas_leaves);
        s->in2_mesh_tris.upload(cs.instanced.mesh_tris);
        s->in2_mesh_pos.upload(cs.instanced.mesh_pos);
        s->in2_mesh_meta.upload(cs.instanced.mesh_meta);
        s->in2_mesh_normals.upload(cs.instanced.mesh_normals);
        s->in2_inst_mats.upload(cs.instanced.inst_mats);
    }
    if (cs.has_textures) {
        s->tex_nodes.upload(cs.tex_nodes);
        s->tex_images.upload(cs.images);
        s->tex_texels.upload(cs.texels);
        s->tex_mat_inputs.upload(cs.mat_inputs);
    }
    ensure_ggx_table(s);
    DScene& d = s->dscene;
    std::memset(&d, 0, sizeof d);
    d.woop = s->woop.as<float4>();
    d.tri_gid = s->tri_gid.as<uint32_t>();
    d.shade = s->shade.as<float4>();
    d.normals = s->normals.as<float4>();
    d.inst = s->inst.as<float4>();
    d.materials = s->materials.as<DMaterial>();
    d.ggx_table = s->ggx_table.as<float>();
    d.area_entries = s->area_entries.as<AliasEntry>();
    d.area_pdf = s->area_pdf.as<float>();
    d.inst_tri_offset = s->inst_tri_offset.as<uint32_t>();
    upload_lights(s);  // light tables, environment
    d.bvh_nodes = s->bvh_nodes.as<uint4>();
    d.n_tris = cs.n_tris;
    d.n_nodes = scene_n_nodes(cs);
    d.has_alpha = cs.has_alpha ? 1u : 0u;
    d.bvh_stack_depth = scene_stack_depth(cs);
    if (cs.instanced.on) {
        d.in2.tlas_leaves = s->in2_tlas_leaves.as<uint4>();
        d.in2.mesh_tris = s->in2_mesh_tris.as<float4>();
        d.in2.mesh_pos = s->in2_mesh_pos.as<uint32_t>();
        d.in2.mesh_meta = s->in2_mesh_meta.as<uint32_t>();
        d.in2.mesh_normals = s->in2_mesh_normals.as<float4>();
        d.in2.inst_mats = s->in2_inst_mats.as<uint32_t>();
        d.in2.on = 1u;
        d.in2.n_instances = (uint32_t)s->flat.instances.size();
    }
    d.plane_share_mask = 0;
    if (cs.bvh_nodes.empty() && !cs.instanced.on)  // exhaustive path (<= 64 triangles): which records repeat their predecessor's plane row
        for (uint32_t k = 1; k < d.n_tris && k < 64; k++)
            if (std::memcmp(&cs.woop[12ull * k + 8], &cs.woop[12ull * (k - 1) + 8], 16) == 0) d.plane_share_mask |= 1ull << k;
    if (cs.has_textures) {
        d.tex.nodes = s->tex_nodes.as<DNode>();
        d.tex.images = s->tex_images.as<DImage>();
        d.tex.texels = s->tex_texels.as<uint32_t>();
        d.tex.mat_inputs = s->tex_mat_inputs.as<MatInputs>();
    }
    if (cs.instanced.on) {  // which instance-triangles take their even neighbour's plane row: one bit each, decided on the device (dinst_trav.h resolve_pending)
        const size_t words = ((size_t)cs.n_tris + 31u) / 32u;
        s->in2_share_bits.alloc(std::max<size_t>(words, 1u) * 4u);
        HIP_CHECK(hipMemsetAsync(s->in2_share_bits.p, 0, s->in2_share_bits.bytes, ctx->stream));
        HIP_CHECK(launch_inst_share_bits(d, s->in2_share_bits.as<uint32_t>(), s->in2_mesh_tris.as<uint32_t>(), ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        d.in2.share_bits = s->in2_share_bits.as<uint32_t>();
    }
    count_device_bytes(s);
}

// the arrays scene_finish uploads, in bytes (the packed light tables repeat the alias tables: 16 B per entry)
static uint64_t compiled_scene_bytes(const CompiledScene& cs) {
    auto b = [](const auto& v) { return (uint64_t)v.size() * sizeof(v[0]); };
    uint64_t n = b(cs.woop) + b(cs.tri_gid) + b(cs.shade) + b(cs.normals) + b(cs.inst) + b(cs.materials) + b(cs.light_entries) + b(cs.light_pdf) +
                 b(cs.light_inst) + b(cs.light_tri_offset) + b(cs.light_n_tris) + b(cs.area_entries) + b(cs.area_pdf) + b(cs.inst_tri_offset) +
                 16ull * (cs.light_entries.size() + cs.area_entries.size() + cs.n_lights) + b(cs.bvh_nodes) + b(cs.tex_nodes) + b(cs.images) + b(cs.texels) +
                 b(cs.mat_inputs);
    n += (uint64_t)punctual_device_records(cs.punct, cs.punct_tree).size() * sizeof(DPunct);
    n += b(cs.env.texels) + 16ull * (cs.env.marginal_entries.size() + cs.env.conditional_entries.size()) + (cs.env.on ? sizeof(DEnv) : 0u);
    const CompiledScene::Instanced& is = cs.instanced;
    return n + b(is.nodes) + b(is.tlas_leaves) + b(is.mesh_tris) + b(is.mesh_pos) + b(is.mesh_meta) + b(is.mesh_normals) + b(is.inst_mats) + (is.on ? std::max<uint64_t>(((uint64_t)cs.n_tris + 31u) / 32u, 1u) * 4u : 0u);
}

extern "C" {

AKR_API int32_t akr_scene_create(akr_context* ctx, const akr_scene_desc* desc, akr_scene** out) {
    if (!desc || !out) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_create: NULL argument");
    *out = nullptr;
    return guarded([&] {
        auto s = std::make_unique<akr_scene>();
        s->ctx = ctx;
        const TuningOptions opt = tuning();  // the one look at the options of this scene's making
        s->flat = FlatScene::from_desc(*desc);
        s->flat.light_tree = opt.light_tree;
        scene_finish(s.get(), opt);
        *out = s.release();
    });
}
AKR_API int32_t akr_scene_load(akr_context* ctx, const char* path, uint32_t width, uint32_t height, akr_scene** out) {
    if (!path || !out) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_load: NULL argument");
    *out = nullptr;
    return guarded([&] {
        auto s = std::make_unique<akr_scene>();
        s->ctx = ctx;
        const TuningOptions opt = tuning();  // the one look at the options of this load
        s->flat = load_scene_json(path, opt);
        s->flat.light_tree = opt.light_tree;
        if (width && height) {
            s->flat.camera.width = width;
            s->flat.camera.height = height;
        }
        scene_finish(s.get(), opt);
        *out = s.release();
    });
}
AKR_API int32_t akr_scene_destroy(akr_scene* scene) {
    if (!scene) return AKR_OK;
    return guarded([&] {
        if (scene->ctx) (void)hipSetDevice(scene->ctx->device);
        delete scene;
    });
}
AKR_API int32_t akr_scene_set_resolution(akr_scene* s, uint32_t width, uint32_t height) {
    if (!s || !width || !height) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_set_resolution: bad argument");
    // (a session's film, sampler states and parameter block are sized for the resolution it began with)
    if (s->sessions.load() != 0) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_set_resolution: a session holds the scene (end it first)");
    if (s->flat.projection.type == AKR_PROJECTION_ORTHOGRAPHIC) {  // (the film's smaller side changes with the aspect: the reach check of akr_scene_set_projection)
        const int32_t rc = guarded([&] { check_lens_reach(s, s->flat.lens, s->flat.projection, width, height); });
        if (rc != AKR_OK) return rc;
    }
    s->flat.camera.width = width;
    s->flat.camera.height = height;
    camera_matrices(s->flat.camera, s->r2c, s->c2w, &s->c2w_identity, &s->flat.projection);
    return AKR_OK;
}
AKR_API int32_t akr_scene_get_info(const akr_scene* s, akr_scene_info* info) {
    if (!s || !info) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_get_info: NULL argument");
    info->width = s->flat.camera.width;
    info->height = s->flat.camera.height;
    info->n_instances = (uint32_t)s->flat.instances.size();
    info->n_triangles = s->cs.n_tris;
    info->n_materials = (uint32_t)s->flat.materials.size();
    info->n_lights = s->cs.n_lights;
    info->n_bvh_nodes = (uint32_t)((s->cs.instanced.on ? s->cs.instanced.nodes.size() : s->cs.bvh_nodes.size()) / kBvhNodeWords);
    info->uses_bvh = (s->cs.bvh_nodes.empty() && !s->cs.instanced.on) ? 0u : (s->cs.instanced.on ? 2u : 1u);  // 2 = two-level (meshes + instances)
    info->device_bytes = s->device_bytes ? s->device_bytes : compiled_scene_bytes(s->cs);  // (a host-only scene: what an upload would take)
    info->node_bytes = (s->cs.bvh_nodes.empty() && !s->cs.instanced.on) ? 0u : kBvhNodeWords * 4u;   // bytes a traversal reads per node visit
    info->node_stride_bytes = (s->cs.bvh_nodes.empty() && !s->cs.instanced.on) ? 0u : kBvhNodeWords * 4u;
    info->tri_bytes = (s->cs.bvh_nodes.empty() && !s->cs.instanced.on) ? 48u : kBvhTriWords * 4u;
    info->bvh_depth = s->cs.bvh_depth;
    return AKR_OK;
}
AKR_API int32_t akr_scene_set_environment(akr_scene* s, const akr_environment_desc* desc) {
    if (!s) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_set_environment: scene is NULL");
    return guarded([&] {
        if (s->sessions.load() != 0) throw std::invalid_argument("akr_scene_set_environment: a session holds the scene (end it first)");
        HostEnvironment env;
        if (desc) env = environment_from_desc(*desc);
        std::swap(s->flat.env, env);
        try {
            compile_environment(s->flat, s->cs);
        } catch (...) {
            std::swap(s->flat.env, env);  // (compile_environment refuses before it changes anything)
            throw;
        }
        if (s->ctx) {
            s->ctx->bind();
            upload_lights(s);
            count_device_bytes(s);
        }
    });
}
AKR_API int32_t akr_scene_get_environment(const akr_scene* s, akr_environment_desc* out) {
    if (!s || !out) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_get_environment: NULL argument");
    const HostEnvironment& e = s->flat.env;
    std::memset(out, 0, sizeof *out);
    for (int k = 0; k < 9; k++) out->rotation[k] = e.rotation[k];
    if (!e.set) return AKR_OK;
    out->width = e.width;
    out->height = e.height;
    out->filter = e.filter;
    out->texels = e.texels.empty() ? nullptr : e.texels.data();
    for (int c = 0; c < 3; c++) out->color[c] = e.color[c];
    out->strength = e.strength;
    return AKR_OK;
}
// the punctual lights changed: light table and records compiled again (the change is taken back if that is refused), uploaded, the colour sets' copies dropped
static void punctual_lights_changed(akr_scene* s, std::vector<akr_punctual_light_desc>& before) {
    try {
        compile_punctual(s->flat, s->cs);
    } catch (...) {
        std::swap(s->flat.punct, before);  // (compile_punctual refuses before it changes anything)
        throw;
    }
    if (s->ctx) {
        s->ctx->bind();
        upload_lights(s);
        count_device_bytes(s);
        std::lock_guard<std::mutex> lock(s->color_sets_mutex);
        for (auto& kv : s->color_sets) kv.second->punct.release();  // folded again by the next session of that pipeline (api_pt.cpp base_begin)
    }
}
AKR_API int32_t akr_scene_add_punctual_light(akr_scene* s, const akr_punctual_light_desc* desc) {
    if (!s || !desc) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_add_punctual_light: NULL argument");
    return guarded([&] {
        if (s->sessions.load() != 0) throw std::invalid_argument("akr_scene_add_punctual_light: a session holds the scene (end it first)");
        akr_punctual_light_desc checked;
        if (!punctual_from_desc(*desc, checked)) return;  // no light
        std::vector<akr_punctual_light_desc> before = s->flat.punct;
        s->flat.punct.push_back(checked);
        punctual_lights_changed(s, before);
    });
}
AKR_API int32_t akr_scene_clear_punctual_lights(akr_scene* s) {
    if (!s) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_clear_punctual_lights: scene is NULL");
    return guarded([&] {
        if (s->sessions.load() != 0) throw std::invalid_argument("akr_scene_clear_punctual_lights: a session holds the scene (end it first)");
        std::vector<akr_punctual_light_desc> before = s->flat.punct;
        s->flat.punct.clear();
        punctual_lights_changed(s, before);
    });
}
AKR_API int32_t akr_scene_set_light_tree(akr_scene* s, uint32_t on) {
    if (!s) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_set_light_tree: scene is NULL");
    return guarded([&] {
        if (s->sessions.load() != 0) throw std::invalid_argument("akr_scene_set_light_tree: a session holds the scene (end it first)");
        const int before_mode = s->flat.light_tree;
        s->flat.light_tree = on ? 1 : 0;
        std::vector<akr_punctual_light_desc> before = s->flat.punct;
        try {
            punctual_lights_changed(s, before);
        } catch (...) {
            s->flat.light_tree = before_mode;
            throw;
        }
    });
}
AKR_API int32_t akr_scene_get_light_tree(const akr_scene* s, uint32_t* on, uint32_t* n_nodes) {
    if (!s) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_get_light_tree: scene is NULL");
    if (on) *on = s->flat.light_tree != 0 ? 1u : 0u;
    if (n_nodes) *n_nodes = (uint32_t)(s->cs.punct_tree.size() / 8);
    return AKR_OK;
}
AKR_API int32_t akr_scene_punctual_light_count(const akr_scene* s, uint32_t* count) {
    if (!s || !count) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_punctual_light_count: NULL argument");
    *count = (uint32_t)s->flat.punct.size();
    return AKR_OK;
}
AKR_API int32_t akr_scene_get_punctual_light(const akr_scene* s, uint32_t index, akr_punctual_light_desc* out) {
    if (!s || !out || index >= s->flat.punct.size()) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_get_punctual_light: bad argument");
    *out = s->flat.punct[index];
    return AKR_OK;
}
AKR_API int32_t akr_scene_set_lens(akr_scene* s, const akr_lens_desc* desc) {
    if (!s) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_set_lens: scene is NULL");
    return guarded([&] {
        if (s->sessions.load() != 0) throw std::invalid_argument("akr_scene_set_lens: a session holds the scene (end it first)");
        HostLens lens;
        if (desc) lens = lens_from_values(desc->radius, desc->focal_distance);
        refuse_lens_on_panorama(lens, s->flat.projection, "akr_scene_set_lens");
        check_lens_reach(s, lens, s->flat.projection);
        s->flat.lens = lens;
    });
}
AKR_API int32_t akr_projection_desc_default(akr_projection_desc* desc) {
    if (!desc) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_projection_desc_default: desc is NULL");
    const HostProjection p;
    desc->type = p.type;
    desc->ortho_scale = p.ortho_scale;
    desc->longitude_min = p.lon_min; desc->longitude_max = p.lon_max;
    desc->latitude_min = p.lat_min; desc->latitude_max = p.lat_max;
    return AKR_OK;
}
AKR_API int32_t akr_scene_set_projection(akr_scene* s, const akr_projection_desc* desc) {
    if (!s) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_set_projection: scene is NULL");
    return guarded([&] {
        if (s->sessions.load() != 0) throw std::invalid_argument("akr_scene_set_projection: a session holds the scene (end it first)");
        HostProjection proj;
        if (desc) proj = projection_from_values(desc->type, desc->ortho_scale, desc->longitude_min, desc->longitude_max, desc->latitude_min, desc->latitude_max);
        refuse_lens_on_panorama(s->flat.lens, proj, "akr_scene_set_projection");
        check_lens_reach(s, s->flat.lens, proj);
        s->flat.projection = proj;
        camera_matrices(s->flat.camera, s->r2c, s->c2w, &s->c2w_identity, &s->flat.projection);
    });
}
AKR_API int32_t akr_scene_get_projection(const akr_scene* s, akr_projection_desc* out) {
    if (!s || !out) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_get_projection: NULL argument");
    const HostProjection& p = s->flat.projection;
    out->type = p.type;
    out->ortho_scale = p.ortho_scale;
    out->longitude_min = p.lon_min; out->longitude_max = p.lon_max;
    out->latitude_min = p.lat_min; out->latitude_max = p.lat_max;
    return AKR_OK;
}
AKR_API int32_t akr_scene_get_lens(const akr_scene* s, akr_lens_desc* out) {
    if (!s || !out) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_get_lens: NULL argument");
    out->radius = s->flat.lens.radius;
    out->focal_distance = s->flat.lens.focal_distance;
    return AKR_OK;
}
AKR_API int32_t akr_scene_get_light(const akr_scene* s, uint32_t light, uint32_t* instance, float* power, float* pdf) {
    if (!s || light >= s->cs.n_lights) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_get_light: bad argument");
    if (instance) *instance = s->cs.light_inst[light];
    if (power) *power = s->cs.light_power[light];
    if (pdf) *pdf = s->cs.light_pdf[light];
    return AKR_OK;
}
AKR_API int32_t akr_scene_get_ggx_table(const akr_scene* s, float* dst) {
    if (!s || !dst) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_get_ggx_table: NULL argument");
    std::memcpy(dst, s->ggx_host.data(), 4096 * sizeof(float));
    return AKR_OK;
}
AKR_API int32_t akr_scene_get_desc_counts(const akr_scene* s, uint32_t* n_meshes, uint32_t* n_instances, uint32_t* n_materials) {
    if (!s) return fail(AKR_ERR_INVALID_ARGUMENT, "scene is NULL");
    if (n_meshes) *n_meshes = (uint32_t)s->flat.meshes.size();
    if (n_instances) *n_instances = (uint32_t)s->flat.instances.size();
    if (n_materials) *n_materials = (uint32_t)s->flat.materials.size();
    return AKR_OK;
}
AKR_API int32_t akr_scene_get_mesh(const akr_scene* s, uint32_t i, akr_mesh_desc* out) {
    if (!s || !out || i >= s->flat.meshes.size()) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_get_mesh: bad argument");
    const HostMesh& m = s->flat.meshes[i];
    out->n_vertices = (uint32_t)(m.vertices.size() / 3);
    out->n_triangles = m.n_triangles();
    out->vertices = m.vertices.data();
    out->indices = m.indices.data();
    out->uvs = m.uvs.empty() ? nullptr : m.uvs.data();
    out->normals = m.normals.empty() ? nullptr : m.normals.data();
    out->tangents = m.tangents.empty() ? nullptr : m.tangents.data();
    out->material_slots = m.slots.empty() ? nullptr : m.slots.data();
    return AKR_OK;
}
AKR_API int32_t akr_scene_get_instance(const akr_scene* s, uint32_t i, akr_instance_desc* out) {
    if (!s || !out || i >= s->flat.instances.size()) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_get_instance: bad argument");
    const HostInstance& h = s->flat.instances[i];
    out->mesh = h.mesh;
    out->n_materials = (uint32_t)h.materials.size();
    out->materials = h.materials.data();
    std::memcpy(out->transform, h.transform, sizeof out->transform);
    return AKR_OK;
}
AKR_API int32_t akr_scene_get_material(const akr_scene* s, uint32_t i, akr_material_desc* out) {
    if (!s || !out || i >= s->flat.materials.size()) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_get_material: bad argument");
    *out = s->flat.materials[i];
    return AKR_OK;
}
AKR_API int32_t akr_scene_get_image_count(const akr_scene* s, uint32_t* n) {
    if (!s || !n) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_get_image_count: NULL argument");
    *n = (uint32_t)s->flat.images.size();
    return AKR_OK;
}
AKR_API int32_t akr_scene_get_image(const akr_scene* s, uint32_t i, akr_image_desc* out) {
    if (!s || !out || i >= s->flat.images.size()) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_get_image: bad argument");
    const HostImage& h = s->flat.images[i];
    out->width = h.width; out->height = h.height; out->format = h.format; out->filter = h.filter; out->address = h.address; out->_pad = 0;
    out->texels = h.words.data();
    return AKR_OK;
}
AKR_API int32_t akr_scene_get_material_graph(const akr_scene* s, uint32_t i, akr_material_graph* out) {
    if (!s || !out || i >= s->flat.materials.size()) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_get_material_graph: bad argument");
    std::memset(out, 0, sizeof *out);
    for (uint32_t& k : out->input) k = AKR_NODE_NONE;
    if (i < s->flat.graphs.size()) {
        const HostGraph& g = s->flat.graphs[i];
        out->n_nodes = (uint32_t)g.nodes.size();
        out->nodes = g.nodes.empty() ? nullptr : g.nodes.data();
        std::memcpy(out->input, g.input, sizeof out->input);
    }
    return AKR_OK;
}
AKR_API int32_t akr_scene_get_camera(const akr_scene* s, akr_camera_desc* out) {
    if (!s || !out) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_get_camera: NULL argument");
    *out = s->flat.camera;
    return AKR_OK;
}

AKR_API int32_t akr_scene_get_array(const akr_scene* s, int32_t which, const void** ptr, uint64_t* bytes) {
    if (!s || !ptr || !bytes) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_get_array: NULL argument");
    const CompiledScene& cs = s->cs;
    auto set = [&](const void* p, size_t n) { *ptr = n ? p : nullptr; *bytes = n; };
    switch (which) {
        case AKR_ARRAY_WOOP: set(cs.woop.data(), cs.woop.size() * 4); break;
        case AKR_ARRAY_TRI_GID: set(cs.tri_gid.data(), cs.tri_gid.size() * 4); break;
        case AKR_ARRAY_SHADE: set(cs.shade.data(), cs.shade.size() * 4); break;
        case AKR_ARRAY_INSTANCES: set(cs.inst.data(), cs.inst.size() * 4); break;
        case AKR_ARRAY_MATERIALS: set(cs.materials.data(), cs.materials.size() * sizeof(DMaterial)); break;
        case AKR_ARRAY_BVH_NODES:
            if (cs.instanced.on) set(cs.instanced.nodes.data(), cs.instanced.nodes.size() * 4);
            else set(cs.bvh_nodes.data(), cs.bvh_nodes.size() * 4);
            break;
        case AKR_ARRAY_LIGHT_ENTRIES: set(cs.light_entries.data(), cs.light_entries.size() * sizeof(AliasEntry)); break;
        case AKR_ARRAY_LIGHT_PDF: set(cs.light_pdf.data(), cs.light_pdf.size() * 4); break;
        case AKR_ARRAY_AREA_ENTRIES: set(cs.area_entries.data(), cs.area_entries.size() * sizeof(AliasEntry)); break;
        case AKR_ARRAY_AREA_PDF: set(cs.area_pdf.data(), cs.area_pdf.size() * 4); break;
        case AKR_ARRAY_INST_TRI_OFFSET: set(cs.inst_tri_offset.data(), cs.inst_tri_offset.size() * 4); break;
        case AKR_ARRAY_R2C: set(s->r2c, 64); break;
        case AKR_ARRAY_C2W: set(s->c2w, 64); break;
        case AKR_ARRAY_TEX_NODES: set(cs.tex_nodes.data(), cs.tex_nodes.size() * sizeof(DNode)); break;
        case AKR_ARRAY_TEX_IMAGES: set(cs.images.data(), cs.images.size() * sizeof(DImage)); break;
        case AKR_ARRAY_TEX_TEXELS: set(cs.texels.data(), cs.texels.size() * 4); break;
        case AKR_ARRAY_MAT_INPUTS: set(cs.mat_inputs.data(), cs.mat_inputs.size() * sizeof(MatInputs)); break;
        case AKR_ARRAY_INST_LEAVES: set(cs.instanced.tlas_leaves.data(), cs.instanced.tlas_leaves.size() * 4); break;
        case AKR_ARRAY_MESH_TRIS: set(cs.instanced.mesh_tris.data(), cs.instanced.mesh_tris.size() * 4); break;
        case AKR_ARRAY_MESH_POS: set(cs.instanced.mesh_pos.data(), cs.instanced.mesh_pos.size() * 4); break;
        case AKR_ARRAY_MESH_META: set(cs.instanced.mesh_meta.data(), cs.instanced.mesh_meta.size() * 4); break;
        case AKR_ARRAY_MESH_NORMALS: set(cs.instanced.mesh_normals.data(), cs.instanced.mesh_normals.size() * 4); break;
        case AKR_ARRAY_ENV_MARGINAL_ENTRIES: set(cs.env.marginal_entries.data(), cs.env.marginal_entries.size() * sizeof(AliasEntry)); break;
        case AKR_ARRAY_ENV_MARGINAL_PDF: set(cs.env.marginal_pdf.data(), cs.env.marginal_pdf.size() * 4); break;
        case AKR_ARRAY_ENV_CONDITIONAL_ENTRIES: set(cs.env.conditional_entries.data(), cs.env.conditional_entries.size() * sizeof(AliasEntry)); break;
        case AKR_ARRAY_ENV_CONDITIONAL_PDF: set(cs.env.conditional_pdf.data(), cs.env.conditional_pdf.size() * 4); break;
        case AKR_ARRAY_ENV_TEXELS: set(cs.env.texels.data(), cs.env.texels.size() * 4); break;
        case AKR_ARRAY_PUNCTUAL_LIGHTS: set(cs.punct.data(), cs.punct.size() * sizeof(DPunct)); break;
        case AKR_ARRAY_LIGHT_TREE: set(cs.punct_tree.data(), cs.punct_tree.size() * 4); break;
        default: return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_get_array: unknown array id");
    }
    return AKR_OK;
}

AKR_API int32_t akr_scene_spec_source(akr_scene* scene, char* dst, uint64_t capacity, uint64_t* length) {
    if (!scene || !length) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_spec_source: NULL argument");
    return guarded([&] {
        std::lock_guard<std::mutex> lock(scene->spec_mutex);
        if (!scene->spec_header_made) {
            scene->spec_header = generate_scene_spec(scene->cs);
            scene->spec_header_made = true;
        }
        *length = scene->spec_header.size();
        if (dst && capacity) {
            const size_t n = std::min<size_t>(capacity - 1, scene->spec_header.size());
            std::memcpy(dst, scene->spec_header.data(), n);
            dst[n] = 0;
        }
    });
}
AKR_API int32_t akr_host_spec_compile(akr_scene* scene, uint32_t flags, uint32_t min_waves, const char* arch, uint64_t* code_bytes, char* log, uint32_t log_len) {
    if (!scene || !code_bytes) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_spec_compile: NULL argument");
    return guarded([&] {
        std::string header;
        {
            std::lock_guard<std::mutex> lock(scene->spec_mutex);
            if (!scene->spec_header_made) {
                scene->spec_header = generate_scene_spec(scene->cs);
                scene->spec_header_made = true;
            }
            header = scene->spec_header;
        }
        if (header.empty()) throw Unsupported("unsupported: the scene has no per-scene code (no texture-fed material, or too many shader kinds)");
        const PtVariant v = pt_variant_from_bits(flags);
        if (!pt_variant_compiled(v)) throw std::invalid_argument("per-scene kernel: the flags name a variant that does not exist (kernels.h pt_variant_compiled)");
        std::vector<char> code;
        std::string text;
        const bool ok = spec_compile(header, v, (int)min_waves, arch && *arch ? arch : "gfx950", code, text);
        if (log && log_len) std::snprintf(log, log_len, "%s", text.c_str());
        if (!ok) throw RenderError("per-scene kernel did not compile: " + text.substr(0, 1500));
        *code_bytes = code.size();
    });
}
// the helper process's entry (akari-cli --spec-compile): generated text in, code object file out; always this process's hiprtc
AKR_API int32_t akr_host_spec_compile_text(const char* spec_header, uint32_t flags, uint32_t min_waves, const char* arch, const char* out_path) {
    if (!spec_header || !arch || !out_path) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_host_spec_compile_text: NULL argument");
    return guarded([&] {
        const PtVariant v = pt_variant_from_bits(flags);
        if (!pt_variant_compiled(v)) throw std::invalid_argument("per-scene kernel: the flags name a variant that does not exist (kernels.h pt_variant_compiled)");
        std::vector<char> code;
        std::string log;
        if (!spec_compile(spec_header, v, (int)min_waves, arch, code, log, /*in_process=*/true)) throw RenderError("per-scene kernel did not compile: " + log.substr(0, 3000));
        FILE* f = std::fopen(out_path, "wb");
        if (!f) throw IoError(std::string("cannot open ") + out_path);
        const size_t n = std::fwrite(code.data(), 1, code.size(), f);
        std::fclose(f);
        if (n != code.size()) throw IoError(std::string("short write to ") + out_path);
    });
}
}  // extern "C"
