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

// ------------------------------------------------------------------------------------------------------------------------ a scene's device tables
// ONE list, kSceneTables: upload, release, both byte counts and akr_scene_get_array walk it, so a new table is one row, plus its
// field of DScene if a kernel reads it. Beside the list, as code of their own: the GGX table (ensure_ggx_table), the kept scenes' share bits (a kernel
// fills them: scene_finish) and the walk-bound word in woop's padding.
struct Bytes { const void* p; size_t n; };
template <typename T>
static Bytes bytes_of(const std::vector<T>& v) { return {v.data(), v.size() * sizeof(T)}; }
// the tables the device reads in a form of its own, packed when a walk's first row asks: the light tables and the environment's so that each level of
// sampling is ONE gather (device/dgeom.h, dscene.h), the punctual lights' records with the tree's nodes behind them
struct Packed {
    bool made = false;
    std::vector<AliasPacked> light_alias, area_alias, env_marginal, env_conditional;
    std::vector<LightRec> lights;
    std::vector<DPunct> punct;
    DEnv env;
    Packed& of(const CompiledScene& cs) {
        if (made) return *this;
        made = true;
        packed_light_tables(cs, light_alias, area_alias, lights);
        punct = punctual_device_records(cs.punct, cs.punct_tree);
        if (cs.env.on) {
            pack_alias(cs.env.marginal_entries, cs.env.marginal_pdf, 0, cs.env.h, env_marginal);
            for (uint32_t y = 0; y < cs.env.h; y++)  // (j is relative to the row)
                pack_alias(cs.env.conditional_entries, cs.env.conditional_pdf, (size_t)y * cs.env.w, cs.env.w, env_conditional);
        }
        return *this;
    }
};
// DScene.env's record: the environment's three tables where the rows before this one put them (null in a host-only scene), and how to read them
static Bytes env_record(const akr_scene& s, Packed& pk) {
    const CompiledScene& cs = s.cs;
    DEnv& rec = pk.env;
    std::memset(&rec, 0, sizeof rec);
    rec.texels = s.env_texels.as<float4>();
    rec.marginal = s.env_marginal.as<AliasPacked>();
    rec.conditional = s.env_conditional.as<AliasPacked>();
    for (int k = 0; k < 9; k++) rec.rot[k] = cs.env.rot_t[k];
    rec.w = cs.env.w;
    rec.h = cs.env.h;
    rec.filter = cs.env.filter;
    rec.light = cs.n_lights - 1;
    return {&rec, cs.env.on ? sizeof rec : 0u};
}
enum When { ALWAYS, TEXTURED, KEPT, ENV };
static bool exists(When w, const CompiledScene& cs) { return w == ALWAYS || (w == TEXTURED && cs.has_textures) || (w == KEPT && cs.instanced.on) || (w == ENV && cs.env.on); }
enum Part {
    GEOM,    // uploaded once, by scene_finish
    LIGHT,   // a light table: uploaded again when the environment or the punctual lights change (upload_lights)
    PACKED,  // ... whose bytes are Packed's: they live as long as the walk that asked, so no AKR_ARRAY_* id may show them (akr_scene_get_array skips the row)
    SHOWN    // no table: host bytes the device reads only inside a packed one -- a row for akr_scene_get_array alone (no buf, `when` and `bind` unread)
};
constexpr int NO_ID = -1;
struct SceneTable {
    int array;                                     // the AKR_ARRAY_* id that shows the host bytes, or NO_ID
    Bytes (*src)(const akr_scene& s, Packed& pk);  // the host bytes
    DevBuf akr_scene::*buf = nullptr;              // owns the table
    Part part = SHOWN;
    When when = ALWAYS;                            // it exists
    void (*bind)(DScene& d, void* p) = nullptr;    // the pointer the kernels find it by; null: no field of DScene
};
#define SRC(v) [](const akr_scene& s, Packed& pk) -> Bytes { (void)s, (void)pk; return bytes_of(v); }
#define TO(field) [](DScene& d, void* p) { d.field = (decltype(d.field))p; }
static const SceneTable kSceneTables[] = {  // in the order of upload
    {AKR_ARRAY_WOOP, SRC(s.cs.woop), &akr_scene::woop, GEOM, ALWAYS, TO(woop)},
    {AKR_ARRAY_TRI_GID, SRC(s.cs.tri_gid), &akr_scene::tri_gid, GEOM, ALWAYS, TO(tri_gid)},
    {AKR_ARRAY_SHADE, SRC(s.cs.shade), &akr_scene::shade, GEOM, ALWAYS, TO(shade)},
    {NO_ID, SRC(s.cs.normals), &akr_scene::normals, GEOM, ALWAYS, TO(normals)},
    {AKR_ARRAY_INSTANCES, SRC(s.cs.inst), &akr_scene::inst, GEOM, ALWAYS, TO(inst)},
    {AKR_ARRAY_MATERIALS, SRC(s.cs.materials), &akr_scene::materials, GEOM, ALWAYS, TO(materials)},
    {AKR_ARRAY_AREA_ENTRIES, SRC(s.cs.area_entries), &akr_scene::area_entries, GEOM, ALWAYS, TO(area_entries)},
    {AKR_ARRAY_AREA_PDF, SRC(s.cs.area_pdf), &akr_scene::area_pdf, GEOM, ALWAYS, TO(area_pdf)},
    {AKR_ARRAY_INST_TRI_OFFSET, SRC(s.cs.inst_tri_offset), &akr_scene::inst_tri_offset, GEOM, ALWAYS, TO(inst_tri_offset)},
    // (a kept scene has no flattened tree, a flattened one no instanced vectors: compile_scene returns from compile_instanced_geometry before it builds one)
    {AKR_ARRAY_BVH_NODES, SRC(s.cs.instanced.on ? s.cs.instanced.nodes : s.cs.bvh_nodes), &akr_scene::bvh_nodes, GEOM, ALWAYS, TO(bvh_nodes)},
    {AKR_ARRAY_INST_LEAVES, SRC(s.cs.instanced.tlas_leaves), &akr_scene::in2_tlas_leaves, GEOM, KEPT, TO(in2.tlas_leaves)},  // meshes + instances (scene_inst.cpp)
    {AKR_ARRAY_MESH_TRIS, SRC(s.cs.instanced.mesh_tris), &akr_scene::in2_mesh_tris, GEOM, KEPT, TO(in2.mesh_tris)},
    {AKR_ARRAY_MESH_POS, SRC(s.cs.instanced.mesh_pos), &akr_scene::in2_mesh_pos, GEOM, KEPT, TO(in2.mesh_pos)},
    {AKR_ARRAY_MESH_META, SRC(s.cs.instanced.mesh_meta), &akr_scene::in2_mesh_meta, GEOM, KEPT, TO(in2.mesh_meta)},
    {AKR_ARRAY_MESH_NORMALS, SRC(s.cs.instanced.mesh_normals), &akr_scene::in2_mesh_normals, GEOM, KEPT, TO(in2.mesh_normals)},
    {NO_ID, SRC(s.cs.instanced.inst_mats), &akr_scene::in2_inst_mats, GEOM, KEPT, TO(in2.inst_mats)},
    {AKR_ARRAY_TEX_NODES, SRC(s.cs.tex_nodes), &akr_scene::tex_nodes, GEOM, TEXTURED, TO(tex.nodes)},
    {AKR_ARRAY_TEX_IMAGES, SRC(s.cs.images), &akr_scene::tex_images, GEOM, TEXTURED, TO(tex.images)},
    {AKR_ARRAY_TEX_TEXELS, SRC(s.cs.texels), &akr_scene::tex_texels, GEOM, TEXTURED, TO(tex.texels)},
    {AKR_ARRAY_MAT_INPUTS, SRC(s.cs.mat_inputs), &akr_scene::tex_mat_inputs, GEOM, TEXTURED, TO(tex.mat_inputs)},
    {AKR_ARRAY_LIGHT_ENTRIES, SRC(s.cs.light_entries), &akr_scene::light_entries, LIGHT, ALWAYS, TO(light_entries)},
    {AKR_ARRAY_LIGHT_PDF, SRC(s.cs.light_pdf), &akr_scene::light_pdf, LIGHT, ALWAYS, TO(light_pdf)},
    {NO_ID, SRC(s.cs.light_inst), &akr_scene::light_inst, LIGHT, ALWAYS, TO(light_inst)},
    {NO_ID, SRC(s.cs.light_tri_offset), &akr_scene::light_tri_offset, LIGHT, ALWAYS, TO(light_tri_offset)},
    {NO_ID, SRC(s.cs.light_n_tris), &akr_scene::light_n_tris, LIGHT, ALWAYS},  // (no reader: DScene.env took its field)
    {NO_ID, SRC(pk.of(s.cs).punct), &akr_scene::punct, PACKED, ALWAYS, TO(punct)},  // under the default colour pipeline (the others': api_pt.cpp color_set)
    {NO_ID, SRC(pk.of(s.cs).light_alias), &akr_scene::light_alias, PACKED, ALWAYS, TO(light_alias)},
    {NO_ID, SRC(pk.of(s.cs).area_alias), &akr_scene::area_alias, PACKED, ALWAYS, TO(area_alias)},
    {NO_ID, SRC(pk.of(s.cs).lights), &akr_scene::lights, PACKED, ALWAYS, TO(lights)},
    {AKR_ARRAY_ENV_TEXELS, SRC(s.cs.env.texels), &akr_scene::env_texels, LIGHT, ENV},  // the environment light (scene_env.cpp): found through env_rec
    {NO_ID, SRC(pk.of(s.cs).env_marginal), &akr_scene::env_marginal, PACKED, ENV},
    {NO_ID, SRC(pk.of(s.cs).env_conditional), &akr_scene::env_conditional, PACKED, ENV},
    {NO_ID, env_record, &akr_scene::env_rec, PACKED, ENV, TO(env)},
    // what the packed tables above were packed from
    {AKR_ARRAY_ENV_MARGINAL_ENTRIES, SRC(s.cs.env.marginal_entries)},
    {AKR_ARRAY_ENV_MARGINAL_PDF, SRC(s.cs.env.marginal_pdf)},
    {AKR_ARRAY_ENV_CONDITIONAL_ENTRIES, SRC(s.cs.env.conditional_entries)},
    {AKR_ARRAY_ENV_CONDITIONAL_PDF, SRC(s.cs.env.conditional_pdf)},
    {AKR_ARRAY_PUNCTUAL_LIGHTS, SRC(s.cs.punct)},
    {AKR_ARRAY_LIGHT_TREE, SRC(s.cs.punct_tree)},
};
#undef SRC
#undef TO
// the light rows or the others: on the device, their pointers in s->dscene; a table that does not exist (any more) released, its pointer null
static void upload_tables(akr_scene* s, bool lights) {
    Packed pk;
    for (const SceneTable& t : kSceneTables) {
        if (t.part == SHOWN || (t.part == GEOM) == lights) continue;
        DevBuf& b = s->*t.buf;
        const Bytes src = exists(t.when, s->cs) ? t.src(*s, pk) : Bytes{nullptr, 0};
        b.upload(src.p, src.n);
        if (t.bind) t.bind(s->dscene, b.p);
    }
}
// the light tables (and the environment's record and tables, and the punctual lights' records) on the device, and their pointers in s->dscene: at scene
// creation and after akr_scene_set_environment / akr_scene_add_punctual_light / akr_scene_clear_punctual_lights
static void upload_lights(akr_scene* s) {
    const CompiledScene& cs = s->cs;
    upload_tables(s, true);
    DScene& d = s->dscene;
    d.n_lights = cs.n_lights;
    d.n_punct = (uint32_t)cs.punct.size();
    for (const DPunct& r : cs.punct)  // (the size is not a matter of the colour pipeline: the colour sets' records have it where these do)
        if (r.radius != 0.0f || r.cos_max != 0.0f) d.n_punct |= kPunctSoftBit;
    d.punct_tree = cs.punct_tree.empty() ? 0u : (uint32_t)cs.punct.size();
}
static size_t share_bits_bytes(const CompiledScene& cs) { return cs.instanced.on ? std::max<size_t>(((size_t)cs.n_tris + 31u) / 32u, 1u) * 4u : 0u; }  // in2_share_bits (scene_finish)
static void count_device_bytes(akr_scene* s) {
    s->device_bytes = s->ggx_table.bytes + s->in2_share_bits.bytes;  // (the walk-bound word lies in woop)
    for (const SceneTable& t : kSceneTables)
        if (t.buf) s->device_bytes += (s->*t.buf).bytes;
}
// A host-only scene's estimate of the same. As akr_scene_info.device_bytes has always answered: without the GGX table, and every
// row's bytes whether or not its table would exist -- which differs only by the images of a scene none of whose materials reads one. It used to be
// written as arithmetic on CompiledScene; the rows give the same because packed_light_tables makes one light_alias entry and one record per light
// (n_lights = light_entries.size(): build_alias_table) and one area_alias entry per triangle of an area light (their light_n_tris sum to
// area_entries.size(): compile_scene appends both together), Packed one marginal entry per row and one conditional entry per texel of the environment.
// It packs those tables to learn their sizes -- O(emissive triangles + environment texels) per akr_scene_get_info of a host-only scene.
static uint64_t compiled_scene_bytes(const akr_scene* s) {
    Packed pk;
    uint64_t n = share_bits_bytes(s->cs);
    for (const SceneTable& t : kSceneTables)
        if (t.buf) n += t.src(*s, pk).n;
    return n;
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
    DScene& d = s->dscene;
    std::memset(&d, 0, sizeof d);
    upload_tables(s, false);
    ensure_ggx_table(s);
    d.ggx_table = s->ggx_table.as<float>();
    upload_lights(s);  // light tables, environment
    d.n_tris = cs.n_tris;
    d.n_nodes = scene_n_nodes(cs);
    d.has_alpha = cs.has_alpha ? 1u : 0u;
    d.bvh_stack_depth = scene_stack_depth(cs);
    d.plane_share_mask = 0;
    if (cs.bvh_nodes.empty() && !cs.instanced.on)  // exhaustive path (<= 64 triangles): which records repeat their predecessor's plane row
        for (uint32_t k = 1; k < d.n_tris && k < 64; k++)
            if (std::memcmp(&cs.woop[12ull * k + 8], &cs.woop[12ull * (k - 1) + 8], 16) == 0) d.plane_share_mask |= 1ull << k;
    if (cs.instanced.on) {  // which instance-triangles take their even neighbour's plane row: one bit each, decided on the device (dinst_trav.h resolve_pending)
        d.in2.on = 1u;
        d.in2.n_instances = (uint32_t)s->flat.instances.size();
        s->in2_share_bits.alloc(share_bits_bytes(cs));
        HIP_CHECK(hipMemsetAsync(s->in2_share_bits.p, 0, s->in2_share_bits.bytes, ctx->stream));
        HIP_CHECK(launch_inst_share_bits(d, s->in2_share_bits.as<uint32_t>(), s->in2_mesh_tris.as<uint32_t>(), ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        d.in2.share_bits = s->in2_share_bits.as<uint32_t>();
    }
    count_device_bytes(s);
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
    info->device_bytes = s->device_bytes ? s->device_bytes : compiled_scene_bytes(s);  // (a host-only scene)
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
        for (auto& kv : s->color_sets) kv.second->punct.release();  // folded again by the next session of that pipeline (api_pt.cpp color_set)
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
    auto set = [&](const void* p, size_t n) { *ptr = n ? p : nullptr; *bytes = n; };
    if (which == AKR_ARRAY_R2C || which == AKR_ARRAY_C2W) {  // (not tables)
        set(which == AKR_ARRAY_R2C ? s->r2c : s->c2w, 64);
        return AKR_OK;
    }
    for (const SceneTable& t : kSceneTables) {
        if (t.array != which || t.array == NO_ID || t.part == PACKED) continue;  // (a packed table's bytes would not outlive this call)
        Packed none;
        const Bytes b = t.src(*s, none);
        set(b.p, b.n);
        return AKR_OK;
    }
    return fail(AKR_ERR_INVALID_ARGUMENT, "akr_scene_get_array: unknown array id");
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
