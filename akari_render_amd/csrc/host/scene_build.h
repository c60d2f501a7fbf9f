// scene_build.h -- host side of the scene: the flat description (what load.rs resolves the scene graph to)
// and its compiled, device-ready form.
#pragma once
#include <cmath>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../../include/akari_hip.h"
#include "../kernels.h"
#include "options.h"

namespace akr {

struct HostMesh {
    std::vector<float> vertices;     // 3 / vertex
    std::vector<uint32_t> indices;   // 3 / triangle
    std::vector<float> uvs;          // 6 / triangle or empty
    std::vector<float> normals;      // 9 / triangle or empty
    std::vector<float> tangents;     // 9 / triangle or empty
    std::vector<uint32_t> slots;     // 1 / triangle or empty
    uint32_t n_triangles() const { return (uint32_t)(indices.size() / 3); }
};
struct HostInstance {
    uint32_t mesh = 0;
    std::vector<uint32_t> materials;
    float transform[16];
};
struct HostImage {
    uint32_t width = 0, height = 0, format = 0, filter = 0, address = 0;
    std::vector<uint32_t> words;  // RGBA8: one word per texel; RGBA32F: four
};
struct HostGraph {
    std::vector<akr_shader_node> nodes;  // empty = constant material
    uint32_t input[AKR_IN_COUNT];
    HostGraph() { for (uint32_t& i : input) i = AKR_NODE_NONE; }
};
// The environment light as given (akr_environment_desc / scene.json "environment"): decoded linear texels, no strength applied.
struct HostEnvironment {
    bool set = false;                // false: none (also after a strength of 0 or an all-black image)
    uint32_t width = 0, height = 0;  // 0 x 0: the constant `color`
    uint32_t filter = 0;             // akr_tex_filter
    std::vector<float> texels;       // RGBA32F, row 0 = v = 0
    float color[3] = {0, 0, 0};
    float strength = 0.0f;
    float rotation[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};  // environment -> world, row-major
};
// The camera's thin lens (akr_lens_desc). radius == 0: a pinhole.
struct HostLens {
    float radius = 0.0f, focal_distance = 0.0f;
};
// an akr_lens_desc checked (throws std::invalid_argument); radius == 0 comes back as "no lens"
inline HostLens lens_from_values(float radius, float focal_distance) {
    if (!std::isfinite(radius) || !std::isfinite(focal_distance) || radius < 0.0f || focal_distance < 0.0f)
        throw std::invalid_argument("lens: radius and focal_distance must be finite and >= 0");
    if (radius > 0.0f && !(focal_distance > 0.0f)) throw std::invalid_argument("lens: a radius > 0 needs a focal_distance > 0");
    HostLens l;
    if (radius > 0.0f) { l.radius = radius; l.focal_distance = focal_distance; }
    return l;
}
// The camera's projection (akr_projection_desc). type 0: the perspective camera, and the other fields at their defaults.
struct HostProjection {
    uint32_t type = 0;  // akr_projection_type
    float ortho_scale = 1.0f;
    float lon_min = -3.14159274f, lon_max = 3.14159274f, lat_min = -1.57079637f, lat_max = 1.57079637f;  // (the f32 nearest to pi, pi / 2)
};
// an akr_projection_desc checked (throws std::invalid_argument); the fields the type does not read come back at their defaults
inline HostProjection projection_from_values(uint32_t type, float ortho_scale, float lon_min, float lon_max, float lat_min, float lat_max) {
    HostProjection p;
    if (type > 2u) throw std::invalid_argument("projection: unknown type (0 perspective, 1 orthographic, 2 panorama)");
    p.type = type;
    if (type == 1u) {
        if (!std::isfinite(ortho_scale) || !(ortho_scale > 0.0f)) throw std::invalid_argument("projection: an orthographic camera needs a finite ortho_scale > 0");
        p.ortho_scale = ortho_scale;
    } else if (type == 2u) {
        const HostProjection full;
        if (!std::isfinite(lon_min) || !std::isfinite(lon_max) || !std::isfinite(lat_min) || !std::isfinite(lat_max))
            throw std::invalid_argument("projection: a panorama's longitude and latitude bounds must be finite");
        if (lon_min < full.lon_min || lon_max > full.lon_max || !(lon_min < lon_max))
            throw std::invalid_argument("projection: a panorama needs -pi <= longitude_min < longitude_max <= pi");
        if (lat_min < full.lat_min || lat_max > full.lat_max || !(lat_min < lat_max))
            throw std::invalid_argument("projection: a panorama needs -pi/2 <= latitude_min < latitude_max <= pi/2");
        p.lon_min = lon_min; p.lon_max = lon_max; p.lat_min = lat_min; p.lat_max = lat_max;
    }
    return p;
}
inline const char* projection_name(uint32_t type) { return type == 1u ? "an orthographic" : (type == 2u ? "a panorama" : "a perspective"); }
// Owning copy of an akr_scene_desc.
struct FlatScene {
    std::vector<HostMesh> meshes;
    std::vector<HostInstance> instances;
    std::vector<akr_material_desc> materials;
    akr_camera_desc camera;
    std::vector<float> ggx_table;  // 4096 or empty
    std::vector<HostImage> images;
    std::vector<HostGraph> graphs;  // empty, or one per material
    HostEnvironment env;
    std::vector<akr_punctual_light_desc> punct;  // akr_scene_add_punctual_light / scene.json "lights": checked, as given (scene_punct.cpp; not part of akr_scene_desc)
    int light_tree = 0;  // akr_scene_set_light_tree, initially option `light_tree`: 1 = the point and spot lights are ONE entry of the light table, chosen among by a light tree
    HostLens lens;  // akr_scene_set_lens, or the file's focal_distance / fstop under option `lens` (not part of akr_scene_desc)
    HostProjection projection;  // akr_scene_set_projection, or the file's camera type (not part of akr_scene_desc / akr_camera_desc)
    static FlatScene from_desc(const akr_scene_desc& d);
};

// Output of the host-side scene compiler: plain arrays ready for hipMemcpy.
struct CompiledScene {
    uint32_t n_tris = 0, n_lights = 0;
    std::vector<float> woop;             // exhaustive path: 12 / triangle; BVH path: kBvhTriWords / triangle (record | gid | pad), traversal order
    std::vector<uint32_t> tri_gid;       // BVH path: traversal order -> global id; empty = identity
    std::vector<float> shade;            // 32 / triangle (8 float4), by global id
    std::vector<float> normals;          // 12 / triangle (3 float4) or empty
    std::vector<float> inst;             // 32 / instance
    std::vector<DMaterial> materials;
    std::vector<uint32_t> inst_tri_offset;
    // lights
    std::vector<AliasEntry> light_entries;
    std::vector<float> light_pdf, light_power;
    std::vector<uint32_t> light_inst, light_tri_offset, light_n_tris;
    std::vector<AliasEntry> area_entries;
    std::vector<float> area_pdf;
    // 6-wide compressed BVH nodes (kBvhNodeWords = 16 words = 64 bytes each, host/bvh.cpp) or empty for the exhaustive path
    std::vector<uint32_t> bvh_nodes;
    uint32_t bvh_depth = 0;              // levels of the wide tree = the most stack entries a traversal can need
    // textures: pruned node lists of the materials with texture-fed inputs, image headers, texel words, raw inputs
    std::vector<DNode> tex_nodes;
    std::vector<DImage> images;
    std::vector<uint32_t> texels;
    std::vector<MatInputs> mat_inputs;   // one per material when any material is textured, else empty
    uint32_t tex_slots = 0;              // value slots per lane the widest node list needs (device/dtex.h), 0 without textures
    // The same node lists before slot allocation (arguments name nodes of the material's own list), element for element with
    // tex_nodes, and the scene's shader kinds: materials whose lists have the same shape share a kind (svm/compiler.rs:16-76); the
    // kind of a material is also in DMaterial.tex_n_nodes >> 16. What host/specialise.cpp turns into per-scene kernel code.
    std::vector<akr_shader_node> tex_nodes_ssa;
    struct ShaderKind {
        std::string signature;            // everything that shapes the code: surface kind, operations, argument topology, modes, image formats, fed inputs
        uint32_t mat_kind = 0, n_nodes = 0;
        std::vector<uint32_t> materials;  // the materials of this kind, ascending
    };
    std::vector<ShaderKind> shader_kinds;
    uint32_t absent = 0;                  // lobes no material of the scene can have (device/dbsdf.h AB_*)
    // Two-level mode (scene_inst.cpp; option `instancing`): the scene is kept as meshes + instances. woop / shade / normals / tri_gid /
    // bvh_nodes above stay EMPTY; nothing is stored per instance-triangle. What the device computes at a hit from these arrays is
    // the flattened record bit for bit (device/dinst.h).
    struct Instanced {
        bool on = false;
        std::vector<uint32_t> nodes;        // TLAS nodes (root = slot 0) followed by every mesh's BLAS nodes; child_base / tri_base are
                                            // relative to the start of their own tree
        std::vector<float> tlas_leaves;     // 16 words per top-level leaf entry (one per instance; more with option rebraid) in TLAS order: world->object
                                            // rows (3 x float4) | BLAS node offset, mesh triangle base, instance id, the node of the mesh's tree to start at
        std::vector<float> mesh_tris;       // 16 words per mesh triangle in BLAS order: v0 | uv0.x, v1 | uv0.y, v2 | uv1.x, uv1.y uv2.x uv2.y | prim
        std::vector<uint32_t> mesh_pos;     // per mesh triangle in MESH order: its position in mesh_tris (relative to the mesh's base)
        std::vector<uint32_t> mesh_meta;    // per mesh triangle in mesh order: material slot | TRI_HAS_* flags << 30
        std::vector<float> mesh_normals;    // 24 words per mesh triangle in mesh order (corner normals, corner tangents) or empty
        std::vector<uint32_t> inst_mats;    // the instances' material lists, concatenated
        std::vector<uint32_t> inst_light;   // light id per instance or 0xffffffff
        uint32_t tlas_nodes = 0, tlas_depth = 0, blas_depth = 0, n_mesh_tris = 0;
        uint32_t n_padding_classes = 0;    // per-mesh trees built: one per (mesh, padding class of its instances), scene_inst.cpp
    } instanced;
    // the environment light (scene_env.cpp): what device/denv.h reads, and its place in the light table (the last entry)
    struct Environment {
        bool on = false;
        uint32_t w = 0, h = 0, filter = 0;
        std::vector<float> texels;                      // RGBA32F, strength applied (a constant colour: kEnvConstW x kEnvConstH texels)
        std::vector<AliasEntry> marginal_entries, conditional_entries;  // rows; the columns of each row (j relative to the row)
        std::vector<float> marginal_pdf, conditional_pdf;
        float rot_t[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};  // world -> environment (R^T), row-major
        float power = 0.0f;                             // selection weight 4 pi R^2 Lbar
    } env;
    // the punctual lights' records under the default colour pipeline (scene_punct.cpp; device/dscene.h DPunct): their entries in the light table come after
    // the emissive instances' and before the environment's, light_inst = kPunctInst
    std::vector<DPunct> punct;
    // the light tree over the point and spot lights (device/dlighttree.h): 2 L - 1 nodes of 8 words, `lo.xyz, power | hi.xyz, child`, breadth-first; empty = no
    // tree. With one, those lights share ONE entry of the light table (light_inst = kPunctTreeInst) behind the suns; `punct` keeps every record in the order given.
    std::vector<uint32_t> punct_tree;
    bool has_textures = false;
    bool has_alpha = false;
    bool needs_ggx_table = false;
    float scene_lo[3], scene_hi[3];
    // an acceleration structure (flattened: bvh_nodes; kept as meshes + instances: instanced.nodes), or the exhaustive walk over <= 64 triangles
    bool has_tree() const { return !bvh_nodes.empty() || instanced.on; }
};

// Padding of the acceleration structure's boxes. It covers the round-off of the slab test and of the triangle test, and both scale
// with the MAGNITUDE of the coordinates involved -- ray origins lie on the scene's surfaces or at the camera -- not with the scene's
// size alone: a building modelled 10 km from the origin loses hits with a padding that looks at its diagonal only (round 5:
// tools/offset_check.py, scenes/cbox shifted by 1000 differed from the oracle in 12 film floats, by 10 000 in 3 621).
inline float bvh_box_padding(const float lo[3], const float hi[3], const float* c2w /* column-major 4x4 */) {
    float diag2 = 0.0f, reach = 0.0f;
    for (int a = 0; a < 3; a++) {
        diag2 += (hi[a] - lo[a]) * (hi[a] - lo[a]);
        const float m = std::fabs(lo[a]) > std::fabs(hi[a]) ? std::fabs(lo[a]) : std::fabs(hi[a]);
        const float c = std::fabs(c2w[12 + a]);
        reach += m > c ? m : c;
    }
    const float diag = __builtin_sqrtf(diag2);
    return 4e-6f * (diag > reach ? diag : reach);
}
// Per axis, the largest |coordinate| of a ray origin of the camera: o = T + (a c2w[0..2] + b c2w[4..6]) with (a, b) on the lens disk, a^2 + b^2 <=
// radius^2 (device/dpath.h lens_ray_camera), plus -- an orthographic camera -- a point of the film rectangle |a| <= half_x, |b| <= half_y
// (ortho_ray_camera; 0, 0 for the cameras whose origins are the camera position or the lens), over the camera's w.
inline void lens_origin_bound(const float* c2w /* column-major 4x4 */, float radius, float half_x, float half_y, float out[3]) {
    const double w = std::fabs((double)c2w[15]) > 0.0 ? std::fabs((double)c2w[15]) : 1.0;
    for (int a = 0; a < 3; a++)
        out[a] = (float)(((double)std::fabs(c2w[12 + a]) + (double)radius * std::sqrt((double)c2w[a] * c2w[a] + (double)c2w[4 + a] * c2w[4 + a]) +
                          (double)half_x * std::fabs((double)c2w[a]) + (double)half_y * std::fabs((double)c2w[4 + a])) / w * 1.000001);
}
// the half-extents of an orthographic camera's film in camera space: the larger image side spans ortho_scale (camera_matrices)
inline void ortho_film_half_extents(float ortho_scale, uint32_t width, uint32_t height, float* half_x, float* half_y) {
    const float t = 0.5f * ortho_scale, fw = (float)width, fh = (float)height;
    *half_x = width > height ? t : t * fw / fh;
    *half_y = width > height ? t * fh / fw : t;
}

// Conditioning of a triangle's (u, v) parametrisation. The inside test computes u = r0 . p + c0 with |r0| = |e2| / |n| (v likewise with
// |r1| = |e1| / |n|): two of its three fma roundings act on partial sums of size S = |r0||p| + |c0| <= 2 |r0||p|, the rounded row and the
// rounded hit point add one unit each -- |du| <= 8 x 2^-24 x |r0| x |p|, p a point of the triangle -- and the triangle the test "sees" is
// displaced by du e1 + dv e2. For a well-shaped triangle that is a few ulp of its coordinates, what bvh_box_padding allows for; but
// |r0||e1| = 1 / sin(angle at the first vertex): a needle whose first vertex holds its small angle is displaced along its long axis by 1 / sin
// times as much, and the exhaustive loop accepts hits that far outside it (round 6: tests/bvh_model.py found such pairs in 9 of 150
// extreme scenes, among them the one film pixel of HISTORY R5.7). k[a] = |r0||e1_a| + |r1||e2_a| per axis (2 for a right angle at the first
// vertex, 2.31 for 60 degrees); a box must reach kTriCondEps x |p| x k[a] beyond the triangle along axis a. kTriCondFree of the flat
// padding is counted towards that (the rest of it covers the slab test's own round-off and the plane's); what exceeds it is added to the
// triangle's own box.
constexpr float kTriCondEps = 10.0f * 5.9604645e-8f;
constexpr float kTriCondFree = 0.64f;
inline void tri_conditioning(const double A[3], const double B[3], const double C[3], float k[3]) {
    const double e1[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, e2[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
    const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double nl = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    const double l1 = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]), l2 = std::sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
    for (int a = 0; a < 3; a++) {
        const double v = nl > 0.0 ? (l2 * std::fabs(e1[a]) + l1 * std::fabs(e2[a])) / nl : 0.0;  // (a degenerate triangle has an all-zero record: never accepted)
        k[a] = v < 1e30 ? (float)(v * 1.0001) : 1e30f;
    }
}
// what a box of a triangle with conditioning k needs along an axis beyond the flat padding `pad`; magnitude = |p| (2-norm) of the triangle's points
inline float tri_cond_extra(float k, float magnitude, float pad) {
    const float need = kTriCondEps * magnitude * k, have = kTriCondFree * pad;
    return need > have ? need - have : 0.0f;
}
// 2-norm of the largest coordinates a box holds
inline float box_magnitude(const float lo[3], const float hi[3]) {
    float m2 = 0.0f;
    for (int a = 0; a < 3; a++) {
        const float m = std::fabs(lo[a]) > std::fabs(hi[a]) ? std::fabs(lo[a]) : std::fabs(hi[a]);
        m2 += m * m;
    }
    return __builtin_sqrtf(m2) * 1.0001f;
}
DMaterial fold_material(const akr_material_desc& m, uint32_t color = 0);
// materials / node lists / raw inputs under the colour pipeline `color` (scene_build.cpp); fills out.materials, out.tex_nodes,
// out.mat_inputs only
void compile_materials(const FlatScene& flat, uint32_t color, CompiledScene& out, std::vector<akr_material_desc>& descs);
void build_alias_table(const std::vector<float>& weights, std::vector<AliasEntry>& entries, std::vector<float>& pdf);
constexpr uint64_t kSpecAutoSamples = 1ull << 31;  // option specialise = -1: a first-use compile (about a second; 20-30 % of the render to win) has to be worth it

void compile_scene(const FlatScene& flat, const TuningOptions& opt, CompiledScene& out);  // opt: the caller's one snapshot of the options
// The sizes of the tables a pt kernel stages in LDS (kernels.h StageTable; ST_GGX: 0) of a compiled scene whose light list has n_lights entries: the ONE
// statement of them, which the launch plan (pt_plan.cpp, n_lights = out.n_lights) takes as they are. A table staged in future is added here.
void stage_table_bytes(const CompiledScene& out, size_t n_lights, size_t bytes[ST_COUNT]);
// ... and their sum, each table padded to 16: what compile_scene (exhaustive or BVH?), compile_environment and compile_punctual (does the scene still
// fit with the entry added?) compare with kStageMaxBytes.
size_t exhaustive_stage_bytes(const CompiledScene& out, size_t n_lights);
// "point light" / "spot light" / "sun light" of the scene's first punctual light: what a refusal names
std::string punctual_light_name(const CompiledScene& cs);
// scene_env.cpp: the environment light of `flat` into `out` (tables, light-table entry); replaces the one `out` has. After compile_scene.
constexpr uint32_t kEnvConstW = 32, kEnvConstH = 16;  // the image a constant colour is stored as
void compile_environment(const FlatScene& flat, CompiledScene& out);
// an akr_environment_desc checked and copied (throws std::invalid_argument); the result's `set` is false for "no environment"
HostEnvironment environment_from_desc(const akr_environment_desc& d);
void rebuild_light_alias(CompiledScene& out);  // n_lights and the selection table from light_power
// scene_punct.cpp: an akr_punctual_light_desc checked and copied to `out` (throws std::invalid_argument); false = "no light" (strength 0 or an all-zero colour)
bool punctual_from_desc(const akr_punctual_light_desc& d, akr_punctual_light_desc& out);
DPunct fold_punctual(const akr_punctual_light_desc& d, uint32_t color);  // the record under the colour pipeline `color`
// the punctual lights of `flat` into `out` (records, light-table entries); replaces those `out` has. After compile_scene; the environment's entry stays last.
void compile_punctual(const FlatScene& flat, CompiledScene& out);
// the light tree's node words over the point and spot lights among `recs` (weights: every record's f32 selection weight); empty with fewer than two of them
std::vector<uint32_t> build_light_tree(const std::vector<DPunct>& recs, const std::vector<float>& weights);
// what DScene.punct points at: the records and, behind them, the tree's nodes padded to whole 64-byte records (DScene.punct_tree = recs.size() with a tree)
std::vector<DPunct> punctual_device_records(const std::vector<DPunct>& recs, const std::vector<uint32_t>& tree);
float triangle_emission_power(const CompiledScene& out, const TexScene& host_tex, uint32_t material, uint32_t prim, vec2 uv0, vec2 uv1, vec2 uv2, float area);
bool instance_may_emit(const CompiledScene& out, const std::vector<akr_material_desc>& descs, const HostInstance& in);
// scene_inst.cpp: does this scene take the two-level route, and its geometry + light tables if so (materials and the instance table
// of `out` must be filled: compile_scene calls it)
bool want_instancing(const FlatScene& flat, const TuningOptions& opt);
struct InstXf;
void compile_instanced_geometry(const FlatScene& flat, const TuningOptions& opt, const std::vector<InstXf>& xf, const std::vector<akr_material_desc>& descs, CompiledScene& out);
// PerspectiveCameraData::new (camera/mod.rs:119-153)
// proj: an orthographic camera's r2c has half its ortho_scale in the place of tan(fov / 2); nullptr or any other type = the perspective matrix
void camera_matrices(const akr_camera_desc& cam, float r2c[16], float c2w[16], uint32_t* c2w_identity, const HostProjection* proj = nullptr);
PcgStartConsts pcg_start_constants();

// scene.json / method.json readers (host/scene_json.cpp); throw std::runtime_error on failure
FlatScene load_scene_json(const std::string& path, const TuningOptions& opt);  // opt: punctual_lights, soft_lights, lens
void parse_method_json(const std::string& text, akr_pt_config* cfg, std::string* film_out);
// all tasks of a RenderTask file (Single | Multi), lib.rs:103-109; allow_sampler_override: pmj02bn -> independent
// most LDS a workgroup of the exhaustive path tracer kernels spends on staged scene tables (4 workgroups per CU, 160 KB of LDS)
constexpr size_t kStageMaxBytes = 32 * 1024;
// the same for the BVH path, whose workgroups already hold 24 KB of traversal stacks each
constexpr size_t kStageMaxBytesBvh = 12 * 1024;

struct ParsedTask {
    bool is_aov = false;     // Method::NormalVis instead of Method::PathTracer
    akr_pt_config cfg;
    akr_aov_config aov;
    bool is_gpt = false;     // Method::GradientPathTracer
    akr_gpt_config gpt;
    bool is_mcmc = false;    // Method::McmcOpt
    akr_mcmc_config mcmc;
    std::string film_out;
};
std::vector<ParsedTask> parse_render_tasks(const std::string& text, bool allow_sampler_override);
// tables of the pmj02bn sampler (host/pmj_tables.cpp): 5 x 65536 x 2 u32 points; 48 x 128 x 128 u16 blue-noise arrays
void make_pmj02_sets(std::vector<uint32_t>& out);
void load_bluenoise(std::vector<uint16_t>& out);
// image writers (host/image_io.cpp)
void write_image(const std::string& path, const float* rgb, uint32_t w, uint32_t h);
// PNG -> RGBA8 in file order (image crate `decode().to_rgba8()` conventions); throws std::runtime_error
void decode_png(const uint8_t* data, size_t n, uint32_t& w, uint32_t& h, std::vector<uint8_t>& rgba);
// JPEG (baseline + progressive Huffman, 8 bit, 1 or 3 components) -> RGBA8 in file order
void decode_jpeg(const uint8_t* data, size_t n, uint32_t& w, uint32_t& h, std::vector<uint8_t>& rgba);
// OpenEXR (single-part scanline; none / RLE / ZIPS / ZIP; half / float / uint channels) -> RGBA f32 in file order
void decode_exr(const uint8_t* data, size_t n, uint32_t& w, uint32_t& h, std::vector<float>& rgba);
// TIFF (classic; strips / tiles; 8 / 16-bit and float samples; none / LZW / deflate / PackBits; predictor) and DDS (DXT1 / 3 / 5)
// -> RGBA8 in file order (host/image_formats.cpp)
void decode_tiff(const uint8_t* data, size_t n, uint32_t& w, uint32_t& h, std::vector<uint8_t>& rgba);
void decode_dds(const uint8_t* data, size_t n, uint32_t& w, uint32_t& h, std::vector<uint8_t>& rgba);
std::vector<uint8_t> inflate_zlib_stream(const uint8_t* data, size_t n);  // the PNG reader's inflate (zlib framing)

}  // namespace akr
