/* akr_oracle.c -- CPU restatement of akari_render's `pt` path tracer (the parity oracle).
 *
 * TEST INFRASTRUCTURE ONLY. Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
 * load the library built from this file; the shipped HIP path never links, includes or calls it.
 *
 * What it restates (reference file:line, all under /root/reference/crates/):
 *   akari_integrator/src/pt.rs:95-323, 329-900 (shift_mapping = None), 916-973, 1056-1159
 *   akari_render/src/scene.rs:49-185, mesh.rs:426-654, camera/mod.rs:70-180, film.rs:32-49,196-229,
 *   sampler/mod.rs:73-217,299-328, light/mod.rs:100-147, light/area.rs:36-130, sampling.rs,
 *   util/distribution.rs:35-88, load.rs:308-444, svm/surface/{mod,diffuse,principled,glass}.rs,
 *   microfacet.rs (see or_bsdf.h); further down, each with its own citation block: svm/eval.rs + image sampling (or_tex.h),
 *   akari_integrator/src/aov.rs, gpt.rs (+ the shift-mapping branches of pt.rs:329-900), mcmc_opt.rs (+ mcmc.rs,
 *   sampler/mcmc.rs, util/distribution.rs:92-115), sampler/mod.rs:329-700 (pmj02bn; the two tables are handed in by the tests).
 *   The environment light has no reference counterpart (hit_envmap returns zero): or_env.h restates DESIGN.md 4.8.
 *   Neither have the punctual lights (light/point.rs is a struct and nothing else) nor the thin lens (generate_ray never uses the
 *   lens fields): or_punct.h restates DESIGN.md 4.14 and 4.15, or_camera_ray below restates 4.9.
 *
 * Parity status: the reference cannot be built or run here (no Rust toolchain; LuisaCompute is an
 * un-vendored path dependency) and its tests hold no numeric fixtures for this path, so
 * this oracle is pinned by (i) known-answer vectors of the published third-party algorithms it restates
 * (PCG32, ChaCha, xxHash32), (ii) the reference's own property tests restated in tests/ (alias-table
 * mass, chi^2 sample-vs-pdf, furnace/energy tests) and (iii) closed-form radiometry checks.
 * Against a real run of the reference: PARITY UNPINNED for BVH hit order, ray-offset constants and the
 * elementary-function bits (LuisaCompute internals), as stated in DESIGN.md.
 *
 * The BVH of the reference (Embree/OptiX through LuisaCompute) is replaced by an exhaustive loop over
 * all triangles with an order-independent closest-hit rule (min t, ties -> lowest global triangle id),
 * which is the definition the HIP BVH traversal must reproduce.
 */
#define _GNU_SOURCE
#include "or_api.h"
#include "or_bsdf.h"
#include "or_tex.h"
#include "or_geom.h"
#include "or_env.h"
#include "or_punct.h"
#include "or_lighttree.h"
#include "or_math.h"
#include "or_rng.h"
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define OR_EXPORT __attribute__((visibility("default")))
#define OR_INVALID 0xffffffffu

/* ------------------------------------------------------------------------------------------------ */
typedef struct { v3 c0, c1, c2, t; float det; } or_xform; /* columns of M3 + translation */

typedef struct {
    or_mesh_desc d; /* deep copies */
} or_mesh;

typedef struct {
    uint32_t mesh, n_materials;
    uint32_t *materials;
    or_xform xf;
    int32_t light;          /* light id or -1 (MeshInstance.light) */
    uint32_t tri_offset;    /* first global triangle id */
    or_alias_table area_sampler; /* valid iff light >= 0 */
} or_instance;

typedef struct or_scene_s {
    uint32_t n_meshes, n_instances, n_materials, n_tris, n_lights;
    or_mesh *meshes;
    or_instance *instances;
    or_material_desc *materials;
    or_material_graph *graphs;   /* n_materials entries (deep copies) or NULL */
    or_image_desc *images;       /* deep copies */
    uint32_t n_images;
    /* world-space triangles for intersection */
    float *woop; /* 12 floats per triangle */
    uint32_t *tri_inst, *tri_prim;
    /* lights: light id -> instance; LightAggregate.light_distribution */
    uint32_t *light_inst;
    float *light_power;
    or_alias_table light_dist;
    /* camera */
    float r2c[16], c2w[16];
    int c2w_identity;
    uint32_t width, height;
    float table[16 * 16 * 16];
    int has_table;
    struct or_bvh *bvh;          /* optional, checker-side only (or_accel.h); NULL = the exhaustive loop below */
    uint32_t color;              /* ColorPipeline of the render in progress (OR_COLOR_*), set by the render entry points; 0 during
                                  * scene creation: the light tables come from the sRGB pipeline (load.rs:316-319) */
    or_env *env;                 /* the environment light (or_env.h) or NULL; it is light n_lights - 1 */
    /* the punctual lights (or_punct.h, DESIGN.md 4.14 "Light list"): lights n_emit .. n_emit + n_punct - 1, in the order given,
     * between the emissive instances and the environment */
    uint32_t n_emit, n_punct;
    or_punctual_light_desc *punct_desc; /* as accepted (normalised); those that were "no light" are not among them */
    or_punct *punct[4];                 /* the folded records per colour pipeline (index = the OR_COLOR_* bits) */
    float lens_radius, lens_focal;      /* the thin lens; radius 0 = the pinhole */
    /* the projection: as accepted, the fields its type does not read at their defaults; fov as the scene was made with;
     * the panorama's six folded constants. An orthographic scene holds ITS raster -> camera matrix in r2c (or_projection_fold). */
    or_projection_desc proj;
    float fov;
    float pano_lon0, pano_dlon, pano_lat1, pano_dlat, pano_inv_w, pano_inv_h;
    /* the light tree (or_lighttree.h). The mode; the nodes when a tree exists (mode 1 and >= 2 local lights), else NULL;
     * and, whatever the mode, per entry of the light list the index of its record in punct[] (OR_INVALID: the entry has none; 0 for the
     * tree's own entry): with a tree the local lights have left the list and a sun's record index is not its rank. */
    uint32_t light_tree, n_lt_nodes;
    or_lt_node *lt_nodes;
    uint32_t *light_rec;
} or_scene;

typedef struct { v3 o, d; float t_min, t_max; uint32_t ex0_inst, ex0_prim, ex1_inst, ex1_prim; } or_ray;
typedef struct {
    or_frame frame; v3 p, ng; v2 bary, uv; uint32_t inst, prim, material; float prim_area; int valid;
} or_si;

static void *or_dup(const void *p, size_t n) { if (!p) return 0; void *q = malloc(n ? n : 1); memcpy(q, p, n); return q; }

/* 4x4 column-major helpers (glam Mat4 semantics, un-fused) */
static void m4_mul(const float *a, const float *b, float *out) { /* out = a * b */
    float r[16];
    for (int c = 0; c < 4; c++)
        for (int i = 0; i < 4; i++)
            r[c * 4 + i] = ((a[0 * 4 + i] * b[c * 4 + 0] + a[1 * 4 + i] * b[c * 4 + 1]) + a[2 * 4 + i] * b[c * 4 + 2]) + a[3 * 4 + i] * b[c * 4 + 3];
    memcpy(out, r, sizeof r);
}
static void m4_scale(float x, float y, float z, float *m) { memset(m, 0, 64); m[0] = x; m[5] = y; m[10] = z; m[15] = 1; }
static void m4_translate(float x, float y, float z, float *m) { m4_scale(1, 1, 1, m); m[12] = x; m[13] = y; m[14] = z; }

static v3 xf_point(const or_xform *x, v3 p) { /* m * p + t, mesh.rs:611-615 */
    return v3add(v3add(v3add(v3scale(x->c0, p.x), v3scale(x->c1, p.y)), v3scale(x->c2, p.z)), x->t);
}
static v3 xf_vector(const or_xform *x, v3 v) {
    return v3add(v3add(v3scale(x->c0, v.x), v3scale(x->c1, v.y)), v3scale(x->c2, v.z));
}
/* (M^T)^-1 * n = (cof0*n.x + cof1*n.y + cof2*n.z) / det, cof_i = cross of the other two columns */
static v3 xf_normal(const or_xform *x, v3 n) {
    v3 k0 = v3cross(x->c1, x->c2), k1 = v3cross(x->c2, x->c0), k2 = v3cross(x->c0, x->c1);
    v3 r = v3add(v3add(v3scale(k0, n.x), v3scale(k1, n.y)), v3scale(k2, n.z));
    return v3divs(r, x->det);
}

static v3 ld3(const float *p, uint32_t i) { return V3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }
static v2 ld2(const float *p, uint32_t i) { return V2(p[2 * i], p[2 * i + 1]); }
/* TriangleInterpolate: (1-u-v) a + u b + v c */
static v3 interp3(v2 b, v3 a0, v3 a1, v3 a2) {
    float w = 1.0f - b.x - b.y;
    return v3add(v3add(v3scale(a0, w), v3scale(a1, b.x)), v3scale(a2, b.y));
}
static v2 interp2(v2 b, v2 a0, v2 a1, v2 a2) {
    float w = 1.0f - b.x - b.y;
    return V2((a0.x * w + a1.x * b.x) + a2.x * b.y, (a0.y * w + a1.y * b.x) + a2.y * b.y);
}

/* ---------------------------------- mesh.rs:487-654 surface_interaction -------------------------- */
static or_si or_surface_interaction(const or_scene *sc, uint32_t inst_id, uint32_t prim_id, v2 bary) {
    const or_instance *inst = &sc->instances[inst_id];
    const or_mesh_desc *g = &sc->meshes[inst->mesh].d;
    /* mats[slots[prim]] when the slot buffer has more than one entry, else mats[0] (mesh.rs:508-521, load.rs:227-229) */
    uint32_t slot = (g->material_slots && g->n_triangles > 1) ? g->material_slots[prim_id] : 0;
    uint32_t material = inst->materials[slot < inst->n_materials ? slot : 0];
    uint32_t i0 = g->indices[3 * prim_id], i1 = g->indices[3 * prim_id + 1], i2 = g->indices[3 * prim_id + 2];
    v3 v0 = ld3(g->vertices, i0), v1 = ld3(g->vertices, i1), v2_ = ld3(g->vertices, i2);
    v3 p_local = interp3(bary, v0, v1, v2_);
    v3 ngc = v3cross(v3sub(v1, v0), v3sub(v2_, v0));
    float len = v3len(ngc);
    float area_local = len * 0.5f;
    v3 ng_local = v3divs(ngc, len);
    uint32_t p3 = prim_id * 3;
    v2 uv0, uv1, uv2;
    if (g->uvs) { uv0 = ld2(g->uvs, p3); uv1 = ld2(g->uvs, p3 + 1); uv2 = ld2(g->uvs, p3 + 2); }
    else { uv0 = V2(0.0f, 0.0f); uv1 = V2(1.0f, 0.0f); uv2 = V2(1.0f, 0.1f); }
    v2 uv = interp2(bary, uv0, uv1, uv2);
    /* tangent (dpdu) */
    v3 tt_local = V3(0, 0, 0);
    int use_default = 0;
    if (g->tangents) {
        v3 t0 = ld3(g->tangents, p3), t1 = ld3(g->tangents, p3 + 1), t2 = ld3(g->tangents, p3 + 2);
        int all_good = or_isfinite(t0.x) && or_isfinite(t0.y) && or_isfinite(t0.z) && or_isfinite(t1.x) && or_isfinite(t1.y) &&
                       or_isfinite(t1.z) && or_isfinite(t2.x) && or_isfinite(t2.y) && or_isfinite(t2.z);
        if (!all_good) use_default = 1; else tt_local = v3normalize(interp3(bary, t0, t1, t2));
    } else use_default = 1;
    if (use_default) {
        v2 duv02 = V2(uv0.x - uv2.x, uv0.y - uv2.y), duv12 = V2(uv1.x - uv2.x, uv1.y - uv2.y);
        v3 dp02 = v3sub(v0, v2_), dp12 = v3sub(v1, v2_);
        float determinant = or_dop(duv02.x, duv12.y, duv02.y, duv12.x);
        int degenerate_uv = fabsf(determinant) < 1e-8f;
        if (!degenerate_uv) {
            float inv_det = 1.0f / determinant;
            tt_local.x = or_dop(duv12.y, dp02.x, duv02.y, dp12.x) * inv_det;
            tt_local.y = or_dop(duv12.y, dp02.y, duv02.y, dp12.y) * inv_det;
            tt_local.z = or_dop(duv12.y, dp02.z, duv02.y, dp12.z) * inv_det;
        }
        if (degenerate_uv || v3len2(tt_local) == 0.0f) tt_local = or_frame_from_n(ng_local).t;
    }
    v3 ns_local = ng_local;
    if (g->normals) ns_local = interp3(bary, ld3(g->normals, p3), ld3(g->normals, p3 + 1), ld3(g->normals, p3 + 2));
    /* apply transform */
    const or_xform *x = &inst->xf;
    v3 p = xf_point(x, p_local);
    v3 tt = xf_vector(x, tt_local);
    v3 c = xf_vector(x, ng_local);
    v3 ng = v3normalize(xf_normal(x, ng_local));
    v3 ns = v3normalize(xf_normal(x, ns_local));
    float area = (area_local == 0.0f || x->det == 0.0f) ? 0.0f : fabsf(area_local * x->det / v3dot(ng, c));
    or_si si;
    si.frame = (tt.x != 0.0f || tt.y != 0.0f || tt.z != 0.0f) ? or_frame_from_n_t(ns, tt) : or_frame_from_n(ns);
    si.p = p; si.ng = ng; si.bary = bary; si.uv = uv; si.inst = inst_id; si.prim = prim_id;
    si.material = material; si.prim_area = area; si.valid = 1;
    return si;
}

/* ---------------------------------- intersection (replaces rtx::Accel) ---------------------------- */
/* Triangle test in Woop's precomputed form ("Ray-triangle intersection with precomputed transformation",
 * the affine map taking the triangle to the unit right triangle in z = 0). Per triangle 12 floats
 * rows[0..2] = (r_i.x, r_i.y, r_i.z, c_i): local = r_i . p + c_i. This is the build's own intersector
 * definition (the reference delegates to Embree/OptiX via LuisaCompute, source absent); the HIP kernels
 * evaluate exactly this sequence. Returns 1 with (t,u,v) when t in [tmin,tmax], u,v >= 0, u+v <= 1. */
static inline int or_tri_test(v3 o, v3 d, const float *w, float tmin, float tmax, float *t_out, float *u_out, float *v_out) {
    float dz = fmaf(w[8], d.x, fmaf(w[9], d.y, w[10] * d.z));
    float oz = fmaf(w[8], o.x, fmaf(w[9], o.y, fmaf(w[10], o.z, w[11])));
    float t = -oz / dz;
    /* hit point, then its affine coordinates in the triangle's frame (rows 0 and 1) */
    float px = fmaf(t, d.x, o.x), py = fmaf(t, d.y, o.y), pz = fmaf(t, d.z, o.z);
    float u = fmaf(w[0], px, fmaf(w[1], py, fmaf(w[2], pz, w[3])));
    float v = fmaf(w[4], px, fmaf(w[5], py, fmaf(w[6], pz, w[7])));
    if (!((t >= tmin) & (t <= tmax) & (u >= 0.0f) & (v >= 0.0f) & (u + v <= 1.0f))) return 0;
    *t_out = t; *u_out = u; *v_out = v;
    return 1;
}
/* host-side precompute of the 12 floats, in double, from the f32 world-space vertices */
static void or_woop_precompute(v3 A, v3 B, v3 C, float *w) {
    double ax = A.x, ay = A.y, az = A.z;
    double e1x = (double)B.x - ax, e1y = (double)B.y - ay, e1z = (double)B.z - az;
    double e2x = (double)C.x - ax, e2y = (double)C.y - ay, e2z = (double)C.z - az;
    double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    double det = nx * nx + ny * ny + nz * nz;
    if (!(det > 0.0)) { for (int i = 0; i < 12; i++) w[i] = 0.0f; return; } /* degenerate: dz = 0 -> t = NaN/inf, never hits */
    double r0x = (e2y * nz - e2z * ny) / det, r0y = (e2z * nx - e2x * nz) / det, r0z = (e2x * ny - e2y * nx) / det;
    double r1x = (ny * e1z - nz * e1y) / det, r1y = (nz * e1x - nx * e1z) / det, r1z = (nx * e1y - ny * e1x) / det;
    double r2x = nx / det, r2y = ny / det, r2z = nz / det;
    w[0] = (float)r0x; w[1] = (float)r0y; w[2] = (float)r0z; w[3] = (float)(-(r0x * ax + r0y * ay + r0z * az));
    w[4] = (float)r1x; w[5] = (float)r1y; w[6] = (float)r1z; w[7] = (float)(-(r1x * ax + r1y * ay + r1z * az));
    w[8] = (float)r2x; w[9] = (float)r2y; w[10] = (float)r2z; w[11] = (float)(-(r2x * ax + r2y * ay + r2z * az));
}
/* Coplanar neighbours share a plane row: triangles 2j and 2j+1 of an instance get the same third row when the second one's
 * vertices lie in the first one's plane to within 1e-6 of the triangle's size (the same rule, stated independently, as
 * akari_render_amd/csrc/host/scene_build.cpp: share_plane_row). Pure data: the tracer below does not know about it. */
static int g_or_share_plane_rows = 1; /* 0: every triangle keeps the plane row computed from its own vertices (the records as
                                       * they were before the rule existed); read by or_scene_create */
OR_EXPORT void or_set_share_plane_rows(int enable) { g_or_share_plane_rows = enable; }
static void or_share_plane_row(const float *wa, float *wb, v3 a, v3 b, v3 c) {
    const double rx = wa[8], ry = wa[9], rz = wa[10], cc = wa[11];
    const double len = sqrt(rx * rx + ry * ry + rz * rz);
    if (!(len > 0.0) || (wb[8] == 0.0f && wb[9] == 0.0f && wb[10] == 0.0f)) return;
    const double tol = 1e-6 * sqrt(len);
    const v3 vb[3] = {a, b, c};
    for (int i = 0; i < 3; i++) {
        const double s = ((rx * (double)vb[i].x + ry * (double)vb[i].y) + rz * (double)vb[i].z) + cc;
        if (!(fabs(s) <= tol)) return;
    }
    wb[8] = wa[8]; wb[9] = wa[9]; wb[10] = wa[10]; wb[11] = wa[11];
}
/* scene.rs:49-86 stochastic alpha test; alpha = alpha of the base-colour node of the hit material */
static inline int or_alpha_test(const or_scene *sc, uint32_t inst, uint32_t prim, float u, float v) {
    const or_instance *in = &sc->instances[inst];
    const or_mesh_desc *g = &sc->meshes[in->mesh].d;
    uint32_t slot = (g->material_slots && g->n_triangles > 1) ? g->material_slots[prim] : 0;
    uint32_t mid = in->materials[slot < in->n_materials ? slot : 0];
    const or_material_desc *m = &sc->materials[mid];
    const uint32_t mkind = m->kind & OR_MAT_KIND_MASK;
    float alpha = (mkind == OR_MAT_PRINCIPLED || mkind == OR_MAT_DIFFUSE) ? m->base_alpha : 1.0f;
    if (sc->graphs && sc->graphs[mid].n_nodes && sc->graphs[mid].input[OR_IN_BASE_COLOR] != OR_NODE_NONE &&
        (mkind == OR_MAT_PRINCIPLED || mkind == OR_MAT_DIFFUSE)) {
        /* SvmEvalMode::Alpha (principled.rs:15-21) at the candidate's uv (mesh.rs:426-485; this restatement uses the
         * uv defaults of surface_interaction for meshes without uvs) */
        uint32_t p3 = prim * 3;
        v2 uv0, uv1, uv2;
        if (g->uvs) { uv0 = ld2(g->uvs, p3); uv1 = ld2(g->uvs, p3 + 1); uv2 = ld2(g->uvs, p3 + 2); }
        else { uv0 = V2(0.0f, 0.0f); uv1 = V2(1.0f, 0.0f); uv2 = V2(1.0f, 0.1f); }
        v2 uv = interp2(V2(u, v), uv0, uv1, uv2);
        or_material_desc at;
        or_material_at(m, &sc->graphs[mid], sc->images, sc->color, uv.x, uv.y, &at);
        alpha = at.base_alpha;
    }
    if (alpha >= 1.0f) return 1;
    float h = (float)or_xxhash32_4(inst, prim, f2u(u), f2u(v)) * (float)(1.0 / 4294967295.0);
    return alpha > h;
}
/* closest hit: scene.rs:88-110,131-153; any hit: scene.rs:155-185. THE definition of a hit: every triangle, in global order.
 * (or_trace_bvh, or_accel.h, skips triangles that cannot pass and is checked against this loop ray by ray.) */
static int or_trace_bvh(const or_scene *sc, const or_ray *r, int any_hit, uint32_t *o_inst, uint32_t *o_prim, v2 *o_bary, or_stats *st);
static int or_trace(const or_scene *sc, const or_ray *r, int any_hit, uint32_t *o_inst, uint32_t *o_prim, v2 *o_bary, or_stats *st) {
    if (sc->bvh) return or_trace_bvh(sc, r, any_hit, o_inst, o_prim, o_bary, st);
    float best_t = 0.0f; uint32_t best = OR_INVALID; v2 best_b = V2(0, 0);
    for (uint32_t k = 0; k < sc->n_tris; k++) {
        float t, u, v;
        if (!or_tri_test(r->o, r->d, sc->woop + 12 * k, r->t_min, r->t_max, &t, &u, &v)) continue;
        uint32_t inst = sc->tri_inst[k], prim = sc->tri_prim[k];
        if (!((inst != r->ex0_inst || prim != r->ex0_prim) && (inst != r->ex1_inst || prim != r->ex1_prim))) continue;
        if (!or_alpha_test(sc, inst, prim, u, v)) continue;
        if (any_hit) { if (st) st->n_tri_tests += k + 1; return 1; }
        if (best == OR_INVALID || t < best_t) { best = k; best_t = t; best_b = V2(u, v); } /* k ascending: ties keep lowest id */
    }
    if (st) st->n_tri_tests += sc->n_tris;
    if (any_hit || best == OR_INVALID) return 0;
    *o_inst = sc->tri_inst[best]; *o_prim = sc->tri_prim[best]; *o_bary = best_b;
    return 1;
}
#include "or_accel.h"

/* ---------------------------------- materials -> closure trees ----------------------------------- */
#define OR_MAX_NODES 24
typedef struct { or_surface n[OR_MAX_NODES]; int count; } or_closure_pool;
static or_surface *pool_new(or_closure_pool *p, int kind) {
    or_surface *s = &p->n[p->count++];
    memset(s, 0, sizeof *s);
    s->kind = kind;
    return s;
}
static or_surface *mk_refl(or_closure_pool *p, v3 color, int fresnel, float eta, float roughness) {
    or_surface *s = pool_new(p, OR_S_MF_REFL);
    s->color = color; s->fresnel = fresnel; s->eta = eta; s->alpha = tr_alpha_from_roughness(roughness, roughness);
    s->roughness = roughness;
    return s;
}
/* principled.rs:11-216 */
static or_surface *or_build_principled(or_closure_pool *p, const or_scene *sc, const or_material_desc *m, const or_si *si) {
    v3 color = V3(m->base_color[0], m->base_color[1], m->base_color[2]);
    v3 transmission_color = V3(sqrtf(color.x), sqrtf(color.y), sqrtf(color.z));
    v3 emission = v3scale(V3(m->emission_color[0], m->emission_color[1], m->emission_color[2]), m->emission_strength);
    float metallic = m->metallic, roughness = m->roughness, eta = m->ior, transmission = m->transmission_weight;
    v3 specular_tint = V3(m->specular_tint[0], m->specular_tint[1], m->specular_tint[2]);
    v3 coat_tint = V3(m->coat_tint[0], m->coat_tint[1], m->coat_tint[2]);
    or_surface *diffuse = pool_new(p, OR_S_DIFFUSE);
    diffuse->color = v3scale(color, OR_INV_PI);
    /* specular (dielectric reflection scaled by f0) */
    float eta_s = eta, f0 = or_f0_from_ior(eta_s);
    if (m->specular_ior_level != 0.5f) { f0 *= 2.0f * m->specular_ior_level; eta_s = or_ior_from_f0(f0); }
    or_surface *specular = mk_refl(p, v3scale(specular_tint, f0), OR_FR_DIELECTRIC, eta_s, roughness);
    or_surface *coat = mk_refl(p, v3scale(V3(1, 1, 1), m->coat_weight), OR_FR_DIELECTRIC, m->coat_ior, m->coat_roughness);
    /* dielectric = Addictive{frac: fr_dielectric(cos wo, eta), a: transmission, b: reflection} */
    or_surface *d_refl = mk_refl(p, color, OR_FR_DIELECTRIC, eta, roughness);
    or_surface *d_trans = pool_new(p, OR_S_MF_TRANS);
    d_trans->color = transmission_color; d_trans->fresnel = OR_FR_DIELECTRIC; d_trans->eta = eta;
    d_trans->alpha = tr_alpha_from_roughness(roughness, roughness); d_trans->roughness = roughness;
    or_surface *dielectric = pool_new(p, OR_S_MIXTURE);
    dielectric->mode = OR_BLEND_ADDICTIVE; dielectric->frac_kind = OR_FRAC_FR_DIELECTRIC; dielectric->frac_eta = eta;
    dielectric->a = d_trans; dielectric->b = d_refl;
    /* metal */
    or_surface *metal = mk_refl(p, V3(1, 1, 1), OR_FR_COMPLEX, 0.0f, roughness);
    or_artistic_to_conductor(color, specular_tint, &metal->fn, &metal->fk);
    /* Mix(transmission){diffuse, dielectric} */
    or_surface *b1 = pool_new(p, OR_S_MIXTURE);
    b1->mode = OR_BLEND_MIX; b1->frac_kind = OR_FRAC_CONST; b1->frac_const = transmission; b1->a = diffuse; b1->b = dielectric;
    /* Coated{top: specular, bottom: b1, E = specular_tint * A(roughness,|cos|,eta_s) * f0} */
    or_surface *b2 = pool_new(p, OR_S_COATED);
    b2->a = specular; b2->b = b1; b2->etop_tint = specular_tint; b2->etop_weight = f0; b2->etop_roughness = roughness;
    b2->etop_eta = eta_s; b2->table = sc->table;
    /* Mix(metallic){b2, metal} */
    or_surface *b3 = pool_new(p, OR_S_MIXTURE);
    b3->mode = OR_BLEND_MIX; b3->frac_kind = OR_FRAC_CONST; b3->frac_const = metallic; b3->a = b2; b3->b = metal;
    or_surface *b4 = pool_new(p, OR_S_EMISSIVE);
    b4->a = b3; b4->emission = emission;
    or_surface *scaled = pool_new(p, OR_S_SCALED);
    scaled->a = b4; scaled->color = v3lerp(V3(1, 1, 1), coat_tint, m->coat_weight);
    or_surface *b5 = pool_new(p, OR_S_COATED);
    b5->a = coat; b5->b = scaled; b5->etop_tint = V3(1, 1, 1); b5->etop_weight = m->coat_weight;
    b5->etop_roughness = m->coat_roughness; b5->etop_eta = m->coat_ior; b5->table = sc->table;
    or_surface *wrap = pool_new(p, OR_S_PRINCIPLED);
    wrap->a = b5; wrap->color = color; wrap->emission = emission;
    /* normal_map(surface, (-nx,-ny,nz), ng, frame, TangentSpace), svm/surface/mod.rs:1380-1417 */
    v3 normal = V3(-m->normal[0], -m->normal[1], m->normal[2]);
    or_surface *nm = pool_new(p, OR_S_CLOSURE);
    nm->a = wrap;
    if (normal.x == 0.0f && normal.y == 0.0f && normal.z == 0.0f) {
        nm->frame.n = V3(0, 0, 1); nm->frame.t = V3(1, 0, 0); nm->frame.s = V3(0, 1, 0);
    } else {
        v3 nn = v3normalize(normal);
        v3 n_world = or_to_world(&si->frame, nn);
        or_frame nf = or_frame_from_n_t(n_world, si->frame.t);
        nm->frame.t = or_to_local(&si->frame, nf.t);
        nm->frame.s = or_to_local(&si->frame, nf.s);
        nm->frame.n = or_to_local(&si->frame, nf.n);
    }
    nm->ng = or_to_local(&si->frame, si->ng);
    return nm;
}
/* svm/eval.rs:468-495 dispatch_surface: SurfaceClosure{inner: shader output, frame: si.frame, ng: si.ng};
 * pt.rs:268-279 for force_diffuse */
static or_surface *or_build_closure(or_closure_pool *p, const or_scene *sc, const or_si *si, int force_diffuse) {
    p->count = 0;
    or_surface *inner;
    if (force_diffuse) {
        inner = pool_new(p, OR_S_DIFFUSE);
        float r = (1.0f * OR_INV_PI) * 0.8f;
        inner->color = V3(r, r, r);
    } else {
        or_material_desc at;
        or_material_at(&sc->materials[si->material], sc->graphs ? &sc->graphs[si->material] : 0, sc->images, sc->color, si->uv.x, si->uv.y, &at);
        const or_material_desc *m = &at;
        switch (m->kind) {
        case OR_MAT_PRINCIPLED: inner = or_build_principled(p, sc, m, si); break;
        case OR_MAT_DIFFUSE: /* diffuse.rs:83-104 */
            inner = pool_new(p, OR_S_DIFFUSE);
            inner->color = v3scale(V3(m->base_color[0], m->base_color[1], m->base_color[2]), OR_INV_PI);
            break;
        case OR_MAT_GLASS: { /* glass.rs:13-45 */
            v3 k = V3(m->base_color[0], m->base_color[1], m->base_color[2]);
            or_surface *refl = mk_refl(p, k, OR_FR_DIELECTRIC, m->ior, m->roughness);
            or_surface *trans = pool_new(p, OR_S_MF_TRANS);
            trans->color = k; trans->fresnel = OR_FR_DIELECTRIC; trans->eta = m->ior;
            trans->alpha = tr_alpha_from_roughness(m->roughness, m->roughness); trans->roughness = m->roughness;
            inner = pool_new(p, OR_S_MIXTURE);
            inner->mode = OR_BLEND_ADDICTIVE; inner->frac_kind = OR_FRAC_FR_DIELECTRIC; inner->frac_eta = m->ior;
            inner->a = trans; inner->b = refl;
            break;
        }
        default: /* OR_MAT_EMISSION, svm/mod.rs:114-123 */
            inner = pool_new(p, OR_S_EMISSIVE);
            inner->a = 0;
            inner->emission = v3scale(V3(m->emission_color[0], m->emission_color[1], m->emission_color[2]), m->emission_strength);
            break;
        }
    }
    or_surface *c = pool_new(p, OR_S_CLOSURE);
    c->a = inner; c->frame = si->frame; c->ng = si->ng;
    return c;
}
/* AreaLightExpr::emission (area.rs:19-31): always the real material, never force_diffuse */
static v3 or_material_emission(const or_scene *sc, const or_si *si, v3 wo) {
    or_closure_pool pool;
    or_surface *c = or_build_closure(&pool, sc, si, 0);
    return or_surf_emission(c, wo);
}

/* ---------------------------------- lights ------------------------------------------------------- */
static float or_mis_weight(float a, float b) { float pa = 1.0f * a, pb = 1.0f * b; return pa / (pa + pb); } /* pt.rs:962-973, power 1 */

typedef struct { v3 li, wi; float pdf; or_ray shadow_ray; int valid; int delta; } or_light_sample;
/* light/mod.rs:115-132 + light/area.rs:51-107 */
static or_light_sample or_sample_direct(const or_scene *sc, v3 pn_p, v3 pn_n, float u_select, v2 u_sample) {
    or_light_sample s;
    memset(&s, 0, sizeof s);
    if (sc->n_lights == 0) return s;
    float light_choice_pdf, u_sel2, pdf_prim, u_unused;
    uint32_t light_idx = or_alias_sample_and_remap(&sc->light_dist, u_select, &light_choice_pdf, &u_sel2);
    if (sc->env && light_idx == sc->n_lights - 1) { /* the environment (4.8 NEE): u_sample picks the direction; unbounded shadow ray */
        v3 wi;
        float pdf;
        int ok = or_env_sample(sc->env, u_sample, &wi, &pdf);
        s.li = or_env_eval(sc->env, sc->color, wi);
        s.shadow_ray.o = or_offset_ray_origin(pn_p, or_face_forward(pn_n, wi));
        s.shadow_ray.d = wi; s.shadow_ray.t_min = 0.0f; s.shadow_ray.t_max = 1e20f;
        s.shadow_ray.ex0_inst = OR_INVALID; s.shadow_ray.ex0_prim = OR_INVALID;
        s.shadow_ray.ex1_inst = OR_INVALID; s.shadow_ray.ex1_prim = OR_INVALID;
        s.wi = wi;
        s.valid = ok;
        s.pdf = pdf * light_choice_pdf;
        return s;
    }
    if (sc->light_inst[light_idx] == OR_PUNCT_INST || sc->light_inst[light_idx] == OR_PUNCT_TREE_INST) {
        /* a punctual light (4.14 / 4.15 Sampling): NEE only, pdf = the choice's. The tree's entry (4.16 Walk) first descends with the
         * number the choice left to one record, and its pdf is the walked product; the sample is that record's with u_sample unchanged. */
        uint32_t record = sc->light_rec[light_idx];
        if (sc->light_inst[light_idx] == OR_PUNCT_TREE_INST && !or_lt_walk(sc->lt_nodes, pn_p, u_sel2, &light_choice_pdf, &record)) {
            s.pdf = light_choice_pdf; s.delta = 1; /* the bound was reached on an inner node: invalid (no tree the build makes) */
            return s;
        }
        const or_punct *L = &sc->punct[sc->color & 3u][record];
        const or_punct_ls ps = or_punct_sample(L, pn_p, pn_n, u_sample);
        s.li = ps.li; s.wi = ps.wi;
        s.shadow_ray.o = ps.ro; s.shadow_ray.d = ps.wi; s.shadow_ray.t_min = 0.0f; s.shadow_ray.t_max = ps.tmax;
        s.shadow_ray.ex0_inst = OR_INVALID; s.shadow_ray.ex0_prim = OR_INVALID;
        s.shadow_ray.ex1_inst = OR_INVALID; s.shadow_ray.ex1_prim = OR_INVALID;
        s.valid = ps.valid;
        s.pdf = light_choice_pdf;
        s.delta = 1;
        return s;
    }
    uint32_t inst_id = sc->light_inst[light_idx];
    uint32_t prim_id = or_alias_sample_and_remap(&sc->instances[inst_id].area_sampler, u_sel2, &pdf_prim, &u_unused);
    v2 bary = or_uniform_sample_triangle(u_sample);
    or_si si = or_surface_interaction(sc, inst_id, prim_id, bary);
    float area = si.prim_area;
    v3 p = si.p, n = si.ng;
    v3 wi = v3sub(p, pn_p);
    if (v3len2(wi) == 0.0f) { s.pdf = pdf_prim * light_choice_pdf; s.wi = wi; return s; }
    float dist2 = v3len2(wi);
    wi = v3divs(wi, sqrtf(dist2));
    v3 emission = or_material_emission(sc, &si, v3neg(wi));
    s.li = v3dot(wi, n) < 0.0f ? emission : V3(0, 0, 0);
    float cos_theta_i = fabsf(v3dot(n, wi));
    float pdf = pdf_prim / area * dist2 / cos_theta_i;
    v3 ro = or_offset_ray_origin(pn_p, or_face_forward(pn_n, wi));
    float dist = sqrtf(dist2);
    s.shadow_ray.o = ro; s.shadow_ray.d = wi; s.shadow_ray.t_min = 0.0f; s.shadow_ray.t_max = dist * (1.0f - 1e-3f);
    s.shadow_ray.ex0_inst = OR_INVALID; s.shadow_ray.ex0_prim = OR_INVALID;
    s.shadow_ray.ex1_inst = inst_id; s.shadow_ray.ex1_prim = prim_id;
    s.wi = wi;
    s.valid = or_isfinite(pdf);
    s.pdf = pdf * light_choice_pdf;
    return s;
}
/* light/mod.rs:134-147 + light/area.rs:109-130 */
static float or_pdf_direct(const or_scene *sc, const or_si *si, v3 pn_p) {
    const or_instance *inst = &sc->instances[si->inst];
    float light_choice_pdf = sc->light_dist.pdf[inst->light];
    float prim_pdf = inst->area_sampler.pdf[si->prim];
    v3 wi = v3sub(si->p, pn_p);
    float dist2 = v3len2(wi);
    wi = v3divs(wi, sqrtf(dist2));
    float pdf = prim_pdf / si->prim_area * dist2 / or_max(fabsf(v3dot(si->ng, wi)), 1e-6f);
    return light_choice_pdf * pdf;
}

/* load.rs:94-127 has_potential_surface_emission, for constant inputs */
static int or_has_potential_emission(const or_material_desc *m) {
    if (m->kind != OR_MAT_PRINCIPLED && m->kind != OR_MAT_EMISSION) return 1; /* (None, None) -> true */
    float power = or_max(or_max(m->emission_color[0], m->emission_color[1]), m->emission_color[2]); /* rgb -> max */
    return !(power * m->emission_strength == 0.0f);
}
/* load.rs:312-343: 16-sample estimate of max(emission) * area per triangle */
static float or_estimate_power(const or_scene *sc, uint32_t inst_id, uint32_t tri) {
    or_pcg32 rng = pcg_new_seq((uint64_t)tri);
    float acc = 0.0f;
    for (int k = 0; k < 16; k++) {
        float a = pcg_next_1d(&rng), b = pcg_next_1d(&rng);
        v2 bary = or_uniform_sample_triangle(V2(a, b));
        or_si si = or_surface_interaction(sc, inst_id, tri, bary);
        float c = pcg_next_1d(&rng), d = pcg_next_1d(&rng);
        v3 wo = or_to_world(&si.frame, or_cos_sample_hemisphere(V2(c, d)));
        v3 e = or_material_emission(sc, &si, wo);
        acc += v3max(e) * si.prim_area;
    }
    return acc / 16.0f;
}

/* ---------------------------------- scene construction ------------------------------------------ */
/* raster -> camera, camera/mod.rs:119-153, with t = tan(fov / 2); an orthographic camera hands in half its scale */
static void or_raster_to_camera(uint32_t width, uint32_t height, float t, float *r2c) {
    float m[16], s[16];
    float fw = (float)width, fh = (float)height;
    m4_scale(1, 1, 1, m);
    m4_scale(1.0f / fw, 1.0f / fh, 1.0f, s); m4_mul(s, m, m);
    m4_scale(2.0f, 2.0f, 1.0f, s); m4_mul(s, m, m);
    m4_translate(-1.0f, -1.0f, 0.0f, s); m4_mul(s, m, m);
    m4_scale(1.0f, -1.0f, 1.0f, s); m4_mul(s, m, m);
    if (width > height) m4_scale(t, t * fh / fw, 1.0f, s); else m4_scale(t * fw / fh, t, 1.0f, s);
    m4_mul(s, m, m);
    m4_translate(0.0f, 0.0f, -1.0f, s); m4_mul(s, m, m);
    memcpy(r2c, m, 64);
}
/* The host's part of a projection (4.17 "Definition"), for the scene's present resolution: the matrix of the camera in use and a
 * panorama's six constants, each rounded once. Runs whenever the projection or the resolution is set. */
static void or_projection_fold(or_scene *sc) {
    const or_projection_desc *p = &sc->proj;
    or_raster_to_camera(sc->width, sc->height, p->type == OR_PROJECTION_ORTHOGRAPHIC ? 0.5f * p->ortho_scale : tanf(sc->fov / 2.0f), sc->r2c);
    sc->pano_lon0 = p->longitude_min;
    sc->pano_dlon = p->longitude_max - p->longitude_min;
    sc->pano_lat1 = p->latitude_max;
    sc->pano_dlat = p->latitude_max - p->latitude_min;
    sc->pano_inv_w = 1.0f / (float)sc->width;
    sc->pano_inv_h = 1.0f / (float)sc->height;
}
static const or_projection_desc OR_PROJECTION_DEFAULT = {OR_PROJECTION_PERSPECTIVE, 1.0f, -3.14159274f, 3.14159274f, -1.57079637f, 1.57079637f};
static void or_camera_setup(or_scene *sc, const or_camera_desc *c) { /* camera/mod.rs:119-153 */
    memcpy(sc->c2w, c->c2w, 64);
    sc->c2w_identity = 1; /* glam abs_diff_eq(IDENTITY, 1e-4), geometry.rs:212-218 */
    for (int i = 0; i < 16; i++) {
        float id = (i % 5 == 0) ? 1.0f : 0.0f;
        if (!(fabsf(c->c2w[i] - id) <= 1e-4f)) sc->c2w_identity = 0;
    }
    sc->width = c->width; sc->height = c->height;
    sc->fov = c->fov;
    sc->proj = OR_PROJECTION_DEFAULT;
    or_projection_fold(sc);
}

OR_EXPORT void or_scene_destroy(or_scene *sc);

OR_EXPORT or_scene *or_scene_create(const or_scene_desc *d) {
    or_scene *sc = (or_scene *)calloc(1, sizeof(or_scene));
    sc->n_meshes = d->n_meshes; sc->n_instances = d->n_instances; sc->n_materials = d->n_materials;
    sc->meshes = (or_mesh *)calloc(d->n_meshes ? d->n_meshes : 1, sizeof(or_mesh));
    for (uint32_t i = 0; i < d->n_meshes; i++) {
        const or_mesh_desc *s = &d->meshes[i];
        or_mesh_desc *m = &sc->meshes[i].d;
        *m = *s;
        m->vertices = (float *)or_dup(s->vertices, 12ull * s->n_vertices);
        m->indices = (uint32_t *)or_dup(s->indices, 12ull * s->n_triangles);
        m->uvs = (float *)or_dup(s->uvs, 24ull * s->n_triangles);
        m->normals = (float *)or_dup(s->normals, 36ull * s->n_triangles);
        m->tangents = (float *)or_dup(s->tangents, 36ull * s->n_triangles);
        m->material_slots = (uint32_t *)or_dup(s->material_slots, 4ull * s->n_triangles);
    }
    sc->materials = (or_material_desc *)or_dup(d->materials, sizeof(or_material_desc) * d->n_materials);
    sc->n_images = d->n_images;
    if (d->n_images) {
        sc->images = (or_image_desc *)or_dup(d->images, sizeof(or_image_desc) * d->n_images);
        for (uint32_t i = 0; i < d->n_images; i++) {
            size_t bytes = (size_t)d->images[i].width * d->images[i].height * (d->images[i].format == OR_IMAGE_RGBA32F ? 16 : 4);
            sc->images[i].texels = or_dup(d->images[i].texels, bytes);
        }
    }
    if (d->material_graphs) {
        sc->graphs = (or_material_graph *)or_dup(d->material_graphs, sizeof(or_material_graph) * d->n_materials);
        for (uint32_t i = 0; i < d->n_materials; i++)
            sc->graphs[i].nodes = (or_shader_node *)or_dup(d->material_graphs[i].nodes, sizeof(or_shader_node) * d->material_graphs[i].n_nodes);
    }
    sc->instances = (or_instance *)calloc(d->n_instances ? d->n_instances : 1, sizeof(or_instance));
    uint32_t n_tris = 0;
    for (uint32_t i = 0; i < d->n_instances; i++) {
        const or_instance_desc *s = &d->instances[i];
        or_instance *in = &sc->instances[i];
        in->mesh = s->mesh; in->n_materials = s->n_materials;
        in->materials = (uint32_t *)or_dup(s->materials, 4ull * s->n_materials);
        const float *m = s->transform;
        in->xf.c0 = V3(m[0], m[1], m[2]); in->xf.c1 = V3(m[4], m[5], m[6]); in->xf.c2 = V3(m[8], m[9], m[10]);
        in->xf.t = V3(m[12], m[13], m[14]);
        in->xf.det = v3dot(in->xf.c0, v3cross(in->xf.c1, in->xf.c2)); /* mesh.rs:309-310 transform_det */
        in->light = -1;
        in->tri_offset = n_tris;
        n_tris += sc->meshes[s->mesh].d.n_triangles;
    }
    sc->n_tris = n_tris;
    sc->woop = (float *)malloc(48ull * n_tris + 4);
    sc->tri_inst = (uint32_t *)malloc(4ull * n_tris + 4); sc->tri_prim = (uint32_t *)malloc(4ull * n_tris + 4);
    for (uint32_t i = 0; i < d->n_instances; i++) {
        const or_instance *in = &sc->instances[i];
        const or_mesh_desc *g = &sc->meshes[in->mesh].d;
        for (uint32_t p = 0; p < g->n_triangles; p++) {
            uint32_t k = in->tri_offset + p;
            v3 a = xf_point(&in->xf, ld3(g->vertices, g->indices[3 * p]));
            v3 b = xf_point(&in->xf, ld3(g->vertices, g->indices[3 * p + 1]));
            v3 c = xf_point(&in->xf, ld3(g->vertices, g->indices[3 * p + 2]));
            or_woop_precompute(a, b, c, sc->woop + 12 * k);
            if ((p & 1u) && g_or_share_plane_rows) or_share_plane_row(sc->woop + 12 * (k - 1), sc->woop + 12 * k, a, b, c);
            sc->tri_inst[k] = i; sc->tri_prim[k] = p;
        }
    }
    if (d->ggx_dielectric_table) { memcpy(sc->table, d->ggx_dielectric_table, sizeof sc->table); sc->has_table = 1; }
    or_camera_setup(sc, &d->camera);
    /* light discovery, load.rs:345-444 */
    sc->light_inst = (uint32_t *)malloc(4ull * (d->n_instances + 1));
    sc->light_power = (float *)malloc(4ull * (d->n_instances + 1));
    for (uint32_t i = 0; i < d->n_instances; i++) {
        or_instance *in = &sc->instances[i];
        int any = 0;
        for (uint32_t k = 0; k < in->n_materials; k++) {
            uint32_t mid = in->materials[k];
            const or_material_desc *md = &sc->materials[mid];
            const or_material_graph *gr = sc->graphs ? &sc->graphs[mid] : 0;
            if (gr && gr->n_nodes && ((md->kind & OR_MAT_KIND_MASK) == OR_MAT_PRINCIPLED || (md->kind & OR_MAT_KIND_MASK) == OR_MAT_EMISSION) &&
                (or_node_varies(gr, gr->input[OR_IN_EMISSION_COLOR]) || or_node_varies(gr, gr->input[OR_IN_EMISSION_STRENGTH]))) {
                any |= 1; /* estimate_emission_tex_intensity_fast -> None (load.rs:76-92) */
            } else {
                or_material_desc at; /* constant nodes feeding the emission inputs are folded first */
                or_material_at(md, gr, sc->images, 0, 0.0f, 0.0f, &at);
                any |= or_has_potential_emission(&at);
            }
        }
        if (!any) continue;
        uint32_t nt = sc->meshes[in->mesh].d.n_triangles;
        float *powers = (float *)malloc(4ull * nt + 4);
        float total = 0.0f;
        for (uint32_t p = 0; p < nt; p++) { powers[p] = or_estimate_power(sc, i, p); total += powers[p]; }
        if (total > 1e-4f) {
            in->light = (int32_t)sc->n_lights;
            sc->light_inst[sc->n_lights] = i;
            sc->light_power[sc->n_lights] = total;
            sc->n_lights++;
            or_alias_build(&in->area_sampler, powers, nt);
        }
        free(powers);
    }
    sc->n_emit = sc->n_lights;
    if (sc->n_lights > 0) or_alias_build(&sc->light_dist, sc->light_power, sc->n_lights);
    return sc;
}

OR_EXPORT void or_scene_destroy(or_scene *sc) {
    if (!sc) return;
    for (uint32_t i = 0; i < sc->n_meshes; i++) {
        or_mesh_desc *m = &sc->meshes[i].d;
        free((void *)m->vertices); free((void *)m->indices); free((void *)m->uvs); free((void *)m->normals);
        free((void *)m->tangents); free((void *)m->material_slots);
    }
    for (uint32_t i = 0; i < sc->n_instances; i++) {
        free(sc->instances[i].materials);
        if (sc->instances[i].light >= 0) or_alias_free(&sc->instances[i].area_sampler);
    }
    if (sc->n_lights > 0) or_alias_free(&sc->light_dist);
    for (uint32_t i = 0; i < sc->n_images; i++) free((void *)sc->images[i].texels);
    if (sc->graphs) for (uint32_t i = 0; i < sc->n_materials; i++) free((void *)sc->graphs[i].nodes);
    free(sc->images); free(sc->graphs);
    free(sc->meshes); free(sc->instances); free(sc->materials);
    free(sc->woop); free(sc->tri_inst); free(sc->tri_prim);
    free(sc->light_inst); free(sc->light_power); free(sc->light_rec); free(sc->lt_nodes);
    or_env_free(sc->env);
    free(sc->punct_desc);
    for (int k = 0; k < 4; k++) free(sc->punct[k]);
    or_scene_free_bvh(sc);
    free(sc);
}

/* ---------------------------------- camera + filter ---------------------------------------------- */
/* IndependentSampler (sampler/mod.rs:161-217): pcg + dim. Pmj02BnSampler (sampler/mod.rs:329-700): pmj != 0, state =
 * Pmj02BnState {seed, dim, pixel, sample_index, spp, w}. The two tables are handed in by the test (or_set_pmj_tables): the
 * reference's own are absent from its tree, the build regenerates them (akari_render_amd/csrc/host/pmj_tables.cpp). */
struct or_mcmc_smp;
typedef struct { or_pcg32 pcg; uint32_t dim; int pmj; uint32_t seed, px, py, sample_index, spp, w; struct or_mcmc_smp *mc; } or_sampler;
static float or_mcmc_next_1d(or_sampler *s); /* LazyMcmcSampler (mcmc_opt.rs:61-119), further down */
static const uint32_t *g_pmj_sets;   /* [5][65536][2] */
static const uint16_t *g_bluenoise;  /* [48][128][128] */
OR_EXPORT void or_set_pmj_tables(const uint32_t *sets, const uint16_t *bluenoise) { g_pmj_sets = sets; g_bluenoise = bluenoise; }
static uint32_t or_permute_element(uint32_t i, uint32_t l, uint32_t w, uint32_t p) { /* sampler/mod.rs:473-507 */
    do {
        i ^= p; i *= 0xe170893du; i ^= p >> 16; i ^= (i & w) >> 4; i ^= p >> 8; i *= 0x0929eb3fu; i ^= p >> 23;
        i ^= (i & w) >> 1; i *= 1u | p >> 27; i *= 0x6935fa69u; i ^= (i & w) >> 11; i *= 0x74dcb303u; i ^= (i & w) >> 2;
        i *= 0x9e501cc3u; i ^= (i & w) >> 2; i *= 0xc860a3dfu; i &= w; i ^= i >> 5;
    } while (i >= l);
    return (i + p) % l;
}
static float or_bluenoise(uint32_t tex, uint32_t px, uint32_t py) { /* uv = p.yx() % 128, texture tex % 48, unorm16 */
    uint32_t tx = py % 128u, ty = px % 128u;
    return (float)g_bluenoise[((size_t)(tex % 48u) * 128u + ty) * 128u + tx] / 65535.0f;
}
#define OR_ONE_MINUS_EPSILON 0.99999994f
/* The "sobol" sampler (sampler_type 2; no reference counterpart beyond the sobolmat data stub, akari_data/src/lib.rs:13,19):
 * Pmj02BnSampler's state and interface, points from an Owen-scrambled Sobol' (0,2)-sequence computed on the fly. */
static uint32_t or_reverse_bits32(uint32_t x) {
    x = (x >> 16) | (x << 16);
    x = ((x & 0xff00ff00u) >> 8) | ((x & 0x00ff00ffu) << 8);
    x = ((x & 0xf0f0f0f0u) >> 4) | ((x & 0x0f0f0f0fu) << 4);
    x = ((x & 0xccccccccu) >> 2) | ((x & 0x33333333u) << 2);
    x = ((x & 0xaaaaaaaau) >> 1) | ((x & 0x55555555u) << 1);
    return x;
}
static uint32_t or_owen_scramble(uint32_t x, uint32_t seed) { /* Laine-Karras hash between two bit reversals */
    x = or_reverse_bits32(x);
    x += seed; x ^= x * 0x6c50b47cu; x ^= x * 0xb82f1e52u; x ^= x * 0xc7afe638u; x ^= x * 0x8d22f6e6u;
    return or_reverse_bits32(x);
}
static uint32_t or_sobol_dim1(uint32_t i) {
    uint32_t v = 0x80000000u, r = 0;
    for (; i; i >>= 1) { if (i & 1u) r ^= v; v ^= v >> 1; }
    return r;
}
static inline float smp_1d(or_sampler *s) {
    if (s->mc) return or_mcmc_next_1d(s);
    if (!s->pmj) { s->dim += 1; return pcg_next_1d(&s->pcg); }
    uint32_t hash = or_xxhash32_4(s->px, s->py, s->dim, s->seed);
    uint32_t index = or_permute_element(s->sample_index, s->spp, s->w, hash);
    if (s->pmj == 2) {
        uint32_t v = or_owen_scramble(or_reverse_bits32(index), or_xxhash32_4(s->py, s->px, s->dim, ~s->seed));
        s->dim += 1;
        return or_min((float)v * 2.3283064365386963e-10f, OR_ONE_MINUS_EPSILON);
    }
    float delta = or_bluenoise(s->dim, s->px, s->py);
    s->dim += 1;
    return or_min(((float)index + delta) / (float)s->spp, OR_ONE_MINUS_EPSILON);
}
static inline v2 smp_2d(or_sampler *s) {
    if (!s->pmj) { float a = smp_1d(s); float b = smp_1d(s); return V2(a, b); }
    uint32_t index = s->sample_index, dim = s->dim, inst = dim / 2;
    if (s->pmj == 2) {
        uint32_t i = or_permute_element(index, s->spp, s->w, or_xxhash32_4(s->px, s->py, dim, s->seed));
        uint32_t vx = or_owen_scramble(or_reverse_bits32(i), or_xxhash32_4(s->py, s->px, dim, ~s->seed));
        uint32_t vy = or_owen_scramble(or_sobol_dim1(i), or_xxhash32_4(s->py, s->px, dim + 1u, ~s->seed));
        s->dim += 2;
        return V2(or_min((float)vx * 2.3283064365386963e-10f, OR_ONE_MINUS_EPSILON), or_min((float)vy * 2.3283064365386963e-10f, OR_ONE_MINUS_EPSILON));
    }
    if (inst >= 5u) index = or_permute_element(s->sample_index, s->spp, s->w, or_xxhash32_4(s->px, s->py, dim, s->seed));
    const uint32_t *p = g_pmj_sets + 2 * ((size_t)65536 * (inst % 5u) + (index % 65536u));
    float ux = (float)p[0] * 2.3283064365386963e-10f, uy = (float)p[1] * 2.3283064365386963e-10f;
    float dx = or_bluenoise(dim, s->px, s->py), dy = or_bluenoise(dim + 1, s->px, s->py);
    ux = ux + dx; uy = uy + dy;
    s->dim += 2;
    ux = ux - floorf(ux); uy = uy - floorf(uy);
    return V2(or_min(ux, OR_ONE_MINUS_EPSILON), or_min(uy, OR_ONE_MINUS_EPSILON));
}
static inline v3 smp_3d(or_sampler *s) { float a = smp_1d(s); v2 b = smp_2d(s); return V3(a, b.x, b.y); }
static inline void smp_start(or_sampler *s) { /* sampler.start() */
    if (!s->pmj) { pcg_advance(&s->pcg, 16384); return; }
    s->dim = 4;
    s->sample_index = s->sample_index == 0xffffffffu ? 0u : s->sample_index + 1u;
}
/* creation from the per-pixel state buffer + Drop at the end of a pass; for pmj02bn the Pcg32 slot carries
 * {state = sample_index, inc = x | y << 32} (the layout the HIP side uses, so that sampler states can be compared) */
static inline or_sampler smp_create(const or_pt_config *cfg, or_pcg32 st, uint32_t spp_total) {
    or_sampler s;
    memset(&s, 0, sizeof s);
    s.pcg = st;
    if (cfg->sampler_type == 1 || cfg->sampler_type == 2) {
        s.pmj = (int)cfg->sampler_type; s.seed = (uint32_t)cfg->sampler_seed; s.spp = spp_total ? spp_total : 1;
        uint32_t w = s.spp - 1; w |= w >> 1; w |= w >> 2; w |= w >> 4; w |= w >> 8; w |= w >> 16;
        s.w = w;
        s.sample_index = (uint32_t)st.state; s.px = (uint32_t)st.inc; s.py = (uint32_t)(st.inc >> 32);
    }
    return s;
}
static inline or_pcg32 smp_drop(or_sampler *s) {
    if (!s->pmj) { pcg_advance(&s->pcg, -(int64_t)s->dim); return s->pcg; }
    or_pcg32 st = {s->sample_index, (uint64_t)s->px | ((uint64_t)s->py << 32)};
    return st;
}

static v2 or_filter_sample(const or_pt_config *cfg, v2 u) { /* film.rs:32-49 */
    if (cfg->filter_type == OR_FILTER_BOX) return V2((u.x - 0.5f) * cfg->filter_radius, (u.y - 0.5f) * cfg->filter_radius);
    float width = cfg->filter_radius;
    float sigma = width / 3.0f;
    float r = sqrtf(-2.0f * or_logf(u.x));
    float theta = 2.0f * OR_PI * u.y;
    float sn, cs;
    or_sincosf(theta, &sn, &cs);
    v2 off = V2((r * cs) * sigma, (r * sn) * sigma);
    return V2(or_clamp(off.x, -width, width), or_clamp(off.y, -width, width));
}
/* Camera -> world of DESIGN.md 4.9 step 4 for a camera-space origin and direction: nothing under the c2w_identity shortcut, else the
 * point formula for the origin (rotation columns and translation, over w) and the rotation for the direction, summed left to right. */
static void or_camera_to_world(const or_scene *sc, v3 *o, v3 *d) {
    if (sc->c2w_identity) return;
    const float *c = sc->c2w;
    const v3 p = *o, v = *d;
    const float r0 = ((c[0] * p.x + c[4] * p.y) + c[8] * p.z) + c[12] * 1.0f;
    const float r1 = ((c[1] * p.x + c[5] * p.y) + c[9] * p.z) + c[13] * 1.0f;
    const float r2 = ((c[2] * p.x + c[6] * p.y) + c[10] * p.z) + c[14] * 1.0f;
    const float r3 = ((c[3] * p.x + c[7] * p.y) + c[11] * p.z) + c[15] * 1.0f;
    *o = v3divs(V3(r0, r1, r2), r3);
    *d = V3((c[0] * v.x + c[4] * v.y) + c[8] * v.z, (c[1] * v.x + c[5] * v.y) + c[9] * v.z, (c[2] * v.x + c[6] * v.y) + c[10] * v.z);
}
/* The camera ray of a film sample for given numbers (camera/mod.rs:70-103; with a lens DESIGN.md 4.9 steps 2 - 5: u_lens -> the point l of
 * the lens disk, the pinhole direction's point on the plane of focus, the ray from l through it; the weight stays the filter's). The
 * orthographic and the panorama camera restate DESIGN.md 4.17 "Definition"; the perspective arm is the text it was. */
static or_ray or_camera_ray(const or_scene *sc, const or_pt_config *cfg, uint32_t px, uint32_t py, v2 u_filter, v2 u_lens) {
    v2 fpixel = V2((float)px + 0.5f, (float)py + 0.5f);
    v2 offset = or_filter_sample(cfg, u_filter);
    v2 pf = V2(fpixel.x + offset.x, fpixel.y + offset.y);
    if (sc->proj.type == OR_PROJECTION_PANORAMA) {
        /* longitude grows to the right from lon0, latitude falls from lat1 with the rows; a film point outside the film continues both */
        const float lambda = sc->pano_lon0 + (pf.x * sc->pano_inv_w) * sc->pano_dlon;
        const float phi = sc->pano_lat1 - (pf.y * sc->pano_inv_h) * sc->pano_dlat;
        float sl, cl, sp, cp;
        or_sincosf(lambda, &sl, &cl);
        or_sincosf(phi, &sp, &cp);
        v3 pd = v3normalize(V3(cp * sl, sp, -(cp * cl)));
        v3 po = V3(0.0f, 0.0f, 0.0f);
        or_camera_to_world(sc, &po, &pd);
        or_ray pr = {po, pd, 0.0f, 1e20f, OR_INVALID, OR_INVALID, OR_INVALID, OR_INVALID};
        return pr;
    }
    const float *m = sc->r2c;
    /* r2c.transform_point((x,y,0)): M * (x,y,0,1), then / w */
    float qx = ((m[0] * pf.x + m[4] * pf.y) + m[8] * 0.0f) + m[12] * 1.0f;
    float qy = ((m[1] * pf.x + m[5] * pf.y) + m[9] * 0.0f) + m[13] * 1.0f;
    float qz = ((m[2] * pf.x + m[6] * pf.y) + m[10] * 0.0f) + m[14] * 1.0f;
    float qw = ((m[3] * pf.x + m[7] * pf.y) + m[11] * 0.0f) + m[15] * 1.0f;
    if (sc->proj.type == OR_PROJECTION_ORTHOGRAPHIC) {
        /* the film point itself is the origin, on the plane z = 0 of camera space; every ray looks along -z. A lens moves the origin over
         * its disk and aims at the point the lens-less ray has on the plane z = -F, which therefore stays sharp */
        const v3 s = v3divs(V3(qx, qy, qz), qw);
        v3 oo = V3(s.x, s.y, 0.0f), od = V3(0.0f, 0.0f, -1.0f);
        if (sc->lens_radius > 0.0f) {
            const v2 ab = or_concentric_disk(u_lens);
            const float lx = sc->lens_radius * ab.x, ly = sc->lens_radius * ab.y;
            oo = V3(s.x + lx, s.y + ly, 0.0f);
            od = v3normalize(V3(-lx, -ly, -sc->lens_focal));
        }
        or_camera_to_world(sc, &oo, &od);
        or_ray rr = {oo, od, 0.0f, 1e20f, OR_INVALID, OR_INVALID, OR_INVALID, OR_INVALID};
        return rr;
    }
    v3 d = v3normalize(v3divs(V3(qx, qy, qz), qw));
    v3 o = V3(0, 0, 0);
    const float *c = sc->c2w;
    if (sc->lens_radius > 0.0f) {
        const v2 ab = or_concentric_disk(u_lens);                            /* step 2 */
        const v3 l = V3(sc->lens_radius * ab.x, sc->lens_radius * ab.y, 0.0f); /* step 3 */
        const float ft = sc->lens_focal / (-d.z);
        const v3 p_focus = v3scale(d, ft);
        d = v3normalize(v3sub(p_focus, l));
        o = l;
        if (!sc->c2w_identity) {                                             /* step 4 */
            const float r0 = ((c[0] * l.x + c[4] * l.y) + c[8] * l.z) + c[12] * 1.0f;
            const float r1 = ((c[1] * l.x + c[5] * l.y) + c[9] * l.z) + c[13] * 1.0f;
            const float r2 = ((c[2] * l.x + c[6] * l.y) + c[10] * l.z) + c[14] * 1.0f;
            const float r3 = ((c[3] * l.x + c[7] * l.y) + c[11] * l.z) + c[15] * 1.0f;
            o = v3divs(V3(r0, r1, r2), r3);
            d = V3((c[0] * d.x + c[4] * d.y) + c[8] * d.z, (c[1] * d.x + c[5] * d.y) + c[9] * d.z, (c[2] * d.x + c[6] * d.y) + c[10] * d.z);
        }
    } else if (!sc->c2w_identity) {
        float ow = c[15];
        o = v3divs(V3(c[12], c[13], c[14]), ow); /* M * (0,0,0,1) */
        d = V3((c[0] * d.x + c[4] * d.y) + c[8] * d.z, (c[1] * d.x + c[5] * d.y) + c[9] * d.z, (c[2] * d.x + c[6] * d.y) + c[10] * d.z);
    }
    or_ray r = {o, d, 0.0f, 1e20f, OR_INVALID, OR_INVALID, OR_INVALID, OR_INVALID};
    return r;
}
/* 4.9 step 1: the lens draws u_lens = next_2d right after the filter's next_2d; the pinhole draws nothing. 4.17 "Sampler dimensions": a
 * camera that is not the perspective one draws the pair whether or not it has a lens, and leaves it unused without one */
static or_ray or_generate_ray(const or_scene *sc, const or_pt_config *cfg, uint32_t px, uint32_t py, or_sampler *smp) {
    const v2 u_filter = smp_2d(smp);
    const int draws_lens = sc->lens_radius > 0.0f || sc->proj.type != OR_PROJECTION_PERSPECTIVE;
    const v2 u_lens = draws_lens ? smp_2d(smp) : V2(0.0f, 0.0f);
    return or_camera_ray(sc, cfg, px, py, u_filter, u_lens);
}

/* ---------------------------------- the path tracer, pt.rs:329-900 ------------------------------- */
static v3 or_radiance(const or_scene *sc, const or_pt_config *cfg, or_ray ray, or_sampler *smp, or_stats *st) {
    v3 radiance = V3(0, 0, 0), beta = V3(1, 1, 1), base = V3(0, 0, 0);
    uint32_t depth = 0;
    float prev_bsdf_pdf = 0.0f;
    v3 prev_ng = V3(0, 0, 0);
    const int use_nee = cfg->use_nee != 0, indirect_only = cfg->indirect_only != 0;
#define ADD_RADIANCE(r)                                                                             \
    do { if (cfg->debug_depth < 0 || depth == (uint32_t)cfg->debug_depth) radiance = v3add(radiance, v3mul(beta, (r))); } while (0)
    for (;;) {
        uint32_t h_inst = 0, h_prim = 0; v2 h_bary = V2(0, 0);
        st->n_closest++;
        if (!or_trace(sc, &ray, 0, &h_inst, &h_prim, &h_bary, st)) { /* pt.rs:381-396 */
            if (sc->env && (!indirect_only || depth > 1)) {
                /* the environment (4.8 Miss), weighted as an emitter; `base` is not captured: directly visible texels are clamped */
                v3 le = or_env_eval(sc->env, sc->color, ray.d);
                float w = 1.0f;
                if (depth != 0 && use_nee) w = or_mis_weight(prev_bsdf_pdf, sc->light_dist.pdf[sc->n_lights - 1] * or_env_pdf(sc->env, ray.d));
                ADD_RADIANCE(v3scale(le, w));
            }
            break;
        }
        or_si si = or_surface_interaction(sc, h_inst, h_prim, h_bary);
        v3 wo = v3neg(ray.d);
        { /* handle_surface_light, pt.rs:230-258 */
            const or_instance *inst = &sc->instances[si.inst];
            v3 direct = V3(0, 0, 0); float w = 0.0f;
            if (inst->light >= 0 && (!indirect_only || depth > 1)) {
                v3 emission = or_material_emission(sc, &si, v3neg(ray.d));
                direct = v3dot(si.ng, ray.d) < 0.0f ? emission : V3(0, 0, 0); /* area.rs:36-49 */
                if (depth == 0 || !use_nee) w = 1.0f;
                else w = or_mis_weight(prev_bsdf_pdf, or_pdf_direct(sc, &si, ray.o));
            }
            (void)prev_ng;
            ADD_RADIANCE(v3scale(direct, w));
        }
        if (depth == 0) base = radiance;
        if (depth >= cfg->max_depth) break;
        depth += 1;
        st->n_shaded++;
        v3 u_direct = smp_3d(smp);
        or_light_sample dl;
        memset(&dl, 0, sizeof dl);
        if (use_nee && (!indirect_only || depth > 1)) { /* sample_light, pt.rs:170-209 */
            dl = or_sample_direct(sc, si.p, si.ng, u_direct.x, V2(u_direct.y, u_direct.z));
            if (dl.valid) { dl.shadow_ray.ex0_inst = si.inst; dl.shadow_ray.ex0_prim = si.prim; }
            else { memset(&dl, 0, sizeof dl); }
        }
        v3 u_bsdf = smp_3d(smp);
        /* sample_surface_and_shade_direct, pt.rs:297-323 */
        or_closure_pool pool;
        or_surface *closure = or_build_closure(&pool, sc, &si, cfg->force_diffuse != 0);
        v3 direct = V3(0, 0, 0);
        if (dl.valid) {
            v3 f; float pdf;
            or_surf_evaluate(closure, wo, dl.wi, &f, &pdf);
            float w = dl.delta ? 1.0f : or_mis_weight(dl.pdf, pdf); /* 4.14: no ray ever hits a punctual light, no MIS partner */
            direct = v3divs(v3scale(v3mul(dl.li, f), w), dl.pdf);
        }
        or_bsdf_sample bs = or_closure_sample(closure, wo, u_bsdf.x, V2(u_bsdf.y, u_bsdf.z));
        if (dl.valid) { /* pt.rs:504-513 */
            st->n_shadow++;
            int occluded = or_trace(sc, &dl.shadow_ray, 1, 0, 0, 0, st);
            if (!occluded) ADD_RADIANCE(direct);
            if (depth == 1) base = radiance;
        }
        beta = v3mul(beta, v3divs(bs.color, bs.pdf)); /* pt.rs:783 (before the validity test) */
        if (bs.pdf <= 0.0f || !bs.valid || v3min(bs.color) < 0.0f) break; /* pt.rs:832-842 */
        if (depth > cfg->rr_depth) { /* pt.rs:211-224, 843-850 */
            float cont_prob = or_clamp(v3max(beta), 0.0f, 1.0f) * 0.95f;
            if (smp_1d(smp) >= cont_prob) break;
            beta = v3mul(beta, v3divs(V3(1, 1, 1), cont_prob));
        }
        prev_bsdf_pdf = bs.pdf; prev_ng = si.ng; /* pt.rs:851-865 */
        ray.o = or_offset_ray_origin(si.p, or_face_forward(si.ng, bs.wi));
        ray.d = bs.wi; ray.t_min = 0.0f; ray.t_max = 1e20f;
        ray.ex0_inst = si.inst; ray.ex0_prim = si.prim; ray.ex1_inst = OR_INVALID; ray.ex1_prim = OR_INVALID;
    }
#undef ADD_RADIANCE
    { /* pt.rs:871-876, clamp_indirect = 1000 */
        v3 ind = v3sub(radiance, base);
        ind = V3(or_clamp(ind.x, 0.0f, 1000.0f), or_clamp(ind.y, 0.0f, 1000.0f), or_clamp(ind.z, 0.0f, 1000.0f));
        radiance = v3add(base, ind);
    }
    return radiance;
}

/* ---------------------------------- render driver, pt.rs:1056-1159 ------------------------------- */
typedef struct {
    const or_scene *sc; const or_pt_config *cfg; float *film; or_pcg32 *states;
    uint32_t pass_spp; volatile uint32_t *next_row; or_stats stats;
    char pad[128]; /* one cache line (and its neighbour) per worker: the counters are bumped per ray */
} __attribute__((aligned(128))) or_job;

/* Tile sharding (no reference counterpart: SURVEY 8e's multi-GPU split): the tile of a pixel belongs to rank (Morton code of the tile's
 * coordinates) mod shard_count -- the product's definition (csrc/kernels.h tile_owner), restated. */
static uint32_t or_spread16(uint32_t x) {
    x &= 0xffffu;
    x = (x | (x << 8)) & 0x00ff00ffu; x = (x | (x << 4)) & 0x0f0f0f0fu; x = (x | (x << 2)) & 0x33333333u; x = (x | (x << 1)) & 0x55555555u;
    return x;
}
static int or_pixel_owned(const or_pt_config *cfg, uint32_t width, uint32_t x, uint32_t y) {
    (void)width;
    if (cfg->shard_count <= 1) return 1;
    uint32_t tw = cfg->tile_w ? cfg->tile_w : 32, th = cfg->tile_h ? cfg->tile_h : 32;
    uint32_t code = or_spread16(x / tw) | (or_spread16(y / th) << 1);
    return (code % cfg->shard_count) == cfg->shard_rank;
}
static void or_render_pixel(or_job *j, uint32_t x, uint32_t y) { /* kernel body, pt.rs:1077-1102 */
    const or_scene *sc = j->sc; const or_pt_config *cfg = j->cfg;
    uint32_t W = sc->width, H = sc->height, i = x + y * W;
    uint64_t N = (uint64_t)W * H;
    or_sampler smp = smp_create(cfg, j->states[i], cfg->spp);
    for (uint32_t s = 0; s < j->pass_spp; s++) {
        smp_start(&smp); /* sampler.start() */
        int32_t sx = (int32_t)x + cfg->pixel_offset[0], sy = (int32_t)y + cfg->pixel_offset[1];
        if (sx < 0) sx = 0; if (sx > (int32_t)W - 1) sx = (int32_t)W - 1;
        if (sy < 0) sy = 0; if (sy > (int32_t)H - 1) sy = (int32_t)H - 1;
        or_ray ray = or_generate_ray(sc, cfg, (uint32_t)sx, (uint32_t)sy, &smp);
        j->stats.n_samples++;
        v3 L = or_radiance(sc, cfg, ray, &smp, &j->stats);
        /* film.add_sample(p, L, w = 1): film.rs:196-229, color.rs:337-351 */
        if (or_isnan(L.x) || or_isnan(L.y) || or_isnan(L.z)) L = V3(0, 0, 0);
        if (cfg->color & OR_COLOR_REPR_ACES) { /* the film is sRGB: color.to_rgb(SRgb), film.rs:218, color.rs:262-275 */
            float c[3] = {L.x, L.y, L.z};
            or_cs_convert(c, 1, 0);
            L = V3(c[0], c[1], c[2]);
        }
        const float w = 1.0f;
        j->film[3 * (uint64_t)i + 0] += L.x * w;
        j->film[3 * (uint64_t)i + 1] += L.y * w;
        j->film[3 * (uint64_t)i + 2] += L.z * w;
        j->film[6 * N + i] += w;
    }
    j->states[i] = smp_drop(&smp); /* Drop of the sampler, sampler/mod.rs:168-177 / 633-640 */
}
static void *or_worker(void *arg) {
    or_job *j = (or_job *)arg;
    uint32_t H = j->sc->height, W = j->sc->width;
    for (;;) {
        uint32_t y = __sync_fetch_and_add(j->next_row, 1);
        if (y >= H) break;
        for (uint32_t x = 0; x < W; x++)
            if (or_pixel_owned(j->cfg, W, x, y)) or_render_pixel(j, x, y);
    }
    return 0;
}

/* init_pcg32_buffer_with_seed, sampler/mod.rs:148-160 */
OR_EXPORT void or_init_pcg32_buffer_with_seed(uint64_t count, uint64_t seed, uint64_t *states /* 2 u64 per entry */) {
    or_stdrng rng;
    or_stdrng_seed_from_u64(&rng, seed);
    for (uint64_t i = 0; i < count; i++) {
        or_pcg32 p = pcg_new_seq_offset(i, or_stdrng_next_u64(&rng));
        states[2 * i] = p.state; states[2 * i + 1] = p.inc;
    }
}

/* SamplerConfig::creator (sampler/mod.rs:702-718): per-pixel states of either sampler */
static void or_init_sampler_states(uint32_t sampler_type, uint64_t n, uint32_t width, uint64_t seed, or_pcg32 *states) {
    if (sampler_type == 1 || sampler_type == 2) {
        for (uint64_t i = 0; i < n; i++) { states[i].state = 0xffffffffull; states[i].inc = (i % width) | ((i / width) << 32); }
    } else {
        or_init_pcg32_buffer_with_seed(n, seed, (uint64_t *)states);
    }
}
/* film: f32[7*N] in the reference layout [rgb*N | splat*N | weight*N] (film.rs:69, 85-90), accumulated into.
 * states: Pcg32[N] in/out (pass NULL to have them initialised from cfg->sampler_seed). Runs ceil(spp/spp_per_pass)
 * passes exactly like the host loop at pt.rs:1126-1149. */
OR_EXPORT int or_pt_render(const or_scene *sc, const or_pt_config *cfg, float *film, uint64_t *states_io, uint32_t n_threads, or_stats *stats_out) {
    ((or_scene *)sc)->color = cfg->color; /* the pipeline every material evaluation of this render sees */
    uint64_t N = (uint64_t)sc->width * sc->height;
    or_pcg32 *states = (or_pcg32 *)states_io;
    int own_states = 0;
    /* Sample-range split (akr_pt_config.sample_begin / sample_count; no reference counterpart): samples [begin, begin + count)
     * of the cfg->spp samples of the whole render. Exact only for the index-based samplers, whose per-pixel state is the index of
     * the sample drawn last (Pmj02BnState.sample_index, sampler/mod.rs:451-466): it starts at begin - 1 instead of u32::MAX.
     * The independent sampler's start() continues the pixel's PCG stream (sampler/mod.rs:192-203): a range is refused. */
    const uint32_t n_samples = cfg->sample_count ? cfg->sample_count : cfg->spp;
    if (cfg->sample_count || cfg->sample_begin) {
        if (cfg->sampler_type != 1 && cfg->sampler_type != 2) return -4;
        if (cfg->sample_count == 0 || (uint64_t)cfg->sample_begin + cfg->sample_count > cfg->spp) return -4;
    }
    if (states && cfg->sample_begin) {
        /* caller-supplied states of a range that does not start at 0: they must already stand at sample begin - 1 (what the previous
         * range left behind); anything else would silently render other samples than the ones asked for */
        for (uint64_t i = 0; i < N; i++)
            if ((uint32_t)states[i].state != cfg->sample_begin - 1u) return -4;
    }
    if (!states) {
        states = (or_pcg32 *)malloc(sizeof(or_pcg32) * N);
        or_init_sampler_states(cfg->sampler_type, N, sc->width, cfg->sampler_seed, states);
        if (cfg->sample_begin)
            for (uint64_t i = 0; i < N; i++) states[i].state = (uint64_t)(cfg->sample_begin - 1u);
        own_states = 1;
    }
    if (n_threads < 1) n_threads = 1;
    if (n_threads > 256) n_threads = 256;
    or_stats total;
    memset(&total, 0, sizeof total);
    uint32_t cnt = 0;
    while (cnt < n_samples) {
        uint32_t cur = n_samples - cnt < cfg->spp_per_pass ? n_samples - cnt : cfg->spp_per_pass;
        volatile uint32_t next_row = 0;
        or_job jobs[256];
        pthread_t th[256];
        for (uint32_t t = 0; t < n_threads; t++) {
            memset(&jobs[t], 0, sizeof(or_job));
            jobs[t].sc = sc; jobs[t].cfg = cfg; jobs[t].film = film; jobs[t].states = states; jobs[t].pass_spp = cur;
            jobs[t].next_row = &next_row;
        }
        for (uint32_t t = 1; t < n_threads; t++) pthread_create(&th[t], 0, or_worker, &jobs[t]);
        or_worker(&jobs[0]);
        for (uint32_t t = 1; t < n_threads; t++) pthread_join(th[t], 0);
        for (uint32_t t = 0; t < n_threads; t++) {
            total.n_samples += jobs[t].stats.n_samples; total.n_closest += jobs[t].stats.n_closest;
            total.n_shadow += jobs[t].stats.n_shadow; total.n_shaded += jobs[t].stats.n_shaded;
            total.n_tri_tests += jobs[t].stats.n_tri_tests;
        }
        cnt += cur;
    }
    if (own_states) free(states);
    if (stats_out) *stats_out = total;
    return 0;
}

static v3 or_cs_convert_v3(v3 c, int from_aces, int to_aces) { float a[3] = {c.x, c.y, c.z}; or_cs_convert(a, from_aces, to_aces); return V3(a[0], a[1], a[2]); }

/* ---------------------------------- aov integrator, akari_integrator/src/aov.rs:57-173 -------------- */
typedef struct {
    uint32_t spp, aov, remap, filter_type; float filter_radius; uint32_t sampler_type; uint64_t sampler_seed;
    uint32_t shard_rank, shard_count, tile_w, tile_h;
    uint32_t color, _pad;
} or_aov_config; /* = akr_aov_config */
enum { OR_AOV_NS = 0, OR_AOV_NG, OR_AOV_TANGENT, OR_AOV_BITANGENT, OR_AOV_ALBEDO, OR_AOV_ROUGHNESS };
typedef struct { const or_scene *sc; const or_aov_config *cfg; or_pt_config pc; float *film; or_pcg32 *states; volatile uint32_t *next_row; uint64_t n_rays; char pad[128]; } __attribute__((aligned(128))) or_aov_job;
static v3 or_aov_remap(const or_aov_config *c, v3 v) { return c->remap ? v3add(v3scale(v, 0.5f), V3(0.5f, 0.5f, 0.5f)) : v; }
static void or_aov_pixel(or_aov_job *j, uint32_t x, uint32_t y) { /* kernel body, aov.rs:78-160 */
    const or_scene *sc = j->sc; const or_aov_config *cfg = j->cfg;
    uint32_t W = sc->width, H = sc->height, i = x + y * W;
    uint64_t N = (uint64_t)W * H;
    or_sampler smp = smp_create(&j->pc, j->states[i], cfg->spp);
    for (uint32_t s = 0; s < cfg->spp; s++) {
        smp_start(&smp);
        or_ray ray = or_generate_ray(sc, &j->pc, x, y, &smp);
        j->n_rays++;
        uint32_t inst, prim; v2 bary;
        v3 c = V3(0, 0, 0);
        if (or_trace(sc, &ray, 0, &inst, &prim, &bary, 0)) {
            or_si si = or_surface_interaction(sc, inst, prim, bary);
            if (cfg->aov == OR_AOV_NG) c = or_aov_remap(cfg, si.ng);
            else if (cfg->aov == OR_AOV_TANGENT) c = or_aov_remap(cfg, si.frame.t);
            else if (cfg->aov == OR_AOV_BITANGENT) c = or_aov_remap(cfg, si.frame.s);
            else {
                or_closure_pool pool;
                or_surface *cl = or_build_closure(&pool, sc, &si, 0);
                v3 wo = v3neg(ray.d);
                if (cfg->aov == OR_AOV_NS) c = or_aov_remap(cfg, or_surf_ns(cl));
                else if (cfg->aov == OR_AOV_ALBEDO) c = v3add(or_surf_albedo(cl, wo), or_surf_emission(cl, wo));
                else { float r = or_surf_roughness(cl, wo, smp_1d(&smp)); c = v3scale(V3(1, 1, 1), r); }
            }
        }
        if (or_isnan(c.x) || or_isnan(c.y) || or_isnan(c.z)) c = V3(0, 0, 0);
        const float w = 1.0f;
        c = v3scale(c, w);
        /* Color::Rgb(v, the space of color_repr) -> the sRGB film: aov.rs:98-124, film.rs:196-229, color.rs:262-275 */
        if (cfg->color & OR_COLOR_REPR_ACES) c = or_cs_convert_v3(c, 1, 0);
        j->film[3 * (uint64_t)i + 0] += c.x;
        j->film[3 * (uint64_t)i + 1] += c.y;
        j->film[3 * (uint64_t)i + 2] += c.z;
        j->film[6 * N + i] += w;
    }
    j->states[i] = smp_drop(&smp);
}
static void *or_aov_worker(void *arg) {
    or_aov_job *j = (or_aov_job *)arg;
    uint32_t H = j->sc->height, W = j->sc->width;
    for (;;) {
        uint32_t y = __sync_fetch_and_add(j->next_row, 1);
        if (y >= H) break;
        for (uint32_t x = 0; x < W; x++)
            if (or_pixel_owned(&j->pc, W, x, y)) or_aov_pixel(j, x, y);
    }
    return 0;
}
OR_EXPORT int or_aov_render(const or_scene *sc, const or_aov_config *cfg, float *film, uint32_t n_threads, uint64_t *n_rays_out) {
    ((or_scene *)sc)->color = cfg->color; /* the pipeline every material evaluation of this render sees */
    uint64_t N = (uint64_t)sc->width * sc->height;
    or_pcg32 *states = (or_pcg32 *)malloc(sizeof(or_pcg32) * N);
    or_init_sampler_states(cfg->sampler_type, N, sc->width, cfg->sampler_seed, states);
    if (n_threads < 1) n_threads = 1;
    if (n_threads > 256) n_threads = 256;
    volatile uint32_t next_row = 0;
    or_aov_job jobs[256];
    pthread_t th[256];
    for (uint32_t t = 0; t < n_threads; t++) {
        memset(&jobs[t], 0, sizeof(or_aov_job));
        jobs[t].sc = sc; jobs[t].cfg = cfg; jobs[t].film = film; jobs[t].states = states; jobs[t].next_row = &next_row;
        jobs[t].pc.filter_type = cfg->filter_type; jobs[t].pc.filter_radius = cfg->filter_radius;
        jobs[t].pc.sampler_type = cfg->sampler_type; jobs[t].pc.sampler_seed = cfg->sampler_seed;
        jobs[t].pc.shard_rank = cfg->shard_rank; jobs[t].pc.shard_count = cfg->shard_count; jobs[t].pc.tile_w = cfg->tile_w; jobs[t].pc.tile_h = cfg->tile_h;
    }
    for (uint32_t t = 1; t < n_threads; t++) pthread_create(&th[t], 0, or_aov_worker, &jobs[t]);
    or_aov_worker(&jobs[0]);
    for (uint32_t t = 1; t < n_threads; t++) pthread_join(th[t], 0);
    uint64_t total = 0;
    for (uint32_t t = 0; t < n_threads; t++) total += jobs[t].n_rays;
    if (n_rays_out) *n_rays_out = total;
    free(states);
    return 0;
}
OR_EXPORT uint32_t or_sizeof_aov_config(void) { return (uint32_t)sizeof(or_aov_config); }

/* ---------------------------------- gpt integrator, akari_integrator/src/gpt.rs ------------------------ */
/* Gradient-domain path tracing: per sample one base path and four offset paths through the neighbouring pixels, all on
 * the SAME random numbers, the offset paths reconnected to the base path by the reconnection shift mapping that lives
 * inside run_pt_hybrid_shift_mapping (pt.rs:329-900, the `Some(sm)` branches). */
typedef struct {
    uint32_t spp, max_depth, rr_depth, spp_per_pass;
    uint32_t use_nee, indirect_only, reconnect, stride;
    uint32_t separate_weights, reconstruction, reconstruction_iter, filter_type;
    float filter_radius; uint32_t sampler_type;
    uint64_t sampler_seed, seed;
    uint32_t color, _pad;
} or_gpt_config; /* = akr_gpt_config */
enum { OR_RECON_NONE = 0, OR_RECON_UNIFORM = 1, OR_RECON_WEIGHTED = 2 };
enum { OR_VT_INVALID = 0, OR_VT_LAST_HIT_LIGHT = 1, OR_VT_LAST_NEE = 2, OR_VT_INTERIOR = 3 }; /* pt.rs:975-980 */
typedef struct { /* ReconnectionVertex, pt.rs:981-1000 */
    v3 direct, indirect; v2 bary; v3 direct_wi; float direct_light_pdf; v3 wo; uint32_t inst_id; v3 wi; uint32_t prim_id;
    float prev_bsdf_pdf, bsdf_pdf, u_bsdf_select, dist; uint32_t depth, type;
} or_recon_vertex;
typedef struct { float min_dist, min_roughness; int is_base; or_recon_vertex *vertex; float jacobian; int success; } or_shift_mapping;

/* PathTracerBase::run_pt_hybrid_shift_mapping with need_shift_mapping = (sm != NULL), min_reconnect_depth = 1,
 * shift_mapping_no_nee = shift_mapping_no_first_nee = false, no denoising features, no cached first hit (pt.rs:329-900).
 * Returns the radiance after the indirect clamp; *base_out = base_replay_throughput. */
static v3 or_radiance_sm(const or_scene *sc, const or_gpt_config *g, or_ray ray, or_sampler *smp, or_shift_mapping *sm, v3 *base_out) {
    v3 radiance = V3(0, 0, 0), beta = V3(1, 1, 1), rrad = V3(0, 0, 0), rbeta = V3(1, 1, 1), base = V3(0, 0, 0);
    uint32_t depth = 0;
    float prev_bsdf_pdf = 0.0f, prev_roughness = 0.0f;
    v3 prev_p = V3(0, 0, 0);
    const int use_nee = g->use_nee != 0, indirect_only = g->indirect_only != 0;
    int rejected = 0;
    or_stats st_; memset(&st_, 0, sizeof st_);
    if (sm && !sm->is_base) { sm->success = 0; sm->jacobian = 0.0f; }
    /* add_radiance / mul_beta, pt.rs:134-155 */
#define ADD_RADIANCE(r) do { v3 r_ = (r); radiance = v3add(radiance, v3mul(beta, r_)); if (sm) rrad = v3add(rrad, v3mul(rbeta, r_)); } while (0)
#define MUL_BETA(r) do { v3 r_ = (r); beta = v3mul(beta, r_); if (sm) rbeta = v3mul(rbeta, r_); } while (0)
    for (;;) {
        uint32_t h_inst = 0, h_prim = 0; v2 h_bary = V2(0, 0);
        if (!or_trace(sc, &ray, 0, &h_inst, &h_prim, &h_bary, &st_)) break;
        or_si si = or_surface_interaction(sc, h_inst, h_prim, h_bary);
        v3 wo = v3neg(ray.d);
        { /* handle_surface_light, pt.rs:230-258 */
            const or_instance *inst = &sc->instances[si.inst];
            v3 direct = V3(0, 0, 0); float w = 0.0f;
            if (inst->light >= 0 && (!indirect_only || depth > 1)) {
                v3 emission = or_material_emission(sc, &si, v3neg(ray.d));
                direct = v3dot(si.ng, ray.d) < 0.0f ? emission : V3(0, 0, 0);
                if (depth == 0 || !use_nee) w = 1.0f;
                else w = or_mis_weight(prev_bsdf_pdf, or_pdf_direct(sc, &si, ray.o));
            }
            ADD_RADIANCE(v3scale(direct, w));
        }
        if (depth == 0) base = radiance;
        const float dist_prev = v3len(v3sub(prev_p, si.p));
        const int dist_crit = sm ? dist_prev >= sm->min_dist : 0, prev_rough_crit = sm ? prev_roughness >= sm->min_roughness : 0;
        if (sm) { /* the reconnection vertex is a light hit by the last segment, pt.rs:418-464 */
            const int is_last = depth == g->max_depth, can_connect = dist_crit && prev_rough_crit;
            if (depth >= 1 && can_connect) {
                if (sm->vertex->type == OR_VT_INVALID && sm->is_base && is_last) {
                    or_recon_vertex v; memset(&v, 0, sizeof v);
                    v.bary = h_bary; v.wo = wo; v.inst_id = si.inst; v.prim_id = si.prim; v.prev_bsdf_pdf = prev_bsdf_pdf;
                    v.dist = dist_prev; v.depth = depth; v.type = OR_VT_LAST_HIT_LIGHT;
                    *sm->vertex = v;
                } else if (!sm->is_base && is_last) { rejected = 1; break; }
            }
        }
        if (depth >= g->max_depth) break;
        depth += 1;
        v3 u_direct = smp_3d(smp);
        or_light_sample dl;
        memset(&dl, 0, sizeof dl);
        if (use_nee && (!indirect_only || depth > 1)) {
            dl = or_sample_direct(sc, si.p, si.ng, u_direct.x, V2(u_direct.y, u_direct.z));
            if (dl.valid) { dl.shadow_ray.ex0_inst = si.inst; dl.shadow_ray.ex0_prim = si.prim; }
            else { memset(&dl, 0, sizeof dl); }
        }
        int occluded = 1;
        v3 u_bsdf = smp_3d(smp);
        or_closure_pool pool;
        or_surface *closure = or_build_closure(&pool, sc, &si, 0);
        v3 direct = V3(0, 0, 0);
        if (dl.valid) { /* sample_surface_and_shade_direct, pt.rs:297-323 */
            v3 f; float pdf;
            or_surf_evaluate(closure, wo, dl.wi, &f, &pdf);
            float w = or_mis_weight(dl.pdf, pdf);
            direct = v3divs(v3scale(v3mul(dl.li, f), w), dl.pdf);
        }
        or_bsdf_sample bs = or_closure_sample(closure, wo, u_bsdf.x, V2(u_bsdf.y, u_bsdf.z));
        const float u_select = u_bsdf.x;
        const float roughness = or_surf_roughness(closure, wo, u_bsdf.x);
        const int rough_crit = sm ? roughness >= sm->min_roughness : 0;
        if (dl.valid) {
            occluded = or_trace(sc, &dl.shadow_ray, 1, 0, 0, 0, &st_);
            if (!occluded) ADD_RADIANCE(direct);
            if (depth == 1) base = radiance;
        }
        if (sm && !sm->is_base && sm->vertex->type != OR_VT_INVALID) { /* perform the reconnection, pt.rs:515-774 */
            const or_recon_vertex rv = *sm->vertex;
            if (depth > 1 && dist_crit && prev_rough_crit && rough_crit) { rejected = 1; break; } /* not reversible */
            if (rv.depth == depth) {
                or_si rsi = or_surface_interaction(sc, rv.inst_id, rv.prim_id, rv.bary);
                const v3 dvec = v3sub(rsi.p, si.p);
                const float dist = v3len(dvec);
                const v3 wi = v3normalize(dvec);
                if (!(dist >= sm->min_dist && rough_crit)) { rejected = 1; break; }
                or_ray vis = {or_offset_ray_origin(si.p, or_face_forward(si.ng, wi)), wi, 0.0f, dist * (1.0f - 1e-3f), si.inst, si.prim, rsi.inst, rsi.prim};
                const float cos_y2 = fabsf(v3dot(rsi.ng, wi)), cos_x2 = fabsf(v3dot(rsi.ng, rv.wo));
                if (cos_y2 == 0.0f) { rejected = 1; break; }
                if (or_trace(sc, &vis, 1, 0, 0, 0, &st_)) { rejected = 1; break; }
                v3 f1; float pdf_y1;
                or_surf_evaluate(closure, wo, wi, &f1, &pdf_y1);
                or_closure_pool pool_y;
                or_surface *cy = or_build_closure(&pool_y, sc, &rsi, 0);
                float roughness_y = 0.0f, pdf_y2 = 0.0f; v3 f2 = V3(0, 0, 0), direct_f = V3(0, 0, 0);
                if (rv.type != OR_VT_LAST_HIT_LIGHT) {
                    or_surf_evaluate(cy, v3neg(wi), rv.wi, &f2, &pdf_y2);
                    roughness_y = or_surf_roughness(cy, v3neg(wi), rv.u_bsdf_select);
                }
                if (rv.direct_wi.x != 0.0f || rv.direct_wi.y != 0.0f || rv.direct_wi.z != 0.0f) {
                    v3 f; float bsdf_pdf;
                    or_surf_evaluate(cy, v3neg(wi), rv.direct_wi, &f, &bsdf_pdf);
                    direct_f = v3scale(f, or_mis_weight(rv.direct_light_pdf, bsdf_pdf));
                }
                if (rv.type != OR_VT_LAST_HIT_LIGHT && roughness_y < sm->min_roughness) { rejected = 1; break; }
                float pdf_ratio = pdf_y1 / rv.prev_bsdf_pdf;
                if (rv.type != OR_VT_LAST_HIT_LIGHT)
                    pdf_ratio *= rv.bsdf_pdf == 0.0f ? (pdf_y2 == 0.0f ? 1.0f : 0.0f) : pdf_y2 / rv.bsdf_pdf;
                if (pdf_ratio <= 0.0f) { rejected = 1; break; }
                v3 throughput;
                {
                    const or_instance *rinst = &sc->instances[rsi.inst];
                    v3 le = V3(0, 0, 0); float light_pdf = 0.0f;
                    if (rinst->light >= 0) {
                        v3 emission = or_material_emission(sc, &rsi, v3neg(vis.d));
                        le = v3dot(rsi.ng, vis.d) < 0.0f ? emission : V3(0, 0, 0);
                        light_pdf = or_pdf_direct(sc, &rsi, si.p);
                    }
                    const float w = use_nee ? or_mis_weight(pdf_y1, light_pdf) : 1.0f;
                    v3 vertex_le = v3scale(le, w);
                    if (indirect_only && depth == 1) vertex_le = V3(0, 0, 0);
                    const v3 f_pdf = v3divs(f1, pdf_y1);
                    float cont_prob = 1.0f; /* compute_contibue_prob(vertex.depth, reconnect_beta * f_pdf), pt.rs:211-218 */
                    if (rv.depth > g->rr_depth) cont_prob = or_clamp(v3max(v3mul(rbeta, f_pdf)), 0.0f, 1.0f) * 0.95f;
                    v3 sum = v3add(vertex_le, v3mul(direct_f, rv.direct));
                    sum = v3add(sum, pdf_y2 > 0.0f ? v3divs(v3mul(f2, rv.indirect), pdf_y2) : V3(0, 0, 0));
                    throughput = v3divs(v3mul(f_pdf, sum), cont_prob);
                }
                ADD_RADIANCE(throughput);
                float jac = (pdf_ratio * fabsf(cos_y2 / cos_x2)) * or_sqr(rv.dist / dist);
                if (!or_isfinite(jac)) jac = 0.0f;
                sm->success = jac > 0.0f;
                sm->jacobian = jac;
                if (!sm->success) rejected = 1;
                break;
            }
        }
        MUL_BETA(v3divs(bs.color, bs.pdf));
        if (sm && depth > 1) { /* the base path picks its reconnection vertex, pt.rs:784-831 */
            const int can_connect = dist_crit && prev_rough_crit && rough_crit;
            if (sm->vertex->type == OR_VT_INVALID && sm->is_base && can_connect) {
                or_recon_vertex v; memset(&v, 0, sizeof v);
                if (dl.valid && !occluded) v.direct = v3divs(dl.li, dl.pdf);
                v.bary = h_bary; v.direct_wi = dl.wi; v.direct_light_pdf = dl.pdf; v.wo = wo; v.inst_id = si.inst; v.wi = bs.wi;
                v.prim_id = si.prim; v.prev_bsdf_pdf = prev_bsdf_pdf; v.bsdf_pdf = bs.pdf; v.u_bsdf_select = u_select;
                v.dist = dist_prev; v.depth = depth - 1; v.type = OR_VT_LAST_NEE;
                *sm->vertex = v;
                rbeta = V3(1, 1, 1); rrad = V3(0, 0, 0);
            }
            if (!sm->is_base && can_connect) { rejected = 1; break; }
        }
        if (bs.pdf <= 0.0f || !bs.valid || v3min(bs.color) < 0.0f) break;
        if (depth > g->rr_depth) {
            float cont_prob = or_clamp(v3max(beta), 0.0f, 1.0f) * 0.95f;
            if (smp_1d(smp) >= cont_prob) break;
            MUL_BETA(v3divs(V3(1, 1, 1), cont_prob));
        }
        prev_bsdf_pdf = bs.pdf; prev_p = si.p; prev_roughness = roughness;
        ray.o = or_offset_ray_origin(si.p, or_face_forward(si.ng, bs.wi));
        ray.d = bs.wi; ray.t_min = 0.0f; ray.t_max = 1e20f;
        ray.ex0_inst = si.inst; ray.ex0_prim = si.prim; ray.ex1_inst = OR_INVALID; ray.ex1_prim = OR_INVALID;
    }
#undef ADD_RADIANCE
#undef MUL_BETA
    {
        v3 ind = v3sub(radiance, base);
        ind = V3(or_clamp(ind.x, 0.0f, 1000.0f), or_clamp(ind.y, 0.0f, 1000.0f), or_clamp(ind.z, 0.0f, 1000.0f));
        radiance = v3add(base, ind);
    }
    if (sm) { /* pt.rs:878-899 */
        if (sm->vertex->type != OR_VT_INVALID && sm->vertex->type != OR_VT_LAST_HIT_LIGHT && sm->is_base) sm->vertex->indirect = rrad;
        if (!sm->is_base && sm->vertex->type == OR_VT_INVALID) { sm->success = !rejected; sm->jacobian = sm->success ? 1.0f : 0.0f; }
    }
    *base_out = base;
    return radiance;
}

/* GradientPathTracer::get_shifted (gpt.rs:118-142): neighbour i of a pixel, mirrored at the image border */
static uint32_t or_gpt_reflect(int32_t x, uint32_t r) { return x < 0 ? (uint32_t)(-x) : ((uint32_t)x >= r ? r - ((uint32_t)x - r) - 1 : (uint32_t)x); }
static void or_gpt_shifted(const or_gpt_config *g, uint32_t W, uint32_t H, uint32_t x, uint32_t y, uint32_t i, uint32_t *sx, uint32_t *sy) {
    static const int ox[4] = {1, 0, -1, 0}, oy[4] = {0, 1, 0, -1};
    *sx = or_gpt_reflect((int32_t)x + ox[i] * (int32_t)g->stride, W);
    *sy = or_gpt_reflect((int32_t)y + oy[i] * (int32_t)g->stride, H);
}
static v3 or_remove_nan(v3 c) { return (or_isnan(c.x) || or_isnan(c.y) || or_isnan(c.z)) ? V3(0, 0, 0) : c; }
/* what one add_splat adds: color.remove_nan() * weight, each component's NaN flushed again (film.rs:167-194) */
static v3 or_splat_value(v3 c, float weight, uint32_t color) {
    c = v3scale(or_remove_nan(c), weight);
    if (color & OR_COLOR_REPR_ACES) c = or_cs_convert_v3(c, 1, 0); /* color.to_rgb(SRgb), film.rs:178 */
    return V3(or_isnan(c.x) ? 0.0f : c.x, or_isnan(c.y) ? 0.0f : c.y, or_isnan(c.z) ? 0.0f : c.z);
}
typedef struct {
    const or_scene *sc; const or_gpt_config *g; or_pt_config pc; or_pcg32 *states; float *own, *shifted[4];
    volatile uint32_t *next_row; char pad[128];
} __attribute__((aligned(128))) or_gpt_job;
/* render_one_spp (gpt.rs:144-351) for one pixel, minus the film writes: own = what this pixel splats onto itself
 * (reconstruction none: the four primal terms summed in order; otherwise the primal sample), shifted[i] = what it splats for
 * neighbour i (none: onto the neighbour pixel; otherwise the gradient sample, sign not yet applied). */
static void or_gpt_pixel(or_gpt_job *j, uint32_t x, uint32_t y) {
    const or_scene *sc = j->sc; const or_gpt_config *g = j->g;
    const uint32_t W = sc->width, H = sc->height, pix = x + y * W;
    const or_pcg32 backup = j->states[pix];
    or_recon_vertex vertex; memset(&vertex, 0, sizeof vertex);
    or_shift_mapping sm_ = {0.03f, 0.2f, 1, &vertex, 0.0f, 0};
    or_shift_mapping *sm = g->reconnect ? &sm_ : 0;
    v3 l[5], rec[5]; float jac[5]; int ok[5];
    for (uint32_t k = 0; k < 5; k++) { /* trace(is_primary, pixel, shift_mapping), gpt.rs:153-203 */
        uint32_t qx = x, qy = y;
        if (k > 0) or_gpt_shifted(g, W, H, x, y, k - 1, &qx, &qy);
        or_sampler smp = smp_create(&j->pc, backup, g->spp); /* sampler_backup.clone_box() */
        smp_start(&smp);
        or_ray ray = or_generate_ray(sc, &j->pc, qx, qy, &smp);
        if (sm) { sm->is_base = k == 0; if (k > 0) { sm->success = 0; sm->jacobian = 0.0f; } }
        v3 base, rad = or_radiance_sm(sc, g, ray, &smp, sm, &base);
        if (sm) {
            l[k] = g->separate_weights ? base : rad;
            jac[k] = sm->jacobian; ok[k] = sm->success;
            rec[k] = v3sub(rad, l[k]);
        } else { l[k] = rad; jac[k] = 1.0f; ok[k] = 0; rec[k] = V3(0, 0, 0); }
    }
    v3 own = V3(0, 0, 0);
    if (g->reconstruction != OR_RECON_NONE) own = or_splat_value(v3add(l[0], rec[0]), 1.0f, g->color);
    for (uint32_t i = 0; i < 4; i++) {
        const uint32_t k = i + 1;
        v3 out;
        if (g->reconstruction == OR_RECON_NONE) {
            const float wp = ok[k] ? 1.0f / (1.0f + jac[k]) : 1.0f, ws = ok[k] ? 1.0f / (1.0f + jac[k]) : 0.0f;
            v3 a, b;
            if (g->separate_weights) {
                a = v3add(v3scale(l[0], 0.5f), v3scale(rec[0], wp));
                b = v3add(v3scale(l[k], 0.5f), v3scale(v3scale(rec[k], ws), jac[k]));
            } else {
                a = v3scale(l[0], wp);
                b = v3scale(v3scale(l[k], ws), jac[k]);
            }
            own = v3add(own, or_splat_value(a, 1.0f, g->color));
            out = or_splat_value(b, 1.0f, g->color);
        } else {
            v3 grad;
            if (sm) {
                if (g->separate_weights) {
                    v3 gr = ok[k] ? v3divs(v3sub(v3scale(rec[k], jac[k]), rec[0]), 1.0f + jac[k]) : v3sub(V3(0, 0, 0), rec[0]);
                    grad = v3add(v3scale(v3sub(l[k], l[0]), 0.5f), gr);
                } else {
                    grad = ok[k] ? v3divs(v3sub(v3scale(l[k], jac[k]), l[0]), 1.0f + jac[k]) : v3sub(V3(0, 0, 0), l[0]);
                }
            } else grad = v3scale(v3sub(l[k], l[0]), 0.5f);
            out = or_splat_value(grad, i < 2 ? 1.0f : -1.0f, g->color);
        }
        j->shifted[i][3 * (uint64_t)pix + 0] = out.x; j->shifted[i][3 * (uint64_t)pix + 1] = out.y; j->shifted[i][3 * (uint64_t)pix + 2] = out.z;
    }
    j->own[3 * (uint64_t)pix + 0] = own.x; j->own[3 * (uint64_t)pix + 1] = own.y; j->own[3 * (uint64_t)pix + 2] = own.z;
    or_sampler b = smp_create(&j->pc, backup, g->spp); /* sampler_backup.start(); its Drop stores the state (dim = 0) */
    smp_start(&b);
    j->states[pix] = smp_drop(&b);
}
static void *or_gpt_worker(void *arg) {
    or_gpt_job *j = (or_gpt_job *)arg;
    for (;;) {
        uint32_t y = __sync_fetch_and_add(j->next_row, 1);
        if (y >= j->sc->height) break;
        for (uint32_t x = 0; x < j->sc->width; x++) or_gpt_pixel(j, x, y);
    }
    return 0;
}
/* The pixels whose neighbour i is pixel c' along one axis of size r: the inverse of or_gpt_reflect(c + o). The reference
 * lets float atomics decide the summation order of a pixel's splats; both implementations here fix it: own terms first, then
 * neighbours i = 0..3, each in the order [unreflected, mirrored at 0, mirrored at r]. */
static int or_gpt_sources(int32_t cp, int32_t o, uint32_t r, uint32_t out[3]) {
    int n = 0;
    const int64_t cand[3] = {(int64_t)cp - o, -(int64_t)cp - o, 2 * (int64_t)r - 1 - cp - o};
    for (int k = 0; k < 3; k++) {
        const int64_t c = cand[k];
        if (c < 0 || c >= (int64_t)r) continue;
        const int64_t q = c + o;
        const int cls = q < 0 ? 1 : (q >= (int64_t)r ? 2 : 0);
        if (cls == k) out[n++] = (uint32_t)c;
    }
    return n;
}
/* film: f32[7N], splat region accumulated into (reconstruction none: += v / 4 per sample, resolve with splat_scale = 1/spp;
 * otherwise written with the reconstructed image, splat_scale = 1). aux (optional, reconstruction != none):
 * [primal 3N | Gx 3(W+1)(H+1) | Gy 3(W+1)(H+1)] = the accumulated sums of gpt.rs:441-455 (divide by spp for the mean). */
OR_EXPORT int or_gpt_render(const or_scene *sc, const or_gpt_config *g, float *film, float *aux, uint32_t n_threads) {
    if (sc->env) return -5; /* no environment in gpt (refused) */
    if (sc->n_punct || sc->lens_radius > 0.0f) return -5; /* nor a punctual light (4.14) or a lens (4.9) */
    if (sc->proj.type != OR_PROJECTION_PERSPECTIVE) return -5; /* nor a projection (4.17): this integrator's rays are the pinhole's */
    ((or_scene *)sc)->color = g->color; /* the pipeline every material evaluation of this render sees */
    const uint32_t W = sc->width, H = sc->height;
    const uint64_t N = (uint64_t)W * H, NG = (uint64_t)(W + 1) * (H + 1);
    if (g->stride < 1 || g->stride >= W || g->stride >= H) return -1;
    if (g->reconstruction == OR_RECON_NONE && !g->reconnect) return -1; /* shift_mapping.unwrap() panics, gpt.rs:276 */
    if (g->sampler_type != 0) return -1;                                /* Pmj02BnSampler::clone_box is todo!() */
    or_pcg32 *states = (or_pcg32 *)malloc(sizeof(or_pcg32) * N);
    or_init_sampler_states(0, N, W, g->sampler_seed, states);
    float *own = (float *)calloc(3 * N, 4), *sh[4];
    for (int i = 0; i < 4; i++) sh[i] = (float *)calloc(3 * N, 4);
    float *acc_p = 0, *acc_gx = 0, *acc_gy = 0, *sqr_p = 0, *sqr_gx = 0, *sqr_gy = 0;
    if (g->reconstruction != OR_RECON_NONE) {
        acc_p = (float *)calloc(3 * N, 4); sqr_p = (float *)calloc(3 * N, 4);
        acc_gx = (float *)calloc(3 * NG, 4); acc_gy = (float *)calloc(3 * NG, 4); sqr_gx = (float *)calloc(3 * NG, 4); sqr_gy = (float *)calloc(3 * NG, 4);
    }
    if (n_threads < 1) n_threads = 1;
    if (n_threads > 256) n_threads = 256;
    static const int ox[4] = {1, 0, -1, 0}, oy[4] = {0, 1, 0, -1};
    for (uint32_t s = 0; s < g->spp; s++) {
        volatile uint32_t next_row = 0;
        or_gpt_job jobs[256];
        pthread_t th[256];
        for (uint32_t t = 0; t < n_threads; t++) {
            memset(&jobs[t], 0, sizeof(or_gpt_job));
            jobs[t].sc = sc; jobs[t].g = g; jobs[t].states = states; jobs[t].own = own; jobs[t].next_row = &next_row;
            for (int i = 0; i < 4; i++) jobs[t].shifted[i] = sh[i];
            jobs[t].pc.filter_type = g->filter_type; jobs[t].pc.filter_radius = g->filter_radius;
            jobs[t].pc.sampler_type = 0; jobs[t].pc.sampler_seed = g->sampler_seed;
        }
        for (uint32_t t = 1; t < n_threads; t++) pthread_create(&th[t], 0, or_gpt_worker, &jobs[t]);
        or_gpt_worker(&jobs[0]);
        for (uint32_t t = 1; t < n_threads; t++) pthread_join(th[t], 0);
        /* update_kernel, gpt.rs:424-461 */
        for (uint32_t y = 0; y < H; y++) for (uint32_t x = 0; x < W; x++) {
            const uint64_t q = x + (uint64_t)y * W, gq = x + (uint64_t)y * (W + 1);
            for (int c = 0; c < 3; c++) {
                if (g->reconstruction == OR_RECON_NONE) {
                    float v = 0.0f;
                    v += own[3 * q + c];
                    for (int i = 0; i < 4; i++) {
                        uint32_t src[3];
                        if (ox[i]) { int n = or_gpt_sources((int32_t)x, ox[i] * (int32_t)g->stride, W, src); for (int k = 0; k < n; k++) v += sh[i][3 * (src[k] + (uint64_t)y * W) + c]; }
                        else { int n = or_gpt_sources((int32_t)y, oy[i] * (int32_t)g->stride, H, src); for (int k = 0; k < n; k++) v += sh[i][3 * (x + (uint64_t)src[k] * W) + c]; }
                    }
                    film[3 * N + 3 * q + c] += v * 0.25f;
                } else {
                    float v = 0.0f, gx = 0.0f, gy = 0.0f;
                    v += own[3 * q + c];
                    if (x >= 1) gx += sh[0][3 * (q - 1) + c];
                    gx += sh[2][3 * q + c];
                    if (y >= 1) gy += sh[1][3 * (q - W) + c];
                    gy += sh[3][3 * q + c];
                    acc_p[3 * q + c] += v; acc_gx[3 * gq + c] += gx; acc_gy[3 * gq + c] += gy;
                    sqr_p[3 * q + c] += v * v; sqr_gx[3 * gq + c] += gx * gx; sqr_gy[3 * gq + c] += gy * gy;
                }
            }
        }
    }
    if (g->reconstruction != OR_RECON_NONE) { /* gpt.rs:495-606 */
        const float spp = (float)g->spp;
        float *old = (float *)malloc(3 * N * 4), *cur = film + 3 * N;
        for (uint64_t k = 0; k < 3 * N; k++) old[k] = acc_p[k] / spp;
        float *prefix = (float *)malloc(4 * (g->reconstruction_iter + 1));
        {
            const float eps = 0.01f;
            prefix[0] = 1.0f;
            for (uint32_t i = 1; i < g->reconstruction_iter; i++) {
                float p2 = 1.0f; for (uint32_t k = 0; k < i - 1; k++) p2 *= 0.5f; /* 0.5f32.powi(i - 1) */
                prefix[i] = prefix[i - 1] * (1.0f / ((eps + 1.0f) + 4.0f * p2));
            }
        }
        for (uint32_t it = 0; it < g->reconstruction_iter; it++) {
            for (uint32_t y = 0; y < H; y++) for (uint32_t x = 0; x < W; x++) for (int c = 0; c < 3; c++) {
                const uint64_t q = x + (uint64_t)y * W;
                const float primal = old[3 * q + c];
                const float primal2 = sqr_p[3 * q + c] / spp;
                const float primal_var = or_max(primal2 - or_sqr(acc_p[3 * q + c] / spp), 1e-6f) / spp;
                const float pw = g->reconstruction == OR_RECON_UNIFORM ? 1.0f : 1.0f / (primal_var * prefix[it]);
                float v = 0.0f, sum_w = 0.0f;
                v += primal * pw; sum_w += pw;
                for (uint32_t i = 0; i < 4; i++) {
                    const int is_x = (i & 1u) == 0; const float sign = i < 2 ? 1.0f : -1.0f;
                    const uint32_t gx_ = x + (i == 0 ? 1u : 0u), gy_ = y + (i == 1 ? 1u : 0u);
                    uint32_t sx, sy; or_gpt_shifted(g, W, H, x, y, i, &sx, &sy);
                    const uint64_t gi = 3 * (gx_ + (uint64_t)gy_ * (W + 1)) + c;
                    const float grad = (is_x ? acc_gx[gi] : acc_gy[gi]) / spp;
                    const float grad2 = (is_x ? sqr_gx[gi] : sqr_gy[gi]) / spp;
                    const float grad_var = or_max((grad2 - or_sqr(grad)) / spp, 1e-6f);
                    const float nb = old[3 * (sx + (uint64_t)sy * W) + c];
                    const float var = primal_var + grad_var;
                    const float w = g->reconstruction == OR_RECON_UNIFORM ? 1.0f : 1.0f / var;
                    v += (nb - sign * grad) * w; sum_w += w;
                }
                cur[3 * q + c] = v / sum_w;
            }
            memcpy(old, cur, 3 * N * 4);
        }
        if (aux) { memcpy(aux, acc_p, 3 * N * 4); memcpy(aux + 3 * N, acc_gx, 3 * NG * 4); memcpy(aux + 3 * N + 3 * NG, acc_gy, 3 * NG * 4); }
        free(old); free(prefix);
    }
    free(states); free(own); for (int i = 0; i < 4; i++) free(sh[i]);
    free(acc_p); free(acc_gx); free(acc_gy); free(sqr_p); free(sqr_gx); free(sqr_gy);
    return 0;
}
OR_EXPORT uint32_t or_sizeof_gpt_config(void) { return (uint32_t)sizeof(or_gpt_config); }

/* ---------------------------------- mcmc_opt integrator, akari_integrator/src/mcmc_opt.rs ------------ */
/* Primary-sample-space Metropolis light transport (Kelemen et al.) with lazily mutated samples: n_chains Markov chains, each
 * a vector of `sample_dimension` primary samples that the path tracer reads instead of random numbers. */
typedef struct {
    uint32_t spp, max_depth, rr_depth, spp_per_pass;
    uint32_t use_nee, mcmc_depth /* 0xffffffff = None -> max_depth */, n_chains, n_bootstrap;
    int32_t direct_spp; uint32_t exponential_mutation;
    float small_sigma, large_step_prob, image_mutation_prob, image_mutation_size /* <= 0 = None */;
    uint32_t adaptive, wis;
    uint64_t seed;
    uint32_t filter_type; float filter_radius; uint32_t sampler_type, color;
    uint64_t sampler_seed;
} or_mcmc_config; /* = akr_mcmc_config */
typedef struct { float cur, backup; uint32_t last_modified, modified_backup; } or_pss; /* PssSample, mcmc_opt.rs:21-26 */
typedef struct { /* MarkovState, mcmc_opt.rs:41-51 */
    uint32_t cur_pixel[2], chain_id; float cur_f, b; uint32_t b_cnt, n_accepted, n_mutations, cur_iter, last_large_iter;
} or_markov_state;
typedef struct or_mcmc_smp {
    or_pss *samples;              /* this chain's sample_dimension entries */
    uint32_t cur_dim, mcmc_dim;
    int mutate;                   /* Some(mutator) */
    int is_large_step, is_image_mutation; uint32_t last_large_iter, cur_iter; float res_x, res_y;
    const or_mcmc_config *cfg;
} or_mcmc_smp;
static float or_erf_inv(float x) { /* util/mod.rs:149-186 */
    float cx = or_clamp(x, -0.99999f, 0.99999f);
    float w = -or_logf((1.0f - cx) * (1.0f + cx));
    float p;
    if (w < 0.5f) {
        w -= 2.5f;
        p = 2.81022636e-08f; p = 3.43273939e-07f + p * w; p = -3.5233877e-06f + p * w; p = -4.39150654e-06f + p * w;
        p = 0.00021858087f + p * w; p = -0.00125372503f + p * w; p = -0.00417768164f + p * w; p = 0.246640727f + p * w; p = 1.50140941f + p * w;
    } else {
        w = sqrtf(w) - 3.0f;
        p = -0.000200214257f; p = 0.000100950558f + p * w; p = 0.00134934322f + p * w; p = -0.00367342844f + p * w;
        p = 0.00573950773f + p * w; p = -0.0076224613f + p * w; p = 0.00943887047f + p * w; p = 1.00167406f + p * w; p = 2.83297682f + p * w;
    }
    return p * cx;
}
static float or_kelemen_mutate(float cur, float u) { /* KELEMEN_MUTATE, sampler/mcmc.rs:111-134; sizes 1/1024 .. 1/64 */
    const float size_high = 1.0f / 64.0f, log_ratio = -2.7725887f; /* -(size_high / size_low).ln() = -ln 16 */
    int add = u < 0.5f;
    u = add ? u * 2.0f : (u - 0.5f) * 2.0f;
    float dv = size_high * or_expf(log_ratio * u);
    if (add) { float n = cur + dv; return n > 1.0f ? n - 1.0f : n; }
    float n = cur - dv;
    return n < 0.0f ? n + 1.0f : n;
}
static or_pss or_mutate_one(or_mcmc_smp *m, uint32_t i, or_pcg32 *rng) { /* Mutator::mutate_one, mcmc_opt.rs:131-226 */
    const or_mcmc_config *c = m->cfg;
    or_pss sp = m->samples[i];
    float u = pcg_next_1d(rng);
    if (sp.last_modified < m->last_large_iter) { sp.cur = pcg_next_1d(rng); sp.last_modified = m->last_large_iter; }
    sp.backup = sp.cur; sp.modified_backup = sp.last_modified;
    if (m->is_large_step) sp.cur = u;
    else {
        const int has_img = c->image_mutation_size > 0.0f;
        const int under_image = has_img && m->is_image_mutation;
        const int should_mutate = !under_image || i < 2;
        const uint32_t target_iter = should_mutate ? m->cur_iter : m->cur_iter - 1;
        const uint32_t n_small = target_iter - sp.last_modified;
        if (c->exponential_mutation) {
            float x = sp.cur;
            for (uint32_t k = 0; k < n_small; k++) {
                float v = pcg_next_1d(rng);
                if (v < 1.0f - c->image_mutation_prob) x = or_kelemen_mutate(x, v / (1.0f - c->image_mutation_prob));
            }
            sp.cur = x;
        } else if (n_small > 0) {
            float dv = sqrtf(2.0f) * or_erf_inv(2.0f * u - 1.0f); /* sample_gaussian(u), sampling.rs:46-48 */
            float n = sp.cur + (dv * c->small_sigma) * sqrtf((1.0f - c->image_mutation_prob) * (float)n_small);
            n = n - floorf(n);
            sp.cur = or_isfinite(n) ? n : 0.0f;
        }
        if (has_img && m->is_image_mutation && i < 2) { /* mutate_image_space_single, sampler/mcmc.rs:180-200 */
            float v = pcg_next_1d(rng);
            int add = v < 0.5f;
            v = add ? v * 2.0f : (v - 0.5f) * 2.0f;
            float off = v * c->image_mutation_size;
            off = add ? off : -off;
            float n = sp.cur + off / (i == 0 ? m->res_x : m->res_y);
            sp.cur = n - floorf(n);
        }
    }
    sp.last_modified = m->cur_iter;
    m->samples[i] = sp;
    return sp;
}
static float or_mcmc_next_1d(or_sampler *s) { /* LazyMcmcSampler::next_1d, mcmc_opt.rs:88-103 */
    or_mcmc_smp *m = s->mc;
    if (m->cur_dim < m->mcmc_dim) {
        float r = m->mutate ? or_mutate_one(m, m->cur_dim, &s->pcg).cur : m->samples[m->cur_dim].cur;
        m->cur_dim += 1;
        return r;
    }
    m->cur_dim += 1;
    return pcg_next_1d(&s->pcg);
}
static uint32_t or_mcmc_dim(const or_mcmc_config *c) { /* sample_dimension, mcmc_opt.rs:230-232 */
    uint32_t d = c->mcmc_depth == 0xffffffffu ? c->max_depth : c->mcmc_depth;
    return 4 + 1 + (1 + d) * (3 + 3 + 1);
}
typedef struct { uint32_t px, py; v3 l; float f; uint32_t dim; } or_mcmc_eval;
/* McmcOpt::evaluate, mcmc_opt.rs:253-305. rng = the independent sampler underneath; samples = the chain's primary samples */
static or_mcmc_eval or_mcmc_evaluate(const or_scene *sc, const or_mcmc_config *c, const or_gpt_config *pt, const or_pt_config *pc, or_pss *samples,
                                     or_pcg32 *rng, or_mcmc_smp *mut /* NULL or a filled-in mutator */, int is_bootstrap) {
    or_mcmc_smp m;
    if (mut) m = *mut; else memset(&m, 0, sizeof m);
    m.samples = samples; m.cur_dim = 0; m.mcmc_dim = is_bootstrap ? 0 : or_mcmc_dim(c); m.mutate = mut != 0; m.cfg = c;
    or_sampler smp; memset(&smp, 0, sizeof smp);
    smp.pcg = *rng; smp.mc = &m;
    v2 u = smp_2d(&smp);
    int32_t ix = (int32_t)(u.x * (float)sc->width), iy = (int32_t)(u.y * (float)sc->height);
    ix = ix < 0 ? 0 : (ix > (int32_t)sc->width - 1 ? (int32_t)sc->width - 1 : ix);
    iy = iy < 0 ? 0 : (iy > (int32_t)sc->height - 1 ? (int32_t)sc->height - 1 : iy);
    or_ray ray = or_generate_ray(sc, pc, (uint32_t)ix, (uint32_t)iy, &smp);
    v3 base;
    v3 l = or_radiance_sm(sc, pt, ray, &smp, 0, &base); /* PathTracer::radiance = run_megakernel, shift_mapping None */
    l = v3scale(l, 1.0f);                                /* * ray_w */
    or_mcmc_eval e = {(uint32_t)ix, (uint32_t)iy, l, or_clamp(v3max(l), 0.0f, 1e5f), m.cur_dim}; /* scalar_contribution */
    *rng = smp.pcg;
    return e;
}
/* out: film (7N floats; the direct pass fills rgb + weight, the chains the splat channels), result[4] = {b (normalisation),
 * acceptance rate, splat scale as f32 bits, contribution as f32 bits} (doubles / reinterpreted), chain_states (10 u32 each). */
OR_EXPORT int or_mcmc_render(const or_scene *sc, const or_mcmc_config *c, float *film, double *result, uint32_t *chain_states, uint32_t n_threads) {
    if (sc->env) return -5; /* no environment in mcmc_opt (refused) */
    if (sc->n_punct || sc->lens_radius > 0.0f) return -5; /* nor a punctual light (4.14) or a lens (4.9) */
    if (sc->proj.type != OR_PROJECTION_PERSPECTIVE) return -5; /* nor a projection (4.17): this integrator's rays are the pinhole's */
    ((or_scene *)sc)->color = c->color; /* the pipeline every material evaluation of this render sees */
    const uint32_t W = sc->width, H = sc->height;
    const uint64_t N = (uint64_t)W * H;
    if (c->n_chains == 0 || c->n_bootstrap == 0 || c->sampler_type > 1) return -1;
    if (c->direct_spp > 0) { /* mcmc_opt.rs:704-729 */
        or_pt_config d; memset(&d, 0, sizeof d);
        d.spp = (uint32_t)c->direct_spp; d.max_depth = 1; d.rr_depth = 1; d.spp_per_pass = c->spp_per_pass; d.use_nee = c->use_nee;
        d.debug_depth = -1; d.filter_type = c->filter_type; d.filter_radius = c->filter_radius; d.sampler_type = c->sampler_type;
        d.sampler_seed = c->sampler_seed; d.shard_count = 1; d.color = c->color;
        if (or_pt_render(sc, &d, film, 0, n_threads, 0) != 0) return -1;
    }
    or_gpt_config pt; memset(&pt, 0, sizeof pt); /* the PathTracer inside McmcOpt::new, mcmc_opt.rs:233-252 */
    pt.max_depth = c->max_depth; pt.rr_depth = c->rr_depth; pt.use_nee = c->use_nee; pt.indirect_only = c->direct_spp >= 0;
    or_pt_config pc; memset(&pc, 0, sizeof pc);
    pc.filter_type = c->filter_type; pc.filter_radius = c->filter_radius;
    const uint32_t dim = or_mcmc_dim(c);
    /* bootstrap, mcmc_opt.rs:310-398 */
    or_pcg32 *seeds = (or_pcg32 *)malloc(sizeof(or_pcg32) * c->n_bootstrap);
    or_init_pcg32_buffer_with_seed(c->n_bootstrap, c->seed, (uint64_t *)seeds);
    float *fs = (float *)malloc(4 * (size_t)c->n_bootstrap);
    for (uint32_t i = 0; i < c->n_bootstrap; i++) {
        or_pcg32 rng = seeds[i];
        fs[i] = or_mcmc_evaluate(sc, c, &pt, &pc, 0, &rng, 0, 1).f;
    }
    /* resample_with_f64, util/distribution.rs:92-115 (the reference sums with rayon; here in index order) */
    double sum = 0.0;
    for (uint32_t i = 0; i < c->n_bootstrap; i++) sum += (double)fs[i];
    if (!(sum > 0.0)) { free(seeds); free(fs); return -2; } /* "Bootstrap failed" */
    double *cdf = (double *)malloc(8 * (size_t)c->n_bootstrap);
    for (uint32_t i = 0; i < c->n_bootstrap; i++) { double p = (double)fs[i] / sum; cdf[i] = i == 0 ? p : cdf[i - 1] + p; }
    uint32_t *resampled = (uint32_t *)malloc(4 * (size_t)c->n_chains);
    {
        or_stdrng rng; or_stdrng_seed_from_u64(&rng, 0);
        for (uint32_t k = 0; k < c->n_chains; k++) {
            double u = (double)(or_stdrng_next_u64(&rng) >> 11) * (1.0 / 9007199254740992.0); /* Standard f64: 53 bits */
            uint32_t lo = 0, hi = c->n_bootstrap; /* partition_point(|x| u >= *x) */
            while (lo < hi) { uint32_t mid = lo + (hi - lo) / 2; if (u >= cdf[mid]) lo = mid + 1; else hi = mid; }
            resampled[k] = lo < c->n_bootstrap - 1 ? lo : c->n_bootstrap - 1;
        }
    }
    or_pss *samples = (or_pss *)calloc((size_t)dim * c->n_chains, sizeof(or_pss));
    or_markov_state *states = (or_markov_state *)calloc(c->n_chains, sizeof(or_markov_state));
    v3 *cur_colors = (v3 *)calloc(c->n_chains, sizeof(v3));
    for (uint32_t i = 0; i < c->n_chains; i++) { /* mcmc_opt.rs:356-386 */
        or_pcg32 rng = seeds[resampled[i]];
        or_pss *sp = samples + (size_t)i * dim;
        for (uint32_t j = 0; j < dim; j++) { sp[j].cur = pcg_next_1d(&rng); sp[j].backup = 0.0f; sp[j].last_modified = 0; sp[j].modified_backup = 0; }
        or_mcmc_eval e = or_mcmc_evaluate(sc, c, &pt, &pc, sp, &rng, 0, 0);
        cur_colors[i] = e.l;
        or_markov_state st = {{e.px, e.py}, i, e.f, 0.0f, 0, 0, 0, 0, 0};
        states[i] = st;
    }
    or_pcg32 *rngs = (or_pcg32 *)malloc(sizeof(or_pcg32) * c->n_chains);
    or_init_pcg32_buffer_with_seed(c->n_chains, c->seed, (uint64_t *)rngs);
    /* render_loop, mcmc_opt.rs:554-683 */
    const uint64_t npixels = N;
    float contribution;
    {
        uint64_t n_mut = npixels * (uint64_t)c->spp, per = n_mut / c->n_chains; if (per < 1) per = 1;
        contribution = (float)((double)n_mut / ((double)per * (double)c->n_chains));
    }
    uint32_t cnt = 0;
    while (cnt < c->spp) {
        uint32_t cur_pass = c->spp - cnt < c->spp_per_pass ? c->spp - cnt : c->spp_per_pass;
        uint64_t per = npixels * (uint64_t)cur_pass / c->n_chains; if (per < 1) per = 1;
        if (per > 0xffffffffull) return -3;
        for (uint32_t i = 0; i < c->n_chains; i++) { /* advance_chain, mcmc_opt.rs:505-552; chains in index order */
            or_pcg32 rng = rngs[i];
            or_markov_state st = states[i];
            v3 cur_color = cur_colors[i];
            or_pss *sp = samples + (size_t)i * dim;
            for (uint64_t it = 0; it < per; it++) {
                if (st.cur_iter == 0xffffffffu - 1) { /* about to overflow */
                    for (uint32_t j = 0; j < dim; j++) { if (sp[j].last_modified < st.last_large_iter) sp[j].cur = pcg_next_1d(&rng); sp[j].last_modified = 0; }
                    st.cur_iter -= st.last_large_iter; st.last_large_iter = 0;
                }
                /* mutate_chain, mcmc_opt.rs:409-503 */
                st.cur_iter += 1;
                or_mcmc_smp mut; memset(&mut, 0, sizeof mut);
                float u = pcg_next_1d(&rng);
                mut.is_large_step = u < c->large_step_prob;
                mut.is_image_mutation = pcg_next_1d(&rng) < c->image_mutation_prob;
                mut.last_large_iter = st.last_large_iter; mut.cur_iter = st.cur_iter; mut.res_x = (float)W; mut.res_y = (float)H;
                or_mcmc_eval e = or_mcmc_evaluate(sc, c, &pt, &pc, sp, &rng, &mut, 0);
                const float proposal_f = e.f;
                if (mut.is_large_step && st.b_cnt < 1024u * 1024u) { st.b += proposal_f; st.b_cnt += 1; }
                const float cur_f = st.cur_f;
                float accept = 0.0f;
                if (or_isfinite(proposal_f)) accept = (cur_f == 0.0f || !or_isfinite(cur_f)) ? 1.0f : or_clamp(proposal_f / cur_f, 0.0f, 1.0f);
                {
                    v3 a = or_splat_value(v3divs(e.l, proposal_f), accept * contribution, c->color);
                    float *d = film + 3 * N + 3 * ((uint64_t)e.px + (uint64_t)e.py * W);
                    d[0] += a.x; d[1] += a.y; d[2] += a.z;
                    v3 b = or_splat_value(v3divs(cur_color, cur_f), (1.0f - accept) * contribution, c->color);
                    d = film + 3 * N + 3 * ((uint64_t)st.cur_pixel[0] + (uint64_t)st.cur_pixel[1] * W);
                    d[0] += b.x; d[1] += b.y; d[2] += b.z;
                }
                if (pcg_next_1d(&rng) < accept) {
                    st.cur_f = proposal_f; cur_color = e.l; st.cur_pixel[0] = e.px; st.cur_pixel[1] = e.py;
                    if (!mut.is_large_step) st.n_accepted += 1; else st.last_large_iter = st.cur_iter;
                } else {
                    st.cur_iter -= 1;
                    uint32_t nd = e.dim < dim ? e.dim : dim;
                    for (uint32_t j = 0; j < nd; j++) { sp[j].cur = sp[j].backup; sp[j].last_modified = sp[j].modified_backup; }
                }
                if (!mut.is_large_step) st.n_mutations += 1;
            }
            cur_colors[i] = cur_color; rngs[i] = rng; states[i] = st;
        }
        cnt += cur_pass;
    }
    { /* reconstruct, mcmc_opt.rs:587-611 */
        double b = sum; uint64_t b_cnt = c->n_bootstrap, acc = 0, mut = 0;
        for (uint32_t i = 0; i < c->n_chains; i++) { b += (double)states[i].b; b_cnt += states[i].b_cnt; acc += states[i].n_accepted; mut += states[i].n_mutations; }
        b = b / (double)b_cnt;
        if (result) {
            result[0] = b; result[1] = (double)acc / (double)mut;
            float scale = (float)b / (float)c->spp;
            result[2] = (double)scale; result[3] = (double)contribution;
        }
    }
    if (chain_states) memcpy(chain_states, states, sizeof(or_markov_state) * c->n_chains);
    free(seeds); free(fs); free(cdf); free(resampled); free(samples); free(states); free(cur_colors); free(rngs);
    return 0;
}
OR_EXPORT uint32_t or_sizeof_mcmc_config(void) { return (uint32_t)sizeof(or_mcmc_config); }

/* number of triangles whose plane row was taken from their even neighbour (or_share_plane_row) */
OR_EXPORT uint32_t or_scene_shared_plane_rows(const or_scene *sc) {
    uint32_t n = 0;
    for (uint32_t k = 1; k < sc->n_tris; k++)
        if (sc->tri_inst[k] == sc->tri_inst[k - 1] && (sc->tri_prim[k] & 1u) && memcmp(sc->woop + 12 * k + 8, sc->woop + 12 * (k - 1) + 8, 16) == 0) n++;
    return n;
}

/* Film resolve, film.rs:120-148 with hdr = true: rgb / (w == 0 ? 1 : w) + splat * splat_scale */
OR_EXPORT void or_film_resolve_scaled(const float *film, uint32_t width, uint32_t height, float splat_scale, float *rgb_out) {
    uint64_t N = (uint64_t)width * height;
    for (uint64_t i = 0; i < N; i++) {
        float w = film[6 * N + i];
        float inv = w == 0.0f ? 1.0f : w;
        for (int c = 0; c < 3; c++) rgb_out[3 * i + c] = film[3 * i + c] / inv + film[3 * N + 3 * i + c] * splat_scale;
    }
}
OR_EXPORT void or_film_resolve(const float *film, uint32_t width, uint32_t height, float *rgb_out) { or_film_resolve_scaled(film, width, height, 1.0f, rgb_out); }

/* ---------------------------------- precomputed table, precompute.rs:56-94,133-145 ---------------- */
static float or_precompute_ggx_dielectric_sample(float roughness, float mu, float ior, or_pcg32 *rng) {
    or_closure_pool pool;
    pool.count = 0;
    or_surface *bsdf = mk_refl(&pool, V3(1, 1, 1), OR_FR_DIELECTRIC, ior, roughness);
    or_surface *c = pool_new(&pool, OR_S_CLOSURE);
    c->a = bsdf; c->frame = or_frame_from_n(V3(0, 0, 1)); c->ng = V3(0, 0, 1);
    v3 wo = V3(sqrtf(1.0f - or_sqr(mu)), 0.0f, mu);
    float u0 = pcg_next_1d(rng), u1 = pcg_next_1d(rng), u2 = pcg_next_1d(rng);
    or_bsdf_sample s = or_closure_sample(c, wo, u0, V2(u1, u2));
    if (s.valid && s.pdf > 0.0f) return s.color.x / s.pdf;
    return 0.0f;
}
/* One table entry (tx,ty,tz) with `samples` samples (reference: 1<<20); `seed_u64` = that entry's value of the
 * StdRng(0) stream (svm/surface/mod.rs:1336-1356). */
OR_EXPORT float or_ggx_dielectric_table_entry(uint32_t tx, uint32_t ty, uint32_t tz, uint32_t samples) {
    const uint32_t dim = 16;
    uint32_t global_id = tx + ty * dim + tz * (dim * dim);
    or_stdrng srng;
    or_stdrng_seed_from_u64(&srng, 0);
    uint64_t seed = 0;
    for (uint32_t i = 0; i <= global_id; i++) seed = or_stdrng_next_u64(&srng);
    or_pcg32 rng = pcg_new_seq_offset(global_id, seed);
    float fx = or_clamp((float)tx / ((float)dim - 1.0f), 1e-4f, 0.9999f);
    float fy = or_clamp((float)ty / ((float)dim - 1.0f), 1e-4f, 0.9999f);
    float fz = or_clamp((float)tz / ((float)dim - 1.0f), 1e-4f, 0.9999f);
    float ior = or_ior_from_f0(or_sqr(or_sqr(fz))); /* ior_parametrization, svm/surface/mod.rs:1100-1103 */
    float sum = 0.0f;
    for (uint32_t s = 0; s < samples; s++) sum += or_precompute_ggx_dielectric_sample(fx, fy, ior, &rng);
    return sum / (float)samples;
}

/* ---------------------------------- small exports for unit / known-answer tests ------------------- */
OR_EXPORT uint32_t or_kat_pcg32(uint64_t state, uint64_t inc, uint32_t n, uint32_t *out) {
    or_pcg32 p = {state, inc};
    for (uint32_t i = 0; i < n; i++) out[i] = pcg_gen_u32(&p);
    return 0;
}
OR_EXPORT void or_kat_pcg32_advance(uint64_t *state, uint64_t inc, int64_t delta) { or_pcg32 p = {*state, inc}; pcg_advance(&p, delta); *state = p.state; }
OR_EXPORT void or_kat_pcg32_new_seq(uint64_t seq, uint64_t *state, uint64_t *inc) { or_pcg32 p = pcg_new_seq(seq); *state = p.state; *inc = p.inc; }
OR_EXPORT float or_kat_next_1d(uint64_t *state, uint64_t inc) { or_pcg32 p = {*state, inc}; float f = pcg_next_1d(&p); *state = p.state; return f; }
OR_EXPORT void or_kat_chacha_block(const uint32_t *key, uint64_t counter, uint64_t stream, int rounds, uint32_t *out) { or_chacha_block(key, counter, stream, rounds, out); }
OR_EXPORT void or_kat_stdrng_u64(uint64_t seed, uint32_t n, uint64_t *out) { or_stdrng r; or_stdrng_seed_from_u64(&r, seed); for (uint32_t i = 0; i < n; i++) out[i] = or_stdrng_next_u64(&r); }
OR_EXPORT uint32_t or_kat_xxhash32_4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return or_xxhash32_4(a, b, c, d); }
OR_EXPORT uint64_t or_kat_mix_bits(uint64_t v) { return or_mix_bits(v); }
OR_EXPORT void or_kat_sincos(float x, float *s, float *c) { or_sincosf(x, s, c); }
OR_EXPORT float or_kat_log(float x) { return or_logf(x); }
OR_EXPORT float or_kat_exp(float x) { return or_expf(x); }
OR_EXPORT float or_kat_pow(float x, float y) { return or_powf(x, y); }
/* or_kat_exp / or_kat_log of every element: what a restatement over a whole frame calls (one call, not one per pixel and tap) */
OR_EXPORT void or_kat_exp_many(uint64_t n, const float *x, float *out) { for (uint64_t i = 0; i < n; i++) out[i] = or_expf(x[i]); }
OR_EXPORT void or_kat_log_many(uint64_t n, const float *x, float *out) { for (uint64_t i = 0; i < n; i++) out[i] = or_logf(x[i]); }
/* the ColorPipeline (OR_COLOR_* bits) the probes below evaluate materials under; renders set it from their config */
OR_EXPORT void or_scene_set_color(or_scene *sc, uint32_t color) { sc->color = color; }
/* dimension pair (dim, dim + 1) of sample `index` of pixel (px, py) of the sobol sampler, as fixed-point-free floats */
OR_EXPORT void or_kat_sobol_2d(uint32_t px, uint32_t py, uint32_t dim, uint32_t seed, uint32_t spp, uint32_t index, float *out2) {
    or_sampler s;
    memset(&s, 0, sizeof s);
    s.pmj = 2; s.seed = seed; s.spp = spp; s.px = px; s.py = py; s.sample_index = index; s.dim = dim;
    uint32_t w = spp - 1; w |= w >> 1; w |= w >> 2; w |= w >> 4; w |= w >> 8; w |= w >> 16;
    s.w = w;
    v2 r = smp_2d(&s);
    out2[0] = r.x; out2[1] = r.y;
}
/* evaluated inputs (26 words each) of `material` at n uv points */
OR_EXPORT void or_material_inputs(const or_scene *sc, uint32_t material, uint32_t n, const float *uv, float *out26) {
    for (uint32_t i = 0; i < n; i++) {
        or_material_desc at;
        or_material_at(&sc->materials[material], sc->graphs ? &sc->graphs[material] : 0, sc->images, sc->color, uv[2 * i], uv[2 * i + 1], &at);
        memcpy(out26 + 26 * (size_t)i, &at, sizeof at);
    }
}
OR_EXPORT void or_tex_sample_many(const or_image_desc *im, uint32_t n, const float *uv, float *out4) {
    for (uint32_t i = 0; i < n; i++) {
        or_val r = or_tex_sample(im, uv[2 * i], uv[2 * i + 1]);
        memcpy(out4 + 4 * (size_t)i, r.v, 16);
    }
}
OR_EXPORT void or_kat_alias_build(const float *w, uint32_t n, uint32_t *j, float *t, float *pdf) {
    or_alias_table at;
    or_alias_build(&at, w, n);
    for (uint32_t i = 0; i < n; i++) { j[i] = at.table[i].j; t[i] = at.table[i].t; pdf[i] = at.pdf[i]; }
    or_alias_free(&at);
}
OR_EXPORT void or_kat_offset_ray_origin(const float *p, const float *n, float *out) {
    v3 r = or_offset_ray_origin(V3(p[0], p[1], p[2]), V3(n[0], n[1], n[2]));
    out[0] = r.x; out[1] = r.y; out[2] = r.z;
}
OR_EXPORT void or_kat_uniform_sample_triangle(float ux, float uy, float *b) { v2 r = or_uniform_sample_triangle(V2(ux, uy)); b[0] = r.x; b[1] = r.y; }
OR_EXPORT void or_kat_cos_sample_hemisphere(float ux, float uy, float *w) { v3 r = or_cos_sample_hemisphere(V2(ux, uy)); w[0] = r.x; w[1] = r.y; w[2] = r.z; }

/* scene introspection (compared with the product's host-side scene compiler) */
OR_EXPORT uint32_t or_scene_num_lights(const or_scene *sc) { return sc->n_lights; }
OR_EXPORT uint32_t or_scene_num_triangles(const or_scene *sc) { return sc->n_tris; }
OR_EXPORT void or_scene_light_info(const or_scene *sc, uint32_t light, uint32_t *inst, float *power, float *pdf) {
    *inst = sc->light_inst[light]; *power = sc->light_power[light]; *pdf = sc->light_dist.pdf[light];
}
OR_EXPORT void or_scene_camera(const or_scene *sc, float *r2c, float *c2w, int *identity) { memcpy(r2c, sc->r2c, 64); memcpy(c2w, sc->c2w, 64); *identity = sc->c2w_identity; }
/* out: p(3) ng(3) n(3) t(3) s(3) uv(2) area material */
OR_EXPORT void or_scene_surface_interaction(const or_scene *sc, uint32_t inst, uint32_t prim, float bu, float bv, float *out) {
    or_si si = or_surface_interaction(sc, inst, prim, V2(bu, bv));
    float r[19] = {si.p.x, si.p.y, si.p.z, si.ng.x, si.ng.y, si.ng.z, si.frame.n.x, si.frame.n.y, si.frame.n.z,
                   si.frame.t.x, si.frame.t.y, si.frame.t.z, si.frame.s.x, si.frame.s.y, si.frame.s.z, si.uv.x, si.uv.y,
                   si.prim_area, (float)si.material};
    memcpy(out, r, sizeof r);
}
/* closest hit for one ray: returns 1 and (inst, prim, u, v) */
OR_EXPORT int or_scene_intersect(const or_scene *sc, const float *o, const float *d, float tmin, float tmax, uint32_t *inst, uint32_t *prim, float *bary) {
    or_ray r = {V3(o[0], o[1], o[2]), V3(d[0], d[1], d[2]), tmin, tmax, OR_INVALID, OR_INVALID, OR_INVALID, OR_INVALID};
    v2 b = V2(0, 0);
    int hit = or_trace(sc, &r, 0, inst, prim, &b, 0);
    bary[0] = b.x; bary[1] = b.y;
    return hit;
}

/* BSDF probes for the chi^2 / furnace tests (akari_test.rs:16-439 restated in tests/): the material `m` at a
 * flat surface with normal +z, world == local. mode 0: evaluate(wo,wi) -> f(3), pdf; mode 1: sample(wo,u) ->
 * wi(3), f(3), pdf, valid. */
OR_EXPORT void or_bsdf_probe(const or_material_desc *m, const float *table, int mode, const float *wo_, const float *in, float *out) {
    or_scene sc;
    memset(&sc, 0, sizeof sc);
    sc.materials = (or_material_desc *)m;
    if (table) memcpy(sc.table, table, sizeof sc.table);
    or_si si;
    memset(&si, 0, sizeof si);
    si.frame = or_frame_from_n(V3(0, 0, 1)); si.ng = V3(0, 0, 1); si.material = 0; si.valid = 1;
    or_closure_pool pool;
    or_surface *c = or_build_closure(&pool, &sc, &si, 0);
    v3 wo = V3(wo_[0], wo_[1], wo_[2]);
    if (mode == 0) {
        v3 f; float pdf;
        or_surf_evaluate(c, wo, V3(in[0], in[1], in[2]), &f, &pdf);
        out[0] = f.x; out[1] = f.y; out[2] = f.z; out[3] = pdf;
    } else {
        or_bsdf_sample s = or_closure_sample(c, wo, in[0], V2(in[1], in[2]));
        out[0] = s.wi.x; out[1] = s.wi.y; out[2] = s.wi.z; out[3] = s.color.x; out[4] = s.color.y; out[5] = s.color.z;
        out[6] = s.pdf; out[7] = (float)s.valid;
    }
}
/* many samples at once: u (3 per sample) -> out (8 per sample) */
OR_EXPORT void or_bsdf_probe_many(const or_material_desc *m, const float *table, const float *wo_, uint32_t n, const float *u, float *out) {
    for (uint32_t i = 0; i < n; i++) or_bsdf_probe(m, table, 1, wo_, u + 3 * i, out + 8 * i);
}
OR_EXPORT void or_bsdf_eval_many(const or_material_desc *m, const float *table, const float *wo_, uint32_t n, const float *wi, float *out) {
    for (uint32_t i = 0; i < n; i++) or_bsdf_probe(m, table, 0, wo_, wi + 3 * i, out + 4 * i);
}
/* ---------------------------------- the environment light (or_env.h) -------------- */
static void or_world_bounds(const or_scene *sc, float lo[3], float hi[3]) { /* over every triangle corner (lo > hi: no geometry) */
    for (int a = 0; a < 3; a++) { lo[a] = INFINITY; hi[a] = -INFINITY; }
    for (uint32_t i = 0; i < sc->n_instances; i++) {
        const or_instance *in = &sc->instances[i];
        const or_mesh_desc *g = &sc->meshes[in->mesh].d;
        for (uint32_t k = 0; k < 3 * g->n_triangles; k++) {
            v3 p = xf_point(&in->xf, ld3(g->vertices, g->indices[k]));
            lo[0] = or_min(lo[0], p.x); lo[1] = or_min(lo[1], p.y); lo[2] = or_min(lo[2], p.z);
            hi[0] = or_max(hi[0], p.x); hi[1] = or_max(hi[1], p.y); hi[2] = or_max(hi[2], p.z);
        }
    }
}
/* The light list (4.14): the emissive instances as or_scene_create found them, the punctual lights in the order given, the environment
 * last; the alias table rebuilt over all of them. With a tree (4.16 "Light table with a tree": the mode is on and there are >= 2 local
 * lights): the emissive instances, the suns in the order given, ONE entry for the tree, the environment; the tree's weight is the f64
 * sum of the local lights' f32 weights in the order given, rounded once; and the tree is built anew (4.16 "Build"). */
static void or_rebuild_light_list(or_scene *sc) {
    if (sc->n_lights > 0) or_alias_free(&sc->light_dist);
    free(sc->lt_nodes);
    sc->lt_nodes = 0; sc->n_lt_nodes = 0;
    const uint32_t cap = sc->n_emit + sc->n_punct + 2;
    sc->light_inst = (uint32_t *)realloc(sc->light_inst, 4ull * cap);
    sc->light_power = (float *)realloc(sc->light_power, 4ull * cap);
    sc->light_rec = (uint32_t *)realloc(sc->light_rec, 4ull * cap);
    for (uint32_t i = 0; i < sc->n_emit; i++) sc->light_rec[i] = OR_INVALID;
    uint32_t n = sc->n_emit;
    if (sc->n_punct) {
        float lo[3], hi[3];
        or_world_bounds(sc, lo, hi);
        const double R = or_punct_bounds_radius(lo, hi);
        float *weights = (float *)malloc(4ull * sc->n_punct);
        uint32_t n_local = 0;
        for (uint32_t k = 0; k < sc->n_punct; k++) {
            weights[k] = or_punct_power(&sc->punct[0][k], R);
            n_local += or_lt_is_local(&sc->punct[0][k]) ? 1u : 0u;
        }
        const int tree = sc->light_tree && n_local >= 2;
        double tree_weight = 0.0;
        for (uint32_t k = 0; k < sc->n_punct; k++) {
            if (tree && or_lt_is_local(&sc->punct[0][k])) { tree_weight += (double)weights[k]; continue; }
            sc->light_inst[n] = OR_PUNCT_INST;
            sc->light_power[n] = weights[k];
            sc->light_rec[n] = k;
            n++;
        }
        if (tree) {
            sc->light_inst[n] = OR_PUNCT_TREE_INST;
            sc->light_power[n] = (float)tree_weight;
            sc->light_rec[n] = 0;
            n++;
            sc->lt_nodes = or_lt_build(sc->punct[0], weights, sc->n_punct, &sc->n_lt_nodes);
        }
        free(weights);
    }
    if (sc->env) {
        sc->light_inst[n] = OR_INVALID;
        sc->light_power[n] = sc->env->power;
        sc->light_rec[n] = OR_INVALID;
        n++;
    }
    sc->n_lights = n;
    if (sc->n_lights > 0) or_alias_build(&sc->light_dist, sc->light_power, sc->n_lights);
}
/* Sets (desc = NULL: removes) the scene's environment: the last entry of the light table, weight 4 pi R^2 Lbar. Returns 0, or -1 for a
 * description akr_scene_set_environment refuses (the scene is left as it was). */
OR_EXPORT int or_scene_set_environment(or_scene *sc, const or_environment_desc *d) {
    or_env *e = 0;
    if (d) {
        float lo[3], hi[3];
        or_world_bounds(sc, lo, hi);
        if (or_env_create(d, lo, hi, &e) != 0) return -1;
    }
    or_env_free(sc->env);
    sc->env = e;
    or_rebuild_light_list(sc);
    return 0;
}
/* ---------------------------------- punctual lights (or_punct.h) and the lens (4.9) -------------- */
/* Replaces the scene's punctual lights by the n given (NULL or 0: removes them). Returns 0, or -1 when akr_scene_add_punctual_light
 * would refuse one of them (the scene is left as it was). A light of strength 0 or an all-zero colour is accepted and is no light. */
OR_EXPORT int or_scene_set_punctual_lights(or_scene *sc, const or_punctual_light_desc *lights, uint32_t n) {
    if (!lights) n = 0;
    or_punctual_light_desc *keep = (or_punctual_light_desc *)malloc(sizeof(or_punctual_light_desc) * (n ? n : 1));
    uint32_t m = 0;
    for (uint32_t i = 0; i < n; i++) {
        const int rc = or_punct_check(&lights[i], &keep[m]);
        if (rc < 0) { free(keep); return -1; }
        if (rc > 0) m++;
    }
    free(sc->punct_desc);
    sc->punct_desc = keep;
    sc->n_punct = m;
    for (uint32_t color = 0; color < 4; color++) {
        free(sc->punct[color]);
        sc->punct[color] = (or_punct *)malloc(sizeof(or_punct) * (m ? m : 1));
        for (uint32_t k = 0; k < m; k++) sc->punct[color][k] = or_punct_fold(&keep[k], color);
    }
    or_rebuild_light_list(sc);
    return 0;
}
/* The folded records under the ColorPipeline bits `color`, 16 words each (may be NULL), and the descriptions as held (may be NULL);
 * returns the count. */
OR_EXPORT uint32_t or_scene_punctual_records(const or_scene *sc, uint32_t color, uint32_t *words16, or_punctual_light_desc *descs) {
    if (words16 && sc->n_punct) memcpy(words16, sc->punct[color & 3u], sizeof(or_punct) * sc->n_punct);
    if (descs && sc->n_punct) memcpy(descs, sc->punct_desc, sizeof(or_punctual_light_desc) * sc->n_punct);
    return sc->n_punct;
}
/* The light table's alias entries ({j, t} records) and pdfs, n_lights each */
OR_EXPORT void or_scene_light_table(const or_scene *sc, or_alias_entry *entries, float *pdf) {
    if (!sc->n_lights) return;
    memcpy(entries, sc->light_dist.table, sizeof(or_alias_entry) * sc->n_lights);
    memcpy(pdf, sc->light_dist.pdf, 4ull * sc->n_lights);
}
/* Known-answer call with the rows of akr_host_light_sample_soft: rows9 = p, n, u_select, u_sample -> out13 = li, wi, pdf, ro, tmax, valid,
 * delta and the light chosen. An emitter or the environment answers the choice's pdf alone. Uses the records of the pipeline set by
 * or_scene_set_color (0 after creation). Returns -1 for a scene without lights. */
static void or_punct_sample_row(const or_scene *sc, uint32_t record, const float *r, float *o) {
    const or_punct_ls s = or_punct_sample(&sc->punct[sc->color & 3u][record], V3(r[0], r[1], r[2]), V3(r[3], r[4], r[5]), V2(r[7], r[8]));
    o[0] = s.li.x; o[1] = s.li.y; o[2] = s.li.z; o[3] = s.wi.x; o[4] = s.wi.y; o[5] = s.wi.z;
    o[7] = s.ro.x; o[8] = s.ro.y; o[9] = s.ro.z; o[10] = s.tmax; o[11] = s.valid ? 1.0f : 0.0f; o[12] = 1.0f;
}
OR_EXPORT int or_punct_sample_many(const or_scene *sc, uint32_t n, const float *rows9, float *out13, uint32_t *light) {
    if (!sc->n_lights) return -1;
    for (uint32_t i = 0; i < n; i++) {
        const float *r = rows9 + 9ull * i;
        float *o = out13 + 13ull * i;
        float pdf, rest;
        const uint32_t idx = or_alias_sample_and_remap(&sc->light_dist, r[6], &pdf, &rest);
        memset(o, 0, 13 * sizeof(float));
        o[6] = pdf;
        light[i] = idx;
        if (sc->light_inst[idx] != OR_PUNCT_INST) continue; /* the tree's entry included: nothing is sampled there */
        or_punct_sample_row(sc, sc->light_rec[idx], r, o);
    }
    return 0;
}
/* ---------------------------------- the light tree (or_lighttree.h) ------------------------------------ */
/* Sets the scene's mode (4.16 "Which lights, and when") and rebuilds the light list; setting the lights while it is on rebuilds the tree. */
OR_EXPORT void or_scene_set_light_tree(or_scene *sc, uint32_t on) {
    sc->light_tree = on ? 1u : 0u;
    or_rebuild_light_list(sc);
}
/* The mode, and the number of nodes (0: no tree exists) */
OR_EXPORT void or_scene_get_light_tree(const or_scene *sc, uint32_t *on, uint32_t *n_nodes) { *on = sc->light_tree; *n_nodes = sc->n_lt_nodes; }
/* The node words, 8 per node (lo.xyz, power | hi.xyz, child); returns the node count */
OR_EXPORT uint32_t or_scene_light_tree_nodes(const or_scene *sc, uint32_t *words) {
    if (words && sc->n_lt_nodes) memcpy(words, sc->lt_nodes, sizeof(or_lt_node) * sc->n_lt_nodes);
    return sc->n_lt_nodes;
}
/* Known-answer call with the rows and columns of akr_host_light_tree_sample: as or_punct_sample_many, but the tree's entry walks (out13[6]
 * = the walked pdf, delta = 1) and samples the record it reaches; record = that record's index, or 0xffffffff when the entry was not the
 * tree. */
OR_EXPORT int or_light_tree_sample_many(const or_scene *sc, uint32_t n, const float *rows9, float *out13, uint32_t *light, uint32_t *record) {
    if (!sc->n_lights) return -1;
    for (uint32_t i = 0; i < n; i++) {
        const float *r = rows9 + 9ull * i;
        float *o = out13 + 13ull * i;
        float pdf, rest;
        const uint32_t idx = or_alias_sample_and_remap(&sc->light_dist, r[6], &pdf, &rest);
        memset(o, 0, 13 * sizeof(float));
        o[6] = pdf;
        light[i] = idx;
        record[i] = OR_LT_NO_RECORD;
        if (sc->light_inst[idx] == OR_PUNCT_INST) or_punct_sample_row(sc, sc->light_rec[idx], r, o);
        if (sc->light_inst[idx] != OR_PUNCT_TREE_INST) continue;
        const int ok = or_lt_walk(sc->lt_nodes, V3(r[0], r[1], r[2]), rest, &pdf, &record[i]);
        o[6] = pdf; o[12] = 1.0f;
        if (ok) or_punct_sample_row(sc, record[i], r, o);
    }
    return 0;
}
OR_EXPORT uint32_t or_sizeof_light_tree_node(void) { return (uint32_t)sizeof(or_lt_node); }
/* Sets (NULL or radius 0: removes) the camera's lens. Returns -1 for what akr_scene_set_lens refuses on the values alone: a non-finite
 * or negative value, a radius > 0 without a focal distance > 0. (The library's further test against the padding of its acceleration
 * structure is the library's own concern: the oracle has no padded boxes.) */
OR_EXPORT int or_scene_set_lens(or_scene *sc, const or_lens_desc *d) {
    if (d) {
        if (!or_isfinite(d->radius) || !or_isfinite(d->focal_distance) || d->radius < 0.0f || d->focal_distance < 0.0f) return -1;
        if (d->radius > 0.0f && !(d->focal_distance > 0.0f)) return -1;
        if (d->radius > 0.0f && sc->proj.type == OR_PROJECTION_PANORAMA) return -1; /* 4.17: a panorama has no lens */
    }
    sc->lens_radius = (d && d->radius > 0.0f) ? d->radius : 0.0f;
    sc->lens_focal = (d && d->radius > 0.0f) ? d->focal_distance : 0.0f;
    return 0;
}
OR_EXPORT void or_scene_get_lens(const or_scene *sc, or_lens_desc *out) { out->radius = sc->lens_radius; out->focal_distance = sc->lens_focal; }
/* Sets (NULL: back to the perspective camera) the camera's projection. Returns -1, and leaves the scene as it was, for what
 * akr_scene_set_projection refuses on the values alone: an unknown type; an orthographic scale that is not finite and > 0; a panorama
 * window with a non-finite bound, a bound outside [-pi, pi] x [-pi/2, pi/2] (the f32 nearest to them, inclusive) or min >= max; a panorama
 * on a scene that has a lens. The fields a type does not read are kept at their defaults. (The library's further test of an orthographic
 * film against the padding of its acceleration structure is the library's own concern, as for the lens.) */
OR_EXPORT int or_scene_set_projection(or_scene *sc, const or_projection_desc *d) {
    or_projection_desc p = OR_PROJECTION_DEFAULT;
    if (d) {
        if (d->type > OR_PROJECTION_PANORAMA) return -1;
        p.type = d->type;
        if (d->type == OR_PROJECTION_ORTHOGRAPHIC) {
            if (!or_isfinite(d->ortho_scale) || !(d->ortho_scale > 0.0f)) return -1;
            p.ortho_scale = d->ortho_scale;
        } else if (d->type == OR_PROJECTION_PANORAMA) {
            const float b[4] = {d->longitude_min, d->longitude_max, d->latitude_min, d->latitude_max};
            for (int i = 0; i < 4; i++) if (!or_isfinite(b[i])) return -1;
            if (b[0] < p.longitude_min || b[1] > p.longitude_max || !(b[0] < b[1])) return -1;
            if (b[2] < p.latitude_min || b[3] > p.latitude_max || !(b[2] < b[3])) return -1;
            if (sc->lens_radius > 0.0f) return -1;
            p.longitude_min = b[0]; p.longitude_max = b[1]; p.latitude_min = b[2]; p.latitude_max = b[3];
        }
    }
    sc->proj = p;
    or_projection_fold(sc);
    return 0;
}
OR_EXPORT void or_scene_get_projection(const or_scene *sc, or_projection_desc *out) { *out = sc->proj; }
/* The film's size; the camera's matrix and a panorama's constants follow it (4.17: the fold is per resolution). -1 for an empty film. */
OR_EXPORT int or_scene_set_resolution(or_scene *sc, uint32_t width, uint32_t height) {
    if (!width || !height) return -1;
    sc->width = width; sc->height = height;
    or_projection_fold(sc);
    return 0;
}
OR_EXPORT uint32_t or_sizeof_projection_desc(void) { return (uint32_t)sizeof(or_projection_desc); }
/* Known-answer call with the rows of akr_host_lens_ray: pixels2 = x, y; u4 = u_filter, u_lens -> out6 = o, d */
OR_EXPORT int or_lens_ray_many(const or_scene *sc, uint32_t filter_type, float filter_radius, uint32_t n, const uint32_t *pixels2, const float *u4, float *out6) {
    if (filter_type > OR_FILTER_GAUSSIAN) return -1;
    or_pt_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.filter_type = filter_type; cfg.filter_radius = filter_radius;
    for (uint32_t i = 0; i < n; i++) {
        const float *u = u4 + 4ull * i;
        const or_ray r = or_camera_ray(sc, &cfg, pixels2[2ull * i], pixels2[2ull * i + 1], V2(u[0], u[1]), V2(u[2], u[3]));
        float *o = out6 + 6ull * i;
        o[0] = r.o.x; o[1] = r.o.y; o[2] = r.o.z; o[3] = r.d.x; o[4] = r.d.y; o[5] = r.d.z;
    }
    return 0;
}
OR_EXPORT uint32_t or_sizeof_punctual_light_desc(void) { return (uint32_t)sizeof(or_punctual_light_desc); }
OR_EXPORT uint32_t or_sizeof_lens_desc(void) { return (uint32_t)sizeof(or_lens_desc); }
OR_EXPORT uint32_t or_sizeof_punct_record(void) { return (uint32_t)sizeof(or_punct); }
/* The environment's size and tables, for comparison with the library's (akr_scene_get_array): returns 0 without one. dims = w, h, filter.
 * Any output pointer may be NULL; entries as {j, t} pairs, row by row for the conditional tables. */
OR_EXPORT int or_scene_env_tables(const or_scene *sc, uint32_t *dims, float *texels, or_alias_entry *marginal, float *marginal_pdf,
                                  or_alias_entry *conditional, float *conditional_pdf) {
    const or_env *e = sc->env;
    if (!e) return 0;
    if (dims) { dims[0] = e->w; dims[1] = e->h; dims[2] = e->filter; }
    if (texels) memcpy(texels, e->texels, 16 * (size_t)e->w * e->h);
    if (marginal) memcpy(marginal, e->marginal.table, sizeof(or_alias_entry) * e->h);
    if (marginal_pdf) memcpy(marginal_pdf, e->marginal.pdf, 4 * (size_t)e->h);
    for (uint32_t y = 0; y < e->h; y++) {
        if (conditional) memcpy(conditional + (size_t)y * e->w, e->conditional[y].table, sizeof(or_alias_entry) * e->w);
        if (conditional_pdf) memcpy(conditional_pdf + (size_t)y * e->w, e->conditional[y].pdf, 4 * (size_t)e->w);
    }
    return 1;
}
/* known-answer entry points in the style of or_tex_sample_many (the probes akr_probe_env_sample / akr_probe_env_pdf restate):
 * u2 (2 / item) -> wi.xyz, pdf, valid (5 / item); directions (3 / item) -> pdf, radiance.rgb under the scene's pipeline (4 / item) */
OR_EXPORT int or_env_sample_many(const or_scene *sc, uint32_t n, const float *u2, float *out5) {
    if (!sc->env) return -1;
    for (uint32_t i = 0; i < n; i++) {
        v3 wi; float pdf;
        int ok = or_env_sample(sc->env, V2(u2[2 * i], u2[2 * i + 1]), &wi, &pdf);
        float r[5] = {wi.x, wi.y, wi.z, pdf, ok ? 1.0f : 0.0f};
        memcpy(out5 + 5 * (size_t)i, r, sizeof r);
    }
    return 0;
}
OR_EXPORT int or_env_pdf_many(const or_scene *sc, uint32_t n, const float *dirs, float *out4) {
    if (!sc->env) return -1;
    for (uint32_t i = 0; i < n; i++) {
        v3 d = V3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
        v3 c = or_env_eval(sc->env, sc->color, d);
        float r[4] = {or_env_pdf(sc->env, d), c.x, c.y, c.z};
        memcpy(out4 + 4 * (size_t)i, r, sizeof r);
    }
    return 0;
}
/* the environment-frame (u, v) and sin(theta) of world directions (3 / item -> 3 / item) */
OR_EXPORT int or_env_uv_many(const or_scene *sc, uint32_t n, const float *dirs, float *out3) {
    if (!sc->env) return -1;
    for (uint32_t i = 0; i < n; i++) {
        float st;
        v2 uv = or_env_uv(or_env_local(sc->env, V3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2])), &st);
        out3[3 * i] = uv.x; out3[3 * i + 1] = uv.y; out3[3 * i + 2] = st;
    }
    return 0;
}
OR_EXPORT void or_kat_atan2_many(uint32_t n, const float *y, const float *x, float *out) {
    for (uint32_t i = 0; i < n; i++) out[i] = or_atan2f(y[i], x[i]);
}
OR_EXPORT float or_kat_atan2(float y, float x) { return or_atan2f(y, x); }
OR_EXPORT uint32_t or_sizeof_environment_desc(void) { return (uint32_t)sizeof(or_environment_desc); }

OR_EXPORT uint32_t or_sizeof_material(void) { return (uint32_t)sizeof(or_material_desc); }
OR_EXPORT uint32_t or_sizeof_config(void) { return (uint32_t)sizeof(or_pt_config); }
OR_EXPORT uint32_t or_sizeof_scene_desc(void) { return (uint32_t)sizeof(or_scene_desc); }
