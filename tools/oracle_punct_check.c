/* oracle_punct_check.c -- a stand-alone run of the CPU oracle's punctual lights, soft lights and thin lens (oracle/or_punct.h, the camera-ray code of
 * oracle/akr_oracle.c) for the host sanitisers. CPU only, its own main, never loaded into Python. It renders one 16 x 16
 * scene (a floor, a blocker, an emitter) with one light of each kind, delta and soft, through a lens -- pt under two colour pipelines and aov --, runs
 * the two known-answer calls on 4096 rows, and walks the setters' refusals and removals. From the repository root:
 *
 *   mkdir -p build && gcc -std=gnu11 -O1 -g -fno-omit-frame-pointer -ffp-contract=off -fno-fast-math -fsanitize=address,undefined \
 *       -fno-sanitize-recover=undefined -pthread -Ioracle tools/oracle_punct_check.c oracle/akr_oracle.c -lm -o build/oracle_punct_check \
 *       && build/oracle_punct_check
 *
 * It prints one summary line and exits 0; a sanitiser report ends it with a non-zero status.
 */
#include "or_api.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef struct or_scene or_scene;
typedef struct {
    uint32_t spp, aov, remap, filter_type; float filter_radius; uint32_t sampler_type; uint64_t sampler_seed;
    uint32_t shard_rank, shard_count, tile_w, tile_h;
    uint32_t color, _pad;
} aov_config; /* = or_aov_config of akr_oracle.c (checked against or_sizeof_aov_config below) */

or_scene *or_scene_create(const or_scene_desc *d);
void or_scene_destroy(or_scene *sc);
int or_pt_render(const or_scene *sc, const or_pt_config *cfg, float *film, uint64_t *states_io, uint32_t n_threads, or_stats *stats_out);
int or_aov_render(const or_scene *sc, const aov_config *cfg, float *film, uint32_t n_threads, uint64_t *n_rays_out);
uint32_t or_sizeof_aov_config(void);
int or_scene_set_punctual_lights(or_scene *sc, const or_punctual_light_desc *lights, uint32_t n);
uint32_t or_scene_punctual_records(const or_scene *sc, uint32_t color, uint32_t *words16, or_punctual_light_desc *descs);
int or_punct_sample_many(const or_scene *sc, uint32_t n, const float *rows9, float *out13, uint32_t *light);
int or_scene_set_lens(or_scene *sc, const or_lens_desc *d);
int or_lens_ray_many(const or_scene *sc, uint32_t filter_type, float filter_radius, uint32_t n, const uint32_t *pixels2, const float *u4, float *out6);
int or_scene_set_environment(or_scene *sc, const or_environment_desc *d);
uint32_t or_scene_num_lights(const or_scene *sc);
void or_scene_set_color(or_scene *sc, uint32_t color);

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "oracle_punct_check: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

static uint32_t g_rng = 12345u;
static float rnd(void) { g_rng = g_rng * 1664525u + 1013904223u; return (float)(g_rng >> 8) * (1.0f / 16777216.0f); }

int main(void) {
    /* a floor in z = 0, a blocker strip above it, a small emitter; the camera on +z looking down -z */
    static const float floor_v[12] = {-1, -1, 0, 1, -1, 0, 1, 1, 0, -1, 1, 0};
    static const float block_v[12] = {0.0f, -1, 0.5f, 0.3f, -1, 0.5f, 0.3f, 1, 0.5f, 0.0f, 1, 0.5f};
    static const float light_v[12] = {-0.8f, -0.2f, 0.9f, -0.4f, -0.2f, 0.9f, -0.4f, 0.2f, 0.9f, -0.8f, 0.2f, 0.9f};
    static const uint32_t up[6] = {0, 1, 2, 0, 2, 3}, down[6] = {0, 2, 1, 0, 3, 2};
    or_mesh_desc meshes[3];
    memset(meshes, 0, sizeof meshes);
    const float *verts[3] = {floor_v, block_v, light_v};
    for (int i = 0; i < 3; i++) { meshes[i].n_vertices = 4; meshes[i].n_triangles = 2; meshes[i].vertices = verts[i]; meshes[i].indices = i == 2 ? down : up; }
    or_material_desc mats[3];
    memset(mats, 0, sizeof mats);
    mats[0].kind = OR_MAT_DIFFUSE; mats[0].base_color[0] = 0.7f; mats[0].base_color[1] = 0.6f; mats[0].base_color[2] = 0.5f; mats[0].base_alpha = 1.0f;
    mats[1].kind = OR_MAT_PRINCIPLED; mats[1].base_color[0] = mats[1].base_color[1] = mats[1].base_color[2] = 0.9f; mats[1].base_alpha = 1.0f;
    mats[1].metallic = 1.0f; mats[1].roughness = 0.3f; mats[1].ior = 1.5f; mats[1].specular_ior_level = 0.5f; mats[1].coat_ior = 1.5f;
    mats[1].specular_tint[0] = mats[1].specular_tint[1] = mats[1].specular_tint[2] = 1.0f;
    mats[2].kind = OR_MAT_EMISSION; mats[2].emission_color[0] = 4.0f; mats[2].emission_color[1] = 3.0f; mats[2].emission_color[2] = 2.0f; mats[2].emission_strength = 1.0f;
    static const uint32_t slot[3] = {0, 1, 2};
    or_instance_desc insts[3];
    memset(insts, 0, sizeof insts);
    for (int i = 0; i < 3; i++) {
        insts[i].mesh = (uint32_t)i; insts[i].n_materials = 1; insts[i].materials = &slot[i];
        insts[i].transform[0] = insts[i].transform[5] = insts[i].transform[10] = insts[i].transform[15] = 1.0f;
    }
    static float table[4096];
    for (int i = 0; i < 4096; i++) table[i] = 0.5f;
    or_scene_desc sd;
    memset(&sd, 0, sizeof sd);
    sd.n_meshes = sd.n_instances = sd.n_materials = 3;
    sd.meshes = meshes; sd.instances = insts; sd.materials = mats; sd.ggx_dielectric_table = table;
    sd.camera.c2w[0] = sd.camera.c2w[5] = sd.camera.c2w[10] = sd.camera.c2w[15] = 1.0f;
    sd.camera.c2w[12] = 0.1f; sd.camera.c2w[14] = 3.0f; /* not the identity: the lens takes the general branch of step 4 */
    sd.camera.fov = 0.7f; sd.camera.width = sd.camera.height = 16;
    or_scene *sc = or_scene_create(&sd);
    CHECK(sc && or_scene_num_lights(sc) == 1);
    CHECK(or_sizeof_aov_config() == sizeof(aov_config));

    /* one light of each kind, delta and soft; one that is "no light"; sizes the kind does not read hold junk */
    or_punctual_light_desc L[7];
    memset(L, 0, sizeof L);
    for (int i = 0; i < 7; i++) { L[i].color[0] = 1.0f + (float)i; L[i].color[1] = 2.0f; L[i].color[2] = 0.5f; L[i].strength = 1.5f; }
    L[0].type = OR_LIGHT_POINT; L[0].position[0] = 0.3f; L[0].position[1] = -0.2f; L[0].position[2] = 1.5f; L[0].angle = NAN;
    L[1] = L[0]; L[1].radius = 0.3f;
    L[2].type = OR_LIGHT_SPOT; L[2].position[0] = 0.25f; L[2].position[1] = 0.5f; L[2].position[2] = 2.0f;
    L[2].direction[0] = 0.1f; L[2].direction[1] = -0.3f; L[2].direction[2] = -1.0f; L[2].cone_angle = 0.5f; L[2].blend = 0.3f;
    L[3] = L[2]; L[3].radius = 0.125f; L[3].blend = 0.0f;
    L[4].type = OR_LIGHT_SUN; L[4].direction[0] = 0.2f; L[4].direction[1] = -0.1f; L[4].direction[2] = -1.0f; L[4].radius = 9.0f;
    L[5] = L[4]; L[5].angle = 0.4f;
    L[6] = L[0]; L[6].strength = 0.0f;
    CHECK(or_scene_set_punctual_lights(sc, L, 7) == 0);
    CHECK(or_scene_punctual_records(sc, 0, 0, 0) == 6 && or_scene_num_lights(sc) == 7);
    uint32_t words[6 * 16];
    or_punctual_light_desc held[6];
    for (uint32_t color = 0; color < 4; color++) CHECK(or_scene_punctual_records(sc, color, words, held) == 6);
    CHECK(held[0].angle == 0.0f && held[4].radius == 0.0f);
    /* refusals leave the scene as it was */
    or_punctual_light_desc bad = L[5];
    bad.angle = 3.14159274f;
    CHECK(or_scene_set_punctual_lights(sc, &bad, 1) == -1);
    bad = L[1]; bad.radius = -1.0f;
    CHECK(or_scene_set_punctual_lights(sc, &bad, 1) == -1);
    bad = L[2]; bad.direction[0] = bad.direction[1] = bad.direction[2] = 0.0f;
    CHECK(or_scene_set_punctual_lights(sc, &bad, 1) == -1 && or_scene_num_lights(sc) == 7);
    /* an environment goes behind them, whichever is set first */
    or_environment_desc env;
    memset(&env, 0, sizeof env);
    env.color[0] = 0.5f; env.color[1] = 0.6f; env.color[2] = 0.7f; env.strength = 1.0f; env.rotation[0] = env.rotation[4] = env.rotation[8] = 1.0f;
    CHECK(or_scene_set_environment(sc, &env) == 0 && or_scene_num_lights(sc) == 8);
    CHECK(or_scene_set_punctual_lights(sc, L, 6) == 0 && or_scene_num_lights(sc) == 8);

    or_lens_desc lens = {0.2f, 3.0f}, bad_lens = {0.1f, 0.0f};
    CHECK(or_scene_set_lens(sc, &bad_lens) == -1 && or_scene_set_lens(sc, &lens) == 0);

    /* known-answer calls */
    enum { N = 4096 };
    float *rows = (float *)malloc(sizeof(float) * 9 * N), *out = (float *)malloc(sizeof(float) * 13 * N), *rays = (float *)malloc(sizeof(float) * 6 * N);
    float *u4 = (float *)malloc(sizeof(float) * 4 * N);
    uint32_t *which = (uint32_t *)malloc(sizeof(uint32_t) * N), *px = (uint32_t *)malloc(sizeof(uint32_t) * 2 * N);
    for (int i = 0; i < N; i++) {
        float *r = rows + 9 * i;
        r[0] = 2.0f * rnd() - 1.0f; r[1] = 2.0f * rnd() - 1.0f; r[2] = 0.4f * rnd() - 0.2f;
        r[3] = 0.0f; r[4] = 0.0f; r[5] = 1.0f; r[6] = rnd(); r[7] = rnd(); r[8] = rnd();
        px[2 * i] = (uint32_t)(rnd() * 16.0f) & 15u; px[2 * i + 1] = (uint32_t)(rnd() * 16.0f) & 15u;
        for (int k = 0; k < 4; k++) u4[4 * i + k] = rnd();
    }
    memcpy(rows, L[0].position, 12); /* p == q */
    u4[2] = u4[3] = 0.5f;            /* the centre of the lens */
    int valid = 0;
    for (uint32_t color = 0; color < 4; color++) {
        or_scene_set_color(sc, color);
        CHECK(or_punct_sample_many(sc, N, rows, out, which) == 0);
    }
    or_scene_set_color(sc, 0);
    for (int i = 0; i < N; i++) { CHECK(which[i] < 8); valid += out[13 * i + 11] != 0.0f; }
    CHECK(or_lens_ray_many(sc, OR_FILTER_BOX, 0.5f, N, px, u4, rays) == 0 && or_lens_ray_many(sc, OR_FILTER_GAUSSIAN, 1.5f, N, px, u4, rays) == 0);
    CHECK(or_lens_ray_many(sc, 7, 0.5f, N, px, u4, rays) == -1);

    /* films: pt under two pipelines and both samplers that need no tables, aov */
    float *film = (float *)calloc(7 * 256, sizeof(float));
    or_pt_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.spp = 8; cfg.spp_per_pass = 4; cfg.max_depth = 5; cfg.rr_depth = 2; cfg.use_nee = 1; cfg.debug_depth = -1;
    cfg.filter_type = OR_FILTER_GAUSSIAN; cfg.filter_radius = 1.5f; cfg.sampler_seed = 3; cfg.shard_count = 1;
    or_stats st;
    uint64_t shadow = 0;
    for (uint32_t color = 0; color < 4; color += 3)
        for (uint32_t sampler = 0; sampler < 3; sampler += 2) { /* independent, sobol */
            cfg.color = color; cfg.sampler_type = sampler;
            CHECK(or_pt_render(sc, &cfg, film, 0, 2, &st) == 0 && st.n_samples == 256 * 8 && st.n_shadow > 0 && st.n_shadow <= st.n_shaded);
            shadow += st.n_shadow;
        }
    for (int i = 0; i < 7 * 256; i++) CHECK(isfinite(film[i]));
    aov_config ac;
    memset(&ac, 0, sizeof ac);
    ac.spp = 4; ac.aov = 4; ac.filter_type = OR_FILTER_BOX; ac.filter_radius = 0.5f; ac.shard_count = 1;
    uint64_t n_rays = 0;
    CHECK(or_aov_render(sc, &ac, film, 2, &n_rays) == 0 && n_rays == 256 * 4);

    /* removal: lights, lens, environment */
    CHECK(or_scene_set_punctual_lights(sc, 0, 0) == 0 && or_scene_num_lights(sc) == 2 && or_scene_punctual_records(sc, 0, words, held) == 0);
    CHECK(or_scene_set_lens(sc, 0) == 0 && or_scene_set_environment(sc, 0) == 0 && or_scene_num_lights(sc) == 1);
    cfg.color = 0; cfg.sampler_type = 0;
    CHECK(or_pt_render(sc, &cfg, film, 0, 2, &st) == 0);
    or_scene_destroy(sc);
    printf("oracle_punct_check: 6 lights, %d of %d samples valid, %llu shadow rays in 4 renders, ok\n", valid, N, (unsigned long long)shadow);
    free(rows); free(out); free(rays); free(u4); free(which); free(px); free(film);
    return 0;
}
