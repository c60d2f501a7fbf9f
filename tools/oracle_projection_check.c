/* oracle_projection_check.c -- a stand-alone program for sanitiser runs of the oracle's camera projections (oracle/akr_oracle.c: or_scene_set_projection,
 * or_projection_fold, or_camera_ray). It builds a closed box with an emitter around the camera, runs the setters with good and bad values
 * and NULLs, a lens on a panorama both ways round, the resolution setter, draws rays through or_lens_ray_many for every projection and both filters (u = 0
 * of the Gaussian filter among them: log(0)), and renders a small pt and aov film per projection. CPU only; nothing here opens a GPU or is loaded into Python.
 * Build and run, from the repository root:
 *   gcc -std=gnu11 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -I oracle \
 *       tools/oracle_projection_check.c oracle/akr_oracle.c -lm -o /tmp/oracle_projection_check && /tmp/oracle_projection_check */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "or_api.h"

struct or_scene_s *or_scene_create(const or_scene_desc *d);
void or_scene_destroy(struct or_scene_s *sc);
int or_scene_set_projection(struct or_scene_s *sc, const or_projection_desc *d);
void or_scene_get_projection(const struct or_scene_s *sc, or_projection_desc *out);
int or_scene_set_resolution(struct or_scene_s *sc, uint32_t width, uint32_t height);
int or_scene_set_lens(struct or_scene_s *sc, const or_lens_desc *d);
int or_lens_ray_many(const struct or_scene_s *sc, uint32_t filter_type, float filter_radius, uint32_t n, const uint32_t *pixels2, const float *u4, float *out6);
int or_pt_render(const struct or_scene_s *sc, const or_pt_config *cfg, float *film, uint64_t *states_io, uint32_t n_threads, or_stats *stats_out);
void or_init_pcg32_buffer_with_seed(uint64_t count, uint64_t seed, uint64_t *states);
uint32_t or_sizeof_projection_desc(void);

static int fails = 0;
static void expect(int ok, const char *what) {
    if (!ok) { fprintf(stderr, "FAILED: %s\n", what); fails++; }
}

int main(void) {
    /* a box [-2, 2]^3 (12 triangles) and a small emitter under its top */
    static const float box_v[8 * 3] = {-2, -2, -2, 2, -2, -2, 2, 2, -2, -2, 2, -2, -2, -2, 2, 2, -2, 2, 2, 2, 2, -2, 2, 2};
    static const uint32_t box_i[12 * 3] = {0, 1, 2, 0, 2, 3, 4, 6, 5, 4, 7, 6, 0, 4, 5, 0, 5, 1, 3, 2, 6, 3, 6, 7, 0, 3, 7, 0, 7, 4, 1, 5, 6, 1, 6, 2};
    static const float em_v[4 * 3] = {-0.5f, 1.75f, -0.5f, 0.5f, 1.75f, -0.5f, 0.5f, 1.75f, 0.5f, -0.5f, 1.75f, 0.5f};
    static const uint32_t em_i[2 * 3] = {0, 1, 2, 0, 2, 3};
    or_mesh_desc meshes[2];
    memset(meshes, 0, sizeof meshes);
    meshes[0].n_vertices = 8; meshes[0].n_triangles = 12; meshes[0].vertices = box_v; meshes[0].indices = box_i;
    meshes[1].n_vertices = 4; meshes[1].n_triangles = 2; meshes[1].vertices = em_v; meshes[1].indices = em_i;
    or_material_desc mats[2];
    memset(mats, 0, sizeof mats);
    mats[0].kind = OR_MAT_DIFFUSE; mats[0].base_color[0] = 0.7f; mats[0].base_color[1] = 0.6f; mats[0].base_color[2] = 0.5f; mats[0].base_alpha = 1.0f;
    mats[1].kind = OR_MAT_EMISSION; mats[1].base_alpha = 1.0f; mats[1].emission_strength = 4.0f;
    mats[1].emission_color[0] = mats[1].emission_color[1] = mats[1].emission_color[2] = 1.0f;
    static const uint32_t slot0[1] = {0}, slot1[1] = {1};
    or_instance_desc insts[2];
    memset(insts, 0, sizeof insts);
    for (int i = 0; i < 2; i++) {
        insts[i].mesh = (uint32_t)i; insts[i].n_materials = 1; insts[i].materials = i ? slot1 : slot0;
        insts[i].transform[0] = insts[i].transform[5] = insts[i].transform[10] = insts[i].transform[15] = 1.0f;
    }
    const float nan = NAN, inf = INFINITY;
    for (int rotated = 0; rotated < 2; rotated++) {
        or_scene_desc sd;
        memset(&sd, 0, sizeof sd);
        sd.n_meshes = 2; sd.n_instances = 2; sd.n_materials = 2;
        sd.meshes = meshes; sd.instances = insts; sd.materials = mats;
        sd.camera.fov = 0.9f; sd.camera.width = 12; sd.camera.height = 8;
        sd.camera.c2w[0] = sd.camera.c2w[5] = sd.camera.c2w[10] = sd.camera.c2w[15] = 1.0f;
        if (rotated) { /* a quarter turn about y and a translation: the full camera -> world */
            memset(sd.camera.c2w, 0, sizeof sd.camera.c2w);
            sd.camera.c2w[2] = -1.0f; sd.camera.c2w[5] = 1.0f; sd.camera.c2w[8] = 1.0f; sd.camera.c2w[12] = 0.5f; sd.camera.c2w[14] = -0.25f; sd.camera.c2w[15] = 1.0f;
        }
        struct or_scene_s *sc = or_scene_create(&sd);
        expect(sc != 0 && or_sizeof_projection_desc() == 24, "create");
        const or_projection_desc good[] = {{OR_PROJECTION_ORTHOGRAPHIC, 2.5f, 0, 0, 0, 0}, {OR_PROJECTION_PANORAMA, 0, -3.14159274f, 3.14159274f, -1.57079637f, 1.57079637f},
                                           {OR_PROJECTION_PANORAMA, nan, 0.5f, 0.515625f, -0.375f, 1.25f}, {OR_PROJECTION_PERSPECTIVE, nan, nan, nan, nan, nan}};
        const or_projection_desc bad[] = {{3u, 1, -1, 1, -1, 1}, {0xffffffffu, 1, -1, 1, -1, 1}, {OR_PROJECTION_ORTHOGRAPHIC, 0, -1, 1, -1, 1}, {OR_PROJECTION_ORTHOGRAPHIC, nan, -1, 1, -1, 1},
                                          {OR_PROJECTION_ORTHOGRAPHIC, -inf, -1, 1, -1, 1}, {OR_PROJECTION_PANORAMA, 1, 1, 1, -1, 1}, {OR_PROJECTION_PANORAMA, 1, -4, 1, -1, 1},
                                          {OR_PROJECTION_PANORAMA, 1, -1, nan, -1, 1}, {OR_PROJECTION_PANORAMA, 1, -1, 1, -2, 1}, {OR_PROJECTION_PANORAMA, 1, -1, 1, 0.5f, 0.25f},
                                          {OR_PROJECTION_PANORAMA, 1, -1, 1, -1, inf}};
        enum { N = 4096 };
        uint32_t *px = (uint32_t *)malloc(sizeof(uint32_t) * 2 * N);
        float *u = (float *)malloc(sizeof(float) * 4 * N), *out = (float *)malloc(sizeof(float) * 6 * N);
        unsigned long long finite = 0, numbers = 0;
        for (size_t g = 0; g < sizeof good / sizeof good[0]; g++) {
            expect(or_scene_set_projection(sc, &good[g]) == 0, "a good description is accepted");
            or_projection_desc before, after;
            or_scene_get_projection(sc, &before);
            for (size_t b = 0; b < sizeof bad / sizeof bad[0]; b++) {
                expect(or_scene_set_projection(sc, &bad[b]) == -1, "a bad description is refused");
                or_scene_get_projection(sc, &after);
                expect(memcmp(&before, &after, sizeof before) == 0, "a refused call changes nothing");
            }
            const or_lens_desc lens = {0.125f, 1.75f};
            if (good[g].type == OR_PROJECTION_PANORAMA) expect(or_scene_set_lens(sc, &lens) == -1, "a panorama takes no lens");
            for (int with_lens = 0; with_lens < (good[g].type == OR_PROJECTION_PANORAMA ? 1 : 2); with_lens++) {
                expect(or_scene_set_lens(sc, with_lens ? &lens : 0) == 0, "lens");
                if (with_lens && good[g].type == OR_PROJECTION_ORTHOGRAPHIC) expect(or_scene_set_projection(sc, &good[1]) == -1, "a lens keeps the panorama out");
                for (int size = 0; size < 3; size++) {
                    const uint32_t w = size == 0 ? 12 : (size == 1 ? 1 : 7), h = size == 0 ? 8 : (size == 1 ? 1 : 15);
                    expect(or_scene_set_resolution(sc, w, h) == 0 && or_scene_set_resolution(sc, 0, h) == -1, "resolution");
                    srand(7);
                    for (int i = 0; i < N; i++) {
                        px[2 * i] = (uint32_t)rand() % w; px[2 * i + 1] = (uint32_t)rand() % h;
                        for (int k = 0; k < 4; k++) u[4 * i + k] = (float)(rand() % 16777216) / 16777216.0f;
                    }
                    u[0] = u[1] = 0.0f; u[4] = 0.0f; u[5] = 0.99999994f; u[10] = u[11] = 0.5f; /* log(0), the largest u, the lens's centre */
                    for (uint32_t ft = 0; ft < 2; ft++) {
                        expect(or_lens_ray_many(sc, ft, ft ? 1.5f : 0.5f, N, px, u, out) == 0, "rays");
                        for (int i = 0; i < 6 * N; i++) { numbers++; finite += isfinite(out[i]) ? 1u : 0u; }
                    }
                    expect(or_lens_ray_many(sc, 2u, 1.0f, N, px, u, out) == -1, "an unknown filter is refused");
                    /* a small render through the projection: pt, depth 3, both samplers that need no table */
                    or_pt_config cfg;
                    memset(&cfg, 0, sizeof cfg);
                    cfg.spp = 2; cfg.spp_per_pass = 2; cfg.max_depth = 3; cfg.rr_depth = 2; cfg.use_nee = 1; cfg.debug_depth = -1;
                    cfg.filter_type = OR_FILTER_GAUSSIAN; cfg.filter_radius = 1.5f; cfg.shard_count = 1; cfg.sampler_seed = 3;
                    for (uint32_t sampler = 0; sampler < 3; sampler += 2) {
                        cfg.sampler_type = sampler;
                        float *film = (float *)calloc(7u * w * h, sizeof(float));
                        uint64_t *states = (uint64_t *)calloc(2u * w * h, sizeof(uint64_t));
                        if (sampler == 0) or_init_pcg32_buffer_with_seed((uint64_t)w * h, 3, states);
                        else for (uint32_t i = 0; i < w * h; i++) { states[2 * i] = 0xffffffffull; states[2 * i + 1] = (i % w) | ((uint64_t)(i / w) << 32); }
                        or_stats st;
                        expect(or_pt_render(sc, &cfg, film, states, 2, &st) == 0 && st.n_samples == 2ull * w * h, "pt");
                        for (uint32_t i = 0; i < 7u * w * h; i++) { numbers++; finite += isfinite(film[i]) ? 1u : 0u; }
                        free(film); free(states);
                    }
                }
                expect(or_scene_set_resolution(sc, 12, 8) == 0, "resolution back");
            }
            expect(or_scene_set_lens(sc, 0) == 0, "lens off");
        }
        expect(or_scene_set_projection(sc, 0) == 0, "NULL resets");
        printf("%s c2w: %llu of %llu numbers finite\n", rotated ? "turned" : "identity", finite, numbers);
        expect(finite == numbers, "every ray and film value is finite");
        free(px); free(u); free(out);
        or_scene_destroy(sc);
    }
    printf(fails ? "%d check(s) failed\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
