/* oracle_light_tree_check.c -- a stand-alone run of the CPU oracle's light tree (oracle/or_lighttree.h, the light list of oracle/akr_oracle.c;
 * DESIGN.md 4.16) for the host sanitisers. CPU only, its own main, never loaded into Python. For L = 2, 3, 5, 8, 33 and 257 it fills a 16 x 16 scene
 * (a floor, an emitter) with L point and spot lights (soft radii, repeated positions, a sun between them), reads the node words, walks 4096 rows
 * through or_light_tree_sample_many (p on a light and 10^6 units away among them), renders a film under two colour pipelines, switches the mode off
 * and on, clears and refills. From the repository root:
 *
 *   mkdir -p build && gcc -std=gnu11 -O1 -g -fno-omit-frame-pointer -ffp-contract=off -fno-fast-math -fsanitize=address,undefined \
 *       -fno-sanitize-recover=undefined -pthread -Ioracle tools/oracle_light_tree_check.c oracle/akr_oracle.c -lm -o build/oracle_light_tree_check \
 *       && build/oracle_light_tree_check
 *
 * It prints one summary line and exits 0; a sanitiser report ends it with a non-zero status.
 */
#include "or_api.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef struct or_scene_s or_scene;
or_scene *or_scene_create(const or_scene_desc *d);
void or_scene_destroy(or_scene *sc);
int or_pt_render(const or_scene *sc, const or_pt_config *cfg, float *film, uint64_t *states_io, uint32_t n_threads, or_stats *stats_out);
int or_scene_set_punctual_lights(or_scene *sc, const or_punctual_light_desc *lights, uint32_t n);
uint32_t or_scene_num_lights(const or_scene *sc);
void or_scene_set_color(or_scene *sc, uint32_t color);

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "oracle_light_tree_check: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

static uint32_t g_rng = 2024u;
static float rnd(void) { g_rng = g_rng * 1664525u + 1013904223u; return (float)(g_rng >> 8) * (1.0f / 16777216.0f); }

int main(void) {
    static const float floor_v[12] = {-1, -1, 0, 1, -1, 0, 1, 1, 0, -1, 1, 0};
    static const float light_v[12] = {-0.8f, -0.2f, 0.9f, -0.4f, -0.2f, 0.9f, -0.4f, 0.2f, 0.9f, -0.8f, 0.2f, 0.9f};
    static const uint32_t up[6] = {0, 1, 2, 0, 2, 3}, down[6] = {0, 2, 1, 0, 3, 2};
    or_mesh_desc meshes[2];
    memset(meshes, 0, sizeof meshes);
    meshes[0].n_vertices = meshes[1].n_vertices = 4; meshes[0].n_triangles = meshes[1].n_triangles = 2;
    meshes[0].vertices = floor_v; meshes[0].indices = up; meshes[1].vertices = light_v; meshes[1].indices = down;
    or_material_desc mats[2];
    memset(mats, 0, sizeof mats);
    mats[0].kind = OR_MAT_DIFFUSE; mats[0].base_color[0] = 0.7f; mats[0].base_color[1] = 0.6f; mats[0].base_color[2] = 0.5f; mats[0].base_alpha = 1.0f;
    mats[1].kind = OR_MAT_EMISSION; mats[1].emission_color[0] = 4.0f; mats[1].emission_color[1] = 3.0f; mats[1].emission_color[2] = 2.0f; mats[1].emission_strength = 1.0f;
    static const uint32_t slot[2] = {0, 1};
    or_instance_desc insts[2];
    memset(insts, 0, sizeof insts);
    for (int i = 0; i < 2; i++) {
        insts[i].mesh = (uint32_t)i; insts[i].n_materials = 1; insts[i].materials = &slot[i];
        insts[i].transform[0] = insts[i].transform[5] = insts[i].transform[10] = insts[i].transform[15] = 1.0f;
    }
    static float table[4096];
    for (int i = 0; i < 4096; i++) table[i] = 0.5f;
    or_scene_desc sd;
    memset(&sd, 0, sizeof sd);
    sd.n_meshes = sd.n_instances = sd.n_materials = 2;
    sd.meshes = meshes; sd.instances = insts; sd.materials = mats; sd.ggx_dielectric_table = table;
    sd.camera.c2w[0] = sd.camera.c2w[5] = sd.camera.c2w[10] = sd.camera.c2w[15] = 1.0f;
    sd.camera.c2w[14] = 3.0f;
    sd.camera.fov = 0.7f; sd.camera.width = sd.camera.height = 16;
    or_scene *sc = or_scene_create(&sd);
    CHECK(sc && or_scene_num_lights(sc) == 1);

    enum { N = 4096, LMAX = 257 };
    static const uint32_t sizes[6] = {2, 3, 5, 8, 33, 257};
    or_punctual_light_desc *L = (or_punctual_light_desc *)calloc(LMAX + 1, sizeof *L);
    uint32_t *words = (uint32_t *)malloc(4 * 8 * (2 * LMAX - 1)), *which = (uint32_t *)malloc(4 * N), *record = (uint32_t *)malloc(4 * N);
    float *rows = (float *)malloc(sizeof(float) * 9 * N), *out = (float *)malloc(sizeof(float) * 13 * N), *film = (float *)calloc(7 * 256, sizeof(float));
    or_pt_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.spp = 4; cfg.spp_per_pass = 4; cfg.max_depth = 4; cfg.rr_depth = 2; cfg.use_nee = 1; cfg.debug_depth = -1;
    cfg.filter_type = OR_FILTER_GAUSSIAN; cfg.filter_radius = 1.5f; cfg.sampler_seed = 3; cfg.shard_count = 1;
    unsigned long long walked = 0, shadow = 0;
    for (int s = 0; s < 6; s++) {
        const uint32_t n = sizes[s];
        for (uint32_t k = 0; k <= n; k++) {
            or_punctual_light_desc *l = &L[k];
            memset(l, 0, sizeof *l);
            l->color[0] = 2.0f; l->color[1] = 1.0f; l->color[2] = 1.5f; l->strength = 0.5f + 3.0f * rnd();
            if (k == 1) { l->type = OR_LIGHT_SUN; l->direction[0] = 0.2f; l->direction[1] = -0.1f; l->direction[2] = -1.0f; continue; } /* between the local lights */
            l->type = k % 4 == 3 ? OR_LIGHT_SPOT : OR_LIGHT_POINT;
            if (k >= 5 && k % 5 == 0) memcpy(l->position, L[k - 2].position, 12); /* a repeated position: the order falls to the index */
            else { l->position[0] = 2.0f * rnd() - 1.0f; l->position[1] = 2.0f * rnd() - 1.0f; l->position[2] = 0.2f + 1.3f * rnd(); }
            if (l->type == OR_LIGHT_SPOT) { l->direction[0] = 0.1f; l->direction[1] = -0.2f; l->direction[2] = -1.0f; l->cone_angle = 0.6f; l->blend = 0.3f; }
            if (k % 3 == 2) l->radius = 0.02f + 0.28f * rnd();
        }
        or_scene_set_light_tree(sc, s % 2);            /* the mode before the lights, and after them */
        CHECK(or_scene_set_punctual_lights(sc, L, n + 1) == 0);
        or_scene_set_light_tree(sc, 1);
        uint32_t on = 0, n_nodes = 0;
        or_scene_get_light_tree(sc, &on, &n_nodes);
        CHECK(on == 1 && n_nodes == 2 * n - 1 && or_scene_light_tree_nodes(sc, words) == n_nodes && or_scene_num_lights(sc) == 3);
        uint32_t leaves = 0;
        for (uint32_t k = 0; k < n_nodes; k++) {
            const uint32_t c = words[8 * k + 7];
            if (c & 0x80000000u) { leaves++; CHECK((c & 0x7fffffffu) <= n && (c & 0x7fffffffu) != 1); }
            else CHECK(c > k && c + 1 < n_nodes);
        }
        CHECK(leaves == n);
        for (int i = 0; i < N; i++) {
            float *r = rows + 9 * i;
            r[0] = 2.0f * rnd() - 1.0f; r[1] = 2.0f * rnd() - 1.0f; r[2] = 0.4f * rnd() - 0.2f;
            r[3] = 0.0f; r[4] = 0.0f; r[5] = 1.0f; r[6] = rnd(); r[7] = rnd(); r[8] = rnd();
        }
        memcpy(rows, L[0].position, 12);                              /* p on a light */
        rows[9] = 1e6f; rows[10] = -1e6f; rows[11] = 1e6f;            /* p 10^6 units away */
        rows[18 + 6] = 0.0f; rows[27 + 6] = 0x1.fffffep-1f;           /* u_select = 0 and the largest float below 1 */
        for (uint32_t color = 0; color < 4; color += 3) {
            or_scene_set_color(sc, color);
            CHECK(or_light_tree_sample_many(sc, N, rows, out, which, record) == 0);
        }
        or_scene_set_color(sc, 0);
        for (int i = 0; i < N; i++) {
            CHECK(which[i] < 3 && ((which[i] == 2) == (record[i] != 0xffffffffu)) && (record[i] == 0xffffffffu || (record[i] <= n && record[i] != 1)));
            walked += which[i] == 2; /* emitter, sun, tree */
        }
        or_stats st;
        for (uint32_t color = 0; color < 4; color += 3) {
            cfg.color = color;
            CHECK(or_pt_render(sc, &cfg, film, 0, 2, &st) == 0 && st.n_samples == 256 * 4 && st.n_shadow > 0 && st.n_shadow <= st.n_shaded);
            shadow += st.n_shadow;
        }
        for (int i = 0; i < 7 * 256; i++) CHECK(isfinite(film[i]));
        /* off: every light an entry of its own, no node; on again; cleared: no tree, the mode stays */
        or_scene_set_light_tree(sc, 0);
        or_scene_get_light_tree(sc, &on, &n_nodes);
        CHECK(on == 0 && n_nodes == 0 && or_scene_light_tree_nodes(sc, words) == 0 && or_scene_num_lights(sc) == n + 2);
        CHECK(or_light_tree_sample_many(sc, N, rows, out, which, record) == 0 && record[5] == 0xffffffffu);
        or_scene_set_light_tree(sc, 1);
        CHECK(or_scene_set_punctual_lights(sc, 0, 0) == 0 && or_scene_num_lights(sc) == 1);
        or_scene_get_light_tree(sc, &on, &n_nodes);
        CHECK(on == 1 && n_nodes == 0);
        CHECK(or_scene_set_punctual_lights(sc, L, 1) == 0 && or_scene_num_lights(sc) == 2); /* one local light: no tree */
        or_scene_get_light_tree(sc, &on, &n_nodes);
        CHECK(n_nodes == 0 && or_pt_render(sc, &cfg, film, 0, 2, &st) == 0);
    }
    or_scene_destroy(sc);
    printf("oracle_light_tree_check: 6 trees, %llu of %d rows walked one, %llu shadow rays in 12 renders, ok\n", walked, 6 * N, shadow);
    free(L); free(words); free(which); free(record); free(rows); free(out); free(film);
    return 0;
}
