// light_tree_host_check.cpp -- a stand-alone program for sanitiser runs of the host side of the light tree: it loads a scene.json, and for
// L = 2, 3, 5, 8, 33 and 257 point / spot lights (some soft, some at repeated positions, a sun between them) builds the tree through the setters, reads the
// node words back, walks 4096 rows through the shared text (device/dlighttree.h) with akr_host_light_tree_sample, and switches the mode off and on, clears
// and re-adds under it. No GPU is opened.
// Build and run as tools/punctual_host_check.cpp (its header has the recipe), with this file in place of that one:
//   hipcc $F -c tools/light_tree_host_check.cpp -I include -o build/asan/main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined build/asan/*.o akari_render_amd/build/obj/*.hip.o -ldl -o build/asan/light_tree_host_check && build/asan/light_tree_host_check scene.json
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "akari_hip.h"
#include "akari_hip_test.h"
#define CHECK(call) do { if ((call) != AKR_OK) { std::fprintf(stderr, "%s: %s\n", #call, akr_last_error()); return 1; } } while (0)
int main(int argc, char** argv) {
    if (argc < 2) { std::fputs("usage: light_tree_host_check <scene.json>\n", stderr); return 2; }
    unsigned s = 12345;
    auto rnd = [&] { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f; };
    const uint32_t n = 4096;
    std::vector<float> rows(9 * n), out(13 * n);
    std::vector<uint32_t> light(n), record(n);
    for (uint32_t i = 0; i < n; i++) {
        float* r = &rows[9 * i];
        r[0] = 2 * rnd() - 1; r[1] = 2 * rnd() - 1; r[2] = 0.0f; r[3] = 0; r[4] = 0; r[5] = 1; r[6] = rnd(); r[7] = rnd(); r[8] = rnd();
    }
    rows[6] = 0.0f;
    rows[9 + 6] = 0.99999994f;
    CHECK(akr_option_set("light_tree", 1));
    uint64_t walked = 0;
    for (uint32_t count : {2u, 3u, 5u, 8u, 33u, 257u}) {
        akr_scene* sc = nullptr;
        CHECK(akr_scene_load(nullptr, argv[1], 0, 0, &sc));
        CHECK(akr_scene_clear_punctual_lights(sc));
        std::vector<akr_punctual_light_desc> lights;
        for (uint32_t k = 0; k < count; k++) {
            akr_punctual_light_desc d = {k % 4 == 3 ? AKR_LIGHT_SPOT : AKR_LIGHT_POINT, {2 * rnd() - 1, 2 * rnd() - 1, 0.2f + rnd()}, {0.1f, -0.2f, -1.0f}, {1, 2, 0.5f}, 0.5f + rnd(), 0.6f, 0.3f,
                                         k % 3 == 1 ? 0.05f + 0.2f * rnd() : 0.0f, 0.0f};
            if (k % 5 == 4) for (int a = 0; a < 3; a++) d.position[a] = lights[k - 1].position[a];  // a repeated position: the tie goes to the index
            lights.push_back(d);
            CHECK(akr_scene_add_punctual_light(sc, &d));
            if (k == 0) {
                akr_punctual_light_desc sun = {AKR_LIGHT_SUN, {0, 0, 0}, {0, 0, -1}, {1, 1, 1}, 1.0f, 0.0f, 0.0f, 0.0f, 0.1f};
                CHECK(akr_scene_add_punctual_light(sc, &sun));
            }
        }
        uint32_t on = 0, n_nodes = 0;
        CHECK(akr_scene_get_light_tree(sc, &on, &n_nodes));
        const void* words = nullptr;
        uint64_t bytes = 0;
        CHECK(akr_scene_get_array(sc, AKR_ARRAY_LIGHT_TREE, &words, &bytes));
        if (on != 1 || n_nodes != 2 * count - 1 || bytes != 32ull * n_nodes) { std::fprintf(stderr, "%u lights: %u nodes, %llu bytes\n", count, n_nodes, (unsigned long long)bytes); return 1; }
        uint64_t sum = 0;
        for (uint64_t w = 0; w < bytes / 4; w++) sum += ((const uint32_t*)words)[w];  // every word is read
        CHECK(akr_host_light_tree_sample(sc, n, rows.data(), out.data(), light.data(), record.data()));
        for (uint32_t i = 0; i < n; i++) {
            if (record[i] != 0xFFFFFFFFu && record[i] > count) { std::fprintf(stderr, "row %u: record %u\n", i, record[i]); return 1; }
            walked += record[i] != 0xFFFFFFFFu;
        }
        // the setters: off (every light an entry of its own), on again, the existing hook on both, cleared and refilled under the mode
        CHECK(akr_scene_set_light_tree(sc, 0));
        CHECK(akr_scene_get_light_tree(sc, &on, &n_nodes));
        if (on != 0 || n_nodes != 0) { std::fputs("mode 0 kept a tree\n", stderr); return 1; }
        CHECK(akr_host_light_tree_sample(sc, n, rows.data(), out.data(), light.data(), record.data()));
        CHECK(akr_host_light_sample_soft(sc, n, rows.data(), out.data(), light.data()));
        CHECK(akr_scene_set_light_tree(sc, 1));
        CHECK(akr_host_light_sample_soft(sc, n, rows.data(), out.data(), light.data()));
        CHECK(akr_scene_clear_punctual_lights(sc));
        CHECK(akr_scene_get_light_tree(sc, &on, &n_nodes));
        if (on != 1 || n_nodes != 0) { std::fputs("a cleared scene kept a tree\n", stderr); return 1; }
        CHECK(akr_scene_add_punctual_light(sc, &lights[0]));
        CHECK(akr_scene_add_punctual_light(sc, &lights[1]));
        CHECK(akr_scene_get_light_tree(sc, &on, &n_nodes));
        if (n_nodes != 3) { std::fputs("two lights: not three nodes\n", stderr); return 1; }
        CHECK(akr_host_light_tree_sample(sc, n, rows.data(), out.data(), light.data(), record.data()));
        akr_scene_destroy(sc);
        (void)sum;
    }
    std::printf("6 trees, %llu of %u rows walked one\n", (unsigned long long)walked, 6 * n);
    return 0;
}
