// soft_light_host_check.cpp -- a stand-alone program for sanitiser runs of the host side of the soft punctual lights: it parses a
// scene.json with one soft light of each kind ("radius" on a point and a spot light, "angle" on a sun), runs the shared light-sampling text
// (device/dpunct.h) through akr_host_light_sample_soft and exercises the setters, the getter and option soft_lights. No GPU is opened.
// Build and run as tools/punctual_host_check.cpp (its header has the recipe), with this file in place of that one:
//   hipcc $F -c tools/soft_light_host_check.cpp -I include -o build/asan/main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined build/asan/*.o akari_render_amd/build/obj/*.hip.o -ldl -o build/asan/soft_light_host_check && build/asan/soft_light_host_check scene.json
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "akari_hip.h"
#include "akari_hip_test.h"
int main(int argc, char** argv) {
    if (argc < 2) { std::fputs("usage: soft_light_host_check <scene.json>\n", stderr); return 2; }
    akr_scene* sc = nullptr;
    if (akr_scene_load(nullptr, argv[1], 0, 0, &sc) != AKR_OK) { std::fprintf(stderr, "load: %s\n", akr_last_error()); return 1; }
    uint32_t n_lights = 0, n_soft = 0;
    akr_scene_punctual_light_count(sc, &n_lights);
    for (uint32_t i = 0; i < n_lights; i++) {
        akr_punctual_light_desc d;
        if (akr_scene_get_punctual_light(sc, i, &d) != AKR_OK) { std::fprintf(stderr, "get: %s\n", akr_last_error()); return 1; }
        n_soft += d.radius > 0.0f || d.angle > 0.0f;
    }
    const uint32_t n = 4096;
    std::vector<float> rows(9 * n), out(13 * n);
    std::vector<uint32_t> light(n);
    unsigned s = 12345;
    auto rnd = [&] { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f; };
    for (uint32_t i = 0; i < n; i++) {
        float* r = &rows[9 * i];
        r[0] = 2 * rnd() - 1; r[1] = 2 * rnd() - 1; r[2] = 0.0f; r[3] = 0; r[4] = 0; r[5] = 1; r[6] = rnd(); r[7] = rnd(); r[8] = rnd();
    }
    if (akr_host_light_sample_soft(sc, n, rows.data(), out.data(), light.data()) != AKR_OK) { std::fprintf(stderr, "sample: %s\n", akr_last_error()); return 1; }
    uint32_t valid = 0;
    for (uint32_t i = 0; i < n; i++) valid += out[13 * i + 11] != 0.0f;
    // the setters: a soft light of each kind, the values that are refused, the size the kind does not read
    akr_punctual_light_desc spot = {AKR_LIGHT_SPOT, {0, 0, 2}, {0, 0, -1}, {1, 1, 1}, 1.0f, 0.4f, 0.2f, 0.25f, 9.0f};
    akr_punctual_light_desc sun = {AKR_LIGHT_SUN, {0, 0, 0}, {0, 0, -1}, {1, 1, 1}, 1.0f, 0.0f, 0.0f, NAN, 0.5f};
    akr_punctual_light_desc bad_radius = spot, bad_angle = sun;
    bad_radius.radius = -1.0f;
    bad_angle.angle = 3.14159274f;
    if (akr_scene_add_punctual_light(sc, &spot) != AKR_OK || akr_scene_add_punctual_light(sc, &sun) != AKR_OK) { std::fprintf(stderr, "setters: %s\n", akr_last_error()); return 1; }
    if (akr_scene_add_punctual_light(sc, &bad_radius) != AKR_ERR_INVALID_ARGUMENT || akr_scene_add_punctual_light(sc, &bad_angle) != AKR_ERR_INVALID_ARGUMENT) { std::fputs("a bad size was accepted\n", stderr); return 1; }
    akr_punctual_light_desc back;
    if (akr_scene_get_punctual_light(sc, n_lights, &back) != AKR_OK || back.radius != 0.25f || back.angle != 0.0f) { std::fputs("getter\n", stderr); return 1; }
    if (akr_host_light_sample_soft(sc, n, rows.data(), out.data(), light.data()) != AKR_OK) { std::fprintf(stderr, "sample: %s\n", akr_last_error()); return 1; }
    if (akr_scene_clear_punctual_lights(sc) != AKR_OK) { std::fprintf(stderr, "clear: %s\n", akr_last_error()); return 1; }
    akr_scene_destroy(sc);
    // option soft_lights = 0: the same file, every light a delta light
    akr_scene* hard = nullptr;
    if (akr_option_set("soft_lights", 0) != AKR_OK || akr_scene_load(nullptr, argv[1], 0, 0, &hard) != AKR_OK) { std::fprintf(stderr, "load (soft_lights = 0): %s\n", akr_last_error()); return 1; }
    uint32_t n_hard = 0, n_hard_soft = 0;
    akr_scene_punctual_light_count(hard, &n_hard);
    for (uint32_t i = 0; i < n_hard; i++) {
        akr_scene_get_punctual_light(hard, i, &back);
        n_hard_soft += back.radius > 0.0f || back.angle > 0.0f;
    }
    akr_scene_destroy(hard);
    if (n_hard != n_lights || n_hard_soft != 0) { std::fputs("soft_lights = 0 kept a size\n", stderr); return 1; }
    std::printf("%u lights, %u of them soft, %u of %u samples valid\n", n_lights, n_soft, valid, n);
    return 0;
}
