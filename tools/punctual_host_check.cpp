// punctual_host_check.cpp -- a stand-alone program for sanitiser runs of the host side of the punctual lights: it parses a scene.json
// with lights, runs the shared light-sampling text (device/dpunct.h) through akr_host_light_sample and exercises the setters. No GPU is opened.
// Build and run, from the repository root after the in-tree build (python -m akari_render_amd.build):
//   F="--offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fno-fast-math -fno-slp-vectorize -x hip -DAKR_TEST_HOOKS=1 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
//   mkdir -p build/asan && for f in akari_render_amd/csrc/host/*.cpp; do [ $(basename $f) = cli_main.cpp ] || hipcc $F -c $f -I akari_render_amd/csrc -I akari_render_amd/build/gen -o build/asan/$(basename $f).o; done
//   hipcc $F -c tools/punctual_host_check.cpp -I include -o build/asan/main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined build/asan/*.o akari_render_amd/build/obj/*.hip.o -ldl -o build/asan/punctual_host_check && build/asan/punctual_host_check scene.json
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "akari_hip.h"
#include "akari_hip_test.h"
int main(int argc, char** argv) {
    if (argc < 2) { std::fputs("usage: punctual_host_check <scene.json>\n", stderr); return 2; }
    akr_scene* sc = nullptr;
    if (akr_scene_load(nullptr, argv[1], 0, 0, &sc) != AKR_OK) { std::fprintf(stderr, "load: %s\n", akr_last_error()); return 1; }
    uint32_t n_lights = 0;
    akr_scene_punctual_light_count(sc, &n_lights);
    const uint32_t n = 4096;
    std::vector<float> rows(7 * n), out(13 * n);
    std::vector<uint32_t> light(n);
    unsigned s = 12345;
    auto rnd = [&] { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f; };
    for (uint32_t i = 0; i < n; i++) {
        float* r = &rows[7 * i];
        r[0] = 2 * rnd() - 1; r[1] = 2 * rnd() - 1; r[2] = 0.0f; r[3] = 0; r[4] = 0; r[5] = 1; r[6] = rnd();
    }
    if (akr_host_light_sample(sc, n, rows.data(), out.data(), light.data()) != AKR_OK) { std::fprintf(stderr, "sample: %s\n", akr_last_error()); return 1; }
    uint32_t valid = 0;
    for (uint32_t i = 0; i < n; i++) valid += out[13 * i + 11] != 0.0f;
    akr_punctual_light_desc extra = {AKR_LIGHT_SPOT, {0, 0, 2}, {0, 0, -1}, {1, 1, 1}, 1.0f, 0.4f, 0.2f};
    if (akr_scene_add_punctual_light(sc, &extra) != AKR_OK || akr_scene_clear_punctual_lights(sc) != AKR_OK) { std::fprintf(stderr, "setters: %s\n", akr_last_error()); return 1; }
    std::printf("%u lights, %u of %u samples valid\n", n_lights, valid, n);
    akr_scene_destroy(sc);
    return 0;
}
