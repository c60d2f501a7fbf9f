// projection_host_check.cpp -- a stand-alone program for sanitiser runs of the host side of the camera projections: it loads one
// scene.json per camera type, runs the setters with good and bad values, and draws 4096 rays per file through the shared ray-generation text
// (device/dpath.h generate_ray_lens_from) with akr_host_lens_ray. No GPU is opened.
// Build and run, from the repository root after the in-tree build (python -m akari_render_amd.build):
//   F="--offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fno-fast-math -fno-slp-vectorize -x hip -DAKR_TEST_HOOKS=1 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
//   mkdir -p build/asan && for f in akari_render_amd/csrc/host/*.cpp; do [ $(basename $f) = cli_main.cpp ] || hipcc $F -c $f -I akari_render_amd/csrc -I akari_render_amd/build/gen -o build/asan/$(basename $f).o; done
//   hipcc $F -c tools/projection_host_check.cpp -I include -o build/asan/main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined build/asan/*.o $(ls akari_render_amd/build/obj/*.o | grep -v '\.cpp\.o$') -ldl -o build/asan/projection_host_check
//   (the device objects of the in-tree build, the pt units among them; the host objects are the sanitised ones)
//   build/asan/projection_host_check perspective.json orthographic.json panorama.json
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>
#include "akari_hip.h"
#include "akari_hip_test.h"

static int fails = 0;
static void expect(bool ok, const char* what) {
    if (!ok) { std::fprintf(stderr, "FAILED: %s (%s)\n", what, akr_last_error()); fails++; }
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fputs("usage: projection_host_check <scene.json> [<scene.json> ...]   (one per camera type)\n", stderr); return 2; }
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (int f = 1; f < argc; f++) {
        akr_scene* sc = nullptr;
        if (akr_scene_load(nullptr, argv[f], 0, 0, &sc) != AKR_OK) { std::fprintf(stderr, "load %s: %s\n", argv[f], akr_last_error()); return 1; }
        akr_projection_desc loaded, d, got;
        expect(akr_scene_get_projection(sc, &loaded) == AKR_OK, "get");
        akr_scene_info info;
        akr_scene_get_info(sc, &info);
        // the setters with bad values: each refused, the state unchanged
        const akr_projection_desc bad[] = {
            {3u, 1.0f, -1.0f, 1.0f, -1.0f, 1.0f}, {AKR_PROJECTION_ORTHOGRAPHIC, 0.0f, -1.0f, 1.0f, -1.0f, 1.0f}, {AKR_PROJECTION_ORTHOGRAPHIC, nan, -1.0f, 1.0f, -1.0f, 1.0f},
            {AKR_PROJECTION_ORTHOGRAPHIC, -inf, -1.0f, 1.0f, -1.0f, 1.0f}, {AKR_PROJECTION_PANORAMA, 1.0f, 1.0f, 1.0f, -1.0f, 1.0f}, {AKR_PROJECTION_PANORAMA, 1.0f, -4.0f, 1.0f, -1.0f, 1.0f},
            {AKR_PROJECTION_PANORAMA, 1.0f, -1.0f, nan, -1.0f, 1.0f}, {AKR_PROJECTION_PANORAMA, 1.0f, -1.0f, 1.0f, -2.0f, 1.0f}, {AKR_PROJECTION_PANORAMA, 1.0f, -1.0f, 1.0f, 0.5f, 0.25f},
            {AKR_PROJECTION_PANORAMA, 1.0f, -1.0f, 1.0f, -1.0f, inf}};
        for (const akr_projection_desc& b : bad) {
            expect(akr_scene_set_projection(sc, &b) == AKR_ERR_INVALID_ARGUMENT, "a bad projection is refused");
            expect(akr_scene_get_projection(sc, &got) == AKR_OK && got.type == loaded.type && got.ortho_scale == loaded.ortho_scale && got.longitude_min == loaded.longitude_min,
                   "a refused call changes nothing");
        }
        expect(akr_scene_set_projection(nullptr, &loaded) == AKR_ERR_INVALID_ARGUMENT && akr_scene_get_projection(sc, nullptr) == AKR_ERR_INVALID_ARGUMENT &&
                   akr_projection_desc_default(nullptr) == AKR_ERR_INVALID_ARGUMENT, "NULL arguments");
        // 4096 rays through the file's own camera, then through every other projection (an orthographic film small enough for any tree), with and without a lens
        const uint32_t n = 4096;
        std::vector<uint32_t> pixels(2 * n);
        std::vector<float> u(4 * n), out(6 * n);
        unsigned s = 12345u + (unsigned)f;
        auto rnd = [&] { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f; };
        for (uint32_t i = 0; i < n; i++) {
            pixels[2 * i] = (uint32_t)(rnd() * (float)info.width) % info.width;
            pixels[2 * i + 1] = (uint32_t)(rnd() * (float)info.height) % info.height;
            for (int k = 0; k < 4; k++) u[4 * i + k] = rnd();
        }
        u[0] = u[1] = 0.0f;  // the Gaussian filter's log(0)
        uint32_t finite = 0, rays = 0;
        for (int pass = 0; pass < 6; pass++) {
            akr_projection_desc_default(&d);
            if (pass == 0) d = loaded;
            else if (pass <= 2) { d.type = AKR_PROJECTION_ORTHOGRAPHIC; d.ortho_scale = 1e-3f; }
            else if (pass == 3) d.type = AKR_PROJECTION_PANORAMA;
            else if (pass == 4) { d.type = AKR_PROJECTION_PANORAMA; d.longitude_min = -0.5f; d.longitude_max = 2.0f; d.latitude_min = -0.25f; }
            expect(akr_scene_set_lens(sc, nullptr) == AKR_OK, "remove the lens");
            expect(akr_scene_set_projection(sc, pass == 5 ? nullptr : &d) == AKR_OK, "set a good projection");
            if (pass == 2 || pass == 5) {
                const akr_lens_desc lens = {1e-4f, 2.0f};
                expect(akr_scene_set_lens(sc, &lens) == AKR_OK, "a lens on an orthographic / a perspective camera");
            }
            if (pass == 3) {
                const akr_lens_desc lens = {1e-4f, 2.0f};
                expect(akr_scene_set_lens(sc, &lens) == AKR_ERR_INVALID_ARGUMENT, "a lens on a panorama is refused");
            }
            for (uint32_t filter = 0; filter < 2; filter++) {
                if (akr_host_lens_ray(sc, filter, filter ? 1.5f : 0.5f, n, pixels.data(), u.data(), out.data()) != AKR_OK) { std::fprintf(stderr, "rays: %s\n", akr_last_error()); return 1; }
                for (uint32_t i = 0; i < 6 * n; i++) finite += std::isfinite(out[i]) ? 1u : 0u;
                rays += n;
            }
        }
        expect(finite == 6 * rays, "every ray is finite");
        std::printf("%s: projection %u as loaded, %u rays, %u of %u numbers finite\n", argv[f], loaded.type, rays, finite, 6 * rays);
        akr_scene_destroy(sc);
    }
    if (fails) { std::fprintf(stderr, "%d checks failed\n", fails); return 1; }
    std::puts("ok");
    return 0;
}
