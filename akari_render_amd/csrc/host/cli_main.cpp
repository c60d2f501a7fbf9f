// akari-cli -- the reference's command line (crates/akari_api/src/bin/akari_cli.rs:8-95) over libakari_hip.so:
//   akari-cli -s scene.json -m method.json [-d <hip device ordinal>] [-v] [--save-intermediate] [--save-stats NAME]
//             [--resolution WxH] [--independent-sampler] [--no-punctual-lights] [--no-soft-lights] [--light-tree] [--depth-of-field] [--lens-radius X] [--focal-distance Y] [--projection P] [--ortho-scale X] [--denoise [N]] [--denoise-variance] [--denoise-features]
//             [--adaptive [X]] [--adaptive-min-spp N] [--display [linear|reinhard|aces|hable]] [--exposure EV] [--auto-exposure] [--bloom [X]]
// -d accepts a HIP device ordinal (the reference's "cpu|cuda|dx|metal" back ends do not exist here; "hip" = 0).
// --gui is not supported. --independent-sampler renders method files that ask for pmj02bn (scenes/cbox/pt.json)
// with the independent sampler and the same seed. --depth-of-field (no reference counterpart: its camera ignores the lens it loads) renders
// through the thin lens of the scene file's focal_distance and fstop (library option "lens"); --lens-radius / --focal-distance override the file's values.
// --no-punctual-lights (library option "punctual_lights" = 0): the scene file's point, spot and sun lights are dropped, which is how the reference renders it.
// --no-soft-lights (library option "soft_lights" = 0): the file's lights are loaded with radius 0 and angle 0, so every shadow they cast has a hard edge.
// --light-tree (library option "light_tree" = 1): the file's point and spot lights are chosen among by a light tree, by power / distance^2.
// --denoise [N] (library option "denoise"): every pt task also writes {stem}.denoised{ext}, filtered with albedo / normal passes of N spp (16 when N is left out).
// --denoise-variance (library option "denoise_variance", with --denoise): the filter's colour weights come from the variance between the two halves of the task's passes.
// --denoise-features (library option "denoise_features"; implies the denoise step): the filter's albedo / normal guides are collected by the pt task's own samples,
// not by passes of their own; N of --denoise then only matters where the session cannot collect them.
// --adaptive [X] (library option "adaptive" = X * 1024; the library's default threshold when X is left out): pt tasks render adaptively, the task's spp the most a pixel
// gets; --adaptive-min-spp N (option "adaptive_min_spp"): the samples a tile receives before it may retire.
// --display [CURVE] (library option "display"; aces when CURVE is left out): every pt task also writes {stem}.display.png, its film (the denoised one with --denoise)
// through akr_display_transform; --exposure EV, --auto-exposure, --bloom [X] (options "display_exposure" = EV * 1024, "display_auto_exposure",
// "display_bloom" = X * 1024, 0.25 when X is left out) set that transform's fields and imply --display.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "akari_hip.h"

static void usage() {
    std::puts("Usage: akari-cli -s <SCENE> -m <METHOD> [-d <DEVICE>] [-v] [--save-intermediate] [--save-stats <NAME>]\n"
              "                 [--resolution <W>x<H>] [--independent-sampler] [--no-punctual-lights] [--no-soft-lights] [--light-tree] [--depth-of-field] [--lens-radius <X>] [--focal-distance <Y>] [--denoise [<N>]] [--denoise-variance] [--denoise-features]\n"
              "                 [--projection perspective|orthographic|panorama] [--ortho-scale <X>]\n"
              "                 [--adaptive [<X>]] [--adaptive-min-spp <N>]\n"
              "                 [--display [linear|reinhard|aces|hable]] [--exposure <EV>] [--auto-exposure] [--bloom [<X>]]\n"
              "  -s, --scene <SCENE>      Scene file to render (akari scene-graph JSON)\n"
              "  -m, --method <METHOD>    Render method config file (\"type\": \"pt\")\n"
              "  -d, --device <DEVICE>    HIP device ordinal (default 0)\n"
              "  -v, --verbose\n"
              "      --save-intermediate  write {name}-{spp}.exr after every pass\n"
              "      --save-stats <NAME>  write NAME.json (RenderStats) and use NAME for intermediate files\n"
              "      --no-punctual-lights drop the scene file's point, spot and sun lights (default: they light the scene)\n"
              "      --light-tree         choose among the scene file's point and spot lights with a light tree, by power / distance^2 (default: by power alone)\n"
              "      --no-soft-lights     load the scene file's lights with radius 0 and angle 0: hard shadows (default: soft shadows where the file gives a size)\n"
              "      --depth-of-field     render through the thin lens of the scene file's focal_distance and fstop (default: a pinhole)\n"
              "      --lens-radius <X>, --focal-distance <Y>  the lens's radius / distance of the plane of focus, instead of the file's\n"
              "      --projection <P>     the camera's projection instead of the scene file's: perspective, orthographic or panorama (equirectangular, the file's window or the full sphere)\n"
              "      --ortho-scale <X>    the world-space length the larger image side of an orthographic camera spans, instead of the file's\n"
              "      --denoise [<N>]      pt tasks also write {stem}.denoised{ext}: an edge-avoiding filter guided by albedo / normal passes of N spp (default 16)\n"
              "      --denoise-variance   with --denoise: per-pixel colour weights from the variance between the two halves of the passes (needs spp > spp_per_pass)\n"
              "      --denoise-features   the denoise step (implied) takes its albedo / normal guides from the pt task's own samples instead of from passes of their own\n"
              "      --adaptive [<X>]     pt tasks render adaptively: tiles whose error estimate is <= X stop receiving samples, spp is the most a pixel gets\n"
              "      --adaptive-min-spp <N>  with --adaptive: samples a tile receives before it may retire\n"
              "      --display [<CURVE>]  pt tasks also write {stem}.display.png: exposure, bloom and a tone curve (linear, reinhard, aces (default), hable)\n"
              "      --exposure <EV>, --auto-exposure, --bloom [<X>]  with --display: exposure in stops, exposure from the luminance histogram, bloom of strength X (default 0.25)");
}

// akari-cli --spec-compile <header file> <out.co> <arch> <flags> <min waves>: the library's helper process for per-scene kernels
// (host/specialise.cpp). The kernel is compiled HERE, in a process that holds nothing but this library and the ROCm installation's
// hiprtc, so that the host application's own copies of the ROCm compiler libraries (PyTorch ships its own) cannot change the code.
static int spec_compile_main(int argc, char** argv) {
    if (argc != 7) { std::fputs("usage: akari-cli --spec-compile <header> <out.co> <arch> <flags> <min_waves>\n", stderr); return 2; }
    std::ifstream hf(argv[2]);
    if (!hf) { std::fprintf(stderr, "akari-cli: cannot open %s\n", argv[2]); return 2; }
    std::stringstream ss;
    ss << hf.rdbuf();
    if (akr_host_spec_compile_text(ss.str().c_str(), (uint32_t)std::atoi(argv[5]), (uint32_t)std::atoi(argv[6]), argv[4], argv[3]) != AKR_OK) {
        std::fprintf(stderr, "%s\n", akr_last_error());
        return 1;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "--spec-compile") return spec_compile_main(argc, argv);
    std::string scene, method, name;
    int device = 0, verbose = 0, save_intermediate = 0, save_stats = 0, indep = 0;
    unsigned w = 0, h = 0;
    int dof = 0, no_punctual = 0, no_soft = 0, light_tree = 0;
    float lens_radius = -1.0f, focal_distance = -1.0f;  // < 0: not given
    int projection = -1;  // akr_projection_type; < 0: not given
    float ortho_scale = -1.0f;
    int denoise = 0, denoise_variance = 0, denoise_features = 0;
    int adaptive = 0, adaptive_min_spp = 0;  // adaptive: the option's value, threshold x 1024
    int display = 0, display_exposure = 0, display_auto = 0, display_bloom = 0, display_fields = 0;  // the options' values; display_fields: one of the three others was given
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto next = [&]() -> const char* { if (i + 1 >= argc) { usage(); std::exit(1); } return argv[++i]; };
        if (a == "-s" || a == "--scene") scene = next();
        else if (a == "-m" || a == "--method") method = next();
        else if (a == "-d" || a == "--device") { std::string d = next(); device = (d == "hip" || d == "gpu") ? 0 : std::atoi(d.c_str()); }
        else if (a == "-v" || a == "--verbose") verbose = 1;
        else if (a == "--save-intermediate") save_intermediate = 1;
        else if (a == "--save-stats") { name = next(); save_stats = 1; }
        else if (a == "--independent-sampler") indep = 1;
        else if (a == "--depth-of-field") dof = 1;
        else if (a == "--no-punctual-lights") no_punctual = 1;
        else if (a == "--no-soft-lights") no_soft = 1;
        else if (a == "--light-tree") light_tree = 1;
        else if (a == "--denoise") {  // the number is optional: taken only if the next argument is one
            denoise = 16;
            if (i + 1 < argc) {
                char* end = nullptr;
                const long v = std::strtol(argv[i + 1], &end, 10);
                if (end != argv[i + 1] && *end == 0) {
                    if (v < 1 || v > 65536) { std::fprintf(stderr, "akari-cli: --denoise wants 1 .. 65536 samples, got '%s'\n", argv[i + 1]); return 1; }
                    denoise = (int)v;
                    i++;
                }
            }
        }
        else if (a == "--denoise-variance") denoise_variance = 1;
        else if (a == "--denoise-features") denoise_features = 1;
        else if (a == "--adaptive") {  // the threshold is optional: taken only if the next argument is a number
            akr_adaptive_config ac;
            akr_adaptive_config_default(&ac);
            float t = ac.threshold;
            if (i + 1 < argc) {
                char* end = nullptr;
                const float v = std::strtof(argv[i + 1], &end);
                if (end != argv[i + 1] && *end == 0) {
                    if (!(v * 1024.0f >= 1.0f && v <= 1024.0f)) { std::fprintf(stderr, "akari-cli: --adaptive wants a threshold in 1/1024 .. 1024, got '%s'\n", argv[i + 1]); return 1; }
                    t = v;
                    i++;
                }
            }
            adaptive = (int)(t * 1024.0f + 0.5f);
        }
        else if (a == "--display") {  // the curve is optional: taken only if the next argument names one
            display = 3;
            static const char* const names[] = {"linear", "reinhard", "aces", "hable"};
            for (int c = 0; i + 1 < argc && c < 4; c++)
                if (std::strcmp(argv[i + 1], names[c]) == 0) {
                    display = c + 1;
                    i++;
                    break;
                }
        }
        else if (a == "--auto-exposure") display_auto = display_fields = 1;
        else if (a == "--exposure") {
            const char* text = next();
            char* end = nullptr;
            const float v = std::strtof(text, &end);
            if (end == text || *end != 0 || !(v >= -64.0f && v <= 64.0f)) { std::fprintf(stderr, "akari-cli: --exposure wants -64 .. 64 stops, got '%s'\n", text); return 1; }
            display_exposure = (int)std::lround(v * 1024.0f);
            display_fields = 1;
        }
        else if (a == "--bloom") {  // the strength is optional: taken only if the next argument is a number
            float s = 0.25f;
            if (i + 1 < argc) {
                char* end = nullptr;
                const float v = std::strtof(argv[i + 1], &end);
                if (end != argv[i + 1] && *end == 0) {
                    if (!(v >= 0.0f && v <= 64.0f)) { std::fprintf(stderr, "akari-cli: --bloom wants a strength in 0 .. 64, got '%s'\n", argv[i + 1]); return 1; }
                    s = v;
                    i++;
                }
            }
            display_bloom = (int)std::lround(s * 1024.0f);
            display_fields = 1;
        }
        else if (a == "--adaptive-min-spp") {
            const char* text = next();
            char* end = nullptr;
            const long v = std::strtol(text, &end, 10);
            if (end == text || *end != 0 || v < 1 || v > 65536) { std::fprintf(stderr, "akari-cli: --adaptive-min-spp wants 1 .. 65536 samples, got '%s'\n", text); return 1; }
            adaptive_min_spp = (int)v;
        }
        else if (a == "--lens-radius" || a == "--focal-distance") {
            const char* text = next();
            char* end = nullptr;
            const float v = std::strtof(text, &end);
            if (end == text || *end != 0 || !(v >= 0.0f)) { std::fprintf(stderr, "akari-cli: %s wants a number >= 0, got '%s'\n", a.c_str(), text); return 1; }
            (a == "--lens-radius" ? lens_radius : focal_distance) = v;
        }
        else if (a == "--projection") {
            const char* text = next();
            static const char* const names[] = {"perspective", "orthographic", "panorama"};
            for (int c = 0; c < 3; c++)
                if (std::strcmp(text, names[c]) == 0) projection = c;
            if (projection < 0) { std::fprintf(stderr, "akari-cli: --projection wants perspective, orthographic or panorama, got '%s'\n", text); return 1; }
        }
        else if (a == "--ortho-scale") {
            const char* text = next();
            char* end = nullptr;
            const float v = std::strtof(text, &end);
            if (end == text || *end != 0 || !(v > 0.0f)) { std::fprintf(stderr, "akari-cli: --ortho-scale wants a number > 0, got '%s'\n", text); return 1; }
            ortho_scale = v;
        }
        else if (a == "--resolution") { if (std::sscanf(next(), "%ux%u", &w, &h) != 2) { usage(); return 1; } }
        else if (a == "--gui") { std::fputs("akari-cli: --gui is not supported by the HIP integrator\n", stderr); return 1; }
        else { usage(); return 1; }
    }
    if (scene.empty() || method.empty()) { usage(); return 1; }
    // a lens needs both numbers: each comes from the command line or, with --depth-of-field, from the scene file
    if (!dof && (lens_radius >= 0.0f) != (focal_distance >= 0.0f)) {
        std::fprintf(stderr, "akari-cli: %s alone describes no lens: give --lens-radius and --focal-distance together, or add --depth-of-field to take the other "
                             "from the scene file's focal_distance / fstop\n", lens_radius >= 0.0f ? "--lens-radius" : "--focal-distance");
        return 1;
    }
    std::ifstream mf(method);
    if (!mf) { std::fprintf(stderr, "akari-cli: cannot open %s\n", method.c_str()); return 1; }
    std::stringstream ss;
    ss << mf.rdbuf();
    akr_context* ctx = nullptr;
    akr_scene* sc = nullptr;
    auto die = [&](const char* what) { std::fprintf(stderr, "akari-cli: %s: %s\n", what, akr_last_error()); std::exit(1); };
    if (akr_context_create(device, &ctx) != AKR_OK) die("device");
    if (dof && akr_option_set("lens", 1) != AKR_OK) die("option lens");
    if (no_punctual && akr_option_set("punctual_lights", 0) != AKR_OK) die("option punctual_lights");
    if (no_soft && akr_option_set("soft_lights", 0) != AKR_OK) die("option soft_lights");
    if (light_tree && akr_option_set("light_tree", 1) != AKR_OK) die("option light_tree");
    if (denoise && akr_option_set("denoise", denoise) != AKR_OK) die("option denoise");
    if (denoise_features && akr_option_set("denoise_features", 1) != AKR_OK) die("option denoise_features");
    if (denoise_variance && !denoise && !denoise_features) { std::fputs("akari-cli: --denoise-variance needs --denoise or --denoise-features\n", stderr); return 1; }
    if (denoise_variance && akr_option_set("denoise_variance", 1) != AKR_OK) die("option denoise_variance");
    if (adaptive_min_spp && !adaptive) { std::fputs("akari-cli: --adaptive-min-spp needs --adaptive\n", stderr); return 1; }
    if (adaptive && akr_option_set("adaptive", adaptive) != AKR_OK) die("option adaptive");
    if (adaptive_min_spp && akr_option_set("adaptive_min_spp", adaptive_min_spp) != AKR_OK) die("option adaptive_min_spp");
    if (display_fields && !display) display = 3;
    if (display && (akr_option_set("display", display) != AKR_OK || akr_option_set("display_auto_exposure", display_auto) != AKR_OK ||
                    akr_option_set("display_exposure", display_exposure) != AKR_OK || akr_option_set("display_bloom", display_bloom) != AKR_OK))
        die("option display");
    if (akr_scene_load(ctx, scene.c_str(), w, h, &sc) != AKR_OK) die("scene");
    if (projection >= 0 || ortho_scale > 0.0f) {  // (before the lens: a panorama refuses one, an orthographic film is checked with it)
        akr_projection_desc pd;
        if (akr_scene_get_projection(sc, &pd) != AKR_OK) die("projection");
        if (projection >= 0) pd.type = (uint32_t)projection;
        if (ortho_scale > 0.0f) pd.ortho_scale = ortho_scale;
        if (akr_scene_set_projection(sc, &pd) != AKR_OK) die("projection");
    }
    if (lens_radius >= 0.0f || focal_distance >= 0.0f) {
        akr_lens_desc lens;
        if (akr_scene_get_lens(sc, &lens) != AKR_OK) die("lens");
        if (lens_radius >= 0.0f) lens.radius = lens_radius;
        if (focal_distance >= 0.0f) lens.focal_distance = focal_distance;
        if (akr_scene_set_lens(sc, &lens) != AKR_OK) die("lens");
    }
    akr_render_session ses;
    ses.save_intermediate = save_intermediate;
    ses.save_stats = save_stats;
    ses.name = name.empty() ? nullptr : name.c_str();
    ses.override_sampler_independent = indep;
    ses.verbose = verbose;
    akr_pt_stats st;
    if (akr_render_task(ctx, sc, ss.str().c_str(), &ses, &st) != AKR_OK) die("render");
    std::printf("Rendering finished in %.2fs\n", st.kernel_ms * 1e-3);
    akr_scene_destroy(sc);
    akr_context_destroy(ctx);
    return 0;
}
