// api_task.cpp -- akr_render_task: the reference's render driver (akari_integrator/src/lib.rs:111-207) (C ABI of libakari_hip.so, include/akari_hip.h; shared internals: api_internal.h)
#include "api_internal.h"

namespace {
struct FilmHolder {  // a film that dies with its scope
    akr_film* f = nullptr;
    FilmHolder() = default;
    explicit FilmHolder(akr_film* film) : f(film) {}
    FilmHolder(const FilmHolder&) = delete;
    FilmHolder& operator=(const FilmHolder&) = delete;
    ~FilmHolder() { if (f) akr_film_destroy(f); }
};

// "{stem}.denoised{ext}" of film.out
std::string denoised_path(const std::string& out) {
    const size_t slash = out.find_last_of("/\\"), dot = out.find_last_of('.');
    if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) return out + ".denoised";
    return out.substr(0, dot) + ".denoised" + out.substr(dot);
}

// Option "denoise" (DESIGN.md 4.10): the feature passes of a finished pt task -- albedo and ns (not remapped) at `spp` samples with the task's
// sampler, seed, filter and colour pipeline, through the scene's lens if it has one -- then akr_denoise with its defaults, in place in `film`.
// half (option "denoise_variance"): the film after the first half of the task's passes; the filter is akr_denoise_variance then.
// own_albedo / own_normal (option "denoise_features"): the guides the task's own session collected; no feature passes then.
void denoise_step(akr_context* ctx, akr_scene* scene, const akr_pt_config& cfg, akr_film* film, akr_film* half, uint32_t spp, bool verbose, akr_film* own_albedo = nullptr,
                  akr_film* own_normal = nullptr) {
    auto check = [](int32_t rc) { if (rc != AKR_OK) throw std::runtime_error(std::string(g_last_error)); };
    akr_denoise_config dc;
    check(akr_denoise_config_default(&dc));
    if (own_albedo && own_normal) {
        check(half ? akr_denoise_variance(ctx, &dc, film, half, own_albedo, own_normal, film) : akr_denoise(ctx, &dc, film, own_albedo, own_normal, film));
        if (verbose) std::fprintf(stderr, "[akari_hip] Denoised (guides collected by the task's own %u spp)\n", cfg.spp);
        return;
    }
    akr_aov_config ac;
    check(akr_aov_config_default(&ac));
    ac.spp = spp;
    ac.remap = 0;
    ac.filter_type = cfg.filter_type;
    ac.filter_radius = cfg.filter_radius;
    ac.sampler_type = cfg.sampler_type;
    ac.sampler_seed = cfg.sampler_seed;
    ac.color = cfg.color;
    FilmHolder albedo, normal;
    check(akr_film_create(ctx, film->width, film->height, &albedo.f));
    check(akr_film_create(ctx, film->width, film->height, &normal.f));
    akr_pt_stats sa, sn;
    ac.aov = AKR_AOV_ALBEDO;
    check(akr_aov_render(ctx, scene, &ac, albedo.f, &sa));
    ac.aov = AKR_AOV_NS;
    check(akr_aov_render(ctx, scene, &ac, normal.f, &sn));
    check(half ? akr_denoise_variance(ctx, &dc, film, half, albedo.f, normal.f, film) : akr_denoise(ctx, &dc, film, albedo.f, normal.f, film));
    if (verbose) std::fprintf(stderr, "[akari_hip] Denoised (feature passes of %u spp: %.2fms)\n", spp, sa.kernel_ms + sn.kernel_ms);
}

// "{stem}.display.png" of film.out
std::string display_path(const std::string& out) {
    const size_t slash = out.find_last_of("/\\"), dot = out.find_last_of('.');
    if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) return out + ".display.png";
    return out.substr(0, dot) + ".display.png";
}

// Option "display" (DESIGN.md 4.12): akr_display_transform of a finished pt task's film (the denoised one when the denoise step ran), in
// place, with the default configuration but for the fields the options carry; the result goes through the PNG writer's OETF
void display_step(akr_context* ctx, const TuningOptions& opts, akr_film* film, const std::string& out, std::vector<float>& rgb, bool verbose) {
    auto check = [](int32_t rc) { if (rc != AKR_OK) throw std::runtime_error(std::string(g_last_error)); };
    akr_display_config dc;
    check(akr_display_config_default(&dc));
    dc.curve = (uint32_t)opts.display;
    dc.auto_exposure = opts.display_auto_exposure != 0 ? 1u : 0u;
    dc.exposure_ev = (float)opts.display_exposure / 1024.0f;
    dc.bloom_strength = (float)opts.display_bloom / 1024.0f;
    float k = 0.0f;
    check(akr_display_transform(ctx, &dc, film, film, &k));
    check(akr_film_resolve(film, rgb.data()));
    write_image(display_path(out), rgb.data(), film->width, film->height);
    if (verbose) std::fprintf(stderr, "[akari_hip] Display transform (curve %u, exposure %g)\n", dc.curve, (double)k);
}
}  // namespace

extern "C" {

AKR_API int32_t akr_render_task(akr_context* ctx, akr_scene* scene, const char* method_json_text, const akr_render_session* session,
                                akr_pt_stats* stats_out) {
    if (!ctx || !scene || !method_json_text) return fail(AKR_ERR_INVALID_ARGUMENT, "akr_render_task: NULL argument");
    akr_render_session ses{0, 0, nullptr, 0, 0};
    if (session) ses = *session;
    const std::string name = ses.name ? ses.name : "default";
    const TuningOptions opts = tuning();  // read once, like a session's options
    // option "denoise_features" implies the denoise step; where its guides cannot come from the task's session (a session that refuses them, an
    // adaptive task) they come from aov passes as ever, of "denoise" spp if that is set, else 16
    const bool denoise_features = opts.denoise_features != 0;
    const int denoise_spp = opts.denoise > 0 ? opts.denoise : (denoise_features ? 16 : 0);
    const bool denoise_variance = denoise_spp > 0 && opts.denoise_variance != 0;
    const int adaptive = opts.adaptive;
    return guarded([&] {
        std::vector<ParsedTask> tasks = parse_render_tasks(method_json_text, ses.override_sampler_independent != 0);
        const uint32_t w = scene->flat.camera.width, h = scene->flat.camera.height;
        std::vector<float> rgb(3ull * w * h);
        for (size_t ti = 0; ti < tasks.size(); ti++) {  // render_single, lib.rs:112-193
            const ParsedTask& task = tasks[ti];
            if (ses.verbose) std::fprintf(stderr, "[akari_hip] task %zu/%zu (%s): %ux%u, %u spp -> %s\n", ti + 1, tasks.size(), task.is_aov ? "aov" : (task.is_gpt ? "gpt" : (task.is_mcmc ? "mcmc_opt" : "pt")), w, h, task.is_aov ? task.aov.spp : (task.is_gpt ? task.gpt.spp : (task.is_mcmc ? task.mcmc.spp : task.cfg.spp)), task.film_out.c_str());
            akr_film* film = nullptr;
            akr_pt_session* se = nullptr;
            auto check = [&](int32_t rc) { if (rc != AKR_OK) { std::string m = g_last_error; if (se) akr_pt_end(se, nullptr); if (film) akr_film_destroy(film); throw std::runtime_error(m); } };
            check(akr_film_create(ctx, w, h, &film));
            if (task.is_aov) {  // Method::NormalVis: one blocking dispatch, no intermediates (aov.rs:161-171)
                akr_pt_stats st;
                check(akr_aov_render(ctx, scene, &task.aov, film, &st));
                if (ses.verbose) std::fprintf(stderr, "[akari_hip] Rendered in %.2fms\n", st.kernel_ms);
                check(akr_film_resolve(film, rgb.data()));
                akr_film_destroy(film);
                film = nullptr;
                write_image(task.film_out, rgb.data(), w, h);
                if (stats_out) *stats_out = st;
                continue;
            }
            if (task.is_mcmc) {  // McmcOpt::render; --save-intermediate / --save-stats as render_loop does (mcmc_opt.rs:640-676)
                akr_pt_stats st;
                akr_mcmc_result res;
                std::string stats_json = "{\"intermediate\":[";
                bool first = true;
                std::function<void(uint32_t, double)> on_pass;
                if (ses.save_intermediate)
                    on_pass = [&](uint32_t cnt, double time_s) {
                        check(akr_film_resolve(film, rgb.data()));
                        std::string path = name + "-" + std::to_string(cnt) + ".exr";
                        write_image(path, rgb.data(), w, h);
                        char buf[512];
                        std::snprintf(buf, sizeof buf, "%s{\"path\":\"%s\",\"time\":%.9g,\"spp\":%u}", first ? "" : ",", path.c_str(), time_s, cnt);
                        stats_json += buf;
                        first = false;
                    };
                check(mcmc_render_impl(ctx, scene, &task.mcmc, film, &res, nullptr, &st, on_pass));
                stats_json += "]}";
                if (ses.save_stats) {
                    std::string path = name + ".json";
                    FILE* f = std::fopen(path.c_str(), "wb");
                    if (!f) throw std::runtime_error("cannot open '" + path + "' for writing");
                    std::fwrite(stats_json.data(), 1, stats_json.size(), f);
                    std::fclose(f);
                }
                if (ses.verbose)
                    std::fprintf(stderr, "[akari_hip] Normalization factor: %g\n[akari_hip] Acceptance rate: %.2f%%\n[akari_hip] Rendering finished in %.2fs\n",
                                 res.normalization, res.acceptance_rate * 100.0, st.kernel_ms * 1e-3);
                check(akr_film_resolve(film, rgb.data()));
                akr_film_destroy(film);
                film = nullptr;
                write_image(task.film_out, rgb.data(), w, h);
                if (stats_out) *stats_out = st;
                continue;
            }
            if (task.is_gpt) {  // GradientPathTracer::render: no intermediates; with a reconstruction also output/gpt_*.exr (gpt.rs:609-636)
                akr_pt_stats st;
                const bool recon = task.gpt.reconstruction != AKR_GPT_RECON_NONE;
                const size_t N = (size_t)w * h, NG = (size_t)(w + 1) * (h + 1);
                std::vector<float> aux(recon ? 3 * N + 6 * NG : 0);
                check(akr_gpt_render(ctx, scene, &task.gpt, film, recon ? aux.data() : nullptr, &st));
                if (ses.verbose) std::fprintf(stderr, "[akari_hip] Rendering finished in %.2fs\n", st.kernel_ms * 1e-3);
                check(akr_film_resolve(film, rgb.data()));
                akr_film_destroy(film);
                film = nullptr;
                if (recon) {
                    const float scale = 1.0f / (float)task.gpt.spp;  // set_splat_scale(1 / spp) on the accumulators
                    for (float& v : aux) v = v * scale;
                    write_image("output/gpt_primal.exr", aux.data(), w, h);
                    write_image("output/gpt_gx.exr", aux.data() + 3 * N, w + 1, h + 1);
                    write_image("output/gpt_gy.exr", aux.data() + 3 * N + 3 * NG, w + 1, h + 1);
                }
                write_image(task.film_out, rgb.data(), w, h);
                if (stats_out) *stats_out = st;
                continue;
            }
            if (adaptive > 0) {  // option "adaptive" (DESIGN.md 4.11): the task's spp is the most a pixel gets, tiles retire by their error estimate
                if (ses.save_intermediate || denoise_variance) {
                    akr_film_destroy(film);
                    throw Unsupported(std::string("unsupported: option adaptive together with ") + (ses.save_intermediate ? "--save-intermediate" : "option denoise_variance"));
                }
                akr_adaptive_config ac;
                check(akr_adaptive_config_default(&ac));
                ac.threshold = (float)adaptive / 1024.0f;
                if (opts.adaptive_min_spp > 0) ac.min_spp = (uint32_t)opts.adaptive_min_spp;
                akr_adaptive_stats as;
                check(akr_pt_adaptive_render(ctx, scene, &task.cfg, &ac, film, nullptr, nullptr, &as));
                const akr_pt_stats& st = as.pt;
                if (ses.save_stats) {
                    std::string path = name + ".json";
                    FILE* f = std::fopen(path.c_str(), "wb");
                    if (!f) throw std::runtime_error("cannot open '" + path + "' for writing");
                    std::fputs("{\"intermediate\":[]}", f);
                    std::fclose(f);
                }
                if (ses.verbose)
                    std::fprintf(stderr, "[akari_hip] Rendering finished in %.2fs (%.1f Msamples/s); adaptive: %u rounds, %llu of %llu samples drawn, %u tiles retired\n", st.kernel_ms * 1e-3,
                                 st.n_samples / (st.kernel_ms * 1e3), as.rounds, (unsigned long long)as.samples_drawn, (unsigned long long)as.samples_uniform, as.tiles_retired);
                check(akr_film_resolve(film, rgb.data()));
                FilmHolder done(film);
                film = nullptr;
                write_image(task.film_out, rgb.data(), w, h);
                if (stats_out) *stats_out = st;
                if (denoise_spp > 0) {
                    denoise_step(ctx, scene, task.cfg, done.f, nullptr, (uint32_t)denoise_spp, ses.verbose != 0);
                    check(akr_film_resolve(done.f, rgb.data()));
                    write_image(denoised_path(task.film_out), rgb.data(), w, h);
                }
                if (opts.display > 0) display_step(ctx, opts, done.f, task.film_out, rgb, ses.verbose != 0);
                continue;
            }
            // option "denoise_variance": the film after the first floor(n_passes / 2) passes is kept as the half film of the denoise step
            FilmHolder half;
            uint32_t half_spp = 0;  // the sample count at which the half is taken; 0 = no half
            if (denoise_variance) {
                if (task.cfg.spp_per_pass == 0 || task.cfg.spp <= task.cfg.spp_per_pass) {
                    akr_film_destroy(film);
                    throw std::invalid_argument("akr_render_task: option denoise_variance needs a task of at least two passes: spp = " + std::to_string(task.cfg.spp) +
                                                " is one pass at spp_per_pass = " + std::to_string(task.cfg.spp_per_pass));
                }
                const uint32_t n_passes = (task.cfg.spp + task.cfg.spp_per_pass - 1) / task.cfg.spp_per_pass;
                half_spp = (n_passes / 2) * task.cfg.spp_per_pass;
                check(akr_film_create(ctx, w, h, &half.f));
            }
            auto take_half = [&] {  // device to device, in the stream's order after the passes so far
                check(guarded([&] {
                    HIP_CHECK(hipMemcpyAsync(half.f->data, film->data, film->n_floats() * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
                    HIP_CHECK(hipStreamSynchronize(ctx->stream));
                }));
            };
            FilmHolder own_albedo, own_normal;  // option "denoise_features": the guide films of the task's session
            bool own_guides = false;
            if (denoise_features) {
                check(akr_film_create(ctx, w, h, &own_albedo.f));
                check(akr_film_create(ctx, w, h, &own_normal.f));
                const int32_t rc = akr_pt_begin_features(ctx, scene, &task.cfg, film, own_albedo.f, own_normal.f, &se);
                if (rc == AKR_OK) own_guides = true;
                else if (rc != AKR_ERR_UNSUPPORTED) check(rc);
                else if (ses.verbose) std::fprintf(stderr, "[akari_hip] denoise_features: %s; the guides come from aov passes of %d spp\n", g_last_error.c_str(), denoise_spp);
            }
            if (!own_guides) check(akr_pt_begin(ctx, scene, &task.cfg, film, &se));
            std::string stats_json = "{\"intermediate\":[";
            uint32_t cnt = 0;
            bool first = true;
            if (half_spp && !ses.save_intermediate) {
                check(akr_pt_passes(se, half_spp / task.cfg.spp_per_pass, 1, &cnt));
                take_half();
            }
            while (cnt < task.cfg.spp) {  // pt.rs:1126-1149
                if (ses.save_intermediate) {
                    check(akr_pt_passes(se, 1, 1, &cnt));
                    if (half_spp && cnt == half_spp) take_half();
                    akr_pt_stats st;
                    check(akr_pt_get_stats(se, &st));
                    check(akr_film_resolve(film, rgb.data()));
                    std::string path = name + "-" + std::to_string(cnt) + ".exr";
                    write_image(path, rgb.data(), w, h);
                    char buf[512];
                    std::snprintf(buf, sizeof buf, "%s{\"path\":\"%s\",\"time\":%.9g,\"spp\":%u}", first ? "" : ",", path.c_str(), st.kernel_ms * 1e-3, cnt);
                    stats_json += buf;
                    first = false;
                } else {
                    check(akr_pt_passes(se, 16, 1, &cnt));
                }
            }
            stats_json += "]}";
            akr_pt_stats st;
            int32_t rc = akr_pt_end(se, &st);
            se = nullptr;
            check(rc);
            if (ses.save_stats) {  // pt.rs:1150-1155
                std::string path = name + ".json";
                FILE* f = std::fopen(path.c_str(), "wb");
                if (!f) throw std::runtime_error("cannot open '" + path + "' for writing");
                std::fwrite(stats_json.data(), 1, stats_json.size(), f);
                std::fclose(f);
            }
            if (ses.verbose) std::fprintf(stderr, "[akari_hip] Rendering finished in %.2fs (%.1f Msamples/s)\n", st.kernel_ms * 1e-3, st.n_samples / (st.kernel_ms * 1e3));
            check(akr_film_resolve(film, rgb.data()));  // film.copy_to_rgba_image(hdr = true), lib.rs:191
            FilmHolder done(film);
            film = nullptr;
            write_image(task.film_out, rgb.data(), w, h);  // util::write_image(&output_image, &config.film.out), lib.rs:192
            if (stats_out) *stats_out = st;
            if (denoise_spp > 0) {  // option "denoise": film.out is written as ever, the denoised image next to it
                denoise_step(ctx, scene, task.cfg, done.f, half.f, (uint32_t)denoise_spp, ses.verbose != 0, own_guides ? own_albedo.f : nullptr, own_guides ? own_normal.f : nullptr);
                check(akr_film_resolve(done.f, rgb.data()));
                write_image(denoised_path(task.film_out), rgb.data(), w, h);
            }
            if (opts.display > 0) display_step(ctx, opts, done.f, task.film_out, rgb, ses.verbose != 0);
        }
    });
}

}  // extern "C"
