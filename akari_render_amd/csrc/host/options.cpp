// options.cpp -- the table of the process-wide options (options.h) and the three things that walk it: the first look at the environment,
// akr_option_set's range check, the lookup by name.
#include "options.h"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <mutex>

namespace akr {
namespace {
// How an environment string becomes a value. The rules are the ones each variable has had since it was added; they differ, and
// akr_option_set's ranges are not applied to Raw values (AKR_SPECIALISE_WAVES=7 goes in).
enum class Env {
    None,    // no environment variable
    Flag1,   // 1 if the first character is '1', else 0
    Bool,    // atoi != 0
    Raw,     // atoi, as it is
    Clamp,   // atoi, clamped to the row's range
    PtMode,  // "wavefront" = 1, "auto" = -1, anything else = 0
};
struct Row {
    const char* name;
    const char* env;  // "" with Env::None
    int TuningOptions::*field;
    Env parse;
    bool ranged;  // akr_option_set refuses values outside [lo, hi]; false = any int
    int lo, hi;
};
constexpr Row any(const char* name, const char* env, int TuningOptions::*f, Env parse) { return {name, env, f, parse, false, INT_MIN, INT_MAX}; }
constexpr Row in(const char* name, const char* env, int TuningOptions::*f, Env parse, int lo, int hi) { return {name, env, f, parse, true, lo, hi}; }
using T = TuningOptions;
constexpr Row kOptions[] = {
    any("force_bvh", "AKR_FORCE_BVH", &T::force_bvh, Env::Flag1),           // scenes of <= 64 triangles get a BVH too
    any("bvh_balanced", "AKR_BVH_BALANCED", &T::bvh_balanced, Env::Flag1),  // the median-split fallback builder instead of SAH
    any("defer_metal", "AKR_PT_DEFER_METAL", &T::defer_metal, Env::Raw),    // -1 auto, 0 off, m > 0: iterations with (i & m) != 0 put conductor hits off
    in("wavefront", "AKR_PT_MODE", &T::wavefront, Env::PtMode, -1, 1),      // the schedule: 1 wavefront wherever it can run, 0 never, -1 the library decides
    any("simple_kernels", "AKR_PT_SIMPLE", &T::simple_kernels, Env::Bool),  // 0 = never the SIMPLE instantiations
    in("defer_on", "", &T::defer_on, Env::None, 0, 3),                      // BVH kernels of textured scenes: 0 / 1 conductor lobe, 2 texture-fed, 3 both
    in("specialise", "AKR_SPECIALISE", &T::specialise, Env::Raw, -1, 1),    // per-scene kernels: -1 auto, 0 never, 1 always
    in("specialise_waves", "AKR_SPECIALISE_WAVES", &T::specialise_waves, Env::Raw, 0, 4),  // waves per SIMD of a per-scene kernel: 0 auto, else 2..4 (1: tuning_set)
    in("max_fused_passes", "", &T::max_fused_passes, Env::None, 0, 64),     // most passes akr_pt_passes fuses into one launch; 0 = adaptive
    in("instancing", "AKR_INSTANCING", &T::instancing, Env::Raw, -1, 1),    // meshes + instances kept as they are: -1 auto, 0 never, 1 always
    in("rebraid", "AKR_REBRAID", &T::rebraid, Env::Clamp, 1, 64),           // kept scenes: (instance, subtree) pairs of the top-level tree per instance
    in("arith", "AKR_ARITH", &T::arith, Env::Bool, 0, 1),                   // 1 = the pt megakernel in the relaxed arithmetic tier
    in("pad_percent", "", &T::pad_percent, Env::None, 1, 10000),            // test hook: box padding in percent of the derived value
    in("wf_groups", "AKR_WF_GROUPS", &T::wf_groups, Env::Clamp, 0, 32),     // wavefront schedule: slot groups; 0 = the library decides
    in("wf_carry", "AKR_WF_CARRY", &T::wf_carry, Env::Clamp, 0, 1 << 30),   // wavefront schedule: carried rays (0 off, 1 on, n > 1 test hook)
    in("sched_trial", "AKR_SCHED_TRIAL", &T::sched_trial, Env::Clamp, -1, 1),  // timed trial of both schedules: -1 where it pays, 0 never, 1 always (tests)
    in("punctual_lights", "AKR_PUNCTUAL_LIGHTS", &T::punctual_lights, Env::Bool, 0, 1),  // akr_scene_load: 0 = the file's point / spot / sun lights are dropped
    in("soft_lights", "AKR_SOFT_LIGHTS", &T::soft_lights, Env::Bool, 0, 1),  // akr_scene_load: 0 = every light is loaded as a delta light
    in("light_tree", "AKR_LIGHT_TREE", &T::light_tree, Env::Bool, 0, 1),    // the initial light-tree mode of a new scene
    in("lens", "AKR_LENS", &T::lens, Env::Bool, 0, 1),                      // akr_scene_load: 1 = the file's focal_distance / fstop become a thin lens
    in("denoise", "AKR_DENOISE", &T::denoise, Env::Clamp, 0, 65536),        // akr_render_task: spp of the denoise step's feature passes; 0 = no step
    in("denoise_variance", "AKR_DENOISE_VARIANCE", &T::denoise_variance, Env::Bool, 0, 1),  // ... the step is akr_denoise_variance
    in("denoise_features", "AKR_DENOISE_FEATURES", &T::denoise_features, Env::Bool, 0, 1),  // ... its guides come from the pt task's own session
    in("denoise_kernel", "AKR_DENOISE_KERNEL", &T::denoise_kernel, Env::Clamp, -1, 1),      // akr_denoise's level kernel: 0 gathering, 1 LDS-tiled, -1 auto
    in("adaptive", "AKR_ADAPTIVE", &T::adaptive, Env::Clamp, 0, 1 << 20),   // akr_render_task: > 0 = adaptive pt renders, threshold n / 1024
    in("adaptive_min_spp", "AKR_ADAPTIVE_MIN_SPP", &T::adaptive_min_spp, Env::Clamp, 0, 65536),  // ... their min_spp; 0 = the default's
    in("display", "AKR_DISPLAY", &T::display, Env::Clamp, 0, 4),            // akr_render_task: 1..4 = the curve of the display transform after a pt task
    in("display_auto_exposure", "AKR_DISPLAY_AUTO_EXPOSURE", &T::display_auto_exposure, Env::Bool, 0, 1),  // ... its auto_exposure
    in("display_exposure", "AKR_DISPLAY_EXPOSURE", &T::display_exposure, Env::Clamp, -65536, 65536),       // ... its exposure_ev x 1024
    in("display_bloom", "AKR_DISPLAY_BLOOM", &T::display_bloom, Env::Clamp, 0, 65536),                     // ... its bloom_strength x 1024
    in("display_kernel", "AKR_DISPLAY_KERNEL", &T::display_kernel, Env::Clamp, -1, 1),  // akr_display_transform's blur: 0 gathering, 1 through LDS, -1 auto
    in("wf_sort", "AKR_WF_SORT", &T::wf_sort, Env::Bool, 0, 1),             // wavefront schedule: ray queues sorted before each trace launch
};
static_assert(sizeof(kOptions) / sizeof(kOptions[0]) * sizeof(int) == sizeof(TuningOptions), "one row of kOptions per member of TuningOptions");

std::mutex g_tuning_mutex;
bool g_tuning_init = false;
TuningOptions g_tuning;
int parse_env(const Row& r, const char* e) {
    switch (r.parse) {
    case Env::Flag1: return e[0] == '1' ? 1 : 0;
    case Env::Bool: return std::atoi(e) != 0 ? 1 : 0;
    case Env::Clamp: return std::max(r.lo, std::min(r.hi, std::atoi(e)));
    case Env::PtMode: return std::strcmp(e, "wavefront") == 0 ? 1 : (std::strcmp(e, "auto") == 0 ? -1 : 0);
    default: return std::atoi(e);
    }
}
void tuning_init_locked() {
    if (g_tuning_init) return;
    g_tuning_init = true;
    for (const Row& r : kOptions)
        if (const char* e = r.parse != Env::None ? std::getenv(r.env) : nullptr) g_tuning.*r.field = parse_env(r, e);
}
const Row* tuning_row(const char* name) {
    for (const Row& r : kOptions)
        if (name && std::strcmp(name, r.name) == 0) return &r;
    return nullptr;
}
}  // namespace
TuningOptions tuning() {
    std::lock_guard<std::mutex> lock(g_tuning_mutex);
    tuning_init_locked();
    return g_tuning;
}
bool tuning_set(const char* name, int value) {
    std::lock_guard<std::mutex> lock(g_tuning_mutex);
    tuning_init_locked();
    const Row* r = tuning_row(name);
    if (!r || (r->ranged && (value < r->lo || value > r->hi))) return false;
    if (r->field == &T::specialise_waves && value == 1) return false;  // (the one hole in a range: no per-scene kernel is built for one wave)
    g_tuning.*r->field = value;
    return true;
}
bool tuning_get(const char* name, int* value) {
    std::lock_guard<std::mutex> lock(g_tuning_mutex);
    tuning_init_locked();
    const Row* r = tuning_row(name);
    if (!r) return false;
    *value = g_tuning.*r->field;
    return true;
}
bool tuning_info(uint32_t index, OptionInfo* out) {
    if (index >= sizeof(kOptions) / sizeof(kOptions[0])) return false;
    const Row& r = kOptions[index];
    *out = {r.name, r.env, TuningOptions{}.*r.field, r.ranged ? 1 : 0, r.lo, r.hi};
    return true;
}

}  // namespace akr
