// options.h -- the process-wide tuning switches and test hooks (akr_option_set / akr_option_get of the C ABI; include/akari_hip.h describes
// every one). Each starts from its default below, then from its environment variable, read ONCE when the first of them is looked at; after
// that only akr_option_set changes it. No launch path calls getenv. A session, a scene load and a setter that recompiles take ONE snapshot
// (tuning()) and read nothing else: what they build is of one option state.
// An option is stated three times: a member here (its default), a row of kOptions (options.cpp: name, environment variable, range, parse
// rule) and an entry of the option comment in include/akari_hip.h.
#pragma once
#include <cstdint>

namespace akr {

struct TuningOptions {
    int force_bvh = 0, bvh_balanced = 0, defer_metal = -1, wavefront = -1, simple_kernels = 1;
    int defer_on = 0;
    int specialise = -1, specialise_waves = 0;
    int max_fused_passes = 0;
    int instancing = -1;
    int rebraid = 1;
    int arith = 0;
    int pad_percent = 100;
    int wf_groups = 0;
    int wf_carry = 1;
    int sched_trial = -1;
    int punctual_lights = 1;
    int soft_lights = 1;
    int light_tree = 0;
    int lens = 0;
    int denoise = 0;
    int denoise_variance = 0;
    int denoise_features = 0;
    int denoise_kernel = -1;
    int adaptive = 0;
    int adaptive_min_spp = 0;
    int display = 0;
    int display_auto_exposure = 0, display_exposure = 0, display_bloom = 0;
    int display_kernel = -1;
    int wf_sort = 0;
};
TuningOptions tuning();                          // a snapshot (thread-safe)
bool tuning_set(const char* name, int value);    // false: unknown name, or a value outside the row's range
bool tuning_get(const char* name, int* value);

// One row of the table, for tests (akr_host_option_info): false past the last row. env = "" without an environment variable;
// ranged = 0: akr_option_set takes any int (lo / hi are then INT32_MIN / INT32_MAX).
struct OptionInfo {
    const char* name;
    const char* env;
    int def, ranged, lo, hi;
};
bool tuning_info(uint32_t index, OptionInfo* out);

}  // namespace akr
