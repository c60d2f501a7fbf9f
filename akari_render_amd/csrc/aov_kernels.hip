// aov_kernels.hip -- the `aov` integrator (crates/akari_integrator/src/aov.rs:57-173) on gfx950: k_aov (aov_kernel.h), LENS = false here.
#define AKR_NODE_ARM_OUT_OF_LINE 1  // the interpreter's math / noise arm as one call in this unit (device/dtex.h; measured)
#include "aov_kernel.h"

namespace akr {

hipError_t launch_aov(const PtParams& p, uint32_t spp, uint32_t aov, uint32_t remap, hipStream_t stream) {
    static constexpr hipError_t (*kEntry[2])(const PtParams&, uint32_t, uint32_t, uint32_t, hipStream_t) = {launch_aov_t<false>, aov_entry_lens};  // by [lens]
    return kEntry[camera_runs_lens_kernels(p.lens_radius, p.projection)](p, spp, aov, remap, stream);
}

}  // namespace akr
