// aov_kernels.hip -- the `aov` integrator (crates/akari_integrator/src/aov.rs:57-173) on gfx950: k_aov (aov_kernel.h), LENS = false here.
#include "aov_kernel.h"

namespace akr {

hipError_t launch_aov(const PtParams& p, uint32_t spp, uint32_t aov, uint32_t remap, hipStream_t stream) {
    if (p.lens_radius > 0.0f) return launch_aov_lens(p, spp, aov, remap, stream);  // a thin lens: aov_lens_kernels.hip
    return launch_aov_t<false>(p, spp, aov, remap, stream);
}

}  // namespace akr
