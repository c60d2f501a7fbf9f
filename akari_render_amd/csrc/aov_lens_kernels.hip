// aov_lens_kernels.hip -- k_aov for a camera with a thin lens (LENS = true; aov_kernel.h): a denoiser's feature buffers see the scene as the
// beauty pass does.
#define AKR_NODE_ARM_OUT_OF_LINE 1  // the interpreter's math / noise arm as one call in this unit (device/dtex.h; measured)
#include "aov_kernel.h"

namespace akr {

hipError_t aov_entry_lens(const PtParams& p, uint32_t spp, uint32_t aov, uint32_t remap, hipStream_t stream) { return launch_aov_t<true>(p, spp, aov, remap, stream); }

}  // namespace akr
