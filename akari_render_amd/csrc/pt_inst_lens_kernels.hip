// pt_inst_lens_kernels.hip -- k_pt_pass_inst of kept scenes seen through a thin lens (LENS = true; device/dpath.h generate_ray_lens_from), without
// and with an environment light: force_diffuse x textures x sampler family x ENV, in a translation unit of their own (pt_inst_kernel.h).
#include "pt_inst_kernel.h"

namespace akr {

hipError_t pt_pass_entry_inst_lens_env(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream) { return pt_pass_entry_inst_t<true, true>(q, v, blocks, lds, stream); }
hipError_t pt_pass_entry_inst_lens(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream) { return pt_pass_entry_inst_t<false, true>(q, v, blocks, lds, stream); }

}  // namespace akr
