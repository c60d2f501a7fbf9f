// pt_inst_env_kernels.hip -- k_pt_pass_inst of kept scenes with an environment light (ENV = true; device/denv.h): force_diffuse x textures x
// sampler family, in a translation unit of their own (pt_inst_kernel.h).
#include "pt_inst_kernel.h"

namespace akr {

hipError_t pt_pass_entry_inst_env(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream) { return pt_pass_entry_inst_t<true, false>(q, v, blocks, lds, stream); }

}  // namespace akr
