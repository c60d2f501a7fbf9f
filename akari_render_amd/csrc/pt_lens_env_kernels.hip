// pt_lens_env_kernels.hip -- k_pt_pass for flattened scenes with an environment light seen through a thin lens (ENV = true, LENS = true), in a
// translation unit of their own.
#include "pt_launch.h"

namespace akr {

hipError_t pt_pass_entry_lens_env(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream) { return pt_pass_entry_t<true, true>(q, v, blocks, lds, stream); }

}  // namespace akr
