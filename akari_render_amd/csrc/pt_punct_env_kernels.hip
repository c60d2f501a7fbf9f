// pt_punct_env_kernels.hip -- k_pt_pass for flattened scenes with punctual lights (PUNCT = true: device/dpunct.h) with an environment light (ENV = true),
// in a translation unit of their own: what kernels.h pt_variant_compiled leaves of k_pt_pass with PUNCT on.
#include "pt_launch.h"

namespace akr {

hipError_t pt_pass_entry_punct_env(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream) { return pt_pass_entry_t<true, false, false, true>(q, v, blocks, lds, stream); }

}  // namespace akr
