// pt_punct_lens_kernels.hip -- k_pt_pass for flattened scenes with punctual lights (PUNCT = true: device/dpunct.h) seen through a thin lens (LENS = true),
// in a translation unit of their own: what kernels.h pt_variant_compiled leaves of k_pt_pass with PUNCT on.
#include "pt_launch.h"

namespace akr {

hipError_t pt_pass_entry_punct_lens(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream) { return pt_pass_entry_t<false, true, false, true>(q, v, blocks, lds, stream); }

}  // namespace akr
