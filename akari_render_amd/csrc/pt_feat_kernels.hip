// pt_feat_kernels.hip -- k_pt_pass for flattened scenes whose session collects the denoiser's albedo and normal guides
// (FEAT = true: device/dpath.h path_step), in a translation unit of their own: what kernels.h pt_variant_compiled leaves of
// k_pt_pass with FEAT on.
#include "pt_launch.h"

namespace akr {

hipError_t pt_pass_entry_feat(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream) { return pt_pass_entry_t<false, false, true>(q, v, blocks, lds, stream); }

}  // namespace akr
