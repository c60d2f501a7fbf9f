// pt_punct_tree_env_kernels.hip -- k_pt_pass for flattened scenes with punctual lights and a light tree over the point and spot ones (PUNCT = LTREE = true:
// device/dlighttree.h) with an environment light (ENV = true), in a translation unit of their own: the kernels of
// pt_punct_env_kernels.hip with the walk in them, so that those stay what they were.
#include "pt_launch.h"

namespace akr {

hipError_t pt_pass_entry_punct_tree_env(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream) { return pt_pass_entry_t<true, false, false, true, true>(q, v, blocks, lds, stream); }

}  // namespace akr
