// pt_lens_env_kernels.hip -- k_pt_pass for flattened scenes with an environment light seen through a thin lens (ENV = true, LENS = true), in a
// translation unit of their own. launch_pt_pass_lens (pt_lens_kernels.hip) hands such scenes here.
#include "pt_launch.h"

namespace akr {

hipError_t launch_pt_pass_lens_env(const PtParams& p, hipStream_t stream) { return launch_pt_pass_t<true, true>(p, stream); }

}  // namespace akr
