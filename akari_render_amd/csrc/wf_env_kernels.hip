// wf_env_kernels.hip -- k_wf_shade of scenes with an environment light (ENV = true; device/denv.h): textures x sampler family x kept or
// flattened scene, in a translation unit of their own (wf_path.h).
#include "wf_path.h"

namespace akr {

hipError_t wf_shade_entry_env(const PtParams& p, const WfBuffers& wf, uint32_t q_out, hipStream_t stream) { return launch_wf_shade_t<true, false>(p, wf, q_out, stream); }

}  // namespace akr
