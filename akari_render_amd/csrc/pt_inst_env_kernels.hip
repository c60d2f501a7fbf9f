// pt_inst_env_kernels.hip -- k_pt_pass_inst of kept scenes with an environment light (ENV = true; device/denv.h): force_diffuse x textures x
// sampler family, in a translation unit of their own (pt_inst_kernel.h). launch_pt_pass_inst (pt_inst_kernels.hip) hands such scenes here.
#include "pt_inst_kernel.h"

namespace akr {

hipError_t launch_pt_pass_inst_env(const PtParams& p, hipStream_t stream) { return launch_pt_pass_inst_t<true>(p, stream); }

}  // namespace akr
