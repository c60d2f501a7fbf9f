// pt_inst_lens_kernels.hip -- k_pt_pass_inst of kept scenes seen through a thin lens (LENS = true; device/dpath.h generate_ray_lens_from), without
// and with an environment light: force_diffuse x textures x sampler family x ENV, in a translation unit of their own (pt_inst_kernel.h).
// launch_pt_pass_inst (pt_inst_kernels.hip) hands such scenes here.
#include "pt_inst_kernel.h"

namespace akr {

hipError_t launch_pt_pass_inst_lens(const PtParams& p, hipStream_t stream) {
    if (p.sc.env) return launch_pt_pass_inst_t<true, true>(p, stream);
    return launch_pt_pass_inst_t<false, true>(p, stream);
}

}  // namespace akr
