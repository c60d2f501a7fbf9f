// wf_lens_kernels.hip -- the wavefront schedule's two kernels that generate camera rays, for a camera with a thin lens (LENS = true; device/dpath.h
// generate_ray_lens_from): k_wf_init (sampler family) and k_wf_shade (textures x sampler family x kept or flattened scene x ENV), in a translation
// unit of their own (wf_path.h).
#include "wf_path.h"

namespace akr {

hipError_t wf_init_entry_lens(const PtParams& p, const WfBuffers& wf, hipStream_t stream) { return launch_wf_init_t<true>(p, wf, stream); }
hipError_t wf_shade_entry_lens_env(const PtParams& p, const WfBuffers& wf, uint32_t q_out, hipStream_t stream) { return launch_wf_shade_t<true, true>(p, wf, q_out, stream); }
hipError_t wf_shade_entry_lens(const PtParams& p, const WfBuffers& wf, uint32_t q_out, hipStream_t stream) { return launch_wf_shade_t<false, true>(p, wf, q_out, stream); }

}  // namespace akr
