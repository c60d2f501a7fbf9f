// pt_kernels_relaxed.hip -- k_pt_pass in the RELAXED arithmetic tier (option `arith` = 1; device/dmath.h AKR_ARITH_RELAXED).
//
// The same source as the plain unit's instantiations (pt_unit_kernels.hip, PT_KIND_PLAIN without ENV and LENS) -- pt_pass.h, every device header -- compiled a second time with
// -ffp-contract=fast, without correctly rounded division / square root, with denormals flushed (build.py RELAXED_FLAGS) and
// with AKR_ARITH_RELAXED = 1, inside another namespace so that neither the kernels nor a header's inline function can be
// mistaken for the contract-bound ones at link time. Films are not the oracle's to the bit, and at fixed seed not within
// north_star's relRMSE < 1e-3 either except on the headline configuration's shard (1e-5 .. 4e-5 outside the few pixels
// where a sample takes another decision, 8e-4 .. 9e-3 with them; tests/test_gpu_relaxed.py): the bit-exact tier stays the default and
// is what verifies this one. The entry point is pt_launch.h's; which sessions come here is decided in akr_pt_begin (host/api_pt.cpp).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

#define AKR_ARITH_RELAXED 1
#define akr akr_rx
#include "pt_launch.h"
#undef akr

// params: the parameter block with the layout's offsets filled in (launch_pt_pass_relaxed, pt_kernels.hip); it is akr::PtParams, in this namespace
extern "C" hipError_t akr_launch_pt_pass_relaxed(const void* params, const PtVariant* v, uint32_t blocks, size_t lds, hipStream_t stream) {
    return akr_rx::pt_pass_entry_t<false, false>(*static_cast<const akr_rx::PtParams*>(params), *v, blocks, lds, stream);  // (refuses inst, env, lens)
}
