// pt_unit_kernels.hip -- the precompiled pt kernels, one translation unit per unit: the build compiles this file kPtUnits times with
// -DAKR_PT_UNIT=<index> (build.py PT_UNITS), each time for the kernels of one (kind, ENV, LENS) and nothing else (kernels.h PtKind,
// pt_unit_flags): what pt_variant_compiled leaves of k_pt_pass (pt_launch.h) or k_pt_pass_inst (pt_inst_kernel.h) with the unit's flags
// fixed. launch_pt_pass (pt_kernels.hip) names all kPtUnits entry points: a unit the build leaves out is an undefined symbol when the
// library is linked or loaded, one it adds beyond kPtUnits does not compile.
#include "pt_inst_kernel.h"

#ifndef AKR_PT_UNIT
#error "pt_unit_kernels.hip is compiled once per unit, with -DAKR_PT_UNIT=<unit index> (build.py PT_UNITS)"
#endif

namespace akr {

template <uint32_t UNIT>
hipError_t pt_pass_entry_unit(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream) {
    static_assert(UNIT < kPtUnits, "build.py compiles a unit that kernels.h does not have");
    constexpr PtVariant U = pt_unit_flags(UNIT);
    if constexpr (U.inst) return pt_pass_entry_inst_t<U.env, U.lens>(q, v, blocks, lds, stream);
    else return pt_pass_entry_t<U.env, U.lens, U.feat, U.punct, U.ltree>(q, v, blocks, lds, stream);
}
template hipError_t pt_pass_entry_unit<AKR_PT_UNIT>(const PtParams& q, const PtVariant& v, uint32_t blocks, size_t lds, hipStream_t stream);

}  // namespace akr
