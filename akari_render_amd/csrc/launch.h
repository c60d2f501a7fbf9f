// launch.h -- how a launcher gets from the run-time properties of a scene (BVH or exhaustive, textures, sampler family, ...) to the one
// instantiation of its kernel template that was compiled for them. Host side only: not among the texts embedded for per-scene kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace akr {

// f(c0, c1, ...) with c_i = std::true_type{} or std::false_type{} as b_i says: inside a generic lambda `auto T` gives the constant T().
// Every combination of the flags is instantiated; one that the caller's rule cannot produce is cut there with `if constexpr`.
template <class F>
void dispatch_bools(F&& f) { f(); }
template <class F, class... Bs>
void dispatch_bools(F&& f, bool b0, Bs... rest) {
    if (b0) dispatch_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else dispatch_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

// One-dimensional launch of 256-thread workgroups. BIG_LDS: the launch may need more dynamic LDS than the 64 KB a kernel gets without
// asking (k_pt_pass: deep traversal stacks + graph-value slots + parked columns); the kernel is then allowed what it needs -- a
// workgroup may have all 160 KB of the CU, fewer workgroups fit.
template <bool BIG_LDS = false, class... P, class... A>
void launch_kernel(void (*kernel)(P...), uint32_t blocks, size_t lds, hipStream_t stream, const A&... args) {
    if (BIG_LDS && lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), lds, stream, args...);
}

}  // namespace akr
