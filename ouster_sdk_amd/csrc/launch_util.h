// launch_util.h -- host-side launch helpers: launch_with_lds (raise the kernel's dynamic-LDS limit once per kernel and device,
// then launch) and launch_ladder, the run-time-to-template dispatch of the fused decode kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "lds_grant.h"

namespace ouster_hip_dev {

// Everything here is `static`: each file that launches keeps its own copies, and the library exports none of them.
// dynamic LDS above 48 KB needs the kernel's attribute raised; `grant` is that kernel's own (one static LdsGrant per kernel)
template <class K, class... A>
static hipError_t launch_with_lds(K kernel, dim3 grid, dim3 block, size_t lds, int device, hipStream_t st, LdsGrant& grant,
                                  const A&... args) {
    const hipError_t e = grant.ensure(lds, device, [&] {
        return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
    return hipGetLastError();
}

// A kernel family F names its kernels and says which of them exist:
//   template <class S, int T, int XYZM, bool POSES> static constexpr auto kernel = k_...<S, T, XYZM, POSES>;
//   static constexpr bool poses;   // is there a POSES form (taken for XYZM 1 / 2 when the call has poses)?
//   static constexpr bool xyzm3;   // is XYZM == 3 (full LUTs) compiled?  Otherwise it is refused with hipErrorInvalidValue.
// Only the kernels a ladder can reach are instantiated.
template <class F, class S, int T, int XYZM, bool POSES, class... A>
static hipError_t launch_rung(dim3 grid, dim3 block, size_t lds, int device, hipStream_t st, const A&... args) {
    static LdsGrant grant;   // of this kernel instantiation
    return launch_with_lds(F::template kernel<S, T, XYZM, POSES>, grid, block, lds, device, st, grant, args...);
}

template <class F, class S, int T, int XYZM, class... A>
static hipError_t launch_xyzm(bool poses, dim3 grid, dim3 block, size_t lds, int device, hipStream_t st, const A&... args) {
    if constexpr (F::poses && (XYZM == 1 || XYZM == 2)) {
        if (poses) return launch_rung<F, S, T, XYZM, true>(grid, block, lds, device, st, args...);
    }
    return launch_rung<F, S, T, XYZM, false>(grid, block, lds, device, st, args...);
}

// kernel F::kernel<S, T, xyzm, poses>(args...) on `grid` x `block` with `lds` bytes of dynamic LDS
template <class F, class S, int T, class... A>
static hipError_t launch_ladder(int xyzm, bool poses, dim3 grid, dim3 block, size_t lds, int device, hipStream_t st, const A&... args) {
    switch (xyzm) {
        case 0: return launch_xyzm<F, S, T, 0>(poses, grid, block, lds, device, st, args...);
        case 1: return launch_xyzm<F, S, T, 1>(poses, grid, block, lds, device, st, args...);
        case 2: return launch_xyzm<F, S, T, 2>(poses, grid, block, lds, device, st, args...);
        default:
            if constexpr (F::xyzm3) return launch_xyzm<F, S, T, 3>(poses, grid, block, lds, device, st, args...);
            else return hipErrorInvalidValue;
    }
}

}  // namespace ouster_hip_dev
