// icp_sums_dev.h -- the workgroup's part of the fixed-shape sum tree that k_icp.hip and k_registration.hip share: a
// workgroup of ICP_WG threads owns ICP_CHUNK consecutive rows, each thread folds its rows in order, then block_sums.  Device only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_icp.h"

#ifdef __HIPCC__
namespace ouster_hip_dev {
namespace {

// acc[NS] of every thread of the workgroup -> partials[chunk][ofs .. ofs + NS): wave butterfly, then the waves in order
template <int NS>
__device__ __forceinline__ void block_sums(double (&acc)[NS], double* partial) {
    __shared__ double lds[ICP_WG / 64][NS];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int s = 0; s < NS; ++s) acc[s] = acc[s] + __shfl_xor(acc[s], off, 64);
    const uint32_t wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    if (lane == 0)
#pragma unroll
        for (int s = 0; s < NS; ++s) lds[wave][s] = acc[s];
    __syncthreads();
    if (threadIdx.x < NS) {
        double v = lds[0][threadIdx.x];
        for (uint32_t w = 1; w < ICP_WG / 64; ++w) v = v + lds[w][threadIdx.x];
        partial[threadIdx.x] = v;
    }
}

}  // namespace
}  // namespace ouster_hip_dev
#endif
