// voxel_dev.h -- the device functions the cell tables of k_voxel.hip (voxels) and k_icp.hip (the target grid of ICP) share: the
// hash of a cell triple, the finite test, and the cell of a coordinate.  A table built by k_voxel_insert is probed with voxel_hash.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_voxel.h"

namespace ouster_hip_dev {

__device__ __forceinline__ uint32_t voxel_hash(const VoxelKey& k) {
    uint32_t h = ((uint32_t)k.x * 73856093u) ^ ((uint32_t)k.y * 19349669u) ^ ((uint32_t)k.z * 83492791u);
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

__device__ __forceinline__ bool finite3(double x, double y, double z) {
    return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
}

// VoxelHashMap::point_to_voxel for one axis; false where no int32 holds the result (NaN included)
__device__ __forceinline__ bool axis_to_voxel(double p, double inv, int32_t& v) {
    const double f = floor(p * inv);
    if (!(f >= -2147483648.0 && f <= 2147483647.0)) return false;
    v = (int32_t)f;
    return true;
}

}  // namespace ouster_hip_dev
