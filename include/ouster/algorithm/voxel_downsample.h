/**
 * @file
 * @brief Voxel-grid down-sampling of a cloud with its normals, on the GPU.
 *
 * The call shape and messages of the reference's ouster/algorithm/voxel_downsample.h.  The work runs on the GPU
 * (csrc/k_voxel.hip) through ouster_hip_voxel_downsample_host; the result equals tests/voxel_model.py bit for bit.  Rows come in
 * first-seen order (the reference: its hash map's iteration order); a point that takes part and whose voxel index no int32 holds
 * is refused with std::invalid_argument, as is a non-finite voxel_size.
 *
 * A resident batch has hip::DeviceFrameBatch::voxel_downsample_with_normals (hip/device_batch.h).
 */
#pragma once

#include <cstddef>
#include <utility>

#include "ouster/core/typedefs.h"
#include "ouster/core/visibility.h"

namespace ouster {
namespace sdk {
namespace algorithm {

/**
 * Average points and unit normals per voxel.  Rows with a non-finite point or normal coordinate, or a normal no longer than
 * 1e-12, take no part; a voxel whose summed unit normals are no longer than 1e-12 is dropped.
 *
 * @param[in] points (N, 3)
 * @param[in] normals (N, 3), normal i belongs to point i; any length
 * @param[in] voxel_size edge of a voxel
 * @throws std::invalid_argument "voxel_downsample_with_normals expects Nx3 inputs", "voxel_downsample_with_normals
 *         points/normals size mismatch", "voxel_downsample_with_normals voxel_size must be > 0"
 * @return (mean point, renormalised mean normal) per voxel, (M, 3) each
 */
OUSTER_API_FUNCTION
std::pair<core::ArrayX3dR, core::ArrayX3dR> voxel_downsample_with_normals(const core::ArrayX3dR& points,
                                                                          const core::ArrayX3dR& normals, double voxel_size);

namespace impl {
/** The same on plain arrays (what the Python binding calls); out_points / out_normals hold `rows` rows.  Returns the rows written. */
OUSTER_API_FUNCTION
std::size_t voxel_downsample_with_normals_arrays(const double* points, std::size_t rows, std::size_t cols, const double* normals,
                                                 std::size_t normal_rows, std::size_t normal_cols, double voxel_size,
                                                 double* out_points, double* out_normals);
}  // namespace impl

}  // namespace algorithm
}  // namespace sdk
}  // namespace ouster
