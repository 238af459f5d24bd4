/**
 * @file
 * @brief Voxel-grid down-sampling of a point cloud, on the GPU.
 *
 * Of the reference's ouster/core/voxel_hash_map.h this header carries VoxelDownsampleStrategy, voxel_downsample_3d and
 * voxel_downsample_xd, with its signatures, defaults and messages.  The work runs on the GPU (csrc/k_voxel.hip) through
 * ouster_hip_voxel_downsample_host; FIRST_N_POINT and RANDOM with max_points_per_voxel > 1 are sequential by nature and run the
 * host restatement (ouster_hip_voxel_downsample_ref).  Results equal tests/voxel_model.py bit for bit.
 *
 * Deviations from the reference: rows come in first-seen order (voxels by the input index of their first contributing point),
 * where the reference emits its hash map's iteration order; a non-finite voxel_size, a non-finite coordinate among the first three
 * columns and one whose voxel index no int32 holds are refused with std::invalid_argument (undefined behaviour there).
 * VoxelHashMap itself (a persistent, updatable map) and the legacy core::voxel_downsample(std::vector<Vector3d>, ...) are not here.
 *
 * Clouds already in device memory go through the C ABI, ouster_hip_voxel_downsample (ouster_hip.h); a resident batch has
 * hip::DeviceFrameBatch::voxel_downsample over its dewarped cloud (hip/device_batch.h).
 */
#pragma once

#include <cstddef>
#include <cstdint>

#include "ouster/core/typedefs.h"
#include "ouster/core/visibility.h"

namespace ouster {
namespace sdk {
namespace core {

using ArrayXXdR = ArrayXXR<double>;   ///< typedefs.h of the reference

/// What a voxel's points are reduced to.
enum class VoxelDownsampleStrategy {
    FIRST_N_POINT,  ///< First n points in a voxel are kept (where n is max_points_per_voxel)
    AVERAGE_POINT,  ///< Compute the average of all points in a voxel
    RANDOM,         ///< Up to n points per voxel; a point that finds its voxel full replaces a pseudo-random slot
};

/**
 * Down-sample an (N, 3) cloud.
 *
 * @param[in] frame points, one per row
 * @param[in] voxel_size edge of a voxel
 * @param[in] max_points_per_voxel points a voxel keeps (FIRST_N_POINT, RANDOM)
 * @param[in] min_pts_threshold points a voxel needs to be emitted (AVERAGE_POINT)
 * @param[in] strategy the reduction
 * @throws std::invalid_argument "max_points_per_voxel must be greater than 0", "voxel_size must be greater than 0",
 *         "voxel_downsample: point outside the int32 voxel grid"
 * @return (M, 3), M <= N; an empty frame gives an empty result before anything is checked
 */
OUSTER_API_FUNCTION
ArrayX3dR voxel_downsample_3d(const ArrayX3dR& frame, double voxel_size, std::size_t max_points_per_voxel = 1,
                              std::size_t min_pts_threshold = 1,
                              VoxelDownsampleStrategy strategy = VoxelDownsampleStrategy::RANDOM);

/**
 * Down-sample an (N, 3 + A) cloud: x, y, z and A attribute columns, which are averaged or selected with their point.
 * Additionally throws "voxel_downsample_xd: frame must be Nx>=3 (x,y,z + optional attributes)".
 */
OUSTER_API_FUNCTION
ArrayXXdR voxel_downsample_xd(const ArrayXXdR& frame, double voxel_size, std::size_t max_points_per_voxel = 1,
                              std::size_t min_pts_threshold = 1,
                              VoxelDownsampleStrategy strategy = VoxelDownsampleStrategy::RANDOM);

namespace impl {
/** Both functions on a plain array (what the Python binding calls): rows x cols doubles, dense.  three_d: cols must be 3
 *  ("voxel_downsample_3d: frame must be Nx3").  Returns the rows written to `out`, which holds `rows` rows.  Throws as the
 *  functions above. */
OUSTER_API_FUNCTION
std::size_t voxel_downsample_arrays(const double* frame, std::size_t rows, std::size_t cols, double voxel_size,
                                    std::size_t max_points_per_voxel, std::size_t min_pts_threshold,
                                    VoxelDownsampleStrategy strategy, bool three_d, double* out);
}  // namespace impl

}  // namespace core
}  // namespace sdk
}  // namespace ouster
