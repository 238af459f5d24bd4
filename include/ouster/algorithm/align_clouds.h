/**
 * @file
 * @brief Point-to-point and point-to-plane ICP between two clouds, on the GPU.
 *
 * The call shape, defaults and messages of point_to_point_align / point_to_plane_align in the reference's
 * ouster/algorithm/align_clouds.h.  The work runs on the GPU (csrc/k_icp.hip) through ouster_hip_icp_align_host: the
 * correspondences, residuals and median of every pass equal tests/icp_model.py bit for bit; the sums behind each solve are reduced
 * in a tree of fixed shape, so a result depends on its inputs only, but is not the reference's left fold bit for bit.  A target
 * point that takes part and whose cell (edge max_corr_dist) no int32 holds is refused with std::invalid_argument.
 *
 * The frame-level align_clouds overloads of the reference are not built.  A resident batch has
 * hip::DeviceFrameBatch::align_voxels (hip/device_batch.h).
 */
#pragma once

#include <cstddef>
#include <cstdint>

#include "ouster/core/typedefs.h"
#include "ouster/core/visibility.h"

namespace ouster {
namespace sdk {
namespace core {
using Matrix4dR = mat4d;   ///< typedefs.h of the reference: a row-major 4x4 of double
}  // namespace core

namespace algorithm {

/**
 * Rigid transform that moves source_points onto target_points by point-to-point ICP: up to 10 passes of nearest neighbours
 * within max_corr_dist, Huber weights from the median residual, and a Kabsch step.
 *
 * @param[in] source_points (N, 3)
 * @param[in] target_points (M, 3)
 * @param[in] initial_guess starting transform
 * @param[in] max_corr_dist largest distance of a correspondence; also the cell of the search grid
 * @throws std::invalid_argument "max_corr_dist must be finite and greater than zero"
 * @return the transform; initial_guess with fewer than 20 points on a side or fewer than 20 correspondences in the first pass
 */
OUSTER_API_FUNCTION
core::Matrix4dR point_to_point_align(const core::ArrayX3dR& source_points, const core::ArrayX3dR& target_points,
                                     const core::Matrix4dR& initial_guess = core::Matrix4dR::Identity(), double max_corr_dist = 0.25);

/**
 * The same by point-to-plane ICP: correspondences are also gated by the angle between the normals, and a pass solves one 6x6
 * Gauss-Newton step on SE(3).  Rows with a non-finite normal or one no longer than 1e-12 take no part.
 *
 * @param[in] source_normals (N, 3), any length
 * @param[in] target_normals (M, 3), any length
 * @param[in] max_normal_angle_deg largest angle between a source normal and its neighbour's, up to sign
 * @throws std::invalid_argument the message above, "max_normal_angle_deg must be finite and in [0, 180]", "source_points and
 *         source_normals must have the same number of rows", "target_points and target_normals must have the same number of rows"
 */
OUSTER_API_FUNCTION
core::Matrix4dR point_to_plane_align(const core::ArrayX3dR& source_points, const core::ArrayX3dR& target_points,
                                     const core::ArrayX3dR& source_normals, const core::ArrayX3dR& target_normals,
                                     const core::Matrix4dR& initial_guess = core::Matrix4dR::Identity(), double max_corr_dist = 0.25,
                                     double max_normal_angle_deg = 20.0);

namespace impl {
/** What a call reports next to the pose. */
struct AlignStats {
    uint32_t iterations = 0;         ///< passes that were run
    uint64_t correspondences = 0;    ///< of the last pass
    bool solved = false;             ///< some pass had at least 20 correspondences
};
/** The same on plain row-major arrays (what the Python binding calls): (rows, 3) clouds, normals nullptr on both sides for point to
 *  point, 16 doubles for the guess and the result. */
OUSTER_API_FUNCTION
AlignStats align_arrays(const double* source_points, std::size_t source_rows, const double* target_points, std::size_t target_rows,
                        const double* source_normals, std::size_t source_normal_rows, const double* target_normals,
                        std::size_t target_normal_rows, const double* initial_guess16, double max_corr_dist,
                        double max_normal_angle_deg, double* pose16);
}  // namespace impl

}  // namespace algorithm
}  // namespace sdk
}  // namespace ouster
