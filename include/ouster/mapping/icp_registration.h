/**
 * @file
 * @brief Frame-to-map registration against the resident voxel map, on the GPU.
 *
 * The call shape, members and defaults of the reference's ouster/mapping/icp_registration.h.  align_points_to_map runs on the GPU
 * (csrc/k_registration.hip through ouster_hip_registration_align_host, ouster_hip.h): one kernel per pass moves the cloud, asks the
 * map and sums the 6 x 6 system; the host solves between the passes.  On a map made with VoxelHashMap3d::on_host the whole
 * algorithm runs on one core.  Results are held to tests/registration_model.py.
 *
 * Deviations from the reference:
 *  - the solve is one L D L^T without pivoting, columns left to right over the lower triangle, where the reference calls Eigen's
 *    pivoting LDLT; Eigen's rule that a zero pivot gives a zero component is kept;
 *  - the sums of a pass are reduced in a tree of fixed shape on the GPU (a left fold on a host map) in place of TBB's
 *    deterministic reduce: a result depends on its inputs only, but is not the reference's bit for bit;
 *  - the rounding orders Eigen leaves open are fixed (squared norms, cross products, the quaternion's rotation of a vector and the
 *    renormalised quaternion product), see the model;
 *  - max_num_threads is stored and has no other effect; 0 reports the hardware concurrency (at least 1);
 *  - refused with std::invalid_argument: a non-finite or negative max_distance, kernel_scale or convergence_criterion; more than
 *    2^30 rows is a std::runtime_error.  A non-finite row or one outside the int32 grid has no correspondence;
 *  - the VoxelHashMapXd overload is not built.
 */
#pragma once

#include <array>
#include <cstddef>
#include <utility>
#include <vector>

#include "ouster/core/typedefs.h"
#include "ouster/core/visibility.h"
#include "ouster/core/voxel_hash_map.h"

namespace ouster {
namespace sdk {

namespace mapping {

/// Row-major 6 x 6 / 6 x 1 of double: operator()(r, c), data().
struct Matrix6d {
    double m[36] = {};
    double& operator()(int r, int c) { return m[r * 6 + c]; }
    double operator()(int r, int c) const { return m[r * 6 + c]; }
    const double* data() const { return m; }
    double* data() { return m; }
};
struct Vector6d {
    double v[6] = {};
    double& operator()(int i) { return v[i]; }
    double operator()(int i) const { return v[i]; }
    const double* data() const { return v; }
    double* data() { return v; }
};
using Point3d = core::VoxelHashMap3d::point_type;
using Correspondences = std::vector<std::pair<Point3d, Point3d>>;   ///< (source, target)
using LinearSystem = std::pair<Matrix6d, Vector6d>;                ///< (JtJ with the lower triangle filled, Jtr)

/// The reference's build_linear_system with Geman-McClure weights; left-fold sums on the host.
/// @throws std::invalid_argument for a non-finite or negative kernel_scale
OUSTER_API_FUNCTION
LinearSystem build_linear_system(const Correspondences& correspondences, double kernel_scale);

class OUSTER_API_CLASS ICPRegistration {
   public:
    OUSTER_API_FUNCTION
    explicit ICPRegistration(int max_num_iteration = 50, double convergence_criterion = 0.0001, int max_num_threads = 0);

    /// Align an (N, 3) frame to the map.  @return the transform; the identity for an empty map, an empty frame or no iterations
    OUSTER_API_FUNCTION
    core::Matrix4dR align_points_to_map(const core::ArrayX3dR& frame, const core::VoxelHashMap3d& voxel_map, double max_distance,
                                        double kernel_scale) const;
    OUSTER_API_FUNCTION
    core::Matrix4dR align_points_to_map(const std::vector<Point3d>& frame, const core::VoxelHashMap3d& voxel_map, double max_distance,
                                        double kernel_scale) const;
    /// Rows already in device memory: rows[n][row_stride] of double, on the map's device.
    OUSTER_API_FUNCTION
    core::Matrix4dR align_device_points_to_map(const double* rows, std::size_t n, std::size_t row_stride, const core::VoxelHashMap3d& voxel_map,
                                               double max_distance, double kernel_scale) const;
    /// On a plain row-major host array (what the Python binding calls)
    OUSTER_API_FUNCTION
    core::Matrix4dR align_array_to_map(const double* rows, std::size_t n, const core::VoxelHashMap3d& voxel_map, double max_distance,
                                       double kernel_scale) const;

    int max_num_iterations_;
    double convergence_criterion_;
    int max_num_threads_;
};

}  // namespace mapping
}  // namespace sdk
}  // namespace ouster
