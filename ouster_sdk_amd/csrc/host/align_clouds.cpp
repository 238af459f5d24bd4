// align_clouds.cpp -- algorithm::point_to_point_align / point_to_plane_align (include/ouster/algorithm/align_clouds.h) over the C
// ABI.  Parameters and shapes are refused on the host first, in the reference's order and with its messages, as
// std::invalid_argument; clouds of fewer than 20 rows return the guess without a GPU; then the GPU is asked for and
// ouster_hip_icp_align_host does the work.
#include "ouster/algorithm/align_clouds.h"

#include <cmath>
#include <cstring>
#include <stdexcept>

#include "host_internal.h"

namespace ouster {
namespace sdk {
namespace algorithm {
namespace impl {

AlignStats align_arrays(const double* source_points, std::size_t source_rows, const double* target_points, std::size_t target_rows,
                        const double* source_normals, std::size_t source_normal_rows, const double* target_normals,
                        std::size_t target_normal_rows, const double* initial_guess16, double max_corr_dist,
                        double max_normal_angle_deg, double* pose16) {
    const bool plane = source_normals != nullptr || target_normals != nullptr;
    // what the C ABI refuses, in its order, before a GPU is asked for
    if (!std::isfinite(max_corr_dist) || max_corr_dist <= 0.0)
        throw std::invalid_argument("max_corr_dist must be finite and greater than zero");
    if (plane) {
        if (!std::isfinite(max_normal_angle_deg) || max_normal_angle_deg < 0.0 || max_normal_angle_deg > 180.0)
            throw std::invalid_argument("max_normal_angle_deg must be finite and in [0, 180]");
        if (source_rows != source_normal_rows)
            throw std::invalid_argument("source_points and source_normals must have the same number of rows");
        if (target_rows != target_normal_rows)
            throw std::invalid_argument("target_points and target_normals must have the same number of rows");
    }
    ouster_hip_icp_desc d{};
    static const double none[3] = {0, 0, 0};   // an empty cloud still needs somewhere to point
    d.source_points = source_rows ? source_points : none, d.target_points = target_rows ? target_points : none;
    if (plane) {
        d.source_normals = source_rows ? source_normals : none, d.target_normals = target_rows ? target_normals : none;
        d.n_source_normals = source_normal_rows, d.n_target_normals = target_normal_rows;
    }
    d.n_source = source_rows, d.n_target = target_rows;
    d.dtype = OUSTER_HIP_F64;
    std::memcpy(d.initial_guess, initial_guess16, sizeof d.initial_guess);
    d.max_corr_dist = max_corr_dist, d.max_normal_angle_deg = max_normal_angle_deg;
    // fewer than 20 rows on a side: the guess, and no GPU is needed for that
    const bool small = source_rows < 20 || target_rows < 20;
    const int rc = ouster_hip_icp_align_host(small ? nullptr : hip::default_ctx() /* throws without a GPU */, &d);
    if (rc != OUSTER_HIP_OK) {
        if (rc == OUSTER_HIP_ERR_INVALID_ARGUMENT) throw std::invalid_argument(ouster_hip_last_error());
        throw std::runtime_error(ouster_hip_last_error());
    }
    std::memcpy(pose16, d.pose, sizeof d.pose);
    AlignStats s;
    s.iterations = d.iterations, s.correspondences = d.correspondences, s.solved = d.solved != 0;
    return s;
}

}  // namespace impl

core::Matrix4dR point_to_point_align(const core::ArrayX3dR& source_points, const core::ArrayX3dR& target_points,
                                     const core::Matrix4dR& initial_guess, double max_corr_dist) {
    double pose[16];
    impl::align_arrays(source_points.data(), source_points.rows(), target_points.data(), target_points.rows(), nullptr, 0, nullptr, 0,
                       initial_guess.data(), max_corr_dist, 20.0, pose);
    return core::Matrix4dR::FromRowMajor(pose);
}

core::Matrix4dR point_to_plane_align(const core::ArrayX3dR& source_points, const core::ArrayX3dR& target_points,
                                     const core::ArrayX3dR& source_normals, const core::ArrayX3dR& target_normals,
                                     const core::Matrix4dR& initial_guess, double max_corr_dist, double max_normal_angle_deg) {
    static const double none[3] = {0, 0, 0};
    double pose[16];
    // an empty normals array still selects the point-to-plane checks
    impl::align_arrays(source_points.data(), source_points.rows(), target_points.data(), target_points.rows(),
                       source_normals.rows() ? source_normals.data() : none, source_normals.rows(),
                       target_normals.rows() ? target_normals.data() : none, target_normals.rows(), initial_guess.data(), max_corr_dist,
                       max_normal_angle_deg, pose);
    return core::Matrix4dR::FromRowMajor(pose);
}

}  // namespace algorithm
}  // namespace sdk
}  // namespace ouster
