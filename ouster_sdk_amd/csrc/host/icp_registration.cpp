// icp_registration.cpp -- mapping::ICPRegistration, build_linear_system and AdaptiveThreshold (include/ouster/mapping/*.h) over the C
// ABI: ouster_hip_registration_*.  The C ABI refuses what it refuses, in its order and with its messages, before a GPU is asked for.
#include "ouster/mapping/icp_registration.h"

#include <stdexcept>
#include <thread>

#include "host_internal.h"
#include "ouster/mapping/adaptive_threshold.h"

namespace ouster {
namespace sdk {
namespace mapping {
namespace {

void check(int rc) {
    if (rc == OUSTER_HIP_OK) return;
    if (rc == OUSTER_HIP_ERR_INVALID_ARGUMENT) throw std::invalid_argument(ouster_hip_last_error());
    throw std::runtime_error(ouster_hip_last_error());
}

const double kNone[3] = {0, 0, 0};   // an empty frame still needs somewhere to point; it is never read

core::Matrix4dR align(const ICPRegistration& reg, const double* rows, std::size_t n, std::size_t stride, bool device_rows,
                      const core::VoxelHashMap3d& map, double max_distance, double kernel_scale) {
    if (!map.handle()) throw std::runtime_error("VoxelHashMap3d: moved from");
    ouster_hip_registration_desc d{};
    d.max_iterations = reg.max_num_iterations_;
    d.convergence_criterion = reg.convergence_criterion_;
    d.max_distance = max_distance, d.kernel_scale = kernel_scale;
    const auto* h = static_cast<const ouster_hip_voxel_map*>(map.handle());
    check(device_rows ? ouster_hip_registration_align(h, rows, OUSTER_HIP_F64, n, stride, &d)
                      : ouster_hip_registration_align_host(h, n ? rows : kNone, OUSTER_HIP_F64, n, stride, &d));
    return core::Matrix4dR::FromRowMajor(d.pose);
}

}  // namespace

LinearSystem build_linear_system(const Correspondences& correspondences, double kernel_scale) {
    std::vector<double> s(3 * correspondences.size() + 3), t(3 * correspondences.size() + 3);
    for (std::size_t i = 0; i < correspondences.size(); ++i)
        for (int c = 0; c < 3; ++c) s[3 * i + c] = correspondences[i].first[c], t[3 * i + c] = correspondences[i].second[c];
    LinearSystem out;
    check(ouster_hip_build_linear_system_ref(s.data(), t.data(), correspondences.size(), kernel_scale, out.first.data(), out.second.data()));
    return out;
}

ICPRegistration::ICPRegistration(int max_num_iteration, double convergence_criterion, int max_num_threads)
    : max_num_iterations_(max_num_iteration),
      convergence_criterion_(convergence_criterion),
      max_num_threads_(max_num_threads > 0 ? max_num_threads : static_cast<int>(std::thread::hardware_concurrency() ? std::thread::hardware_concurrency() : 1)) {}

core::Matrix4dR ICPRegistration::align_points_to_map(const core::ArrayX3dR& frame, const core::VoxelHashMap3d& voxel_map, double max_distance,
                                                     double kernel_scale) const {
    return align(*this, frame.data(), frame.rows(), 3, false, voxel_map, max_distance, kernel_scale);
}

core::Matrix4dR ICPRegistration::align_points_to_map(const std::vector<Point3d>& frame, const core::VoxelHashMap3d& voxel_map,
                                                     double max_distance, double kernel_scale) const {
    return align(*this, frame.empty() ? kNone : frame.front().data(), frame.size(), 3, false, voxel_map, max_distance, kernel_scale);
}

core::Matrix4dR ICPRegistration::align_device_points_to_map(const double* rows, std::size_t n, std::size_t row_stride,
                                                            const core::VoxelHashMap3d& voxel_map, double max_distance, double kernel_scale) const {
    return align(*this, rows, n, row_stride, true, voxel_map, max_distance, kernel_scale);
}

core::Matrix4dR ICPRegistration::align_array_to_map(const double* rows, std::size_t n, const core::VoxelHashMap3d& voxel_map, double max_distance,
                                                    double kernel_scale) const {
    return align(*this, rows, n, 3, false, voxel_map, max_distance, kernel_scale);
}

void AdaptiveThreshold::update_model_deviation(const core::mat4d& current_deviation) {
    const double model_error = ouster_hip_registration_model_error(current_deviation.data(), max_range_);
    if (model_error > min_motion_threshold_) {
        model_sse_ += model_error * model_error;
        num_samples_++;
    }
}

}  // namespace mapping
}  // namespace sdk
}  // namespace ouster
