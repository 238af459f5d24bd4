/**
 * @file
 * @brief Surface normals of a destaggered point cloud, on the GPU.
 *
 * The call shapes, defaults and error messages of the reference's ouster/algorithm/normals.h.  The work runs on the GPU
 * (csrc/k_normals.hip) through ouster_hip_normals_host; everything that can be refused is refused on the host first.  The result
 * equals a float64 restatement of the reference that rounds every operation on its own (tests/normals_model.py), bit for bit.
 *
 * Clouds that are already in device memory go through the C ABI, ouster_hip_normals (ouster_hip.h); a resident batch has
 * hip::DeviceFrameBatch::normals / normals_device / download_normals (hip/device_batch.h), which read its staggered planes and
 * clouds in place.  hip::FrameStream and hip::ShardedBatch are not in this change: they have no normals method yet.
 */
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>

#include "ouster/core/typedefs.h"
#include "ouster/core/visibility.h"

namespace ouster {
namespace sdk {
namespace algorithm {

/// Default target neighbour distance in meters (25 mm).
constexpr double DEFAULT_TARGET_DISTANCE_METER = 0.025;
/// Default minimum incidence angle (1 deg, ~0.01745 rad) used for AOI gating.
constexpr double DEFAULT_MIN_ANGLE_INCIDENCE_RAD = 1 * 3.14159265358979323846 / 180.0;

/**
 * Normals of a single return.
 *
 * @param[in] xyz destaggered cloud, (H * W, 3)
 * @param[in] range destaggered range image, (H, W)
 * @param[in] sensor_origins_xyz per-column sensor origins in the frame of the points, (W, 3); zeros for a sensor-frame cloud
 * @param[in] pixel_search_range axial pixel radius of the neighbour search
 * @param[in] min_angle_of_incidence_rad minimum angle between a beam and the surface
 * @param[in] target_distance_m neighbour distance the search aims for
 * @throws std::runtime_error "normals: xyz dimensions mismatch", "normals: sensor_origins size must match image width",
 *         "normals: target_distance_m must be positive", "normals: min_angle_of_incidence_rad must be positive"
 * @return (H * W, 3) normals, row-major, zero where none could be made
 */
OUSTER_API_FUNCTION
core::ArrayX3dR normals(const core::PointCloudXYZd& xyz, const core::img_t<uint32_t>& range,
                        const core::ArrayX3dR& sensor_origins_xyz, size_t pixel_search_range = 1,
                        double min_angle_of_incidence_rad = DEFAULT_MIN_ANGLE_INCIDENCE_RAD,
                        double target_distance_m = DEFAULT_TARGET_DISTANCE_METER);

/**
 * Normals of both returns; each return's pixels are neighbour candidates of the other, and the vertical pixel subtent of the
 * first return serves both.  Additionally throws "normals: range2 dimensions mismatch".
 *
 * @return (first return's normals, second return's normals)
 */
OUSTER_API_FUNCTION
std::pair<core::ArrayX3dR, core::ArrayX3dR> normals(const core::PointCloudXYZd& xyz, const core::img_t<uint32_t>& range,
                                                    const core::PointCloudXYZd& xyz2, const core::img_t<uint32_t>& range2,
                                                    const core::ArrayX3dR& sensor_origins_xyz, size_t pixel_search_range = 1,
                                                    double min_angle_of_incidence_rad = DEFAULT_MIN_ANGLE_INCIDENCE_RAD,
                                                    double target_distance_m = DEFAULT_TARGET_DISTANCE_METER);

namespace impl {
/** The two overloads on plain arrays (what the Python binding calls): xyz2 == range2 == nullptr selects the single form.
 *  Shapes are checked as the overloads check them; out / out2 are (h * w, 3). */
OUSTER_API_FUNCTION
void normals_arrays(const double* xyz, size_t xyz_rows, const uint32_t* range, size_t h, size_t w, const double* xyz2,
                    size_t xyz2_rows, const uint32_t* range2, size_t h2, size_t w2, const double* origins, size_t n_origins,
                    size_t pixel_search_range, double min_angle_of_incidence_rad, double target_distance_m, double* out,
                    double* out2);
}  // namespace impl

}  // namespace algorithm
}  // namespace sdk
}  // namespace ouster
