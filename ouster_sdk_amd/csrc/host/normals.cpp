// normals.cpp -- algorithm::normals over the C ABI (include/ouster/algorithm/normals.h).  Shapes and parameters are refused on
// the host first, in the reference's order and with its messages (ouster_algorithm/src/normals.cpp:84-89, 412-417, 436-445), as
// std::runtime_error; then the GPU is asked for and ouster_hip_normals_host does the work.
#include "ouster/algorithm/normals.h"

#include <algorithm>
#include <limits>
#include <stdexcept>

#include "host_internal.h"

namespace ouster {
namespace sdk {
namespace algorithm {
namespace impl {

void normals_arrays(const double* xyz, size_t xyz_rows, const uint32_t* range, size_t h, size_t w, const double* xyz2,
                    size_t xyz2_rows, const uint32_t* range2, size_t h2, size_t w2, const double* origins, size_t n_origins,
                    size_t pixel_search_range, double min_angle_of_incidence_rad, double target_distance_m, double* out,
                    double* out2) {
    const bool dual = xyz2 || range2;
    if (xyz_rows != h * w || (dual && xyz2_rows != h * w)) throw std::runtime_error("normals: xyz dimensions mismatch");
    if (dual && (h2 != h || w2 != w)) throw std::runtime_error("normals: range2 dimensions mismatch");
    if (n_origins != w) throw std::runtime_error("normals: sensor_origins size must match image width");
    ouster_hip_normals_consts unused;
    if (ouster_hip_normals_constants(w ? static_cast<uint32_t>(w) : 1, h ? static_cast<uint32_t>(h) : 1, min_angle_of_incidence_rad,
                                     target_distance_m, 0, 0.0, 0, &unused) != OUSTER_HIP_OK)
        throw std::runtime_error(ouster_hip_last_error());
    if (h * w == 0) return;
    if (h > 0xffffffffu || w > 0xffffffffu) throw std::runtime_error("normals: image too large");
    ouster_hip_normals_desc d{};
    d.xyz = xyz, d.range = range, d.xyz2 = xyz2, d.range2 = range2;
    d.normals = out, d.normals2 = out2;
    d.sensor_origins = origins;
    d.xyz_rows = xyz_rows, d.xyz2_rows = xyz2_rows;
    d.n_frames = 1, d.h = static_cast<uint32_t>(h), d.w = static_cast<uint32_t>(w);
    d.range2_h = static_cast<uint32_t>(h2), d.range2_w = static_cast<uint32_t>(w2);
    d.n_origins = static_cast<uint32_t>(n_origins);
    d.pixel_search_range = static_cast<uint32_t>(std::min<size_t>(pixel_search_range, std::numeric_limits<uint32_t>::max()));
    d.xyz_dtype = OUSTER_HIP_F64;
    d.min_angle_of_incidence_rad = min_angle_of_incidence_rad, d.target_distance_m = target_distance_m;
    ouster_hip_ctx* ctx = hip::default_ctx();   // throws without a GPU
    const int rc = ouster_hip_normals_host(ctx, &d);
    if (rc != OUSTER_HIP_OK) throw std::runtime_error(ouster_hip_last_error());
}

}  // namespace impl

core::ArrayX3dR normals(const core::PointCloudXYZd& xyz, const core::img_t<uint32_t>& range,
                        const core::ArrayX3dR& sensor_origins_xyz, size_t pixel_search_range, double min_angle_of_incidence_rad,
                        double target_distance_m) {
    core::ArrayX3dR out(range.rows() * range.cols());
    impl::normals_arrays(xyz.data(), xyz.rows(), range.data(), range.rows(), range.cols(), nullptr, 0, nullptr, 0, 0,
                         sensor_origins_xyz.data(), sensor_origins_xyz.rows(), pixel_search_range, min_angle_of_incidence_rad,
                         target_distance_m, out.data(), nullptr);
    return out;
}

std::pair<core::ArrayX3dR, core::ArrayX3dR> normals(const core::PointCloudXYZd& xyz, const core::img_t<uint32_t>& range,
                                                    const core::PointCloudXYZd& xyz2, const core::img_t<uint32_t>& range2,
                                                    const core::ArrayX3dR& sensor_origins_xyz, size_t pixel_search_range,
                                                    double min_angle_of_incidence_rad, double target_distance_m) {
    std::pair<core::ArrayX3dR, core::ArrayX3dR> out{core::ArrayX3dR(range.rows() * range.cols()),
                                                    core::ArrayX3dR(range.rows() * range.cols())};
    // an empty second return still selects the dual form: its shape checks come first
    static const double no_xyz = 0.0;
    static const uint32_t no_range = 0;
    impl::normals_arrays(xyz.data(), xyz.rows(), range.data(), range.rows(), range.cols(), xyz2.data() ? xyz2.data() : &no_xyz,
                         xyz2.rows(), range2.data() ? range2.data() : &no_range, range2.rows(), range2.cols(),
                         sensor_origins_xyz.data(), sensor_origins_xyz.rows(), pixel_search_range, min_angle_of_incidence_rad,
                         target_distance_m, out.first.data(), out.second.data());
    return out;
}

}  // namespace algorithm
}  // namespace sdk
}  // namespace ouster
