// voxel_downsample.cpp -- core::voxel_downsample_3d / _xd (include/ouster/core/voxel_hash_map.h) and
// algorithm::voxel_downsample_with_normals (include/ouster/algorithm/voxel_downsample.h) over the C ABI.  Shapes and parameters
// are refused on the host first, in the reference's order and with its messages, as std::invalid_argument; then the GPU is asked
// for and ouster_hip_voxel_downsample_host does the work.  FIRST_N_POINT and RANDOM with max_points_per_voxel > 1 need no GPU:
// they run ouster_hip_voxel_downsample_ref.
#include "ouster/algorithm/voxel_downsample.h"
#include "ouster/core/voxel_hash_map.h"

#include <cmath>
#include <cstring>
#include <stdexcept>

#include "host_internal.h"

namespace ouster {
namespace sdk {
namespace {

[[noreturn]] void throw_last(int rc) {
    if (rc == OUSTER_HIP_ERR_INVALID_ARGUMENT) throw std::invalid_argument(ouster_hip_last_error());
    throw std::runtime_error(ouster_hip_last_error());
}

}  // namespace

namespace core {
namespace impl {

std::size_t voxel_downsample_arrays(const double* frame, std::size_t rows, std::size_t cols, double voxel_size,
                                    std::size_t max_points_per_voxel, std::size_t min_pts_threshold,
                                    VoxelDownsampleStrategy strategy, bool three_d, double* out) {
    if (three_d && cols != 3) throw std::invalid_argument("voxel_downsample_3d: frame must be Nx3");
    if (rows == 0) return 0;   // before any other check, as in the reference
    ouster_hip_voxel_desc d{};
    d.points = frame, d.out = out;
    d.n = rows, d.out_capacity = rows;
    d.cols = static_cast<uint32_t>(cols > 0xffffffffu ? 0xffffffffu : cols);
    d.dtype = OUSTER_HIP_F64;
    d.voxel_size = voxel_size;
    d.max_points_per_voxel = max_points_per_voxel, d.min_pts_threshold = min_pts_threshold;
    d.strategy = static_cast<int32_t>(strategy);
    // what the C ABI refuses, in its order, before a GPU is asked for
    if (cols < 3) throw std::invalid_argument("voxel_downsample_xd: frame must be Nx>=3 (x,y,z + optional attributes)");
    if (strategy != VoxelDownsampleStrategy::FIRST_N_POINT && strategy != VoxelDownsampleStrategy::AVERAGE_POINT &&
        strategy != VoxelDownsampleStrategy::RANDOM)
        throw std::invalid_argument("voxel_downsample: unknown strategy");
    if (max_points_per_voxel == 0) throw std::invalid_argument("max_points_per_voxel must be greater than 0");
    if (!(voxel_size > 0.0) || !std::isfinite(voxel_size)) throw std::invalid_argument("voxel_size must be greater than 0");
    uint64_t n_out = 0;
    // FIRST_N_POINT / RANDOM keeping several points are sequential by nature: host code, no GPU needed
    const bool on_host = strategy != VoxelDownsampleStrategy::AVERAGE_POINT && max_points_per_voxel > 1;
    const int rc = on_host ? ouster_hip_voxel_downsample_ref(&d, &n_out)
                           : ouster_hip_voxel_downsample_host(hip::default_ctx() /* throws without a GPU */, &d, &n_out);
    if (rc != OUSTER_HIP_OK) throw_last(rc);
    return static_cast<std::size_t>(n_out);
}

}  // namespace impl

namespace {
template <class A>
A shrink(const A& full, std::size_t rows, std::size_t cols) {
    A out(rows, cols);
    std::memcpy(out.data(), full.data(), rows * cols * sizeof(double));
    return out;
}
}  // namespace

ArrayX3dR voxel_downsample_3d(const ArrayX3dR& frame, double voxel_size, std::size_t max_points_per_voxel,
                              std::size_t min_pts_threshold, VoxelDownsampleStrategy strategy) {
    if (frame.rows() == 0) return ArrayX3dR(0);
    ArrayX3dR full(frame.rows());
    const std::size_t n = impl::voxel_downsample_arrays(frame.data(), frame.rows(), 3, voxel_size, max_points_per_voxel,
                                                        min_pts_threshold, strategy, true, full.data());
    return shrink(full, n, 3);
}

ArrayXXdR voxel_downsample_xd(const ArrayXXdR& frame, double voxel_size, std::size_t max_points_per_voxel,
                              std::size_t min_pts_threshold, VoxelDownsampleStrategy strategy) {
    if (frame.rows() == 0) return ArrayXXdR(0, frame.cols());
    ArrayXXdR full(frame.rows(), frame.cols());
    const std::size_t n = impl::voxel_downsample_arrays(frame.data(), frame.rows(), frame.cols(), voxel_size, max_points_per_voxel,
                                                        min_pts_threshold, strategy, false, full.data());
    return shrink(full, n, frame.cols());
}

}  // namespace core

namespace algorithm {
namespace impl {

std::size_t voxel_downsample_with_normals_arrays(const double* points, std::size_t rows, std::size_t cols, const double* normals,
                                                 std::size_t normal_rows, std::size_t normal_cols, double voxel_size,
                                                 double* out_points, double* out_normals) {
    if (cols != 3 || normal_cols != 3) throw std::invalid_argument("voxel_downsample_with_normals expects Nx3 inputs");
    if (rows != normal_rows) throw std::invalid_argument("voxel_downsample_with_normals points/normals size mismatch");
    if (!(voxel_size > 0.0) || !std::isfinite(voxel_size))
        throw std::invalid_argument("voxel_downsample_with_normals voxel_size must be > 0");
    if (rows == 0) return 0;
    ouster_hip_voxel_desc d{};
    d.points = points, d.normals = normals, d.out = out_points, d.out_normals = out_normals;
    d.n = rows, d.out_capacity = rows, d.cols = 3;
    d.dtype = OUSTER_HIP_F64;
    d.voxel_size = voxel_size;
    d.max_points_per_voxel = 1, d.min_pts_threshold = 1;
    ouster_hip_ctx* ctx = hip::default_ctx();   // throws without a GPU
    uint64_t n_out = 0;
    const int rc = ouster_hip_voxel_downsample_host(ctx, &d, &n_out);
    if (rc != OUSTER_HIP_OK) throw_last(rc);
    return static_cast<std::size_t>(n_out);
}

}  // namespace impl

std::pair<core::ArrayX3dR, core::ArrayX3dR> voxel_downsample_with_normals(const core::ArrayX3dR& points,
                                                                          const core::ArrayX3dR& normals, double voxel_size) {
    core::ArrayX3dR full_p(points.rows()), full_n(points.rows());
    const std::size_t n = impl::voxel_downsample_with_normals_arrays(points.data(), points.rows(), 3, normals.data(), normals.rows(), 3,
                                                                     voxel_size, full_p.data(), full_n.data());
    std::pair<core::ArrayX3dR, core::ArrayX3dR> out{core::ArrayX3dR(n), core::ArrayX3dR(n)};
    std::memcpy(out.first.data(), full_p.data(), n * 24);
    std::memcpy(out.second.data(), full_n.data(), n * 24);
    return out;
}

}  // namespace algorithm
}  // namespace sdk
}  // namespace ouster
