// pose_util.h -- dense dewarp: apply each column's pose to the points of that column.
// Same signatures as ouster_core/include/ouster/core/pose_util.h:38-103 (dewarp<T>(points,
// poses)) and pose_util.h:456-493 + impl/dewarp_impl.h:23-115 (range-gated, compacting
// dewarp(LidarFrame | FrameSet, XYZLut, min_range, max_range) with optional provenance); the
// per-point work runs on the GPU (ouster_hip_dewarp / ouster_hip_dewarp_frames).
// transform (pose_util.h:118-173), dewarp(points, Vector16d) (:97-103) and interp_pose (:194-434; src/transform_vector.cpp:40-60,
// 96-104, src/transform_homogeneous.cpp:31-62, impl/transform_typedefs.h:16-17) keep the reference's signatures as well: what
// interp_pose computes once per pair of known poses is done on the host, the per-x and per-point work on the GPU
// (ouster_hip_interp_pose_host / ouster_hip_transform_host), and without a GPU they throw std::runtime_error like the rest.
// Every validation error comes first, as std::invalid_argument with the reference's message.
#pragma once

#include <array>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <type_traits>
#include <vector>

#include "ouster/core/lidar_frame.h"
#include "ouster/core/typedefs.h"
#include "ouster/core/xyzlut.h"

namespace ouster {
namespace sdk {
namespace core {

/** W x 16: one flattened row-major 4x4 pose per column (MatrixX16dR in the reference). */
using Poses = ArrayXXR<double>;

/** Stand-in for Eigen::Vector3<T> (three contiguous T, like the reference's element type). */
template <typename T>
using Vector3 = std::array<T, 3>;

/** The part of FrameSet the dewarp needs: frames by index, null = invalid index
 *  (FrameSet::valid_indices, frame_set.h). */
using FrameSet = std::vector<std::shared_ptr<LidarFrame>>;

/** Stand-in for Eigen's 1 x 16 row vector: one flattened row-major 4x4 pose (Vector16<T> in the reference). */
template <typename T>
using Vector16 = std::array<T, 16>;
using Vector16d = Vector16<double>;

namespace impl {
/** x_interp [n], x_known [k], poses_known [k][16] f64 -> out [n][16] of double or float.  Validates (sizes are the caller's),
 *  then the per-x work on the GPU. */
void interp_pose_device(const double* x_interp, size_t n, const double* x_known, const double* poses_known, size_t k, bool f64,
                        void* out);
void interp_pose_pair_device(const double* x_interp, size_t n, double t0, const double* x0, double t1, const double* x1,
                             double* out);
void transform_device(const void* points, const double* pose16, void* out, bool f64, size_t n);

void dewarp_device(const void* points, const double* poses, void* out, bool f64, size_t h, size_t w);

/** Batched GPU implementation behind the frame dewarps: frames[i] uses luts[i]; results are
 *  appended to the output vectors (pointers may be null).  Returns the points, x/y/z of T. */
void dewarp_frames_device(const std::vector<const LidarFrame*>& frames,
                          const std::vector<const DeviceLut*>& luts,
                          const std::vector<uint32_t>& frame_index, double min_range,
                          double max_range, bool f64, std::vector<unsigned char>& points,
                          std::vector<uint32_t>* frame_idxs, std::vector<uint32_t>* col_idxs,
                          std::vector<uint64_t>* timestamps_ns);

/** impl/dewarp_impl.h:23-81 */
template <typename T>
std::vector<Vector3<T>> dewarp_impl(const LidarFrame& lidar_frame, const XYZLutT<T>& xyzlut,
                                    double min_range, double max_range,
                                    std::vector<uint32_t>* col_idxs,
                                    std::vector<uint64_t>* timestamps_ns) {
    std::vector<unsigned char> raw;
    dewarp_frames_device({&lidar_frame}, {&xyzlut.device()}, {0}, min_range, max_range,
                         sizeof(T) == 8, raw, nullptr, col_idxs, timestamps_ns);
    std::vector<Vector3<T>> out(raw.size() / sizeof(Vector3<T>));
    if (!raw.empty()) std::memcpy(out.data(), raw.data(), raw.size());
    return out;
}

/** impl/dewarp_impl.h:86-115 */
template <typename T>
std::vector<Vector3<T>> dewarp_impl(const FrameSet& frame_set, const std::vector<XYZLutT<T>>& xyzluts,
                                    double min_range, double max_range,
                                    std::vector<uint32_t>* frame_idxs,
                                    std::vector<uint32_t>* col_idxs,
                                    std::vector<uint64_t>* timestamps_ns) {
    if (frame_set.size() != xyzluts.size())
        throw std::invalid_argument("Number of frames and number of XYZLuts must be the same");
    std::vector<const LidarFrame*> frames;
    std::vector<const DeviceLut*> luts;
    std::vector<uint32_t> index;
    for (size_t i = 0; i < frame_set.size(); ++i) {
        if (!frame_set[i]) continue;
        frames.push_back(frame_set[i].get());
        luts.push_back(&xyzluts[i].device());
        index.push_back(static_cast<uint32_t>(i));
    }
    std::vector<unsigned char> raw;
    dewarp_frames_device(frames, luts, index, min_range, max_range, sizeof(T) == 8, raw, frame_idxs,
                         col_idxs, timestamps_ns);
    std::vector<Vector3<T>> out(raw.size() / sizeof(Vector3<T>));
    if (!raw.empty()) std::memcpy(out.data(), raw.data(), raw.size());
    return out;
}
}  // namespace impl

/** @throw std::invalid_argument on shape mismatches. */
template <typename T>
void dewarp(ImgRef<T> dewarped, const ImgRef<const T>& points, const Poses& poses) {
    const size_t W = poses.rows();
    if (poses.cols() != 16 || W == 0 || points.cols() != 3 || dewarped.cols() != 3 ||
        points.rows() != dewarped.rows() || points.rows() % W != 0)
        throw std::invalid_argument("dewarp: unexpected dimensions");
    impl::dewarp_device(points.data(), poses.data(), dewarped.data(), sizeof(T) == 8,
                        points.rows() / W, W);
}

template <typename T>
PointCloudXYZ<T> dewarp(const PointCloudXYZ<T>& points, const Poses& poses) {
    PointCloudXYZ<T> out(points.rows());
    dewarp<T>(ImgRef<T>(out), ImgRef<const T>(points), poses);
    return out;
}

/** One pose for every point (pose_util.h:97-103). */
inline PointCloudXYZd dewarp(const PointCloudXYZd& points, const Vector16d& pose) {
    PointCloudXYZd out(points.rows());
    impl::dewarp_device(points.data(), pose.data(), out.data(), true, points.rows(), 1);
    return out;
}

/** R p + t for every point, in T; the pose is a flattened row-major 4x4 of T (pose_util.h:118-131).
 *  @throw std::invalid_argument on shape mismatches. */
template <typename T>
void transform(ImgRef<T> transformed, const ImgRef<const T>& points, const Vector16<T>& pose) {
    if (points.cols() != 3 || transformed.cols() != 3 || points.rows() != transformed.rows())
        throw std::invalid_argument("transform: unexpected dimensions");
    double p[16];
    for (int i = 0; i < 16; ++i) p[i] = static_cast<double>(pose[i]);
    impl::transform_device(points.data(), p, transformed.data(), sizeof(T) == 8, points.rows());
}

template <typename T>
PointCloudXYZ<T> transform(const PointCloudXYZ<T>& points, const Vector16<T>& pose) {
    PointCloudXYZ<T> out(points.rows());
    transform<T>(ImgRef<T>(out.data(), out.rows(), 3), ImgRef<const T>(points.data(), points.rows(), 3), pose);
    return out;
}

inline PointCloudXYZd transform(const PointCloudXYZd& points, const Vector16d& pose) {
    return transform<double>(points, pose);
}

/** Interpolation between two known poses (pose_util.h:316-326); x_interp outside [t0, t1] extrapolates.
 *  @throw std::invalid_argument for |t1 - t0| < epsilon or x_interp that decreases anywhere. */
template <typename T>
std::vector<mat4d> interp_pose(const std::vector<T>& x_interp, T t0, const mat4d& x0, T t1, const mat4d& x1) {
    static_assert(std::is_same<T, double>::value, "interp_pose: the time type is double");
    std::vector<mat4d> out(x_interp.size());
    impl::interp_pose_pair_device(x_interp.data(), x_interp.size(), t0, x0.data(), t1, x1.data(),
                                  out.empty() ? nullptr : out[0].m);
    return out;
}

/** Piecewise interpolation over k >= 2 known poses at strictly increasing x_known (pose_util.h:360-377): x in
 *  [x_known[j], x_known[j + 1]) uses that pair, x outside the known range the first / last pair.
 *  @throw std::invalid_argument with the reference's messages; also for x_interp that decreases anywhere, which is a superset
 *  of where the reference throws. */
template <typename T>
std::vector<mat4d> interp_pose(const std::vector<T>& x_interp, const std::vector<T>& x_known,
                               const std::vector<mat4d>& poses_known) {
    static_assert(std::is_same<T, double>::value, "interp_pose: the time type is double");
    static_assert(sizeof(mat4d) == 16 * sizeof(double), "mat4d is 16 packed doubles");
    if (x_known.size() != poses_known.size()) throw std::invalid_argument("x_known and poses_known sizes are not matching");
    std::vector<mat4d> out(x_interp.size());
    impl::interp_pose_device(x_interp.data(), x_interp.size(), x_known.data(), poses_known.empty() ? nullptr : poses_known[0].m,
                             x_known.size(), true, out.empty() ? nullptr : out[0].m);
    return out;
}

/** The same on flattened poses, k x 16 of Scalar in and N x 16 of Scalar out (pose_util.h:408-434): computed in double, the
 *  result cast to Scalar. */
template <typename T, typename Scalar>
ArrayXXR<Scalar> interp_pose(const std::vector<T>& x_interp, const std::vector<T>& x_known, const ArrayXXR<Scalar>& poses_known) {
    static_assert(std::is_same<T, double>::value, "interp_pose: the time type is double");
    static_assert(std::is_same<Scalar, double>::value || std::is_same<Scalar, float>::value, "interp_pose: poses are float or double");
    if (x_known.size() != poses_known.rows()) throw std::invalid_argument("x_known and poses_known sizes are not matching");
    if (poses_known.rows() && poses_known.cols() != 16) throw std::invalid_argument("interp_pose: poses_known must be k x 16");
    std::vector<double> known(poses_known.size());
    for (size_t i = 0; i < known.size(); ++i) known[i] = static_cast<double>(poses_known.data()[i]);
    ArrayXXR<Scalar> out(x_interp.size(), 16);
    impl::interp_pose_device(x_interp.data(), x_interp.size(), x_known.data(), known.data(), x_known.size(), sizeof(Scalar) == 8,
                             out.data());
    return out;
}

/** Range-gated dewarp of one frame with its per-column body_to_world poses
 *  (pose_util.h:456-485): points of valid columns with min_range <= r <= max_range [m]. */
template <typename T>
std::vector<Vector3<T>> dewarp(const LidarFrame& lidar_frame, const XYZLutT<T>& xyzlut,
                               double min_range, double max_range) {
    return impl::dewarp_impl<T>(lidar_frame, xyzlut, min_range, max_range, nullptr, nullptr);
}

/** FrameSet form (pose_util.h:475-493): frames concatenated in index order. */
template <typename T>
std::vector<Vector3<T>> dewarp(const FrameSet& frame_set, const std::vector<XYZLutT<T>>& xyzluts,
                               double min_range, double max_range) {
    return impl::dewarp_impl<T>(frame_set, xyzluts, min_range, max_range, nullptr, nullptr, nullptr);
}

}  // namespace core
}  // namespace sdk
}  // namespace ouster
