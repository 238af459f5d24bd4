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
#include <memory>
#include <vector>

#include "ouster/core/typedefs.h"
#include "ouster/core/visibility.h"
#include "ouster/hip/context.h"

namespace ouster {
namespace sdk {

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

/**
 * A target cloud kept on the GPU, and many sources aligned against it per call.
 *
 * A project extension: the reference has no such class.  Scan-to-map and frame-to-keyframe align many sources (every frame of a
 * batch, every sensor of a rig) against one target that does not change; the two functions above rebuild the target's search
 * grid on every call and handle one source.  An IcpTarget builds the grid once and keeps it in device memory; align_many() runs
 * all its sources in lock step, one launch sequence and one read-back per pass whatever their number.  For each source the result
 * equals, bit for bit, that of point_to_point_align / point_to_plane_align on that source alone.
 *
 * The method is fixed by the constructor: a target with normals serves point to plane only, one without serves point to point
 * only.  Move-only.  The target shares ownership of the hip::Context it was made on (the calling thread's current one: the
 * batch's own inside DeviceFrameBatch::make_icp_target) and every alignment runs on that context, so a target outlives the batch or
 * the thread that made it.  Errors throw std::invalid_argument (arguments, with the messages of the functions above and of
 * include/ouster_hip.h) or std::runtime_error.
 */
class OUSTER_API_CLASS IcpTarget {
   public:
    /** Point to point.  @throws std::invalid_argument "max_corr_dist must be finite and greater than zero", a target point outside
     *  the int32 cell grid */
    OUSTER_API_FUNCTION
    explicit IcpTarget(const core::ArrayX3dR& points, double max_corr_dist = 0.25);
    /** Point to plane.  @throws also "target_points and target_normals must have the same number of rows" */
    OUSTER_API_FUNCTION
    IcpTarget(const core::ArrayX3dR& points, const core::ArrayX3dR& normals, double max_corr_dist = 0.25);
    OUSTER_API_FUNCTION
    ~IcpTarget();
    OUSTER_API_FUNCTION
    IcpTarget(IcpTarget&& other) noexcept;
    OUSTER_API_FUNCTION
    IcpTarget& operator=(IcpTarget&& other) noexcept;
    IcpTarget(const IcpTarget&) = delete;
    IcpTarget& operator=(const IcpTarget&) = delete;

    /** For batch code: rows already in device memory ((n, 3) doubles, dense; normals nullptr for point to point), on the default
     *  context's device. */
    OUSTER_API_FUNCTION
    static IcpTarget from_device(const double* points, const double* normals, std::size_t rows, double max_corr_dist = 0.25);
    /** The same from host arrays (what the Python binding calls); normals nullptr for point to point. */
    OUSTER_API_FUNCTION
    static IcpTarget from_arrays(const double* points, std::size_t rows, const double* normals, std::size_t normal_rows,
                                 double max_corr_dist = 0.25);

    /** Point to point, one source. */
    OUSTER_API_FUNCTION
    core::Matrix4dR align(const core::ArrayX3dR& source, const core::Matrix4dR& initial_guess = core::Matrix4dR::Identity()) const;
    /** Point to plane, one source. */
    OUSTER_API_FUNCTION
    core::Matrix4dR align(const core::ArrayX3dR& source, const core::ArrayX3dR& source_normals,
                          const core::Matrix4dR& initial_guess = core::Matrix4dR::Identity(), double max_normal_angle_deg = 20.0) const;
    /** Point to point, many sources in one call.  guesses: one per source, or empty for identities.  stats: nullptr, or what each
     *  source's loop reported. */
    OUSTER_API_FUNCTION
    std::vector<core::Matrix4dR> align_many(const std::vector<core::ArrayX3dR>& sources, const std::vector<core::Matrix4dR>& guesses = {},
                                            std::vector<impl::AlignStats>* stats = nullptr) const;
    /** Point to plane, many sources in one call. */
    OUSTER_API_FUNCTION
    std::vector<core::Matrix4dR> align_many(const std::vector<core::ArrayX3dR>& sources, const std::vector<core::ArrayX3dR>& normals,
                                            const std::vector<core::Matrix4dR>& guesses = {}, double max_normal_angle_deg = 20.0,
                                            std::vector<impl::AlignStats>* stats = nullptr) const;
    /** The same on plain row-major host arrays (what the Python binding calls): points[k] is (rows[k], 3); normals nullptr, or
     *  normals[k] of normal_rows[k] rows; guesses16 nullptr or 16 doubles per source; poses16: 16 doubles per source. */
    OUSTER_API_FUNCTION
    void align_arrays(const double* const* points, const std::size_t* rows, const double* const* normals, const std::size_t* normal_rows,
                      std::size_t n_sources, const double* guesses16, double max_normal_angle_deg, double* poses16,
                      impl::AlignStats* stats) const;
    /** For batch code: one source of rows in device memory ((rows, 3) doubles, dense). */
    OUSTER_API_FUNCTION
    impl::AlignStats align_device(const double* points, const double* normals, std::size_t rows, const double* initial_guess16,
                                  double max_normal_angle_deg, double* pose16) const;

    OUSTER_API_FUNCTION std::size_t size() const;            ///< rows given
    OUSTER_API_FUNCTION bool has_normals() const;
    OUSTER_API_FUNCTION std::size_t device_bytes() const;    ///< device memory held
    OUSTER_API_FUNCTION double max_corr_dist() const;
    /** The GPU the target lives on; -1 for a target of fewer than 20 rows, which lives on none. */
    OUSTER_API_FUNCTION int device() const;

   private:
    IcpTarget() = default;
    void* handle_ = nullptr;               // ouster_hip_icp_target
    std::shared_ptr<hip::Context> ctx_;    // the context it was made on, kept alive with it (empty: fewer than 20 rows, no GPU asked for)
};

}  // namespace algorithm
}  // namespace sdk
}  // namespace ouster
