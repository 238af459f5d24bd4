/**
 * @file
 * @brief Voxel-grid down-sampling of a point cloud and the resident voxel map, on the GPU.
 *
 * Of the reference's ouster/core/voxel_hash_map.h this header carries VoxelDownsampleStrategy, voxel_downsample_3d,
 * voxel_downsample_xd and VoxelHashMap3d (below), with its signatures, defaults and messages.  The work runs on the GPU (csrc/k_voxel.hip) through
 * ouster_hip_voxel_downsample_host; FIRST_N_POINT and RANDOM with max_points_per_voxel > 1 are sequential by nature and run the
 * host restatement (ouster_hip_voxel_downsample_ref).  Results equal tests/voxel_model.py bit for bit.
 *
 * Deviations from the reference: rows come in first-seen order (voxels by the input index of their first contributing point),
 * where the reference emits its hash map's iteration order; a non-finite voxel_size, a non-finite coordinate among the first three
 * columns and one whose voxel index no int32 holds are refused with std::invalid_argument (undefined behaviour there).
 *
 * VoxelHashMap3d is the Vector3i / Vector3d / DefaultVoxelBucket / first_n_point specialisation of the reference's VoxelHashMap: a
 * persistent, updatable map that lives in device memory (csrc/k_voxel_map.hip through ouster_hip_voxel_map_*, ouster_hip.h).
 * Results equal tests/voxel_map_model.py bit for bit.  Its deviations from the reference:
 *  - pointcloud() and extract_voxels_far_from_location() emit voxels in creation order (earlier calls first, first-seen input order
 *    within a call), a voxel's points in admission order, survivors of a removal in their old order; the reference emits its hash
 *    map's iteration order.  Two maps fed the same calls return the same bytes;
 *  - a squared distance is ((dx dx + dy dy) + dz dz), each operation rounded on its own: the project's fixed rounding order.  Eigen's
 *    squaredNorm leaves the order open, so the reference's own result may differ in the last bit between builds;
 *  - refused with std::invalid_argument where the reference is undefined: a non-finite voxel_size or max_distance, ceil(max_distance
 *    / voxel_size) + 1 above 2^31 - 1, a point or location with a non-finite coordinate or a cell no int32 holds (the whole call, with
 *    the map unchanged).  A neighbour cell no int32 holds is skipped; a query outside the grid has no neighbour.  The cell distance
 *    of a removal is exact, equal to the reference wherever its 32-bit arithmetic does not overflow;
 *  - update() checks its position before it adds anything.
 * Not carried: the Xd, Average, PointNormal, Indexed, reservoir and random specialisations, get_voxel_bucket, pointcloud_vector, the
 * legacy core::voxel_downsample(std::vector<Vector3d>, ...).  get_closest_neighbors (many queries per call) is a project extension.
 *
 * Clouds already in device memory go through the C ABI, ouster_hip_voxel_downsample (ouster_hip.h); a resident batch has
 * hip::DeviceFrameBatch::voxel_downsample over its dewarped cloud (hip/device_batch.h).
 */
#pragma once

#include <array>
#include <cfloat>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <tuple>
#include <vector>

#include "ouster/core/typedefs.h"
#include "ouster/core/visibility.h"

namespace ouster {
namespace sdk {
namespace hip {
class Context;
}
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

/**
 * core::VoxelHashMap3d on the GPU: the reference's member names and defaults; rows are ArrayX3dR, a single point is three doubles.
 * Move-only.  The map shares ownership of the hip::Context it was made on (the calling thread's current one) and every call runs
 * on that context.  Errors throw std::invalid_argument (arguments, with the reference's messages and those of ouster_hip.h) or
 * std::runtime_error.  Calls on one map are not thread-safe.
 */
class OUSTER_API_CLASS VoxelHashMap3d {
   public:
    using point_type = std::array<double, 3>;
    using voxel_type = std::array<int32_t, 3>;

    /** @throws std::invalid_argument "max_points_per_voxel must be greater than 0", "voxel_size must be greater than 0",
     *  "max_distance must be greater than 0", "num_attributes must be 0 for a fixed-size PointType" (in this order), "voxel map:
     *  max_distance / voxel_size exceeds the int32 voxel grid"; std::runtime_error without a GPU */
    OUSTER_API_FUNCTION
    explicit VoxelHashMap3d(double voxel_size, double max_distance = 100.0, std::size_t max_points_per_voxel = 20,
                            std::size_t min_pts_threshold = 1, std::size_t num_attributes = 0);
    /** A project extension: the same map in host memory on one core (csrc/host/voxel_map_util.cpp); needs no GPU. */
    OUSTER_API_FUNCTION
    static VoxelHashMap3d on_host(double voxel_size, double max_distance = 100.0, std::size_t max_points_per_voxel = 20,
                                  std::size_t min_pts_threshold = 1, std::size_t num_attributes = 0);
    OUSTER_API_FUNCTION ~VoxelHashMap3d();
    OUSTER_API_FUNCTION VoxelHashMap3d(VoxelHashMap3d&& other) noexcept;
    OUSTER_API_FUNCTION VoxelHashMap3d& operator=(VoxelHashMap3d&& other) noexcept;
    VoxelHashMap3d(const VoxelHashMap3d&) = delete;
    VoxelHashMap3d& operator=(const VoxelHashMap3d&) = delete;

    OUSTER_API_FUNCTION bool empty() const;
    OUSTER_API_FUNCTION void clear();
    /** Rows in input order.  @throws std::invalid_argument "voxel map: point outside the int32 voxel grid" (the map is unchanged) */
    OUSTER_API_FUNCTION void add_points(const ArrayX3dR& points);
    OUSTER_API_FUNCTION void add_points(const std::vector<point_type>& points);
    /** add_points, then remove_voxels_far_from_location(position) */
    OUSTER_API_FUNCTION void update(const ArrayX3dR& points, const point_type& position);
    OUSTER_API_FUNCTION void remove_voxels_far_from_location(const point_type& origin);
    OUSTER_API_FUNCTION ArrayX3dR extract_voxels_far_from_location(const point_type& origin);
    OUSTER_API_FUNCTION ArrayX3dR pointcloud() const;
    /** The closest held point and its squared distance; none below max_distance_sq: (0, 0, 0) and max_distance_sq */
    OUSTER_API_FUNCTION
    std::tuple<point_type, double> get_closest_neighbor(const point_type& query, double max_distance_sq = DBL_MAX) const;
    /** A project extension, the hot path: one neighbour per row of `queries`, each pair bit-identical to the single call.
     *  dist_sq is resized to queries.rows(). */
    OUSTER_API_FUNCTION
    ArrayX3dR get_closest_neighbors(const ArrayX3dR& queries, std::vector<double>& dist_sq, double max_distance_sq = DBL_MAX) const;

    OUSTER_API_FUNCTION
    static voxel_type point_to_voxel(const point_type& point, double inv_voxel_size);
    std::size_t max_points_per_voxel() const { return max_points_per_voxel_; }
    std::size_t min_pts_threshold() const { return min_pts_threshold_; }

    /** Project extensions: room for `voxels` voxels (a later call within it allocates nothing); what the map holds */
    OUSTER_API_FUNCTION void reserve(std::size_t voxels);
    OUSTER_API_FUNCTION std::size_t num_voxels() const;
    OUSTER_API_FUNCTION std::size_t num_points() const;
    OUSTER_API_FUNCTION std::size_t device_bytes() const;
    /** The GPU the map lives on; -1 for a host map */
    OUSTER_API_FUNCTION int device() const;
    /** The C ABI handle (ouster_hip_voxel_map*), for batch code */
    void* handle() const { return handle_; }

    /** On plain row-major arrays (what the Python binding calls) */
    OUSTER_API_FUNCTION void add_points_array(const double* points, std::size_t rows);
    OUSTER_API_FUNCTION void closest_array(const double* queries, std::size_t rows, double max_distance_sq, double* points, double* dist_sq) const;

   private:
    VoxelHashMap3d() = default;
    void* handle_ = nullptr;               // ouster_hip_voxel_map
    std::shared_ptr<hip::Context> ctx_;    // the context it was made on, kept alive with it (empty: a host map)
    std::size_t max_points_per_voxel_ = 0, min_pts_threshold_ = 0;
};

}  // namespace core
}  // namespace sdk
}  // namespace ouster
