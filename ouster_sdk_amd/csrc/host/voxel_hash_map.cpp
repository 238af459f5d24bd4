// voxel_hash_map.cpp -- core::VoxelHashMap3d (include/ouster/core/voxel_hash_map.h) over the C ABI: ouster_hip_voxel_map_* behind
// a move-only handle.  The C ABI refuses what it refuses, in its order and with its messages, before a GPU is asked for.
#include "ouster/core/voxel_hash_map.h"

#include <cmath>
#include <stdexcept>
#include <string>

#include "host_internal.h"

namespace ouster {
namespace sdk {
namespace core {
namespace {

[[noreturn]] void raise(int rc) {
    if (rc == OUSTER_HIP_ERR_INVALID_ARGUMENT) throw std::invalid_argument(ouster_hip_last_error());
    throw std::runtime_error(ouster_hip_last_error());
}
void check(int rc) {
    if (rc != OUSTER_HIP_OK) raise(rc);
}

ouster_hip_voxel_map* handle_of(void* h) {
    if (!h) throw std::runtime_error("VoxelHashMap3d: moved from");
    return static_cast<ouster_hip_voxel_map*>(h);
}

ouster_hip_voxel_map_info info_of(void* h) {
    ouster_hip_voxel_map_info i{};
    check(ouster_hip_voxel_map_info_read(handle_of(h), &i));
    return i;
}

const double kNone[3] = {0, 0, 0};   // an empty array still needs somewhere to point; it is never read

// first without a context: every refusal comes before a GPU is asked for; only "ctx is NULL" asks for the thread's current context
void* create(ouster_hip_voxel_map_desc d, bool host, std::shared_ptr<hip::Context>& ctx) {
    d.flags = host ? OUSTER_HIP_VOXEL_MAP_HOST : 0u;
    ouster_hip_voxel_map* h = nullptr;
    int rc = ouster_hip_voxel_map_create(nullptr, &d, &h);
    if (rc == OUSTER_HIP_ERR_INVALID_ARGUMENT && std::string(ouster_hip_last_error()) == "ctx is NULL") {
        hip::default_ctx();   // throws without a GPU
        ctx = hip::Context::current();
        rc = ouster_hip_voxel_map_create(ctx->handle(), &d, &h);
    }
    check(rc);
    return h;
}

ouster_hip_voxel_map_desc desc_of(double voxel_size, double max_distance, std::size_t max_points, std::size_t min_pts, std::size_t attributes) {
    ouster_hip_voxel_map_desc d{};
    d.voxel_size = voxel_size, d.max_distance = max_distance;
    d.max_points_per_voxel = max_points, d.min_pts_threshold = min_pts, d.num_attributes = attributes;
    return d;
}

}  // namespace

VoxelHashMap3d::VoxelHashMap3d(double voxel_size, double max_distance, std::size_t max_points_per_voxel, std::size_t min_pts_threshold,
                               std::size_t num_attributes)
    : max_points_per_voxel_(max_points_per_voxel), min_pts_threshold_(min_pts_threshold) {
    handle_ = create(desc_of(voxel_size, max_distance, max_points_per_voxel, min_pts_threshold, num_attributes), false, ctx_);
}

VoxelHashMap3d VoxelHashMap3d::on_host(double voxel_size, double max_distance, std::size_t max_points_per_voxel,
                                       std::size_t min_pts_threshold, std::size_t num_attributes) {
    VoxelHashMap3d m;
    m.max_points_per_voxel_ = max_points_per_voxel, m.min_pts_threshold_ = min_pts_threshold;
    m.handle_ = create(desc_of(voxel_size, max_distance, max_points_per_voxel, min_pts_threshold, num_attributes), true, m.ctx_);
    return m;
}

VoxelHashMap3d::~VoxelHashMap3d() { ouster_hip_voxel_map_destroy(static_cast<ouster_hip_voxel_map*>(handle_)); }

VoxelHashMap3d::VoxelHashMap3d(VoxelHashMap3d&& o) noexcept
    : handle_(o.handle_), ctx_(std::move(o.ctx_)), max_points_per_voxel_(o.max_points_per_voxel_), min_pts_threshold_(o.min_pts_threshold_) {
    o.handle_ = nullptr;
}

VoxelHashMap3d& VoxelHashMap3d::operator=(VoxelHashMap3d&& o) noexcept {
    if (this != &o) {
        ouster_hip_voxel_map_destroy(static_cast<ouster_hip_voxel_map*>(handle_));
        handle_ = o.handle_, ctx_ = std::move(o.ctx_);
        max_points_per_voxel_ = o.max_points_per_voxel_, min_pts_threshold_ = o.min_pts_threshold_;
        o.handle_ = nullptr;
    }
    return *this;
}

bool VoxelHashMap3d::empty() const { return info_of(handle_).voxels == 0; }
void VoxelHashMap3d::clear() { check(ouster_hip_voxel_map_clear(handle_of(handle_))); }
void VoxelHashMap3d::reserve(std::size_t voxels) { check(ouster_hip_voxel_map_reserve(handle_of(handle_), voxels)); }
std::size_t VoxelHashMap3d::num_voxels() const { return info_of(handle_).voxels; }
std::size_t VoxelHashMap3d::num_points() const { return info_of(handle_).points; }
std::size_t VoxelHashMap3d::device_bytes() const { return info_of(handle_).device_bytes; }
int VoxelHashMap3d::device() const { return ctx_ ? ctx_->device() : -1; }

void VoxelHashMap3d::add_points_array(const double* points, std::size_t rows) {
    check(ouster_hip_voxel_map_add_points_host(handle_of(handle_), rows ? points : kNone, OUSTER_HIP_F64, rows, 3));
}

void VoxelHashMap3d::add_points(const ArrayX3dR& points) { add_points_array(points.data(), points.rows()); }

void VoxelHashMap3d::add_points(const std::vector<point_type>& points) {
    add_points_array(points.empty() ? kNone : points.front().data(), points.size());
}

void VoxelHashMap3d::update(const ArrayX3dR& points, const point_type& position) {
    check(ouster_hip_voxel_map_update_host(handle_of(handle_), points.rows() ? points.data() : kNone, OUSTER_HIP_F64, points.rows(), 3,
                                           position.data()));
}

void VoxelHashMap3d::remove_voxels_far_from_location(const point_type& origin) {
    check(ouster_hip_voxel_map_remove_far(handle_of(handle_), origin.data()));
}

ArrayX3dR VoxelHashMap3d::extract_voxels_far_from_location(const point_type& origin) {
    // no more rows than the map holds can come back
    ArrayX3dR all(num_points());
    uint64_t n = 0;
    check(ouster_hip_voxel_map_extract_far_host(handle_of(handle_), origin.data(), all.data(), all.rows(), &n));
    ArrayX3dR out(static_cast<std::size_t>(n));
    for (std::size_t i = 0; i < 3 * static_cast<std::size_t>(n); ++i) out.data()[i] = all.data()[i];
    return out;
}

ArrayX3dR VoxelHashMap3d::pointcloud() const {
    ArrayX3dR out(num_points());
    uint64_t n = 0;
    check(ouster_hip_voxel_map_pointcloud_host(handle_of(handle_), out.data(), out.rows(), &n));
    return out;
}

void VoxelHashMap3d::closest_array(const double* queries, std::size_t rows, double max_distance_sq, double* points, double* dist_sq) const {
    check(ouster_hip_voxel_map_closest_host(handle_of(handle_), rows ? queries : kNone, OUSTER_HIP_F64, rows, 3, max_distance_sq, points, dist_sq));
}

std::tuple<VoxelHashMap3d::point_type, double> VoxelHashMap3d::get_closest_neighbor(const point_type& query, double max_distance_sq) const {
    point_type p{};
    double d = max_distance_sq;
    closest_array(query.data(), 1, max_distance_sq, p.data(), &d);
    return std::make_tuple(p, d);
}

ArrayX3dR VoxelHashMap3d::get_closest_neighbors(const ArrayX3dR& queries, std::vector<double>& dist_sq, double max_distance_sq) const {
    ArrayX3dR out(queries.rows());
    dist_sq.assign(queries.rows(), max_distance_sq);
    double none = 0.0;
    closest_array(queries.data(), queries.rows(), max_distance_sq, queries.rows() ? out.data() : &none, queries.rows() ? dist_sq.data() : &none);
    return out;
}

VoxelHashMap3d::voxel_type VoxelHashMap3d::point_to_voxel(const point_type& point, double inv_voxel_size) {
    voxel_type v{};
    for (int k = 0; k < 3; ++k) {
        const double f = std::floor(point[k] * inv_voxel_size);
        if (!(f >= -2147483648.0 && f <= 2147483647.0)) throw std::invalid_argument("voxel map: point outside the int32 voxel grid");
        v[k] = static_cast<int32_t>(f);
    }
    return v;
}

}  // namespace core
}  // namespace sdk
}  // namespace ouster
