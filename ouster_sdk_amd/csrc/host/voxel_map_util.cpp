// voxel_map_util.cpp -- the plain C++ half of the resident voxel map inside libouster_hip.so: what the constructor refuses, with
// the reference's messages, and HostVoxelMap, the restatement of core::VoxelHashMap3d on one core
// (ouster_core/src/voxel_hash_map.cpp:13-226): std::unordered_map plus creation-order vectors.  Built with -ffp-contract=off, an
// object of its own (Makefile): its rows are compared bit for bit with tests/voxel_map_model.py.
#include <cmath>
#include <cstring>

#include "../voxel_map_host.h"

namespace ouster_hip_dev {

const char* voxel_map_validate(const ouster_hip_voxel_map_desc* d) {
    if (d->max_points_per_voxel == 0) return "max_points_per_voxel must be greater than 0";
    if (!(d->voxel_size > 0.0) || !std::isfinite(d->voxel_size)) return "voxel_size must be greater than 0";
    if (!(d->max_distance > 0.0) || !std::isfinite(d->max_distance)) return "max_distance must be greater than 0";
    if (d->num_attributes != 0) return "num_attributes must be 0 for a fixed-size PointType";
    const double reach = std::ceil(d->max_distance * (1.0 / d->voxel_size));
    if (!(reach + 1.0 <= 2147483647.0)) return "voxel map: max_distance / voxel_size exceeds the int32 voxel grid";
    return nullptr;
}

VoxelMapParams voxel_map_params(const ouster_hip_voxel_map_desc* d) {
    VoxelMapParams p;
    p.voxel_size = d->voxel_size, p.max_distance = d->max_distance;
    p.max_points = d->max_points_per_voxel, p.min_pts = d->min_pts_threshold;
    p.resolution_sq = d->voxel_size * d->voxel_size / static_cast<double>(d->max_points_per_voxel);
    p.inv = 1.0 / d->voxel_size;
    p.max_voxel_dist = static_cast<int64_t>(std::ceil(d->max_distance * p.inv)) + 1;
    return p;
}

bool voxel_map_cell(const double* p, double inv, int32_t* cell) {
    for (int k = 0; k < 3; ++k) {
        const double f = std::floor(p[k] * inv);
        if (!(f >= -2147483648.0 && f <= 2147483647.0)) return false;
        cell[k] = static_cast<int32_t>(f);
    }
    return true;
}

bool voxel_map_far(const int32_t* cell, const int32_t* origin, int64_t max_voxel_dist) {
    // |d| < 2^32 per axis; an axis at 2^31 or more is far by itself (max_voxel_dist < 2^31), below that the sum stays under 2^64
    uint64_t sum = 0;
    for (int k = 0; k < 3; ++k) {
        const int64_t d = static_cast<int64_t>(cell[k]) - static_cast<int64_t>(origin[k]);
        const uint64_t a = static_cast<uint64_t>(d < 0 ? -d : d);
        if (a >= (1ull << 31)) return true;
        sum += a * a;
    }
    return sum >= static_cast<uint64_t>(max_voxel_dist) * static_cast<uint64_t>(max_voxel_dist);
}

namespace {
inline void load_row(const void* points, bool f32, uint64_t i, uint64_t stride, double* row) {
    if (f32) {
        const float* p = static_cast<const float*>(points) + i * stride;
        for (int c = 0; c < 3; ++c) row[c] = static_cast<double>(p[c]);
    } else {
        std::memcpy(row, static_cast<const double*>(points) + i * stride, 3 * sizeof(double));
    }
}
}  // namespace

bool HostVoxelMap::add_points(const void* points, bool f32, uint64_t n, uint64_t stride) {
    double row[3];
    Key key;
    for (uint64_t i = 0; i < n; ++i) {   // a refused call leaves the map unchanged: look at every row first
        load_row(points, f32, i, stride, row);
        if (!voxel_map_cell(row, p_.inv, key.v)) return false;
    }
    for (uint64_t i = 0; i < n; ++i) {
        load_row(points, f32, i, stride, row);
        voxel_map_cell(row, p_.inv, key.v);
        auto it = index_.find(key);
        if (it == index_.end()) {
            it = index_.emplace(key, buckets_.size()).first;
            cells_.insert(cells_.end(), key.v, key.v + 3);
            buckets_.emplace_back();
        }
        std::vector<double>& b = buckets_[it->second];
        const uint64_t held = b.size() / 3;
        if (held == p_.max_points) continue;
        bool close = false;
        for (uint64_t q = 0; q < held && !close; ++q) {
            const double dx = b[3 * q] - row[0], dy = b[3 * q + 1] - row[1], dz = b[3 * q + 2] - row[2];
            close = (dx * dx + dy * dy) + dz * dz < p_.resolution_sq;
        }
        if (close) continue;
        b.insert(b.end(), row, row + 3);
        ++n_points_;
    }
    return true;
}

uint64_t HostVoxelMap::count_far(const int32_t* origin) const {
    uint64_t rows = 0;
    for (size_t v = 0; v < buckets_.size(); ++v)
        if (voxel_map_far(&cells_[3 * v], origin, p_.max_voxel_dist)) rows += buckets_[v].size() / 3;
    return rows;
}

void HostVoxelMap::remove_far(const int32_t* origin, double* out) {
    size_t keep = 0;
    bool erased = false;
    for (size_t v = 0; v < buckets_.size(); ++v) {
        if (voxel_map_far(&cells_[3 * v], origin, p_.max_voxel_dist)) {
            const std::vector<double>& b = buckets_[v];
            if (out && !b.empty()) std::memcpy(out, b.data(), b.size() * sizeof(double)), out += b.size();
            n_points_ -= b.size() / 3;
            erased = true;
            continue;
        }
        if (keep != v) {
            std::memmove(&cells_[3 * keep], &cells_[3 * v], 3 * sizeof(int32_t));
            buckets_[keep] = std::move(buckets_[v]);
        }
        ++keep;
    }
    if (!erased) return;
    cells_.resize(3 * keep);
    buckets_.resize(keep);
    reindex();
}

void HostVoxelMap::reindex() {
    index_.clear();
    Key key;
    for (size_t v = 0; v < buckets_.size(); ++v) {
        std::memcpy(key.v, &cells_[3 * v], sizeof key.v);
        index_.emplace(key, v);
    }
}

void HostVoxelMap::pointcloud(double* out) const {
    for (const std::vector<double>& b : buckets_)
        if (!b.empty()) std::memcpy(out, b.data(), b.size() * sizeof(double)), out += b.size();
}

void HostVoxelMap::clear() {
    index_.clear();
    cells_.clear();
    buckets_.clear();
    n_points_ = 0;
}

void HostVoxelMap::reserve(uint64_t voxels) {
    cells_.reserve(3 * voxels);
    buckets_.reserve(voxels);
    index_.reserve(voxels);
}

void HostVoxelMap::closest(const double* query, double max_distance_sq, double* point, double* dist_sq) const {
    // voxel_hash_map.cpp:158-166
    static const int8_t SHIFTS[27][3] = {
        {0, 0, 0},   {1, 0, 0},   {-1, 0, 0},  {0, 1, 0},   {0, -1, 0},  {0, 0, 1},   {0, 0, -1},  {1, 1, 0},   {1, -1, 0},
        {-1, 1, 0},  {-1, -1, 0}, {1, 0, 1},   {1, 0, -1},  {-1, 0, 1},  {-1, 0, -1}, {0, 1, 1},   {0, 1, -1},  {0, -1, 1},
        {0, -1, -1}, {1, 1, 1},   {1, 1, -1},  {1, -1, 1},  {1, -1, -1}, {-1, 1, 1},  {-1, 1, -1}, {-1, -1, 1}, {-1, -1, -1}};
    point[0] = point[1] = point[2] = 0.0;
    double best = max_distance_sq;
    *dist_sq = best;
    int32_t voxel[3];
    if (!voxel_map_cell(query, p_.inv, voxel)) return;
    for (const auto& shift : SHIFTS) {
        Key key;
        bool inside = true;
        for (int d = 0; d < 3; ++d) {
            const int64_t c = static_cast<int64_t>(voxel[d]) + shift[d];
            inside = inside && c >= INT32_MIN && c <= INT32_MAX;
            key.v[d] = static_cast<int32_t>(c);
        }
        if (!inside) continue;
        double lb_sq = 0.0;
        for (int d = 0; d < 3; ++d) {
            const double lo = static_cast<double>(key.v[d]) * p_.voxel_size;
            const double hi = lo + p_.voxel_size;
            if (query[d] < lo) {
                const double delta = lo - query[d];
                lb_sq = lb_sq + delta * delta;
            } else if (query[d] > hi) {
                const double delta = query[d] - hi;
                lb_sq = lb_sq + delta * delta;
            }
        }
        if (lb_sq >= best) continue;
        const auto it = index_.find(key);
        if (it == index_.end()) continue;
        const std::vector<double>& b = buckets_[it->second];
        for (size_t q = 0; q + 2 < b.size(); q += 3) {
            const double dx = b[q] - query[0], dy = b[q + 1] - query[1], dz = b[q + 2] - query[2];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 < best) {
                best = d2;
                point[0] = b[q], point[1] = b[q + 1], point[2] = b[q + 2];
            }
        }
    }
    *dist_sq = best;
}

}  // namespace ouster_hip_dev
