// voxel_map_host.h -- the host half of the resident voxel map (csrc/host/voxel_map_util.cpp): validation with the reference's
// messages, the derived values, and HostVoxelMap, the plain C++ restatement of core::VoxelHashMap3d behind a handle made with
// OUSTER_HIP_VOXEL_MAP_HOST.  Plain C++, no HIP: the C ABI (capi_voxel_map.hip) calls it before anything touches the GPU, and
// tests/cpp builds it alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <unordered_map>
#include <vector>

#include "../../include/ouster_hip.h"

namespace ouster_hip_dev {

constexpr const char* VOXEL_MAP_MSG_GRID = "voxel map: point outside the int32 voxel grid";
constexpr const char* VOXEL_MAP_MSG_CAPACITY = "voxel map: out_capacity is too small";
constexpr uint64_t VOXEL_MAP_MAX_ROWS = 1ull << 30;

// what the constructor derives (voxel_hash_map.cpp:39-40, :115)
struct VoxelMapParams {
    double voxel_size = 0.0, max_distance = 0.0;
    double inv = 0.0;              // 1.0 / voxel_size
    double resolution_sq = 0.0;    // voxel_size * voxel_size / max_points_per_voxel
    uint64_t max_points = 0, min_pts = 0;
    int64_t max_voxel_dist = 0;    // int(ceil(max_distance * inv)) + 1, at most 2^31 - 1
};

// nullptr, or the message the constructor refuses with, in the reference's order; then the two of this project
const char* voxel_map_validate(const ouster_hip_voxel_map_desc* d);
VoxelMapParams voxel_map_params(const ouster_hip_voxel_map_desc* d);
// VoxelHashMap::point_to_voxel; false where no int32 holds a cell (NaN and the infinities included)
bool voxel_map_cell(const double* p, double inv, int32_t* cell);
// a cell at squared distance >= max_voxel_dist^2 of the origin's; exact for any pair of int32 cells
bool voxel_map_far(const int32_t* cell, const int32_t* origin, int64_t max_voxel_dist);

class HostVoxelMap {
public:
    explicit HostVoxelMap(const VoxelMapParams& p) : p_(p) {}
    // false: a row outside the grid, nothing changed
    bool add_points(const void* points, bool f32, uint64_t n, uint64_t stride);
    // the points of the voxels that are far, in order; the voxels stay
    uint64_t count_far(const int32_t* origin) const;
    // erases them; out: nullptr, or room for count_far() rows
    void remove_far(const int32_t* origin, double* out);
    void pointcloud(double* out) const;
    void closest(const double* query, double max_distance_sq, double* point, double* dist_sq) const;
    void clear();
    void reserve(uint64_t voxels);
    uint64_t voxels() const { return cells_.size() / 3; }
    uint64_t points() const { return n_points_; }
    uint64_t capacity() const { return cells_.capacity() / 3; }
    const VoxelMapParams& params() const { return p_; }

private:
    struct Key {
        int32_t v[3];
        bool operator==(const Key& o) const { return v[0] == o.v[0] && v[1] == o.v[1] && v[2] == o.v[2]; }
    };
    struct KeyHash {
        size_t operator()(const Key& k) const {
            return ((size_t)(uint32_t)k.v[0] * 73856093u) ^ ((size_t)(uint32_t)k.v[1] * 19349669u) ^ ((size_t)(uint32_t)k.v[2] * 83492791u);
        }
    };
    void reindex();
    VoxelMapParams p_;
    std::unordered_map<Key, uint64_t, KeyHash> index_;   // cell -> voxel id
    std::vector<int32_t> cells_;                          // [voxels][3], creation order
    std::vector<std::vector<double>> buckets_;            // per voxel: its points, 3 doubles each, in admission order
    uint64_t n_points_ = 0;
};

// the C ABI's error channel (ouster_hip_capi.hip): stores the thread's message, returns `code`
int fail_msg(int code, const char* msg);

}  // namespace ouster_hip_dev
