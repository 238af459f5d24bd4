// voxel_map_dev.h -- what a query of the resident voxel map is made of, for every kernel that asks one: the probe of the map's table
// and the nearest-neighbour search of voxel_hash_map.cpp:158-215 (k_vmap_closest of k_voxel_map.hip, k_reg_pass of
// k_registration.hip).  One body, so that both give the same bits: tests/voxel_map_model.py, get_closest_neighbor.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_voxel_map.h"
#include "voxel_dev.h"

namespace ouster_hip_dev {
namespace {

// the id of `k` in the map's table, VOXEL_NO_ID if it is not there
__device__ __forceinline__ uint32_t vmap_lookup(const VMapDev& m, const VoxelKey& k) {
    if (m.n_vox == 0) return VOXEL_NO_ID;
    uint32_t s = voxel_hash(k) & m.table_mask;
    for (uint32_t probe = 0; probe <= m.table_mask; ++probe) {
        const int32_t id = m.table[s];
        if (id == VOXEL_EMPTY) return VOXEL_NO_ID;
        if ((uint32_t)id < m.n_vox) {
            const VoxelKey o = m.s.cell[id];
            if (o.x == k.x && o.y == k.y && o.z == k.z) return (uint32_t)id;
        }
        s = (s + 1) & m.table_mask;
    }
    return VOXEL_NO_ID;
}

// voxel_hash_map.cpp:158-166
__constant__ int8_t VMAP_SHIFTS[27][3] = {
    {0, 0, 0},   {1, 0, 0},   {-1, 0, 0},  {0, 1, 0},   {0, -1, 0},  {0, 0, 1},   {0, 0, -1},  {1, 1, 0},   {1, -1, 0},
    {-1, 1, 0},  {-1, -1, 0}, {1, 0, 1},   {1, 0, -1},  {-1, 0, 1},  {-1, 0, -1}, {0, 1, 1},   {0, 1, -1},  {0, -1, 1},
    {0, -1, -1}, {1, 1, 1},   {1, 1, -1},  {1, -1, 1},  {1, -1, -1}, {-1, 1, 1},  {-1, 1, -1}, {-1, -1, 1}, {-1, -1, -1}};

// the point of the map nearest to q and its squared distance, among those strictly nearer than max_distance_sq; none: (0, 0, 0) and
// max_distance_sq
__device__ __forceinline__ void vmap_closest_point(const VMapDev& m, const double (&q)[3], double max_distance_sq, double& bx, double& by,
                                                   double& bz, double& best) {
    bx = 0.0, by = 0.0, bz = 0.0, best = max_distance_sq;
    int32_t voxel[3];
    const bool inside = axis_to_voxel(q[0], m.inv, voxel[0]) & axis_to_voxel(q[1], m.inv, voxel[1]) & axis_to_voxel(q[2], m.inv, voxel[2]);
    if (inside && m.n_vox != 0) {
        for (int sft = 0; sft < 27; ++sft) {
            int64_t cell[3];
            bool ok = true;
            for (int d = 0; d < 3; ++d) {
                cell[d] = (int64_t)voxel[d] + VMAP_SHIFTS[sft][d];
                ok = ok && cell[d] >= -2147483648ll && cell[d] <= 2147483647ll;
            }
            if (!ok) continue;
            double lb_sq = 0.0;
            for (int d = 0; d < 3; ++d) {
                const double lo = (double)cell[d] * m.voxel_size;
                const double hi = lo + m.voxel_size;
                if (q[d] < lo) {
                    const double delta = lo - q[d];
                    lb_sq = lb_sq + delta * delta;
                } else if (q[d] > hi) {
                    const double delta = q[d] - hi;
                    lb_sq = lb_sq + delta * delta;
                }
            }
            if (lb_sq >= best) continue;
            const VoxelKey k{(int32_t)cell[0], (int32_t)cell[1], (int32_t)cell[2], 1};
            const uint32_t id = vmap_lookup(m, k);
            if (id == VOXEL_NO_ID) continue;
            const uint32_t cnt = m.s.count[id] <= m.P ? m.s.count[id] : m.P;
            const double* held = m.s.pts + (uint64_t)id * m.P * 3;
            for (uint32_t h = 0; h < cnt; ++h) {
                const double x = held[3 * h], y = held[3 * h + 1], z = held[3 * h + 2];
                const double dx = x - q[0], dy = y - q[1], dz = z - q[2];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 < best) best = d2, bx = x, by = y, bz = z;
            }
        }
    }
}

}  // namespace
}  // namespace ouster_hip_dev
