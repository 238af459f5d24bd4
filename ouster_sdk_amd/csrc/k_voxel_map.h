// k_voxel_map.h -- launch interface of the resident voxel map's kernels (k_voxel_map.hip): the map's arrays, the per-call
// workspace, and the steps of add_points, removal, pointcloud and the nearest-neighbour query.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "k_voxel.h"

namespace ouster_hip_dev {

constexpr uint32_t VMAP_STATUS_TABLE = 4;   // a probe went all the way round the map's table: cannot happen with 2 slots per voxel

// one set of the map's arrays, indexed by voxel id (the creation order)
struct VMapSet {
    VoxelKey* cell = nullptr;    // [cap]
    uint32_t* count = nullptr;   // [cap] points held
    double* pts = nullptr;       // [cap][P][3]
};

struct VMapDev {
    VMapSet s;
    int32_t* table = nullptr;    // [table_mask + 1] voxel ids, VOXEL_EMPTY where free
    uint32_t table_mask = 0;
    uint32_t n_vox = 0;          // ids in use
    uint32_t cap = 0;            // voxels the arrays hold
    uint32_t P = 0;              // max_points_per_voxel
    double voxel_size = 0.0, inv = 0.0, resolution_sq = 0.0;
};

// what the steps leave for the host, in the workspace
struct VMapHeader {
    uint32_t status;        // VMAP_STATUS_TABLE, or 0
    uint32_t n_new;         // add: call-local voxels the map does not hold yet
    uint32_t n_keep;        // removal: voxels that stay
    uint32_t n_evicted;     // removal: points of the voxels that go
    uint64_t n_admitted;    // add: points admitted
    uint64_t n_cloud;       // pointcloud: rows
};
static_assert(sizeof(VMapHeader) == 32, "one read-back");

// add_points: on top of the call-local grid of k_voxel.hip (VoxelArgs: keys, sidx, seg_begin, seg_end, hdr->n_vox)
struct VMapAddArgs {
    VMapHeader* hdr;
    uint32_t* found;     // [n] per call-local voxel: its id in the map, VOXEL_NO_ID if new; after publish: its id
    uint32_t* is_new;    // [n] 1 / 0
    uint32_t* new_pos;   // [n] exclusive scan of is_new
};

// removal
struct VMapFarArgs {
    VMapHeader* hdr;
    int32_t origin[3];
    int64_t max_voxel_dist;
    uint32_t* keep;      // [n_vox] 1: the voxel stays
    uint32_t* keep_pos;  // [n_vox] exclusive scan: its new id
    uint32_t* gone;      // [n_vox] points of a voxel that goes, else 0
    uint32_t* gone_pos;  // [n_vox] exclusive scan: its first row in `out`
    double* out;         // nullptr, or room for hdr->n_evicted rows
};

struct VMapClosestArgs {
    const void* queries;    // [q][stride] of f32 / f64
    uint64_t stride;
    uint32_t q;
    int32_t f32;
    double max_distance_sq;
    double* out_points;     // [q][3]
    double* out_dist_sq;    // [q]
};

#if OUSTER_DEVICE_WIDE
// bytes of rocPRIM temporary storage for scans of n elements (the call-local grid's own needs are voxel_temp_bytes)
hipError_t vmap_temp_bytes(uint32_t n, size_t* bytes);
// the header resets, the call-local grid (k_voxel.hip's keys and voxel_group_run), k_vmap_find, the scan of the new flags, hdr->n_new.  Publishes nothing.
hipError_t vmap_add_prepare(const VoxelArgs& a, const VMapDev& m, const VMapAddArgs& x, void* temp, size_t temp_bytes, hipStream_t st);
// k_vmap_publish, k_vmap_admit: m has room for n_vox + n_new voxels
hipError_t vmap_add_commit(const VoxelArgs& a, const VMapDev& m, const VMapAddArgs& x, hipStream_t st);
// k_vmap_far, both scans, hdr->n_keep / n_evicted
hipError_t vmap_far_prepare(const VMapDev& m, const VMapFarArgs& f, void* temp, size_t temp_bytes, hipStream_t st);
// the survivors to `to` at their new ids, the evicted points to f.out
hipError_t vmap_far_commit(const VMapDev& m, const VMapSet& to, const VMapFarArgs& f, hipStream_t st);
// the table from the cells of ids 0 .. m.n_vox - 1 (reset first)
hipError_t vmap_rebuild(const VMapDev& m, VMapHeader* hdr, hipStream_t st);
// pos: [n_vox] scratch; out: room for every point held
hipError_t vmap_cloud(const VMapDev& m, uint32_t* pos, double* out, void* temp, size_t temp_bytes, hipStream_t st);
hipError_t vmap_closest(const VMapDev& m, const VMapClosestArgs& c, hipStream_t st);
#endif

}  // namespace ouster_hip_dev
