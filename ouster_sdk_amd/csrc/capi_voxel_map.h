// capi_voxel_map.h -- the handle behind ouster_hip_voxel_map, for the translation units of the C ABI that read a map:
// capi_voxel_map.hip (which owns it) and capi_registration.hip (which queries it).  Internal to libouster_hip.so.
#pragma once
#include "capi_internal.h"
#include "k_voxel_map.h"
#include "voxel_map_host.h"

struct ouster_hip_voxel_map {
    using VMapSet = ouster_hip_dev::VMapSet;
    ouster_hip_ctx* ctx = nullptr;
    ouster_hip_dev::VoxelMapParams p;
    ouster_hip_dev::HostVoxelMap* host = nullptr;   // OUSTER_HIP_VOXEL_MAP_HOST: everything below stays empty
    VMapSet set[2];                 // the arrays in use and the set a removal compacts into
    int cur = 0;
    int32_t* table = nullptr;
    uint32_t table_mask = 0;
    uint64_t cap = 0;               // voxels each set holds
    uint32_t n_vox = 0;
    uint64_t n_pts = 0;
    size_t bytes = 0;
};

namespace ouster_hip_dev {

// the map as a kernel reads it
inline VMapDev dev_of(const ouster_hip_voxel_map* m) {
    VMapDev d;
    d.s = m->set[m->cur];
    d.table = m->table, d.table_mask = m->table_mask;
    d.n_vox = m->n_vox, d.cap = (uint32_t)m->cap, d.P = (uint32_t)m->p.max_points;
    d.voxel_size = m->p.voxel_size, d.inv = m->p.inv, d.resolution_sq = m->p.resolution_sq;
    return d;
}

}  // namespace ouster_hip_dev
