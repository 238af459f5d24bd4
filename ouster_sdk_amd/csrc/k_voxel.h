// k_voxel.h -- launch interface of the voxel down-sampling kernels (k_voxel.hip): keys, hash insert, voxel ids in first-seen
// order, the inverted index (segments of a stable sort by voxel id), the reduction per voxel and the compacting write.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/ouster_hip.h"
#include "voxel_host.h"

namespace ouster_hip_dev {

constexpr int32_t VOXEL_EMPTY = -1;            // a free slot of the hash table (the table is memset to 0xff on every call)
constexpr uint32_t VOXEL_NO_ID = 0xffffffffu;  // "no voxel": never a sort key (skipped rows get id n, which sorts last)
constexpr uint32_t VOXEL_STATUS_GRID = 1;      // a row outside the int32 voxel grid (or non-finite)
constexpr uint32_t VOXEL_STATUS_TABLE = 2;     // the probe loop ran through the whole table: cannot happen with capacity > n

struct alignas(16) VoxelKey {
    int32_t x, y, z;
    int32_t valid;   // 0: the row takes no part (skipped by the with-normals rules, or refused)
};

// what a call reads back
struct VoxelHeader {
    uint32_t status;   // 0, or one VOXEL_STATUS_* value (the last store wins): no output row is written
    uint32_t n_vox;    // voxels with at least one valid row
    uint64_t n_out;    // rows the result has (written only if status == 0 and n_out <= out_capacity)
};
static_assert(sizeof(VoxelHeader) == 16, "one 16-byte read-back");

struct VoxelArgs {
    const void* points;       // [n][stride] of f32 / f64
    const double* normals;    // VOXEL_FORM_NORMALS: [n][3]
    uint64_t stride;          // elements per input row
    uint32_t n, cols;
    int32_t f32;              // points are float (widened on load)
    int32_t form;             // VoxelForm
    double inv;               // 1.0 / voxel_size
    uint64_t min_pts;
    // the context's workspace; [n] unless noted
    VoxelHeader* hdr;
    VoxelKey* keys;
    int32_t* table;           // [table_mask + 1] point indices, VOXEL_EMPTY where free
    uint32_t table_mask;
    uint32_t* slot;           // the table slot of a valid row's voxel
    uint32_t* first;          // 1: the row has the smallest index of its voxel
    uint32_t* first_id;       // exclusive scan of `first`: the id of the voxel a first row opens
    uint32_t *vid, *idx;      // sort input: voxel id per row (n for a row that takes no part), row index
    uint32_t *svid, *sidx;    // sort output: rows grouped by voxel, input order within a voxel
    uint32_t *seg_begin, *seg_end;   // [n_vox] the voxel's range in svid / sidx
    double* rows;             // AVERAGE, NORMALS: [n][cols or 6] the input rows in sorted order, f64; a voxel's result replaces the
                              //   first row of its segment
    uint32_t *keep, *pos;     // AVERAGE, NORMALS: 1 where voxel v is emitted, and the exclusive scan: its output row
    double* out;              // [out_capacity][cols]
    double* out_normals;      // NORMALS: [out_capacity][3]
    uint64_t out_capacity;
};

constexpr uint32_t VOXEL_WG = 256;

hipError_t launch_voxel_keys(const VoxelArgs& a, hipStream_t st);      // keys, status
hipError_t launch_voxel_insert(const VoxelArgs& a, hipStream_t st);    // table, slot
hipError_t launch_voxel_first(const VoxelArgs& a, hipStream_t st);     // first
hipError_t launch_voxel_ids(const VoxelArgs& a, hipStream_t st);       // vid, idx, hdr->n_vox (after the scan first -> first_id)
hipError_t launch_voxel_segments(const VoxelArgs& a, hipStream_t st);  // seg_begin, seg_end (after the sort)
hipError_t launch_voxel_gather(const VoxelArgs& a, hipStream_t st);    // rows (AVERAGE, NORMALS)
hipError_t launch_voxel_reduce(const VoxelArgs& a, hipStream_t st);    // rows, keep (AVERAGE, NORMALS)
hipError_t launch_voxel_write(const VoxelArgs& a, hipStream_t st);     // out, out_normals, hdr->n_out (after the scan keep -> pos)

// bits of the sort key: ids 0 .. n
inline uint32_t voxel_sort_bits(uint32_t n) {
    uint32_t bits = 1;
    while (bits < 32 && (n >> bits) != 0) ++bits;
    return bits;
}

// The run functions of k_voxel.hip, k_icp.hip's grid and k_voxel_map.hip call rocPRIM's scan and radix sort: they are compiled by
// hipcc, and by the host-lanes build of tests/cpp, whose hip/hip_runtime.h announces itself and stands in for those two calls.
#if defined(__HIPCC__) || defined(OUSTER_HOST_LANES)
#define OUSTER_DEVICE_WIDE 1
#else
#define OUSTER_DEVICE_WIDE 0
#endif

// every step of a run function: the first error ends the run
#define RUN_TRY(expr)                      \
    do {                                   \
        const hipError_t e_ = (expr);      \
        if (e_ != hipSuccess) return e_;   \
    } while (0)

#if OUSTER_DEVICE_WIDE
// the bytes of temporary storage the scan and the sort of a grouping of n rows need
hipError_t voxel_temp_bytes(uint32_t n, size_t* bytes);
// Groups the rows by voxel, on the stream and without a synchronisation: table reset, insert, first, exclusive scan of the first
// flags, ids, stable radix sort of the row indices over voxel_sort_bits(n) bits, segments.  a.keys are written already (and
// a.hdr reset) by what runs before on the stream; fills slot .. seg_end and a.hdr->n_vox.  The one place this sequence is written:
// the row order of every result of voxel_run, icp_grid_run and vmap_add_prepare depends on it.
// temp: at least voxel_temp_bytes(n), 256-byte aligned.  ev: nullptr, or 5 events, recorded after the table reset (which so stays in
// the caller's phase of resets and keys, as include/ouster_hip.h names it), after the insert, after the ids, after the sort and
// after the segments.
hipError_t voxel_group_run(const VoxelArgs& a, void* temp, size_t temp_bytes, hipStream_t st, hipEvent_t* ev = nullptr);
// The whole down-sampling: header reset, keys, the grouping, then gather + reduce + scan (AVERAGE, NORMALS) and the write.
// ev: nullptr, or OUSTER_HIP_VOXEL_PHASES + 1 events: ev[0] is recorded before the first step and ev[k + 1] after phase k (reset +
// keys, insert, first + scan + ids, sort, segments, gather + reduce + scan, write).
hipError_t voxel_run(const VoxelArgs& a, void* temp, size_t temp_bytes, hipStream_t st, hipEvent_t* ev = nullptr);
#endif

}  // namespace ouster_hip_dev
