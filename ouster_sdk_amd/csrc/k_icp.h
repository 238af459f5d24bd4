// k_icp.h -- launch interface of the ICP kernels (k_icp.hip): the target grid (keys, then the cell table, ids, stable sort and
// segments of k_voxel.hip, then the slots and the gathered rows), the correspondences of a pass, the median of their residuals and
// the sums behind the solve.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/ouster_hip.h"
#include "icp_host.h"
#include "k_voxel.h"

namespace ouster_hip_dev {

constexpr uint32_t ICP_WG = 256;
constexpr uint32_t ICP_ROWS_PER_THREAD = 4;
constexpr uint32_t ICP_CHUNK = ICP_WG * ICP_ROWS_PER_THREAD;   // ouster_hip_icp_chunk_rows(): rows one workgroup of the sum kernels owns
constexpr uint64_t ICP_NO_KEY = ~0ull;                          // the sort key of a row without a correspondence: after every |r|
constexpr uint32_t ICP_STATUS_GRID = 1;                         // a participating target row outside the int32 cell grid

// a slot of the cell table as the queries read it: the cell and where its rows start in the gathered order; begin < 0: free
struct alignas(16) IcpSlot {
    int32_t x, y, z;
    int32_t begin;
};

// what a pass reads back (after the VoxelHeader of the grid)
struct IcpHeader {
    uint32_t status;   // 0 or ICP_STATUS_GRID
    uint32_t count;    // correspondences of the pass
    double median, huber_delta;
    double centroid_x[3], centroid_q[3];
    double sums[OUSTER_HIP_ICP_SUMS];
};
struct IcpReadback {
    VoxelHeader grid;   // status: the table ran full (cannot happen); n_vox: cells
    IcpHeader pass;
};

struct IcpArgs {
    const void *src, *tgt, *src_n, *tgt_n;   // [n][stride] of f32 / f64
    uint64_t src_stride, tgt_stride, src_n_stride, tgt_n_stride;
    uint32_t n_src, n_tgt;
    int32_t f32, plane;
    double inv;            // 1.0 / max_corr_dist
    double max_d2;         // max_corr_dist * max_corr_dist
    double max_corr_dist;
    double cos_gate;
    double pose[16];       // of the pass
    IcpReadback* rb;
    // target side, [n_tgt] unless noted: what the k_voxel.hip launchers fill (VoxelArgs), then
    VoxelKey* keys;
    int32_t* table;
    uint32_t table_mask;
    uint32_t *first_id, *svid, *sidx, *seg_begin, *seg_end;
    IcpSlot* slots;        // [table_mask + 1]
    uint32_t* slot_end;    // [table_mask + 1]
    double* rows;          // [n_tgt][3 or 6] the participating target points (and unit normals) in cell order
    // source side, [n_src]
    int32_t* nn;
    double* r;
    uint64_t *key, *key_sorted;
    uint32_t* flag;
    double* xq;            // [n_src][6]: x, then q (point) or the unit target normal (plane)
    double* partials;      // [chunks][OUSTER_HIP_ICP_SUMS]
};

inline uint32_t icp_chunks(uint32_t n_src) { return (n_src + ICP_CHUNK - 1) / ICP_CHUNK; }

// What a query of the grid reads and writes, whoever owns the grid: the call's workspace (IcpArgs) or a resident target
// (ouster_hip_icp_target).  The per-row outputs are indexed by the row's place in the (concatenated) outputs.
struct IcpQuery {
    int32_t plane;
    uint32_t table_mask, n_tgt;
    double inv, max_d2, cos_gate;
    const IcpSlot* slots;
    const uint32_t *slot_end, *sidx;
    const double* rows;
    int32_t* nn;
    double* r;
    uint64_t* key;
    uint32_t* flag;
    double* xq;
};

// ---- many sources against one resident target (ouster_hip_icp_target_align / _step) ----
static_assert(ICP_CHUNK == ICP_CHUNK_ROWS, "the chunk table of icp_host.h cuts the sources into the sum kernels' runs");

// a row of the source table: written by the host, sent again (poses and flags) once per pass
struct IcpSource {
    const void *src, *src_n;   // [n][stride] of f32 / f64
    uint64_t src_stride, src_n_stride;
    uint32_t n;                // rows
    uint32_t first;            // its first row in the concatenated per-row outputs
    uint32_t first_chunk, chunks;
    int32_t active, reserved;  // 0: every kernel skips the source and leaves its header alone
    double pose[16];           // of the pass
};

struct IcpManyArgs {
    IcpQuery q;                // the target, the constants, the concatenated per-row outputs [n_rows]
    const IcpSource* sources;  // [n_sources]
    const IcpChunk* chunks;    // [n_chunks]
    const uint32_t *seg_begin, *seg_end;   // [n_sources] a source's rows in the outputs; empty (end == begin) while inactive
    IcpHeader* hdr;            // [n_sources] what a pass reads back
    uint32_t* counts;          // [n_sources] the segmented sum of the flags
    uint64_t* key_sorted;      // [n_rows]
    double* partials;          // [n_chunks][OUSTER_HIP_ICP_SUMS]
    uint32_t n_sources, n_chunks, n_rows;
    int32_t f32;               // of the sources
    double max_corr_dist;
};

hipError_t launch_icp_keys(const IcpArgs& a, hipStream_t st);         // keys, pass.status
hipError_t launch_icp_slots(const IcpArgs& a, hipStream_t st);        // slots, slot_end (after the segments)
hipError_t launch_icp_gather(const IcpArgs& a, hipStream_t st);       // rows
hipError_t launch_icp_correspond(const IcpArgs& a, hipStream_t st);   // nn, r, key, flag, xq
hipError_t launch_icp_rows_used(const IcpArgs& a, hipStream_t st);    // pass.count: the rows that take part (after the grid)
hipError_t launch_icp_correspond_many(const IcpManyArgs& m, hipStream_t st);   // the same of every active source, a workgroup per chunk

// The device-wide pieces: the bytes of temporary storage a call needs, the grid once per call and one pass, both on the stream
// without a synchronisation.  `va` carries the target-side arrays for voxel_group_run of k_voxel.h (n = n_tgt); the grid needs
// voxel_temp_bytes(n_tgt) of temp and is compiled wherever the grouping is, the rest by hipcc only.
// ev: nullptr, or events recorded after the grid (1) / after correspond, median and sums (3).
#if OUSTER_DEVICE_WIDE
hipError_t icp_grid_run(const IcpArgs& a, const VoxelArgs& va, void* temp, size_t temp_bytes, hipStream_t st);
#endif
#ifdef __HIPCC__
hipError_t icp_temp_bytes(uint32_t n_src, uint32_t n_tgt, size_t* bytes);
hipError_t icp_pass_run(const IcpArgs& a, void* temp, size_t temp_bytes, hipStream_t st, hipEvent_t* ev = nullptr);
// The many-source pass: correspond, a segmented sum of the flags and a segmented radix sort of the keys over the sources' rows,
// the medians, the sum kernels and a fold per source; the active sources' headers are complete when the stream gets there.
hipError_t icp_many_temp_bytes(uint32_t n_rows, uint32_t n_sources, size_t* bytes);
hipError_t icp_many_pass_run(const IcpManyArgs& m, void* temp, size_t temp_bytes, hipStream_t st);
#endif

}  // namespace ouster_hip_dev
