// k_voxel_map.hip -- the resident voxel map (core::VoxelHashMap3d) on the GPU, held bit for bit to tests/voxel_map_model.py.  Built
// with -ffp-contract=off: every multiply, add and subtract below is one IEEE double operation in the model's order.  No
// floating-point atomic anywhere; a voxel's points are only ever written by the one thread that owns the voxel in that launch.
//
// add_points   the batch alone goes through k_voxel.hip's own steps (keys, then voxel_group_run: insert, first, scan, ids, stable
//              sort, segments): call-local voxels in first-seen order with contiguous, input-ordered segments.
//   k_vmap_find     one thread per call-local voxel probes the map's table: an id already in use, or "new".
//   (exclusive scan of the "new" flags: new voxels are numbered in first-seen order after the ids in use; the host reads the count
//   and grows the arrays before anything is published)
//   k_vmap_publish  writes cell and count 0 of the new ids and inserts them with atomicCAS on a free slot (the cells of a call are
//                   unique, so nothing is joined); a probe that wraps all the way round stores a status word.
//   k_vmap_admit    one thread per call-local voxel walks its segment in input order against the points the voxel holds, appends
//                   what first_n_point admits and stops at P.  A segment of thousands of candidates in one lane is bounded and
//                   correct; it is the known slow case (a cloud that falls into very few voxels), like the fold of k_voxel_reduce.
// removal      k_vmap_far (keep flags, exact integer distance), two scans, k_vmap_compact into the second set of arrays in the
//              old order (never in place), k_vmap_rebuild of the table from the surviving cells.
// queries      k_vmap_closest, one thread per query: voxel_hash_map.cpp:158-215 operation for operation.
//              k_vmap_cloud writes pointcloud() through a scan of the counts.
#include <hip/hip_runtime.h>

#include "k_voxel_map.h"
#include "voxel_dev.h"
#include "voxel_map_dev.h"

#if OUSTER_DEVICE_WIDE
#include <rocprim/device/device_scan.hpp>
#endif

namespace ouster_hip_dev {
namespace {

// takes a free slot for `id`; false: every slot is held
__device__ __forceinline__ bool vmap_insert(const VMapDev& m, const VoxelKey& k, uint32_t id) {
    uint32_t s = voxel_hash(k) & m.table_mask;
    for (uint32_t probe = 0; probe <= m.table_mask; ++probe) {
        if (atomicCAS(&m.table[s], VOXEL_EMPTY, (int32_t)id) == VOXEL_EMPTY) return true;
        s = (s + 1) & m.table_mask;
    }
    return false;
}

// the key of call-local voxel v (v < hdr->n_vox): that of the first row of its segment
__device__ __forceinline__ bool vmap_local_key(const VoxelArgs& a, uint32_t v, VoxelKey& k) {
    const uint32_t p = a.seg_begin[v];
    if (p >= a.n) return false;
    const uint32_t i = a.sidx[p];
    if (i >= a.n) return false;
    k = a.keys[i];
    return k.valid != 0;
}

__global__ void __launch_bounds__(VOXEL_WG) k_vmap_find(VoxelArgs a, VMapDev m, VMapAddArgs x) {
    const uint32_t v = blockIdx.x * VOXEL_WG + threadIdx.x;
    if (v >= a.n) return;
    uint32_t found = VOXEL_NO_ID, is_new = 0;
    VoxelKey k;
    if (a.hdr->status == 0 && v < a.hdr->n_vox && vmap_local_key(a, v, k)) {
        found = vmap_lookup(m, k);
        is_new = found == VOXEL_NO_ID;
    }
    x.found[v] = found;
    x.is_new[v] = is_new;
}

__global__ void k_vmap_add_header(VoxelArgs a, VMapAddArgs x) {
    x.hdr->n_new = x.new_pos[a.n - 1] + x.is_new[a.n - 1];
}

__global__ void __launch_bounds__(VOXEL_WG) k_vmap_publish(VoxelArgs a, VMapDev m, VMapAddArgs x) {
    const uint32_t v = blockIdx.x * VOXEL_WG + threadIdx.x;
    if (v >= a.n || v >= a.hdr->n_vox || !x.is_new[v]) return;
    VoxelKey k;
    const uint64_t id = (uint64_t)m.n_vox + x.new_pos[v];
    if (id >= m.cap || !vmap_local_key(a, v, k)) {   // the host made room for n_vox + n_new: reported, not written past
        x.hdr->status = VMAP_STATUS_TABLE;
        return;
    }
    k.valid = 1;
    m.s.cell[id] = k;
    m.s.count[id] = 0;
    x.found[v] = (uint32_t)id;
    if (!vmap_insert(m, k, (uint32_t)id)) x.hdr->status = VMAP_STATUS_TABLE;
}

template <class T>
__global__ void __launch_bounds__(VOXEL_WG) k_vmap_admit(VoxelArgs a, VMapDev m, VMapAddArgs x) {
    const uint32_t v = blockIdx.x * VOXEL_WG + threadIdx.x;
    if (v >= a.n || v >= a.hdr->n_vox) return;
    const uint32_t id = x.found[v];
    if (id >= m.cap) return;
    const uint32_t b = a.seg_begin[v], e = a.seg_end[v];
    if (b > e || e > a.n) return;
    double* held = m.s.pts + (uint64_t)id * m.P * 3;
    uint32_t c = m.s.count[id];
    const uint32_t before = c;
    for (uint32_t q = b; q < e && c < m.P; ++q) {
        const uint32_t i = a.sidx[q];
        if (i >= a.n) continue;
        const T* p = static_cast<const T*>(a.points) + (uint64_t)i * a.stride;
        const double px = (double)p[0], py = (double)p[1], pz = (double)p[2];
        bool close = false;
        for (uint32_t h = 0; h < c && !close; ++h) {
            const double dx = held[3 * h] - px, dy = held[3 * h + 1] - py, dz = held[3 * h + 2] - pz;
            close = (dx * dx + dy * dy) + dz * dz < m.resolution_sq;
        }
        if (close) continue;
        held[3 * c] = px, held[3 * c + 1] = py, held[3 * c + 2] = pz;
        ++c;
    }
    if (c != before) {
        m.s.count[id] = c;
        atomicAdd((unsigned long long*)&x.hdr->n_admitted, (unsigned long long)(c - before));
    }
}

__global__ void __launch_bounds__(VOXEL_WG) k_vmap_far(VMapDev m, VMapFarArgs f) {
    const uint32_t id = blockIdx.x * VOXEL_WG + threadIdx.x;
    if (id >= m.n_vox) return;
    const VoxelKey k = m.s.cell[id];
    const int32_t cell[3] = {k.x, k.y, k.z};
    // |d| < 2^32 per axis; an axis at 2^31 or more is far by itself (max_voxel_dist < 2^31), below that the sum stays under 2^64
    bool far = false;
    uint64_t sum = 0;
    for (int d = 0; d < 3; ++d) {
        const int64_t delta = (int64_t)cell[d] - (int64_t)f.origin[d];
        const uint64_t mag = (uint64_t)(delta < 0 ? -delta : delta);
        if (mag >= (1ull << 31)) far = true;
        else sum += mag * mag;
    }
    far = far || sum >= (uint64_t)f.max_voxel_dist * (uint64_t)f.max_voxel_dist;
    f.keep[id] = !far;
    f.gone[id] = far ? m.s.count[id] : 0u;
}

__global__ void k_vmap_far_header(VMapDev m, VMapFarArgs f) {
    f.hdr->n_keep = f.keep_pos[m.n_vox - 1] + f.keep[m.n_vox - 1];
    f.hdr->n_evicted = f.gone_pos[m.n_vox - 1] + f.gone[m.n_vox - 1];
}

// one thread per (voxel, slot): the survivors to `to` at their new ids, the evicted points to f.out
__global__ void __launch_bounds__(VOXEL_WG) k_vmap_compact(VMapDev m, VMapSet to, VMapFarArgs f) {
    const uint64_t t = (uint64_t)blockIdx.x * VOXEL_WG + threadIdx.x;
    const uint64_t id = t / m.P;
    const uint32_t s = (uint32_t)(t % m.P);
    if (id >= m.n_vox) return;
    const uint32_t cnt = m.s.count[id] <= m.P ? m.s.count[id] : m.P;
    const double* src = m.s.pts + t * 3;
    if (f.keep[id]) {
        const uint64_t nid = f.keep_pos[id];
        if (nid > id) return;   // a survivor only ever moves towards the front
        if (s == 0) to.cell[nid] = m.s.cell[id], to.count[nid] = cnt;
        if (s < cnt) {
            double* dst = to.pts + (nid * m.P + s) * 3;
            dst[0] = src[0], dst[1] = src[1], dst[2] = src[2];
        }
    } else if (f.out && s < cnt) {
        const uint64_t r = (uint64_t)f.gone_pos[id] + s;
        if (r >= f.hdr->n_evicted) return;
        double* dst = f.out + r * 3;
        dst[0] = src[0], dst[1] = src[1], dst[2] = src[2];
    }
}

__global__ void __launch_bounds__(VOXEL_WG) k_vmap_rebuild(VMapDev m, VMapHeader* hdr) {
    const uint32_t id = blockIdx.x * VOXEL_WG + threadIdx.x;
    if (id >= m.n_vox) return;
    if (!vmap_insert(m, m.s.cell[id], id)) hdr->status = VMAP_STATUS_TABLE;
}

__global__ void __launch_bounds__(VOXEL_WG) k_vmap_cloud(VMapDev m, const uint32_t* pos, double* out) {
    const uint64_t t = (uint64_t)blockIdx.x * VOXEL_WG + threadIdx.x;
    const uint64_t id = t / m.P;
    const uint32_t s = (uint32_t)(t % m.P);
    if (id >= m.n_vox) return;
    const uint32_t cnt = m.s.count[id] <= m.P ? m.s.count[id] : m.P;
    if (s >= cnt) return;
    const double* src = m.s.pts + t * 3;
    double* dst = out + ((uint64_t)pos[id] + s) * 3;
    dst[0] = src[0], dst[1] = src[1], dst[2] = src[2];
}

template <class T>
__global__ void __launch_bounds__(VOXEL_WG) k_vmap_closest(VMapDev m, VMapClosestArgs c) {
    const uint32_t i = blockIdx.x * VOXEL_WG + threadIdx.x;
    if (i >= c.q) return;
    const T* src = static_cast<const T*>(c.queries) + (uint64_t)i * c.stride;
    const double q[3] = {(double)src[0], (double)src[1], (double)src[2]};
    double bx, by, bz, best;
    vmap_closest_point(m, q, c.max_distance_sq, bx, by, bz, best);
    double* dst = c.out_points + 3 * (uint64_t)i;
    dst[0] = bx, dst[1] = by, dst[2] = bz;
    c.out_dist_sq[i] = best;
}

inline dim3 vmap_grid(uint64_t n) { return dim3((uint32_t)((n + VOXEL_WG - 1) / VOXEL_WG)); }

}  // namespace

#if OUSTER_DEVICE_WIDE
hipError_t vmap_temp_bytes(uint32_t n, size_t* bytes) {
    uint32_t* u = nullptr;
    *bytes = 0;
    return rocprim::exclusive_scan(nullptr, *bytes, u, u, 0u, (size_t)(n ? n : 1), rocprim::plus<uint32_t>());
}

hipError_t vmap_add_prepare(const VoxelArgs& a, const VMapDev& m, const VMapAddArgs& x, void* temp, size_t temp_bytes, hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    RUN_TRY(hipMemsetAsync(a.hdr, 0, sizeof(VoxelHeader), st));
    RUN_TRY(hipMemsetAsync(x.hdr, 0, sizeof(VMapHeader), st));
    RUN_TRY(launch_voxel_keys(a, st));
    RUN_TRY(voxel_group_run(a, temp, temp_bytes, st));
    hipLaunchKernelGGL(k_vmap_find, vmap_grid(a.n), dim3(VOXEL_WG), 0, st, a, m, x);
    RUN_TRY(hipGetLastError());
    size_t bytes = temp_bytes;
    RUN_TRY(rocprim::exclusive_scan(temp, bytes, x.is_new, x.new_pos, 0u, (size_t)a.n, rocprim::plus<uint32_t>(), st));
    hipLaunchKernelGGL(k_vmap_add_header, dim3(1), dim3(1), 0, st, a, x);
    return hipGetLastError();
}

hipError_t vmap_add_commit(const VoxelArgs& a, const VMapDev& m, const VMapAddArgs& x, hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_vmap_publish, vmap_grid(a.n), dim3(VOXEL_WG), 0, st, a, m, x);
    RUN_TRY(hipGetLastError());
    if (a.f32) hipLaunchKernelGGL(k_vmap_admit<float>, vmap_grid(a.n), dim3(VOXEL_WG), 0, st, a, m, x);
    else hipLaunchKernelGGL(k_vmap_admit<double>, vmap_grid(a.n), dim3(VOXEL_WG), 0, st, a, m, x);
    return hipGetLastError();
}

hipError_t vmap_far_prepare(const VMapDev& m, const VMapFarArgs& f, void* temp, size_t temp_bytes, hipStream_t st) {
    if (m.n_vox == 0) return hipSuccess;
    RUN_TRY(hipMemsetAsync(f.hdr, 0, sizeof(VMapHeader), st));
    hipLaunchKernelGGL(k_vmap_far, vmap_grid(m.n_vox), dim3(VOXEL_WG), 0, st, m, f);
    RUN_TRY(hipGetLastError());
    size_t bytes = temp_bytes;
    RUN_TRY(rocprim::exclusive_scan(temp, bytes, f.keep, f.keep_pos, 0u, (size_t)m.n_vox, rocprim::plus<uint32_t>(), st));
    bytes = temp_bytes;
    RUN_TRY(rocprim::exclusive_scan(temp, bytes, f.gone, f.gone_pos, 0u, (size_t)m.n_vox, rocprim::plus<uint32_t>(), st));
    hipLaunchKernelGGL(k_vmap_far_header, dim3(1), dim3(1), 0, st, m, f);
    return hipGetLastError();
}

hipError_t vmap_far_commit(const VMapDev& m, const VMapSet& to, const VMapFarArgs& f, hipStream_t st) {
    if (m.n_vox == 0) return hipSuccess;
    hipLaunchKernelGGL(k_vmap_compact, vmap_grid((uint64_t)m.n_vox * m.P), dim3(VOXEL_WG), 0, st, m, to, f);
    return hipGetLastError();
}

hipError_t vmap_rebuild(const VMapDev& m, VMapHeader* hdr, hipStream_t st) {
    if (!m.table) return hipSuccess;
    RUN_TRY(hipMemsetAsync(m.table, 0xff, ((size_t)m.table_mask + 1) * sizeof(int32_t), st));
    if (m.n_vox == 0) return hipSuccess;
    hipLaunchKernelGGL(k_vmap_rebuild, vmap_grid(m.n_vox), dim3(VOXEL_WG), 0, st, m, hdr);
    return hipGetLastError();
}

hipError_t vmap_cloud(const VMapDev& m, uint32_t* pos, double* out, void* temp, size_t temp_bytes, hipStream_t st) {
    if (m.n_vox == 0) return hipSuccess;
    size_t bytes = temp_bytes;
    RUN_TRY(rocprim::exclusive_scan(temp, bytes, m.s.count, pos, 0u, (size_t)m.n_vox, rocprim::plus<uint32_t>(), st));
    hipLaunchKernelGGL(k_vmap_cloud, vmap_grid((uint64_t)m.n_vox * m.P), dim3(VOXEL_WG), 0, st, m, pos, out);
    return hipGetLastError();
}

hipError_t vmap_closest(const VMapDev& m, const VMapClosestArgs& c, hipStream_t st) {
    if (c.q == 0) return hipSuccess;
    if (c.f32) hipLaunchKernelGGL(k_vmap_closest<float>, vmap_grid(c.q), dim3(VOXEL_WG), 0, st, m, c);
    else hipLaunchKernelGGL(k_vmap_closest<double>, vmap_grid(c.q), dim3(VOXEL_WG), 0, st, m, c);
    return hipGetLastError();
}
#endif

}  // namespace ouster_hip_dev
