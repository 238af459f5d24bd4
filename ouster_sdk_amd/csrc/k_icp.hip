// k_icp.hip -- point_to_point_align / point_to_plane_align (ouster_algorithm/src/align_clouds.cpp:1590-1874) on the GPU, held to
// tests/icp_model.py.  Built with -ffp-contract=off: every multiply, add, divide and sqrt below is one IEEE double operation in the
// model's order.  No floating-point atomic anywhere.
//
// The target grid, once per call (cell = max_corr_dist):
// k_icp_keys        one thread per target row: does it take part (finite point; with normals a finite normal longer than 1e-12),
//                   its int32 cell, the status word where no int32 holds it.
// (k_voxel.hip)     voxel_group_run -- k_voxel_insert, k_voxel_first, scan, k_voxel_ids, stable radix sort by cell id,
//                   k_voxel_segments: a cell's rows contiguous and in ascending index.
// k_icp_slots       one thread per table slot: the cell and the range of its rows, so that a probe reads one 16-byte slot.
// k_icp_gather      the participating points (and unit normals) widened and copied in sorted order; sidx keeps the original index.
// A pass:
// k_icp_correspond  one thread per source row: transform, 27 probes in the model's order (dx outer, dz inner), each cell's rows in
//                   order, strict < against a best that starts at max_corr_dist^2; writes nn, r, the |r| sort key, the flag, x and q / n.
// (rocPRIM)         the count is the integer sum of the flags; the keys are radix-sorted, which is exact and order-free.
// k_icp_median      one thread: elements mid (and mid - 1) of the sorted keys, sigma and the Huber delta.
// k_icp_sums_point_a / _b, k_icp_sums_plane
//                   a workgroup owns ICP_CHUNK consecutive rows: each thread folds its ICP_ROWS_PER_THREAD rows in order, the wave
//                   combines by xor butterfly (6 levels), lane 0 of each wave stores to LDS and one thread per sum folds the waves
//                   in order: one partial per sum and chunk.  k_icp_fold (one workgroup) folds the partials in index order.  A tree
//                   of fixed shape, 3 + 6 + 3 additions deep below the partial fold: the result depends on the inputs only.
// Many sources against a resident target (ouster_hip_icp_target_*): the grid is built once, as above, and what a query reads is
// kept by the handle.  A pass is one launch sequence for all sources:
// k_icp_correspond_many, k_icp_sums_point_a_many / _b_many, k_icp_sums_plane_many
//                   a workgroup per chunk of the chunk table {source, first row within the source, rows}: every source is cut
//                   into the runs of ICP_CHUNK rows the single call uses, and the bodies are the single call's (correspond_row,
//                   sums_point, sums_plane, block_sums) with the source's pose, pointers and header.
// (rocPRIM)         a segmented sum of the flags and a segmented radix sort of the keys, a segment per source.
// k_icp_median_many a thread per source; k_icp_fold_many: a workgroup per source folds that source's chunks in index order.
//                   Equal chunking and equal fold order: a source's sums are those of a call of its own, bit for bit.  A chunk of
//                   an inactive source (fewer than 20 rows, or out of the loop already) returns at once.
#include <hip/hip_runtime.h>

#include "icp_sums_dev.h"
#include "k_icp.h"
#include "voxel_dev.h"

#ifdef __HIPCC__
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/device/device_segmented_reduce.hpp>
#endif

namespace ouster_hip_dev {
namespace {

template <class T>
__device__ __forceinline__ void load3(const void* base, uint64_t stride, uint32_t i, double& a, double& b, double& c) {
    const T* p = static_cast<const T*>(base) + (uint64_t)i * stride;
    a = (double)p[0], b = (double)p[1], c = (double)p[2];
}

__device__ __forceinline__ double norm3(double a, double b, double c) { return sqrt((a * a + b * b) + c * c); }

template <class T>
__global__ void __launch_bounds__(ICP_WG) k_icp_keys(IcpArgs a) {
    const uint32_t j = blockIdx.x * ICP_WG + threadIdx.x;
    if (j >= a.n_tgt) return;
    double x, y, z;
    load3<T>(a.tgt, a.tgt_stride, j, x, y, z);
    bool take = finite3(x, y, z);
    if (take && a.plane) {
        double m0, m1, m2;
        load3<T>(a.tgt_n, a.tgt_n_stride, j, m0, m1, m2);
        take = finite3(m0, m1, m2) && !(norm3(m0, m1, m2) <= ICP_NORMAL_EPS);
    }
    VoxelKey k{0, 0, 0, 0};
    if (take) {
        const bool ok = axis_to_voxel(x, a.inv, k.x) & axis_to_voxel(y, a.inv, k.y) & axis_to_voxel(z, a.inv, k.z);
        if (ok) {
            k.valid = 1;
        } else {
            k = VoxelKey{0, 0, 0, 0};
            a.rb->pass.status = ICP_STATUS_GRID;
        }
    }
    a.keys[j] = k;
}

__global__ void __launch_bounds__(ICP_WG) k_icp_slots(IcpArgs a) {
    const uint32_t s = blockIdx.x * ICP_WG + threadIdx.x;
    if (s > a.table_mask) return;
    const int32_t j = a.table[s];
    IcpSlot slot{0, 0, 0, -1};
    uint32_t end = 0;
    if (j >= 0 && (uint32_t)j < a.n_tgt) {
        const VoxelKey k = a.keys[j];
        const uint32_t v = a.first_id[j];
        if (k.valid && v < a.n_tgt) {
            const uint32_t b = a.seg_begin[v], e = a.seg_end[v];
            if (b <= e && e <= a.n_tgt) slot = IcpSlot{k.x, k.y, k.z, (int32_t)b}, end = e;
        }
    }
    a.slots[s] = slot;
    a.slot_end[s] = end;
}

template <class T>
__global__ void __launch_bounds__(ICP_WG) k_icp_gather(IcpArgs a) {
    const uint32_t p = blockIdx.x * ICP_WG + threadIdx.x;
    if (p >= a.n_tgt || a.svid[p] >= a.n_tgt) return;
    const uint32_t j = a.sidx[p];
    if (j >= a.n_tgt) return;
    double x, y, z;
    load3<T>(a.tgt, a.tgt_stride, j, x, y, z);
    if (a.plane) {
        double m0, m1, m2;
        load3<T>(a.tgt_n, a.tgt_n_stride, j, m0, m1, m2);
        const double len = norm3(m0, m1, m2);
        double* dst = a.rows + 6 * (uint64_t)p;
        dst[0] = x, dst[1] = y, dst[2] = z;
        dst[3] = m0 / len, dst[4] = m1 / len, dst[5] = m2 / len;
    } else {
        double* dst = a.rows + 3 * (uint64_t)p;
        dst[0] = x, dst[1] = y, dst[2] = z;
    }
}

// the single call's own grid and per-row outputs, as a query reads and writes them
__device__ __forceinline__ IcpQuery icp_query(const IcpArgs& a) {
    return IcpQuery{a.plane, a.table_mask, a.n_tgt, a.inv, a.max_d2, a.cos_gate, a.slots, a.slot_end, a.sidx, a.rows,
                    a.nn, a.r, a.key, a.flag, a.xq};
}

// One source row against the grid.  `a` carries the target and the call's constants; the source's own pointers, its pose P and
// its first row `out` in the per-row outputs are the caller's: k_icp_correspond passes those of `a`, k_icp_correspond_many those of
// the chunk's source.
template <class T>
__device__ __forceinline__ void correspond_row(const IcpQuery& a, const void* src, uint64_t src_stride, const void* src_n,
                                               uint64_t src_n_stride, const double* P, uint32_t row, uint64_t out) {
    const uint32_t W = a.plane ? 6u : 3u;
    double p0, p1, p2, m0 = 0.0, m1 = 0.0, m2 = 0.0;
    load3<T>(src, src_stride, row, p0, p1, p2);
    bool live = true;
    if (a.plane) {
        load3<T>(src_n, src_n_stride, row, m0, m1, m2);
        const double len = norm3(m0, m1, m2);
        live = finite3(m0, m1, m2) && !(len <= ICP_NORMAL_EPS);
        m0 = m0 / len, m1 = m1 / len, m2 = m2 / len;
    }
    const double x0 = ((P[0] * p0 + P[1] * p1) + P[2] * p2) + P[3];
    const double x1 = ((P[4] * p0 + P[5] * p1) + P[6] * p2) + P[7];
    const double x2 = ((P[8] * p0 + P[9] * p1) + P[10] * p2) + P[11];
    int32_t c0 = 0, c1 = 0, c2 = 0;
    live = live && finite3(x0, x1, x2);
    // a query whose cell no int32 holds has no neighbour
    if (live) live = axis_to_voxel(x0, a.inv, c0) & axis_to_voxel(x1, a.inv, c1) & axis_to_voxel(x2, a.inv, c2);
    int64_t best = -1;
    double best_d2 = a.max_d2;
    if (live) {
        for (int dx = -1; dx <= 1; ++dx)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dz = -1; dz <= 1; ++dz) {
                    const int64_t cx = (int64_t)c0 + dx, cy = (int64_t)c1 + dy, cz = (int64_t)c2 + dz;
                    if (cx < INT32_MIN || cx > INT32_MAX || cy < INT32_MIN || cy > INT32_MAX || cz < INT32_MIN || cz > INT32_MAX) continue;
                    const VoxelKey k{(int32_t)cx, (int32_t)cy, (int32_t)cz, 1};
                    uint32_t s = voxel_hash(k) & a.table_mask;
                    // the table has more slots than rows: a free slot ends every chain; bounded by the table's size all the same
                    for (uint32_t probe = 0; probe <= a.table_mask; ++probe) {
                        const IcpSlot slot = a.slots[s];
                        if (slot.begin < 0) break;
                        if (slot.x == k.x && slot.y == k.y && slot.z == k.z) {
                            uint32_t e = a.slot_end[s];
                            if (e > a.n_tgt) e = a.n_tgt;
                            for (uint32_t p = (uint32_t)slot.begin; p < e; ++p) {
                                const double* t = a.rows + (uint64_t)W * p;
                                const double e0 = t[0] - x0, e1 = t[1] - x1, e2 = t[2] - x2;
                                const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
                                if (d2 < best_d2) best_d2 = d2, best = p;
                            }
                            break;
                        }
                        s = (s + 1) & a.table_mask;
                    }
                }
    }
    int32_t nn = -1;
    double r = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (best >= 0) {
        const double* t = a.rows + (uint64_t)W * (uint64_t)best;
        const double e0 = x0 - t[0], e1 = x1 - t[1], e2 = x2 - t[2];
        bool keep = true;
        if (a.plane) {
            const double w0 = (P[0] * m0 + P[1] * m1) + P[2] * m2;
            const double w1 = (P[4] * m0 + P[5] * m1) + P[6] * m2;
            const double w2 = (P[8] * m0 + P[9] * m1) + P[10] * m2;
            s0 = t[3], s1 = t[4], s2 = t[5];
            const double align = fabs((s0 * w0 + s1 * w1) + s2 * w2);
            keep = __builtin_isfinite(align) && !(align < a.cos_gate);
            r = (s0 * e0 + s1 * e1) + s2 * e2;
        } else {
            s0 = t[0], s1 = t[1], s2 = t[2];
            r = norm3(e0, e1, e2);
        }
        keep = keep && __builtin_isfinite(r);
        const uint32_t j = a.sidx[best];
        if (keep && j < a.n_tgt) nn = (int32_t)j;
    }
    if (nn < 0) r = 0.0, s0 = s1 = s2 = 0.0;
    a.nn[out] = nn;
    a.r[out] = r;
    a.key[out] = nn >= 0 ? (uint64_t)__double_as_longlong(fabs(r)) : ICP_NO_KEY;
    a.flag[out] = nn >= 0;
    double* o = a.xq + 6 * out;
    o[0] = x0, o[1] = x1, o[2] = x2, o[3] = s0, o[4] = s1, o[5] = s2;
}

template <class T>
__global__ void __launch_bounds__(ICP_WG) k_icp_correspond(IcpArgs a) {
    const uint32_t i = blockIdx.x * ICP_WG + threadIdx.x;
    if (i >= a.n_src) return;
    correspond_row<T>(icp_query(a), a.src, a.src_stride, a.src_n, a.src_n_stride, a.pose, i, i);
}

// The same for many sources in one launch: a workgroup per chunk of the chunk table, thread t on rows first + t + 256 k of the
// chunk's source (the map of the sum kernels), with that source's pointers and pose.  A chunk of an inactive source returns at once.
template <class T>
__global__ void __launch_bounds__(ICP_WG) k_icp_correspond_many(IcpManyArgs m) {
    if (blockIdx.x >= m.n_chunks) return;
    const IcpChunk c = m.chunks[blockIdx.x];
    if (c.source >= m.n_sources) return;
    const IcpSource* s = m.sources + c.source;
    if (!s->active) return;
    for (uint32_t k = 0; k < ICP_ROWS_PER_THREAD; ++k) {
        const uint32_t t = threadIdx.x + ICP_WG * k;
        if (t >= c.rows || c.first + t >= s->n || (uint64_t)s->first + c.first + t >= m.n_rows) continue;
        correspond_row<T>(m.q, s->src, s->src_stride, s->src_n, s->src_n_stride, s->pose, c.first + t, s->first + c.first + t);
    }
}

// one thread, after the grid: the rows that take part are sorted first, so the end of the last cell counts them -> pass.count
// (what ouster_hip_icp_target_create reports; a pass overwrites it)
__global__ void k_icp_rows_used(IcpArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint32_t cells = a.rb->grid.n_vox;
    uint32_t used = 0;
    if (cells && cells <= a.n_tgt) used = a.seg_end[cells - 1];
    a.rb->pass.count = used <= a.n_tgt ? used : a.n_tgt;
}

// What follows the correspondences uses cross-lane operations and several kernel arguments: device only.  The host-lanes build of
// tests/cpp/icp_lanes.cpp compiles everything above, one thread per lane; these are tests/test_gpu_icp.py's business.
#ifdef __HIPCC__
// the median of the `count` smallest of a source's n sorted keys, sigma and the Huber delta -> h
__device__ __forceinline__ void median_of(IcpHeader* h, uint32_t count, const uint64_t* key_sorted, uint32_t n, double max_corr_dist) {
    double median = 0.0, delta = 0.0;
    if (count >= ICP_MIN_POINTS && count <= n) {
        const uint32_t mid = count / 2;
        const double hi = __longlong_as_double((long long)key_sorted[mid]);
        median = (count & 1u) ? hi : 0.5 * (__longlong_as_double((long long)key_sorted[mid - 1]) + hi);
        double sigma = 1.4826 * median;
        if (!__builtin_isfinite(sigma) || sigma < 1e-4) sigma = fmax(1e-3, 0.25 * max_corr_dist);
        delta = 1.5 * sigma;
    }
    h->median = median;
    h->huber_delta = delta;
}

__global__ void k_icp_median(IcpArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    IcpHeader* h = &a.rb->pass;
    median_of(h, h->count, a.key_sorted, a.n_src, a.max_corr_dist);
}

// one thread per source: the count of the segmented reduction into the source's header, then the same arithmetic
__global__ void __launch_bounds__(64) k_icp_median_many(IcpManyArgs m) {
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    if (k >= m.n_sources) return;
    const IcpSource* s = m.sources + k;
    if (!s->active || (uint64_t)s->first + s->n > m.n_rows) return;
    IcpHeader* h = m.hdr + k;
    const uint32_t count = m.counts[k];
    h->status = 0;
    h->count = count;
    median_of(h, count, m.key_sorted + s->first, s->n, m.max_corr_dist);
}

__device__ __forceinline__ double huber_weight(double r, double delta) {
    const double ar = fabs(r);
    return (ar <= delta || delta <= 0.0) ? 1.0 : delta / ar;
}

// the rows a workgroup of the sum kernels folds: rows base + t + 256 k below n of one source, whose per-row outputs start at
// nn / r / xq; the source's header and where the partial goes
struct IcpRows {
    const int32_t* nn;
    const double *r, *xq;
    uint64_t base;
    uint32_t n;
    const IcpHeader* h;
    double* partial;   // [OUSTER_HIP_ICP_SUMS] of this chunk
};

__device__ __forceinline__ IcpRows rows_of(const IcpArgs& a) {
    return IcpRows{a.nn, a.r, a.xq, (uint64_t)blockIdx.x * ICP_CHUNK, a.n_src, &a.rb->pass,
                   a.partials + (uint64_t)blockIdx.x * OUSTER_HIP_ICP_SUMS};
}

// false: the chunk's source is inactive (the whole workgroup leaves)
__device__ __forceinline__ bool rows_of(const IcpManyArgs& m, IcpRows& v) {
    if (blockIdx.x >= m.n_chunks) return false;
    const IcpChunk c = m.chunks[blockIdx.x];
    if (c.source >= m.n_sources) return false;
    const IcpSource* s = m.sources + c.source;
    if (!s->active || (uint64_t)s->first + s->n > m.n_rows) return false;
    v = IcpRows{m.q.nn + s->first, m.q.r + s->first, m.q.xq + 6 * (uint64_t)s->first, c.first, s->n, m.hdr + c.source,
                m.partials + (uint64_t)blockIdx.x * OUSTER_HIP_ICP_SUMS};
    return true;
}

// mode 0: w, w x, w q.  mode 1: (w (x - cx)_i) (q - cq)_j with the centroids of the header
template <int MODE>
__device__ __forceinline__ void sums_point(const IcpRows& a) {
    constexpr int NS = MODE == 0 ? 7 : 9;
    const IcpHeader* h = a.h;
    const double delta = h->huber_delta;
    double cx[3] = {0, 0, 0}, cq[3] = {0, 0, 0};
    if (MODE == 1)
        for (int k = 0; k < 3; ++k) cx[k] = h->centroid_x[k], cq[k] = h->centroid_q[k];
    double acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = 0.0;
    const uint64_t base = a.base;
    for (uint32_t k = 0; k < ICP_ROWS_PER_THREAD; ++k) {
        const uint64_t i = base + threadIdx.x + (uint64_t)ICP_WG * k;
        if (i >= a.n || a.nn[i] < 0) continue;
        const double w = huber_weight(a.r[i], delta);
        const double* o = a.xq + 6 * i;
        if (MODE == 0) {
            acc[0] = acc[0] + w;
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[1 + c] = acc[1 + c] + w * o[c], acc[4 + c] = acc[4 + c] + w * o[3 + c];
        } else {
            double wx[3], dq[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) wx[c] = w * (o[c] - cx[c]), dq[c] = o[3 + c] - cq[c];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[3 * r + c] = acc[3 * r + c] + wx[r] * dq[c];
        }
    }
    block_sums<NS>(acc, a.partial + (MODE == 0 ? 0 : 7));
}

__device__ __forceinline__ void sums_plane(const IcpRows& a) {
    constexpr int NS = 27;
    const double delta = a.h->huber_delta;
    double acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = 0.0;
    const uint64_t base = a.base;
    for (uint32_t k = 0; k < ICP_ROWS_PER_THREAD; ++k) {
        const uint64_t i = base + threadIdx.x + (uint64_t)ICP_WG * k;
        if (i >= a.n || a.nn[i] < 0) continue;
        const double r = a.r[i], w = huber_weight(r, delta);
        const double* o = a.xq + 6 * i;
        const double j[6] = {o[1] * o[5] - o[2] * o[4], o[2] * o[3] - o[0] * o[5], o[0] * o[4] - o[1] * o[3], o[3], o[4], o[5]};
        int at = 0;
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
            for (int q = p; q < 6; ++q, ++at) acc[at] = acc[at] + w * (j[p] * j[q]);
#pragma unroll
        for (int p = 0; p < 6; ++p) acc[21 + p] = acc[21 + p] + (-w) * (j[p] * r);
    }
    block_sums<NS>(acc, a.partial);
}

__global__ void __launch_bounds__(ICP_WG) k_icp_sums_point_a(IcpArgs a) { sums_point<0>(rows_of(a)); }
__global__ void __launch_bounds__(ICP_WG) k_icp_sums_point_b(IcpArgs a) { sums_point<1>(rows_of(a)); }
__global__ void __launch_bounds__(ICP_WG) k_icp_sums_plane(IcpArgs a) { sums_plane(rows_of(a)); }

// The many-source forms: a workgroup per chunk of the chunk table, the same per-thread fold and the same tree, into partials[chunk].
// (The test is uniform over the workgroup: all of it leaves, or all of it reaches the barrier of block_sums.)
__global__ void __launch_bounds__(ICP_WG) k_icp_sums_point_a_many(IcpManyArgs m) {
    IcpRows v;
    if (rows_of(m, v)) sums_point<0>(v);
}
__global__ void __launch_bounds__(ICP_WG) k_icp_sums_point_b_many(IcpManyArgs m) {
    IcpRows v;
    if (rows_of(m, v)) sums_point<1>(v);
}
__global__ void __launch_bounds__(ICP_WG) k_icp_sums_plane_many(IcpManyArgs m) {
    IcpRows v;
    if (rows_of(m, v)) sums_plane(v);
}

// sum `ofs + t` of the header is the left fold of the chunks' partials in index order; centroids: then cx = sum w x / sum w, cq
// likewise (the divisions of the reference's loop)
__device__ __forceinline__ void fold_partials(IcpHeader* h, const double* partials, uint32_t ofs, uint32_t ns, uint32_t chunks, int centroids) {
    if (threadIdx.x < ns) {
        double v = 0.0;
        for (uint32_t c = 0; c < chunks; ++c) v = v + partials[(uint64_t)c * OUSTER_HIP_ICP_SUMS + ofs + threadIdx.x];
        h->sums[ofs + threadIdx.x] = v;
    }
    __syncthreads();
    if (centroids && threadIdx.x < 3) {
        const double w = h->sums[0];
        h->centroid_x[threadIdx.x] = h->sums[1 + threadIdx.x] / w;
        h->centroid_q[threadIdx.x] = h->sums[4 + threadIdx.x] / w;
    }
}

// one workgroup
__global__ void __launch_bounds__(64) k_icp_fold(IcpArgs a, uint32_t ofs, uint32_t ns, uint32_t chunks, int centroids) {
    fold_partials(&a.rb->pass, a.partials, ofs, ns, chunks, centroids);
}

// one workgroup per source: that source's chunks, in index order
__global__ void __launch_bounds__(64) k_icp_fold_many(IcpManyArgs m, uint32_t ofs, uint32_t ns, int centroids) {
    if (blockIdx.x >= m.n_sources) return;
    const IcpSource* s = m.sources + blockIdx.x;
    if (!s->active || (uint64_t)s->first_chunk + s->chunks > m.n_chunks) return;
    fold_partials(m.hdr + blockIdx.x, m.partials + (uint64_t)s->first_chunk * OUSTER_HIP_ICP_SUMS, ofs, ns, s->chunks, centroids);
}

#endif

inline dim3 icp_grid(uint64_t n) { return dim3((uint32_t)((n + ICP_WG - 1) / ICP_WG)); }

}  // namespace

hipError_t launch_icp_keys(const IcpArgs& a, hipStream_t st) {
    if (a.n_tgt == 0) return hipSuccess;
    if (a.f32) hipLaunchKernelGGL(k_icp_keys<float>, icp_grid(a.n_tgt), dim3(ICP_WG), 0, st, a);
    else hipLaunchKernelGGL(k_icp_keys<double>, icp_grid(a.n_tgt), dim3(ICP_WG), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_icp_slots(const IcpArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_icp_slots, icp_grid((uint64_t)a.table_mask + 1), dim3(ICP_WG), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_icp_gather(const IcpArgs& a, hipStream_t st) {
    if (a.n_tgt == 0) return hipSuccess;
    if (a.f32) hipLaunchKernelGGL(k_icp_gather<float>, icp_grid(a.n_tgt), dim3(ICP_WG), 0, st, a);
    else hipLaunchKernelGGL(k_icp_gather<double>, icp_grid(a.n_tgt), dim3(ICP_WG), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_icp_correspond(const IcpArgs& a, hipStream_t st) {
    if (a.n_src == 0) return hipSuccess;
    if (a.table_mask < a.n_tgt) return hipErrorInvalidValue;   // more slots than rows: what ends every probe chain
    if (a.f32) hipLaunchKernelGGL(k_icp_correspond<float>, icp_grid(a.n_src), dim3(ICP_WG), 0, st, a);
    else hipLaunchKernelGGL(k_icp_correspond<double>, icp_grid(a.n_src), dim3(ICP_WG), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_icp_rows_used(const IcpArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_icp_rows_used, dim3(1), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_icp_correspond_many(const IcpManyArgs& m, hipStream_t st) {
    if (m.n_chunks == 0) return hipSuccess;
    if (m.q.table_mask < m.q.n_tgt) return hipErrorInvalidValue;   // more slots than rows: what ends every probe chain
    if (m.f32) hipLaunchKernelGGL(k_icp_correspond_many<float>, dim3(m.n_chunks), dim3(ICP_WG), 0, st, m);
    else hipLaunchKernelGGL(k_icp_correspond_many<double>, dim3(m.n_chunks), dim3(ICP_WG), 0, st, m);
    return hipGetLastError();
}

#if OUSTER_DEVICE_WIDE
hipError_t icp_grid_run(const IcpArgs& a, const VoxelArgs& va, void* temp, size_t temp_bytes, hipStream_t st) {
    if (a.n_tgt == 0 || va.n != a.n_tgt) return hipErrorInvalidValue;
    // every call starts from a clean header (and, in voxel_group_run, an empty table)
    RUN_TRY(hipMemsetAsync(a.rb, 0, sizeof(IcpReadback), st));
    RUN_TRY(launch_icp_keys(a, st));
    RUN_TRY(voxel_group_run(va, temp, temp_bytes, st));
    RUN_TRY(launch_icp_slots(a, st));
    return launch_icp_gather(a, st);
}
#endif

#ifdef __HIPCC__
hipError_t icp_temp_bytes(uint32_t n_src, uint32_t n_tgt, size_t* bytes) {
    size_t grid = 0, sort = 0, reduce = 0;
    hipError_t e = voxel_temp_bytes(n_tgt, &grid);
    if (e != hipSuccess) return e;
    uint64_t* k = nullptr;
    uint32_t* u = nullptr;
    e = rocprim::radix_sort_keys(nullptr, sort, k, k, (size_t)n_src, 0, 64);
    if (e != hipSuccess) return e;
    e = rocprim::reduce(nullptr, reduce, u, u, 0u, (size_t)n_src, rocprim::plus<uint32_t>());
    if (e != hipSuccess) return e;
    *bytes = grid > sort ? grid : sort;
    if (reduce > *bytes) *bytes = reduce;
    return hipSuccess;
}

hipError_t icp_many_temp_bytes(uint32_t n_rows, uint32_t n_sources, size_t* bytes) {
    size_t sort = 0, reduce = 0;
    uint64_t* k = nullptr;
    uint32_t* u = nullptr;
    RUN_TRY(rocprim::segmented_radix_sort_keys(nullptr, sort, k, k, n_rows, n_sources, u, u, 0, 64));
    RUN_TRY(rocprim::segmented_reduce(nullptr, reduce, u, u, n_sources, u, u, rocprim::plus<uint32_t>(), 0u));
    *bytes = sort > reduce ? sort : reduce;
    return hipSuccess;
}

hipError_t icp_many_pass_run(const IcpManyArgs& m, void* temp, size_t temp_bytes, hipStream_t st) {
    if (m.n_sources == 0 || m.n_chunks == 0 || m.n_rows == 0) return hipErrorInvalidValue;
    RUN_TRY(launch_icp_correspond_many(m, st));
    // an inactive source's segment is empty (seg_end == seg_begin): nothing of it is reduced or sorted
    size_t bytes = temp_bytes;
    RUN_TRY(rocprim::segmented_reduce(temp, bytes, m.q.flag, m.counts, m.n_sources, m.seg_begin, m.seg_end, rocprim::plus<uint32_t>(), 0u, st));
    bytes = temp_bytes;
    RUN_TRY(rocprim::segmented_radix_sort_keys(temp, bytes, m.q.key, m.key_sorted, m.n_rows, m.n_sources, m.seg_begin, m.seg_end, 0, 64, st));
    hipLaunchKernelGGL(k_icp_median_many, dim3((m.n_sources + 63) / 64), dim3(64), 0, st, m);
    RUN_TRY(hipGetLastError());
    if (m.q.plane) {
        hipLaunchKernelGGL(k_icp_sums_plane_many, dim3(m.n_chunks), dim3(ICP_WG), 0, st, m);
        RUN_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_icp_fold_many, dim3(m.n_sources), dim3(64), 0, st, m, 0u, 27u, 0);
        RUN_TRY(hipGetLastError());
    } else {
        hipLaunchKernelGGL(k_icp_sums_point_a_many, dim3(m.n_chunks), dim3(ICP_WG), 0, st, m);
        RUN_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_icp_fold_many, dim3(m.n_sources), dim3(64), 0, st, m, 0u, 7u, 1);
        RUN_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_icp_sums_point_b_many, dim3(m.n_chunks), dim3(ICP_WG), 0, st, m);
        RUN_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_icp_fold_many, dim3(m.n_sources), dim3(64), 0, st, m, 7u, 9u, 0);
        RUN_TRY(hipGetLastError());
    }
    return hipSuccess;
}

hipError_t icp_pass_run(const IcpArgs& a, void* temp, size_t temp_bytes, hipStream_t st, hipEvent_t* ev) {
    if (a.n_src == 0) return hipErrorInvalidValue;
    const uint32_t chunks = icp_chunks(a.n_src);
    RUN_TRY(launch_icp_correspond(a, st));
    if (ev) RUN_TRY(hipEventRecord(ev[0], st));
    size_t bytes = temp_bytes;
    RUN_TRY(rocprim::reduce(temp, bytes, a.flag, &a.rb->pass.count, 0u, (size_t)a.n_src, rocprim::plus<uint32_t>(), st));
    bytes = temp_bytes;
    RUN_TRY(rocprim::radix_sort_keys(temp, bytes, a.key, a.key_sorted, (size_t)a.n_src, 0, 64, st));
    hipLaunchKernelGGL(k_icp_median, dim3(1), dim3(64), 0, st, a);
    RUN_TRY(hipGetLastError());
    if (ev) RUN_TRY(hipEventRecord(ev[1], st));
    if (a.plane) {
        hipLaunchKernelGGL(k_icp_sums_plane, dim3(chunks), dim3(ICP_WG), 0, st, a);
        RUN_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_icp_fold, dim3(1), dim3(64), 0, st, a, 0u, 27u, chunks, 0);
        RUN_TRY(hipGetLastError());
    } else {
        hipLaunchKernelGGL(k_icp_sums_point_a, dim3(chunks), dim3(ICP_WG), 0, st, a);
        RUN_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_icp_fold, dim3(1), dim3(64), 0, st, a, 0u, 7u, chunks, 1);
        RUN_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_icp_sums_point_b, dim3(chunks), dim3(ICP_WG), 0, st, a);
        RUN_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_icp_fold, dim3(1), dim3(64), 0, st, a, 7u, 9u, chunks, 0);
        RUN_TRY(hipGetLastError());
    }
    if (ev) RUN_TRY(hipEventRecord(ev[2], st));
    return hipSuccess;
}
#endif

}  // namespace ouster_hip_dev
