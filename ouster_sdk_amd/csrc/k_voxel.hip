// k_voxel.hip -- voxel down-sampling (core::voxel_downsample_3d / _xd, algorithm::voxel_downsample_with_normals) on the GPU, held
// bit for bit to tests/voxel_model.py.  Built with -ffp-contract=off: every multiply, add, divide and sqrt below is one IEEE double
// operation in the model's order.  A voxel's sum is a left fold over its points in input order -- store and sum over an inverted
// index with a fixed order; no floating-point atomic anywhere.
//
// k_voxel_keys     one thread per row: the validity tests of the form, int32 voxel indices, the status word on a refusal.
// k_voxel_insert   open addressing in a table of row indices: atomicCAS takes a free slot, a slot held by a row of the same voxel
//                  is joined with atomicMin, anything else sends the probe on.  A slot never becomes free again and only ever passes
//                  between rows of one voxel, so all rows of a voxel stop at the same slot, which ends up holding their smallest
//                  index whatever the arrival order.  No lane waits for another; the loop is bounded by the table's size.
// k_voxel_first / k_voxel_ids   a row opens a voxel if the slot holds its own index; the exclusive scan of these flags numbers the
//                  voxels in first-seen order, and every row reads its voxel's id through its slot.
// (stable radix sort of row indices by voxel id: each voxel's rows contiguous and in input order)
// k_voxel_segments the range of each voxel in the sorted order.
// k_voxel_gather   AVERAGE, NORMALS: the rows, widened, in sorted order, so that a segment is one contiguous stream.
// k_voxel_reduce   one thread per voxel walks its segment in order; the result replaces the segment's first row.
// k_voxel_write    (after the scan of the keep flags) rows to their place in the output; nothing on a refusal or a short output.
#include <hip/hip_runtime.h>

#include "k_voxel.h"
#include "voxel_dev.h"

#if OUSTER_DEVICE_WIDE
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#endif

namespace ouster_hip_dev {
namespace {

template <class T>
__global__ void __launch_bounds__(VOXEL_WG) k_voxel_keys(VoxelArgs a) {
    const uint32_t i = blockIdx.x * VOXEL_WG + threadIdx.x;
    if (i >= a.n) return;
    const T* p = static_cast<const T*>(a.points) + (uint64_t)i * a.stride;
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    bool take = true;
    if (a.form == VOXEL_FORM_NORMALS) {
        const double* m = a.normals + 3 * (uint64_t)i;
        const double m0 = m[0], m1 = m[1], m2 = m[2];
        take = finite3(x, y, z) && finite3(m0, m1, m2);
        if (take) take = !(sqrt((m0 * m0 + m1 * m1) + m2 * m2) <= 1e-12);
    }
    VoxelKey k{0, 0, 0, 0};
    if (take) {
        const bool ok = axis_to_voxel(x, a.inv, k.x) & axis_to_voxel(y, a.inv, k.y) & axis_to_voxel(z, a.inv, k.z);
        if (ok) {
            k.valid = 1;
        } else {
            k = VoxelKey{0, 0, 0, 0};
            a.hdr->status = VOXEL_STATUS_GRID;
        }
    }
    a.keys[i] = k;
}

__global__ void __launch_bounds__(VOXEL_WG) k_voxel_insert(VoxelArgs a) {
    const uint32_t i = blockIdx.x * VOXEL_WG + threadIdx.x;
    if (i >= a.n) return;
    const VoxelKey k = a.keys[i];
    if (!k.valid) return;
    uint32_t s = voxel_hash(k) & a.table_mask;
    for (uint32_t probe = 0; probe <= a.table_mask; ++probe) {
        const int32_t cur = atomicCAS(&a.table[s], VOXEL_EMPTY, (int32_t)i);
        if (cur == VOXEL_EMPTY) {
            a.slot[i] = s;
            return;
        }
        const VoxelKey o = a.keys[cur];   // the table was reset for this call: cur is a valid row of it
        if (o.x == k.x && o.y == k.y && o.z == k.z) {
            if ((uint32_t)cur > i) atomicMin(&a.table[s], (int32_t)i);
            a.slot[i] = s;
            return;
        }
        s = (s + 1) & a.table_mask;
    }
    // every slot is held by another voxel: impossible with more slots than rows; reported, not looped on.  The status values are
    // plain stores and not combined: whichever lands last is read back, and any non-zero value refuses the call
    a.slot[i] = 0;
    a.hdr->status = VOXEL_STATUS_TABLE;
}

__global__ void __launch_bounds__(VOXEL_WG) k_voxel_first(VoxelArgs a) {
    const uint32_t i = blockIdx.x * VOXEL_WG + threadIdx.x;
    if (i >= a.n) return;
    a.first[i] = a.keys[i].valid && a.table[a.slot[i]] == (int32_t)i;
}

__global__ void __launch_bounds__(VOXEL_WG) k_voxel_ids(VoxelArgs a) {
    const uint32_t i = blockIdx.x * VOXEL_WG + threadIdx.x;
    if (i >= a.n) return;
    uint32_t v = a.n;
    if (a.keys[i].valid) {
        const int32_t j = a.table[a.slot[i]];
        if (j >= 0 && (uint32_t)j < a.n) v = a.first_id[j];
    }
    a.vid[i] = v;
    a.idx[i] = i;
    if (i == a.n - 1) a.hdr->n_vox = a.first_id[i] + a.first[i];
}

__global__ void __launch_bounds__(VOXEL_WG) k_voxel_segments(VoxelArgs a) {
    const uint32_t p = blockIdx.x * VOXEL_WG + threadIdx.x;
    if (p >= a.n) return;
    const uint32_t v = a.svid[p], prev = p ? a.svid[p - 1] : VOXEL_NO_ID;
    if (v != prev) {
        if (v < a.n) a.seg_begin[v] = p;
        if (p && prev < a.n) a.seg_end[prev] = p;
    }
    if (p == a.n - 1 && v < a.n) a.seg_end[v] = a.n;
}

template <class T>
__global__ void __launch_bounds__(VOXEL_WG) k_voxel_gather(VoxelArgs a) {
    const uint32_t p = blockIdx.x * VOXEL_WG + threadIdx.x;
    if (p >= a.n || a.svid[p] >= a.n) return;
    const uint32_t i = a.sidx[p];
    if (i >= a.n) return;
    const T* src = static_cast<const T*>(a.points) + (uint64_t)i * a.stride;
    if (a.form == VOXEL_FORM_NORMALS) {
        double* dst = a.rows + 6 * (uint64_t)p;
        const double* m = a.normals + 3 * (uint64_t)i;
        for (int c = 0; c < 3; ++c) dst[c] = (double)src[c], dst[3 + c] = m[c];
    } else {
        double* dst = a.rows + (uint64_t)a.cols * p;
        for (uint32_t c = 0; c < a.cols; ++c) dst[c] = (double)src[c];
    }
}

__global__ void __launch_bounds__(VOXEL_WG) k_voxel_reduce(VoxelArgs a) {
    const uint32_t v = blockIdx.x * VOXEL_WG + threadIdx.x;
    if (v >= a.n) return;
    if (v >= a.hdr->n_vox) {
        a.keep[v] = 0;
        return;
    }
    const uint64_t b = a.seg_begin[v], e = a.seg_end[v];
    const double count = (double)(e - b);
    if (a.form == VOXEL_FORM_NORMALS) {
        double p0 = 0.0, p1 = 0.0, p2 = 0.0, n0 = 0.0, n1 = 0.0, n2 = 0.0;
        for (uint64_t q = b; q < e; ++q) {
            const double* r = a.rows + 6 * q;
            const double m0 = r[3], m1 = r[4], m2 = r[5];
            const double len = sqrt((m0 * m0 + m1 * m1) + m2 * m2);
            p0 = p0 + r[0], p1 = p1 + r[1], p2 = p2 + r[2];
            n0 = n0 + m0 / len, n1 = n1 + m1 / len, n2 = n2 + m2 / len;
        }
        const double len = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
        double* r = a.rows + 6 * b;
        r[0] = p0 / count, r[1] = p1 / count, r[2] = p2 / count;
        r[3] = n0 / len, r[4] = n1 / len, r[5] = n2 / len;
        a.keep[v] = !(len <= 1e-12);
        return;
    }
    const uint64_t cols = a.cols;
    {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (uint64_t q = b; q < e; ++q) {
            const double* r = a.rows + cols * q;
            s0 = s0 + r[0], s1 = s1 + r[1], s2 = s2 + r[2];
        }
        double* r = a.rows + cols * b;
        r[0] = s0 / count, r[1] = s1 / count, r[2] = s2 / count;
    }
    for (uint64_t c = 3; c < cols; ++c) {   // attribute columns, one at a time: column c of the first row is read before it is replaced
        double s = 0.0;
        for (uint64_t q = b; q < e; ++q) s = s + a.rows[cols * q + c];
        a.rows[cols * b + c] = s / count;
    }
    a.keep[v] = (e - b) >= a.min_pts;
}

template <class T>
__global__ void __launch_bounds__(VOXEL_WG) k_voxel_write(VoxelArgs a) {
    const uint32_t v = blockIdx.x * VOXEL_WG + threadIdx.x;
    if (v >= a.n) return;
    const uint32_t n_vox = a.hdr->n_vox;
    const bool copies = a.form == VOXEL_FORM_FIRST || a.form == VOXEL_FORM_LAST;
    const uint64_t total = copies ? (uint64_t)n_vox : (uint64_t)a.pos[a.n - 1] + a.keep[a.n - 1];
    if (v == 0) a.hdr->n_out = total;
    if (a.hdr->status != 0 || total > a.out_capacity || v >= n_vox) return;
    if (copies) {
        const uint32_t p = a.form == VOXEL_FORM_FIRST ? a.seg_begin[v] : a.seg_end[v] - 1;
        if (p >= a.n) return;
        const uint32_t i = a.sidx[p];
        if (i >= a.n) return;
        const T* src = static_cast<const T*>(a.points) + (uint64_t)i * a.stride;
        double* dst = a.out + (uint64_t)a.cols * v;
        for (uint32_t c = 0; c < a.cols; ++c) dst[c] = (double)src[c];
        return;
    }
    if (!a.keep[v]) return;
    const uint64_t r = a.pos[v];
    if (r >= total) return;
    if (a.form == VOXEL_FORM_NORMALS) {
        const double* src = a.rows + 6 * (uint64_t)a.seg_begin[v];
        for (int c = 0; c < 3; ++c) a.out[3 * r + c] = src[c], a.out_normals[3 * r + c] = src[3 + c];
    } else {
        const double* src = a.rows + (uint64_t)a.cols * a.seg_begin[v];
        double* dst = a.out + (uint64_t)a.cols * r;
        for (uint32_t c = 0; c < a.cols; ++c) dst[c] = src[c];
    }
}

inline dim3 voxel_grid(uint32_t n) { return dim3((n + VOXEL_WG - 1) / VOXEL_WG); }

}  // namespace

hipError_t launch_voxel_keys(const VoxelArgs& a, hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    if (a.f32) hipLaunchKernelGGL(k_voxel_keys<float>, voxel_grid(a.n), dim3(VOXEL_WG), 0, st, a);
    else hipLaunchKernelGGL(k_voxel_keys<double>, voxel_grid(a.n), dim3(VOXEL_WG), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_voxel_insert(const VoxelArgs& a, hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    if (a.table_mask < a.n) return hipErrorInvalidValue;   // more slots than rows: what bounds the probe loop
    hipLaunchKernelGGL(k_voxel_insert, voxel_grid(a.n), dim3(VOXEL_WG), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_voxel_first(const VoxelArgs& a, hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_voxel_first, voxel_grid(a.n), dim3(VOXEL_WG), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_voxel_ids(const VoxelArgs& a, hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_voxel_ids, voxel_grid(a.n), dim3(VOXEL_WG), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_voxel_segments(const VoxelArgs& a, hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_voxel_segments, voxel_grid(a.n), dim3(VOXEL_WG), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_voxel_gather(const VoxelArgs& a, hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    if (a.f32) hipLaunchKernelGGL(k_voxel_gather<float>, voxel_grid(a.n), dim3(VOXEL_WG), 0, st, a);
    else hipLaunchKernelGGL(k_voxel_gather<double>, voxel_grid(a.n), dim3(VOXEL_WG), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_voxel_reduce(const VoxelArgs& a, hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_voxel_reduce, voxel_grid(a.n), dim3(VOXEL_WG), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_voxel_write(const VoxelArgs& a, hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    if (a.f32) hipLaunchKernelGGL(k_voxel_write<float>, voxel_grid(a.n), dim3(VOXEL_WG), 0, st, a);
    else hipLaunchKernelGGL(k_voxel_write<double>, voxel_grid(a.n), dim3(VOXEL_WG), 0, st, a);
    return hipGetLastError();
}

#if OUSTER_DEVICE_WIDE
hipError_t voxel_temp_bytes(uint32_t n, size_t* bytes) {
    size_t scan = 0, sort = 0;
    uint32_t* u = nullptr;
    hipError_t e = rocprim::exclusive_scan(nullptr, scan, u, u, 0u, (size_t)n, rocprim::plus<uint32_t>());
    if (e != hipSuccess) return e;
    e = rocprim::radix_sort_pairs(nullptr, sort, u, u, u, u, (size_t)n, 0, voxel_sort_bits(n));
    if (e != hipSuccess) return e;
    *bytes = scan > sort ? scan : sort;
    return hipSuccess;
}

hipError_t voxel_group_run(const VoxelArgs& a, void* temp, size_t temp_bytes, hipStream_t st, hipEvent_t* ev) {
    if (a.n == 0) return hipSuccess;
    int phase = 0;
    auto mark = [&]() -> hipError_t { return ev ? hipEventRecord(ev[phase++], st) : hipSuccess; };
    // a stale table is the obvious bug of a reused workspace: every call starts from an empty one
    RUN_TRY(hipMemsetAsync(a.table, 0xff, ((size_t)a.table_mask + 1) * sizeof(int32_t), st));
    RUN_TRY(mark());
    RUN_TRY(launch_voxel_insert(a, st));
    RUN_TRY(mark());
    RUN_TRY(launch_voxel_first(a, st));
    size_t bytes = temp_bytes;
    RUN_TRY(rocprim::exclusive_scan(temp, bytes, a.first, a.first_id, 0u, (size_t)a.n, rocprim::plus<uint32_t>(), st));
    RUN_TRY(launch_voxel_ids(a, st));
    RUN_TRY(mark());
    bytes = temp_bytes;
    RUN_TRY(rocprim::radix_sort_pairs(temp, bytes, a.vid, a.svid, a.idx, a.sidx, (size_t)a.n, 0, voxel_sort_bits(a.n), st));
    RUN_TRY(mark());
    RUN_TRY(launch_voxel_segments(a, st));
    return mark();
}

hipError_t voxel_run(const VoxelArgs& a, void* temp, size_t temp_bytes, hipStream_t st, hipEvent_t* ev) {
    if (a.n == 0) return hipSuccess;
    const bool folds = a.form == VOXEL_FORM_AVERAGE || a.form == VOXEL_FORM_NORMALS;
    // ev[0] before the first step; ev[1] .. ev[5] are the grouping's, whose first closes the phase of the resets and the keys;
    // ev[6], ev[7] after the fold and the write
    if (ev) RUN_TRY(hipEventRecord(ev[0], st));
    RUN_TRY(hipMemsetAsync(a.hdr, 0, sizeof(VoxelHeader), st));
    RUN_TRY(launch_voxel_keys(a, st));
    RUN_TRY(voxel_group_run(a, temp, temp_bytes, st, ev ? ev + 1 : nullptr));
    if (folds) {
        RUN_TRY(launch_voxel_gather(a, st));
        RUN_TRY(launch_voxel_reduce(a, st));
        size_t bytes = temp_bytes;
        RUN_TRY(rocprim::exclusive_scan(temp, bytes, a.keep, a.pos, 0u, (size_t)a.n, rocprim::plus<uint32_t>(), st));
    }
    if (ev) RUN_TRY(hipEventRecord(ev[6], st));
    RUN_TRY(launch_voxel_write(a, st));
    return ev ? hipEventRecord(ev[7], st) : hipSuccess;
}
#endif

}  // namespace ouster_hip_dev
