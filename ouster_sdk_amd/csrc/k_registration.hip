// k_registration.hip -- one pass of ICPRegistration (mapping::ICPRegistration::align_points_to_map, icp_registration.cpp:32-93,
// 101-182) against the resident voxel map, held to tests/registration_model.py.  Built with -ffp-contract=off: every multiply, add,
// subtract and divide below is one IEEE double operation in the model's order.  No floating-point atomic anywhere.
//
// k_reg_pass   a workgroup of ICP_WG threads owns ICP_CHUNK consecutive rows, thread t the rows base + t + 256 k, k = 0..3, in that
//              order.  Per row: load (pass 0: the caller's row, widened; later: the moved row of the workspace with the previous
//              pass's estimate applied: model apply()), write the moved row back, ask the map (vmap_closest_point, the body of
//              k_vmap_closest), form the flag, the Geman-McClure weight and the 16 terms (model terms()).  A row without a
//              correspondence adds +0.0 and counts 0.  The correspondences stay in registers.  Then the tree of k_icp.hip: the
//              thread's rows in order, block_sums (wave butterfly, lane 0 to LDS, one thread per sum folds the waves in order):
//              one partial per sum and chunk; the count goes the same way as an integer.
// k_reg_fold   one workgroup: sum s of the header is the left fold of the chunks' partials in index order; the count likewise.
// (fold_partials of k_icp.hip writes an IcpHeader with that call's stride and centroids; the fold here is the same loop over this
// pass's header.)
#include <hip/hip_runtime.h>

#include "icp_sums_dev.h"
#include "k_registration.h"
#include "voxel_dev.h"
#include "voxel_map_dev.h"

namespace ouster_hip_dev {
namespace {

// model cross(): a_y b_z - a_z b_y, ...
__device__ __forceinline__ void reg_cross(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// model apply(): (v + w uv) + q x uv with uv = 2 (q x v), then + t
__device__ __forceinline__ void reg_apply_row(const RegPassArgs& a, double (&s)[3]) {
    const double qv[3] = {a.q[0], a.q[1], a.q[2]};
    double uv[3], c[3];
    reg_cross(qv, s, uv);
    uv[0] = uv[0] + uv[0], uv[1] = uv[1] + uv[1], uv[2] = uv[2] + uv[2];
    reg_cross(qv, uv, c);
#pragma unroll
    for (int d = 0; d < 3; ++d) s[d] = ((s[d] + a.q[3] * uv[d]) + c[d]) + a.t[d];
}

// model terms(): the 16 entries of SUMS for source s and target q
__device__ __forceinline__ void reg_terms_row(const double (&s)[3], double qx, double qy, double qz, double k, double (&t)[REG_NS]) {
    const double sx = s[0], sy = s[1], sz = s[2];
    const double rx = sx - qx, ry = sy - qy, rz = sz - qz;
    const double r2 = (rx * rx + ry * ry) + rz * rz;
    const double w = (k * k) / ((k + r2) * (k + r2));
    const double wsx = w * sx, wsy = w * sy, wsz = w * sz;
    const double wsx2 = wsx * sx, wsy2 = wsy * sy, wsz2 = wsz * sz;
    const double cx = sy * rz - sz * ry, cy = sz * rx - sx * rz, cz = sx * ry - sy * rx;
    t[0] = w, t[1] = wsx, t[2] = wsy, t[3] = wsz;
    t[4] = wsy2 + wsz2, t[5] = wsx * sy, t[6] = wsx2 + wsz2, t[7] = wsx * sz, t[8] = wsy * sz, t[9] = wsx2 + wsy2;
    t[10] = w * rx, t[11] = w * ry, t[12] = w * rz;
    t[13] = w * cx, t[14] = w * cy, t[15] = w * cz;
}

// what thread `thread` of workgroup `block` does before the tree: its rows base + thread + 256 k, k = 0..3, in that order, folded into
// acc and count.  (Outside the device-only part: tests/cpp/registration_lanes.cpp runs it on the CPU, one thread per lane.)
template <class T>
__device__ __forceinline__ void reg_thread_rows(const VMapDev& m, const RegPassArgs& a, uint32_t block, uint32_t thread, double (&acc)[REG_NS],
                                                uint32_t& count) {
#pragma unroll
    for (int s = 0; s < REG_NS; ++s) acc[s] = 0.0;
    count = 0;
    const uint64_t base = (uint64_t)block * ICP_CHUNK;
    for (uint32_t k = 0; k < ICP_ROWS_PER_THREAD; ++k) {
        const uint64_t i = base + thread + (uint64_t)ICP_WG * k;
        if (i >= a.n) continue;
        const T* src = static_cast<const T*>(a.src) + i * a.stride;
        double s[3] = {(double)src[0], (double)src[1], (double)src[2]};
        if (a.apply) reg_apply_row(a, s);
        double* mv = a.moved + 3 * i;
        mv[0] = s[0], mv[1] = s[1], mv[2] = s[2];
        double bx, by, bz, best;
        vmap_closest_point(m, s, a.max_d2, bx, by, bz, best);
        const bool flag = best < a.max_d2;
        if (a.flags) {
            a.flags[i] = flag;
            double* nb = a.neighbours + 3 * i;
            nb[0] = bx, nb[1] = by, nb[2] = bz;
            a.dist_sq[i] = best;
        }
        double t[REG_NS];
        reg_terms_row(s, bx, by, bz, a.k, t);
#pragma unroll
        for (int c = 0; c < REG_NS; ++c) t[c] = flag ? t[c] : 0.0;
        if (a.terms)
#pragma unroll
            for (int c = 0; c < REG_NS; ++c) a.terms[i * REG_NS + c] = t[c];
#pragma unroll
        for (int c = 0; c < REG_NS; ++c) acc[c] = acc[c] + t[c];
        count += flag;
    }
}

// sum `t` of the header is the left fold of the chunks' partials in index order (the loop of k_icp.hip's fold_partials, over
// this pass's header); the count likewise
__device__ __forceinline__ void reg_fold_chunks(const RegPassArgs& a, uint32_t chunks, uint32_t thread) {
    if (thread < REG_NS) {
        double v = 0.0;
        for (uint32_t c = 0; c < chunks; ++c) v = v + a.partials[(uint64_t)c * REG_NS + thread];
        a.hdr->sums[thread] = v;
    } else if (thread == REG_NS) {
        uint64_t v = 0;
        for (uint32_t c = 0; c < chunks; ++c) v = v + a.counts[c];
        a.hdr->count = v;
    }
}

#ifdef __HIPCC__
// the count through the same tree, as an integer: wave butterfly, lane 0 to LDS, one thread folds the waves in order
__device__ __forceinline__ void block_count(uint32_t c, uint32_t* out) {
    __shared__ uint32_t lds[ICP_WG / 64];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c = c + __shfl_xor(c, off, 64);
    const uint32_t wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    if (lane == 0) lds[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t v = lds[0];
        for (uint32_t w = 1; w < ICP_WG / 64; ++w) v = v + lds[w];
        *out = v;
    }
}

template <class T>
__global__ void __launch_bounds__(ICP_WG) k_reg_pass(VMapDev m, RegPassArgs a) {
    double acc[REG_NS];
    uint32_t count;
    reg_thread_rows<T>(m, a, blockIdx.x, threadIdx.x, acc, count);
    block_sums<REG_NS>(acc, a.partials + (uint64_t)blockIdx.x * REG_NS);
    block_count(count, a.counts + blockIdx.x);
}

// one workgroup
__global__ void __launch_bounds__(64) k_reg_fold(RegPassArgs a, uint32_t chunks) { reg_fold_chunks(a, chunks, threadIdx.x); }
#endif

}  // namespace

#ifdef __HIPCC__
hipError_t reg_pass_run(const VMapDev& m, const RegPassArgs& a, bool from_f32, hipStream_t st) {
    if (a.n == 0 || !a.src || !a.moved || !a.partials || !a.counts || !a.hdr || a.stride < 3) return hipErrorInvalidValue;
    if (a.flags && (!a.neighbours || !a.dist_sq)) return hipErrorInvalidValue;
    const uint32_t chunks = reg_chunks(a.n);
    if (from_f32) hipLaunchKernelGGL(k_reg_pass<float>, dim3(chunks), dim3(ICP_WG), 0, st, m, a);
    else hipLaunchKernelGGL(k_reg_pass<double>, dim3(chunks), dim3(ICP_WG), 0, st, m, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_reg_fold, dim3(1), dim3(64), 0, st, a, chunks);
    return hipGetLastError();
}
#endif

}  // namespace ouster_hip_dev
