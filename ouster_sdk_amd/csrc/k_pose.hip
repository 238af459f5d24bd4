// k_pose.hip -- core::interp_pose per x and core::transform per point, for gfx950.
//   reference: ouster_core/include/ouster/core/pose_util.h:118-131 (transform), :206-235 (interp_pose_range),
//   src/transform_vector.cpp:40-60, 96-104 (RotV::exp, vee, PoseV::exp), impl/transform_typedefs.h:16-17 (EPS, NUMERIC_EPS).
// What is computed once per pair of known poses -- log(inv(a) b) / (t1 - t0) -- comes from the host as a table
// (csrc/host/pose_util.cpp); a thread finds its x's segment, min(k - 2, #{j >= 1 : x_known[j] <= x}), by binary search, takes
// exp((x - t0) * scaled_twist) and multiplies it onto a.  Built with -ffp-contract=off: every step rounds on its own, in the
// order of tests/pose_model.py, so sin / cos are the only operations that can differ from the model's float64 form.
#include "k_pose.h"

namespace ouster_hip_dev {
namespace {

constexpr double EPS = 2.220446049250313e-16;          // std::numeric_limits<double>::epsilon()
constexpr double NUMERIC_EPS = 1.4901161193847656e-08;  // its square root, 2^-26

__device__ __forceinline__ void mul3(const double (&a)[3][3], const double (&b)[3][3], double (&r)[3][3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) r[i][j] = (a[i][0] * b[0][j] + a[i][1] * b[1][j]) + a[i][2] * b[2][j];
}

__device__ __forceinline__ void skew(double x, double y, double z, double (&a)[3][3]) {
    a[0][0] = 0.0, a[0][1] = -z, a[0][2] = y;
    a[1][0] = z, a[1][1] = 0.0, a[1][2] = -x;
    a[2][0] = -y, a[2][1] = x, a[2][2] = 0.0;
}

// a @ exp((x - t0) * scaled_twist) of one table row, 16 values row-major
__device__ __forceinline__ void pose_eval(const double* __restrict__ seg, double x, double (&out)[16]) {
    const double d = x - seg[0];
    const double r0 = d * seg[17], r1 = d * seg[18], r2 = d * seg[19];
    const double t0 = d * seg[20], t1 = d * seg[21], t2 = d * seg[22];
    const double angle = sqrt((r0 * r0 + r1 * r1) + r2 * r2);
    const double s = sin(angle), c = cos(angle);
    double h[4][4];   // exp(delta): rotation, V t, bottom row 0 0 0 1
    double a[3][3];
    if (angle < NUMERIC_EPS) {
        skew(r0, r1, r2, a);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) h[i][j] = (i == j ? 1.0 : 0.0) + a[i][j];
    } else {
        skew(r0 / angle, r1 / angle, r2 / angle, a);
        const double k = 1.0 - c;
        double ka[3][3], aa[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) ka[i][j] = k * a[i][j];
        mul3(ka, a, aa);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) h[i][j] = ((i == j ? 1.0 : 0.0) + s * a[i][j]) + aa[i][j];
    }
    double v[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    if (!(angle < EPS)) {
        skew(r0 / angle, r1 / angle, r2 / angle, a);
        const double k1 = 1.0 - c, k2 = angle - s;
        double k2a[3][3], p2[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) k2a[i][j] = k2 * a[i][j];
        mul3(k2a, a, p2);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) v[i][j] = (v[i][j] + (k1 * a[i][j]) / angle) + p2[i][j] / angle;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        h[i][3] = (v[i][0] * t0 + v[i][1] * t1) + v[i][2] * t2;
        h[3][i] = 0.0;
    }
    h[3][3] = 1.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            out[4 * i + j] = ((seg[1 + 4 * i] * h[0][j] + seg[2 + 4 * i] * h[1][j]) + seg[3 + 4 * i] * h[2][j]) + seg[4 + 4 * i] * h[3][j];
}

// The time of thread i and whether it has work: false past the end and, in the column form, for a column whose status bit 0 is clear
template <bool COLUMNS>
__device__ __forceinline__ bool pose_time(const PoseInterpArgs& a, uint64_t i, double& x) {
    if (i >= a.n) return false;
    if (COLUMNS) {
        if ((a.status[i] & 1u) == 0u) return false;
        x = (double)a.timestamp[i] * 1e-9;
    } else {
        x = a.x[i];
    }
    return true;
}

// #{j >= 1 : x_known[j] <= x} by binary search -- the first j in [1, k) whose time is above x, minus one -- capped at k - 2
__device__ __forceinline__ void pose_of(const PoseInterpArgs& a, double x, double (&m)[16]) {
    uint32_t lo = 1, hi = a.k;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.x_known[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    const uint32_t segment = min(a.k - 2, lo - 1);
    pose_eval(a.segments + (size_t)segment * POSE_SEG_DOUBLES, x, m);
}

// The direct form (knob "pose_direct", kept for A/B): one thread per x, every lane stores its own row -- 128 B in double, 64 B
// in float, 48 B of pose_rows -- 16 B per store instruction, so one instruction of a wave touches 64 separate lines.
template <bool COLUMNS>
__global__ __launch_bounds__(256) void k_pose_interp_direct(PoseInterpArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    double x;
    if (!pose_time<COLUMNS>(a, i, x)) return;
    double m[16];
    pose_of(a, x, m);
    if (a.dtype == OUSTER_HIP_F64) {
        double2* o = reinterpret_cast<double2*>(static_cast<double*>(a.out) + i * 16);
#pragma unroll
        for (int q = 0; q < 8; ++q) o[q] = make_double2(m[2 * q], m[2 * q + 1]);
    } else {
        float4* o = reinterpret_cast<float4*>(static_cast<float*>(a.out) + i * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = make_float4((float)m[4 * q], (float)m[4 * q + 1], (float)m[4 * q + 2], (float)m[4 * q + 3]);
    }
    if (COLUMNS && a.pose_rows) {
        float4* o = reinterpret_cast<float4*>(a.pose_rows + i * 12);
#pragma unroll
        for (int q = 0; q < 3; ++q) o[q] = make_float4((float)m[4 * q], (float)m[4 * q + 1], (float)m[4 * q + 2], (float)m[4 * q + 3]);
    }
}

// The default form.  One thread per x computes its row; the 256 rows of a workgroup are staged in LDS (rows 18 doubles apart:
// 16-byte aligned, and a wave's row writes spread over the banks) and go out lane-linear: store instruction q of lane t writes
// the 16 bytes at (q * 256 + t) * 16 of the workgroup's 32 KB (double), 16 KB (float) or 12 KB (pose_rows) of output, so a
// wave writes 1 KB of consecutive memory per instruction.  A 16-byte piece lies inside one row (128, 64 and 48 are multiples
// of 16); a row without work -- past n, or a column whose status bit 0 is clear -- has its flag clear and none of its pieces
// is stored: those bytes stay as they are.
constexpr int POSE_LDS_ROW = 18;

template <bool COLUMNS>
__global__ __launch_bounds__(256) void k_pose_interp(PoseInterpArgs a) {
    __shared__ double s_m[256 * POSE_LDS_ROW];
    __shared__ uint32_t s_live[256];
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * 256;
    double x;
    const bool live = pose_time<COLUMNS>(a, base + t, x);
    s_live[t] = live ? 1u : 0u;
    if (live) {
        double m[16];
        pose_of(a, x, m);
        double2* row = reinterpret_cast<double2*>(s_m + t * POSE_LDS_ROW);
#pragma unroll
        for (int q = 0; q < 8; ++q) row[q] = make_double2(m[2 * q], m[2 * q + 1]);
    }
    __syncthreads();
    if (a.dtype == OUSTER_HIP_F64) {
        double2* o = reinterpret_cast<double2*>(static_cast<double*>(a.out) + base * 16);
#pragma unroll
        for (uint32_t q = 0; q < 8; ++q) {
            const uint32_t piece = q * 256 + t, r = piece >> 3, c = (piece & 7u) * 2;   // 8 pieces of 2 doubles per row
            if (s_live[r]) o[piece] = *reinterpret_cast<const double2*>(s_m + r * POSE_LDS_ROW + c);
        }
    } else {
        float4* o = reinterpret_cast<float4*>(static_cast<float*>(a.out) + base * 16);
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            const uint32_t piece = q * 256 + t, r = piece >> 2, c = (piece & 3u) * 4;   // 4 pieces of 4 floats per row
            const double* v = s_m + r * POSE_LDS_ROW + c;
            if (s_live[r]) o[piece] = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
        }
    }
    if (COLUMNS && a.pose_rows) {
        float4* o = reinterpret_cast<float4*>(a.pose_rows + base * 12);
#pragma unroll
        for (uint32_t q = 0; q < 3; ++q) {
            const uint32_t piece = q * 256 + t, r = piece / 3, c = (piece - r * 3) * 4;   // 3 pieces of 4 floats per row
            const double* v = s_m + r * POSE_LDS_ROW + c;
            if (s_live[r]) o[piece] = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
        }
    }
}

// rotation * p + translation in T, row by row: the expression of the dense dewarp (k_dewarp.hip, k_dewarp), here without
// contraction, which is how the reference's host loop is compiled
template <class T>
__global__ __launch_bounds__(256) void k_pose_transform(PoseTransformArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const double* m = a.pose;
    const T* p = static_cast<const T*>(a.points) + i * 3;
    const T x = p[0], y = p[1], z = p[2];
    T* o = static_cast<T*>(a.out) + i * 3;
    o[0] = (T)m[0] * x + (T)m[1] * y + (T)m[2] * z + (T)m[3];
    o[1] = (T)m[4] * x + (T)m[5] * y + (T)m[6] * z + (T)m[7];
    o[2] = (T)m[8] * x + (T)m[9] * y + (T)m[10] * z + (T)m[11];
}

}  // namespace

hipError_t launch_pose_interp(const PoseInterpArgs& a, hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    const uint64_t blocks = (a.n + 255) / 256;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)blocks), wg(256);
    if (a.direct_stores) {
        if (a.x) hipLaunchKernelGGL(k_pose_interp_direct<false>, grid, wg, 0, st, a);
        else hipLaunchKernelGGL(k_pose_interp_direct<true>, grid, wg, 0, st, a);
    } else {
        if (a.x) hipLaunchKernelGGL(k_pose_interp<false>, grid, wg, 0, st, a);
        else hipLaunchKernelGGL(k_pose_interp<true>, grid, wg, 0, st, a);
    }
    return hipGetLastError();
}

hipError_t launch_pose_transform(const PoseTransformArgs& a, hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    const uint64_t blocks = (a.n + 255) / 256;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    if (a.dtype == OUSTER_HIP_F32) hipLaunchKernelGGL(k_pose_transform<float>, dim3((uint32_t)blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_pose_transform<double>, dim3((uint32_t)blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace ouster_hip_dev
