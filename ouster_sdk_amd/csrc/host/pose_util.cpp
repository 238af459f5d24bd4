// pose_util.cpp -- the host half of core::interp_pose: what is computed once per pair of known poses, and the validation.
//   reference: ouster_core/include/ouster/core/pose_util.h:194-286 (interp_pose_range, interp_pose), src/transform_homogeneous.cpp:31-62
//   (RotH::log, PoseH::log), src/transform_vector.cpp:52-60 (RotV::vee), impl/transform_typedefs.h:16-17 (EPS).  a.inverse() and
//   vee(...).inverse() there are Eigen's general inverses of the full 4x4 and 3x3: cofactors here.
// Plain C++ without HIP, part of libouster_hip.so; built with -ffp-contract=off so that every step rounds on its own, like
// tests/pose_model.py (whose float64 form this file follows operation for operation) and like the kernel (csrc/k_pose.hip).
#include <cfloat>
#include <cmath>
#include <cstdio>

#include "../../../include/ouster_hip.h"
#include "../pose_host.h"

namespace ouster_hip_dev {
namespace {

constexpr double EPS = DBL_EPSILON;

// full n x n product, every sum left to right
template <int N>
void matmul(const double (&a)[N][N], const double (&b)[N][N], double (&r)[N][N]) {
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) {
            double s = a[i][0] * b[0][j];
            for (int k = 1; k < N; ++k) s = s + a[i][k] * b[k][j];
            r[i][j] = s;
        }
}

double det3(const double (&m)[4][4], const int (&r)[3], const int (&c)[3]) {
    return m[r[0]][c[0]] * (m[r[1]][c[1]] * m[r[2]][c[2]] - m[r[1]][c[2]] * m[r[2]][c[1]]) -
           m[r[0]][c[1]] * (m[r[1]][c[0]] * m[r[2]][c[2]] - m[r[1]][c[2]] * m[r[2]][c[0]]) +
           m[r[0]][c[2]] * (m[r[1]][c[0]] * m[r[2]][c[1]] - m[r[1]][c[1]] * m[r[2]][c[0]]);
}

void others(int skip, int n, int* out) {
    for (int x = 0, o = 0; x < n; ++x)
        if (x != skip) out[o++] = x;
}

void inv4(const double (&m)[4][4], double (&out)[4][4]) {
    double cof[4][4];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            int r[3], c[3];
            others(i, 4, r);
            others(j, 4, c);
            const double minor = det3(m, r, c);
            cof[i][j] = (i + j) % 2 == 0 ? minor : -minor;
        }
    const double det = ((m[0][0] * cof[0][0] + m[0][1] * cof[0][1]) + m[0][2] * cof[0][2]) + m[0][3] * cof[0][3];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) out[i][j] = cof[j][i] / det;
}

void inv3(const double (&m)[3][3], double (&out)[3][3]) {
    double cof[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            int r[2], c[2];
            others(i, 3, r);
            others(j, 3, c);
            const double minor = m[r[0]][c[0]] * m[r[1]][c[1]] - m[r[0]][c[1]] * m[r[1]][c[0]];
            cof[i][j] = (i + j) % 2 == 0 ? minor : -minor;
        }
    const double det = (m[0][0] * cof[0][0] + m[0][1] * cof[0][1]) + m[0][2] * cof[0][2];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) out[i][j] = cof[j][i] / det;
}

void skew(const double (&v)[3], double (&a)[3][3]) {
    a[0][0] = 0, a[0][1] = -v[2], a[0][2] = v[1];
    a[1][0] = v[2], a[1][1] = 0, a[1][2] = -v[0];
    a[2][0] = -v[1], a[2][1] = v[0], a[2][2] = 0;
}

// RotV::vee: I + (1 - cos) A / angle + (angle - sin) A A / angle, identity below EPS
void vee(const double (&r)[3], double angle, double sin_angle, double cos_angle, double (&out)[3][3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) out[i][j] = i == j ? 1.0 : 0.0;
    if (angle < EPS) return;
    const double ax[3] = {r[0] / angle, r[1] / angle, r[2] / angle};
    double a[3][3], k2a[3][3], t2[3][3];
    skew(ax, a);
    const double k1 = 1.0 - cos_angle, k2 = angle - sin_angle;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) k2a[i][j] = k2 * a[i][j];
    matmul<3>(k2a, a, t2);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) out[i][j] = (out[i][j] + (k1 * a[i][j]) / angle) + t2[i][j] / angle;
}

// PoseH::log: rotation (with the reference's clamps and its two branches) then translation
void pose_log(const double (&m)[4][4], double (&twist)[6]) {
    double c = 0.5 * (((m[0][0] + m[1][1]) + m[2][2]) - 1.0);
    c = std::fmax(c, -1.0 + EPS);
    c = std::fmin(c, 1.0 - EPS);
    const double angle = std::acos(c);
    double v[3] = {m[2][1] - m[1][2], m[0][2] - m[2][0], m[1][0] - m[0][1]};
    const double sq = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    if (sq > EPS) {
        const double n = std::sqrt(sq);
        for (double& x : v) x = (x / n) * angle;
    } else {
        for (double& x : v) x = x / 2.0;
    }
    const double s = std::sin(angle);
    double vm[3][3], vi[3][3];
    vee(v, angle, s, c, vm);
    inv3(vm, vi);
    for (int i = 0; i < 3; ++i) {
        twist[i] = v[i];
        twist[3 + i] = (vi[i][0] * m[0][3] + vi[i][1] * m[1][3]) + vi[i][2] * m[2][3];
    }
}

}  // namespace

// PoseV::exp (transform_vector.cpp:40-50, 96-104), as tests/pose_model.py pose_exp: the ICP step of host/icp_util.cpp
void pose_exp(const double* twist6, double* out16) {
    const double r[3] = {twist6[0], twist6[1], twist6[2]};
    const double angle = std::sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    const double s = std::sin(angle), c = std::cos(angle);
    double a[3][3], rot[3][3], vm[3][3];
    if (angle < std::sqrt(EPS)) {
        skew(r, a);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) rot[i][j] = (i == j ? 1.0 : 0.0) + a[i][j];
    } else {
        const double ax[3] = {r[0] / angle, r[1] / angle, r[2] / angle};
        double ka[3][3], aa[3][3];
        skew(ax, a);
        const double k = 1.0 - c;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) ka[i][j] = k * a[i][j];
        matmul<3>(ka, a, aa);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) rot[i][j] = ((i == j ? 1.0 : 0.0) + s * a[i][j]) + aa[i][j];
    }
    vee(r, angle, s, c, vm);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) out16[4 * i + j] = rot[i][j];
        out16[4 * i + 3] = (vm[i][0] * twist6[3] + vm[i][1] * twist6[4]) + vm[i][2] * twist6[5];
    }
    out16[12] = out16[13] = out16[14] = 0.0;
    out16[15] = 1.0;
}

void pose_compose(const double* a16, const double* b16, double* out16) {
    double a[4][4], b[4][4], r[4][4];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) a[i][j] = a16[4 * i + j], b[i][j] = b16[4 * i + j];
    matmul<4>(a, b, r);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) out16[4 * i + j] = r[i][j];
}

const char* pose_validate_known(const double* x_known, const double* poses_known, uint32_t k) {
    if (k < 2) return "Not enough evaluation poses for interpolation";
    if (!x_known || !poses_known) return "x_known and poses_known sizes are not matching";
    for (uint32_t i = 0; i + 1 < k; ++i)
        if (!(x_known[i] < x_known[i + 1])) return "input x_known values are not monotonically increasing or values repeated";
    return nullptr;
}

const char* pose_validate_pair(double t0, double t1) {
    return std::fabs(t1 - t0) < DBL_EPSILON ? "Cannot interpolate with zero duration between poses" : nullptr;
}

const char* pose_validate_interp(const double* x, size_t n, char* msg, size_t msg_size) {
    for (size_t i = 1; i < n; ++i)
        if (x[i] < x[i - 1]) {
            std::snprintf(msg, msg_size, "x_interp values must be monotonically increasing: %f < %f", x[i], x[i - 1]);
            return msg;
        }
    return nullptr;
}

void pose_segment(double t0, const double* a16, double t1, const double* b16, double* seg) {
    double a[4][4], b[4][4], ai[4][4], rel[4][4], twist[6];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) a[i][j] = a16[4 * i + j], b[i][j] = b16[4 * i + j];
    inv4(a, ai);
    matmul<4>(ai, b, rel);
    pose_log(rel, twist);
    const double f = 1.0 / (t1 - t0);
    seg[0] = t0;
    for (int i = 0; i < 16; ++i) seg[1 + i] = a16[i];
    for (int i = 0; i < 6; ++i) seg[17 + i] = f * twist[i];
    seg[23] = 0.0;
}

}  // namespace ouster_hip_dev

extern "C" int ouster_hip_pose_segments(const double* x_known, const double* poses_known, uint32_t k, double* segments) {
    using namespace ouster_hip_dev;
    if (const char* msg = pose_validate_known(x_known, poses_known, k)) return fail_msg(OUSTER_HIP_ERR_INVALID_ARGUMENT, msg);
    if (!segments) return fail_msg(OUSTER_HIP_ERR_INVALID_ARGUMENT, "segments is NULL");
    for (uint32_t i = 0; i + 1 < k; ++i)
        pose_segment(x_known[i], poses_known + 16 * (size_t)i, x_known[i + 1], poses_known + 16 * (size_t)(i + 1),
                     segments + (size_t)POSE_SEG_DOUBLES * i);
    return OUSTER_HIP_OK;
}
