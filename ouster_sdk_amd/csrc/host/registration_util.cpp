// registration_util.cpp -- the host half of ICPRegistration (csrc/registration_host.h), operation for operation
// tests/registration_model.py.  Built with -ffp-contract=off: every multiply, add, subtract, divide and sqrt is one IEEE double
// operation in the model's order.  Plain C++, no HIP.
#include "../registration_host.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace ouster_hip_dev {

namespace {

constexpr double REG_EPS = 1e-10;   // Sophus::Constants<double>::epsilon()

inline void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// the unit quaternion's rotation of a vector: (v + w uv) + q x uv with uv = 2 (q x v)
inline void rotate(const double* q, const double* v, double* out) {
    double uv[3], c[3];
    cross3(q, v, uv);
    uv[0] = uv[0] + uv[0], uv[1] = uv[1] + uv[1], uv[2] = uv[2] + uv[2];
    cross3(q, uv, c);
    const double r0 = (v[0] + q[3] * uv[0]) + c[0], r1 = (v[1] + q[3] * uv[1]) + c[1], r2 = (v[2] + q[3] * uv[2]) + c[2];
    out[0] = r0, out[1] = r1, out[2] = r2;
}

bool bad(double v) { return !std::isfinite(v) || v < 0.0; }

}  // namespace

const char* reg_validate(const void* map, const void* points, int32_t dtype, uint64_t n, uint64_t row_stride, double max_distance,
                         double kernel_scale, double convergence, bool* unsupported) {
    *unsupported = false;
    if (!map) return "map is NULL";
    if (dtype != OUSTER_HIP_F32 && dtype != OUSTER_HIP_F64) return "dtype must be F32 or F64";
    if (row_stride && row_stride < 3) return "row_stride is smaller than 3";
    if (n && !points) return "NULL pointer";
    if (n > REG_MAX_ROWS) {
        *unsupported = true;
        return "registration: more than 2^30 rows";
    }
    if (bad(max_distance)) return "registration: max_distance must be finite and not negative";
    if (bad(kernel_scale)) return "registration: kernel_scale must be finite and not negative";
    if (bad(convergence)) return "registration: convergence_criterion must be finite and not negative";
    return nullptr;
}

void reg_terms(const double* s, const double* q, double kernel_scale, double* t) {
    const double sx = s[0], sy = s[1], sz = s[2];
    const double rx = sx - q[0], ry = sy - q[1], rz = sz - q[2];
    const double r2 = (rx * rx + ry * ry) + rz * rz;
    const double k = kernel_scale;
    const double w = (k * k) / ((k + r2) * (k + r2));
    const double wsx = w * sx, wsy = w * sy, wsz = w * sz;
    const double wsx2 = wsx * sx, wsy2 = wsy * sy, wsz2 = wsz * sz;
    const double cx = sy * rz - sz * ry, cy = sz * rx - sx * rz, cz = sx * ry - sy * rx;
    t[0] = w, t[1] = wsx, t[2] = wsy, t[3] = wsz;
    t[4] = wsy2 + wsz2, t[5] = wsx * sy, t[6] = wsx2 + wsz2, t[7] = wsx * sz, t[8] = wsy * sz, t[9] = wsx2 + wsy2;
    t[10] = w * rx, t[11] = w * ry, t[12] = w * rz;
    t[13] = w * cx, t[14] = w * cy, t[15] = w * cz;
}

void reg_system(const double* s, double* jtj, double* jtr) {
    for (int i = 0; i < 36; ++i) jtj[i] = 0.0;
    jtj[0] = jtj[7] = jtj[14] = s[0];
    jtj[3 * 6 + 1] = -s[3], jtj[3 * 6 + 2] = s[2];
    jtj[4 * 6 + 0] = s[3], jtj[4 * 6 + 2] = -s[1];
    jtj[5 * 6 + 0] = -s[2], jtj[5 * 6 + 1] = s[1];
    jtj[3 * 6 + 3] = s[4];
    jtj[4 * 6 + 3] = -s[5], jtj[4 * 6 + 4] = s[6];
    jtj[5 * 6 + 3] = -s[7], jtj[5 * 6 + 4] = -s[8], jtj[5 * 6 + 5] = s[9];
    for (int i = 0; i < 6; ++i) jtr[i] = s[10 + i];
}

void reg_solve6(const double* jtj, const double* jtr, double* x) {
    constexpr int n = 6;
    double L[n][n] = {}, d[n] = {}, y[n] = {};
    for (int j = 0; j < n; ++j) {
        double v = jtj[j * n + j];
        for (int k = 0; k < j; ++k) v = v - (L[j][k] * L[j][k]) * d[k];
        d[j] = v;
        for (int i = j + 1; i < n; ++i) {
            double a = jtj[i * n + j];
            for (int k = 0; k < j; ++k) a = a - (L[i][k] * L[j][k]) * d[k];
            L[i][j] = v != 0.0 ? a / v : 0.0;
        }
    }
    for (int i = 0; i < n; ++i) {
        double a = -jtr[i];
        for (int k = 0; k < i; ++k) a = a - L[i][k] * y[k];
        y[i] = a;
    }
    for (int i = 0; i < n; ++i) y[i] = d[i] != 0.0 ? y[i] / d[i] : 0.0;
    for (int i = n - 1; i >= 0; --i) {
        double a = y[i];
        for (int k = i + 1; k < n; ++k) a = a - L[k][i] * x[k];
        x[i] = a;
    }
}

RegPose reg_exp(const double* dx) {
    const double* u = dx;
    const double* o = dx + 3;
    const double theta_sq = (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2];
    double imag, real, a, b;
    if (theta_sq < REG_EPS * REG_EPS) {
        const double theta_po4 = theta_sq * theta_sq;
        imag = (0.5 - (1.0 / 48.0) * theta_sq) + (1.0 / 3840.0) * theta_po4;
        real = (1.0 - (1.0 / 8.0) * theta_sq) + (1.0 / 384.0) * theta_po4;
        a = 0.5, b = 0.0;
    } else {
        const double theta = std::sqrt(theta_sq);
        const double half = 0.5 * theta;
        imag = std::sin(half) / theta;
        real = std::cos(half);
        a = (1.0 - std::cos(theta)) / theta_sq;
        b = (theta - std::sin(theta)) / (theta_sq * theta);
    }
    RegPose p;
    p.v[0] = imag * o[0], p.v[1] = imag * o[1], p.v[2] = imag * o[2], p.v[3] = real;
    double c1[3], c2[3];
    cross3(o, u, c1);
    cross3(o, c1, c2);
    for (int k = 0; k < 3; ++k) p.v[4 + k] = (u[k] + a * c1[k]) + b * c2[k];
    return p;
}

void reg_apply(const RegPose& p, const double* in, double* out) {
    double r[3];
    rotate(p.v, in, r);
    out[0] = r[0] + p.v[4], out[1] = r[1] + p.v[5], out[2] = r[2] + p.v[6];
}

RegPose reg_compose(const RegPose& A, const RegPose& B) {
    const double ax = A.v[0], ay = A.v[1], az = A.v[2], aw = A.v[3];
    const double bx = B.v[0], by = B.v[1], bz = B.v[2], bw = B.v[3];
    const double w = ((aw * bw - ax * bx) - ay * by) - az * bz;
    const double x = ((aw * bx + ax * bw) + ay * bz) - az * by;
    const double y = ((aw * by + ay * bw) + az * bx) - ax * bz;
    const double z = ((aw * bz + az * bw) + ax * by) - ay * bx;
    const double n = std::sqrt(((x * x + y * y) + z * z) + w * w);
    double r[3];
    rotate(A.v, B.v + 4, r);
    RegPose p;
    p.v[0] = x / n, p.v[1] = y / n, p.v[2] = z / n, p.v[3] = w / n;
    p.v[4] = A.v[4] + r[0], p.v[5] = A.v[5] + r[1], p.v[6] = A.v[6] + r[2];
    return p;
}

void reg_matrix(const RegPose& p, double* m) {
    const double x = p.v[0], y = p.v[1], z = p.v[2], w = p.v[3];
    const double tx = x + x, ty = y + y, tz = z + z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    m[0] = 1.0 - (tyy + tzz), m[1] = txy - twz, m[2] = txz + twy, m[3] = p.v[4];
    m[4] = txy + twz, m[5] = 1.0 - (txx + tzz), m[6] = tyz - twx, m[7] = p.v[5];
    m[8] = txz - twy, m[9] = tyz + twx, m[10] = 1.0 - (txx + tyy), m[11] = p.v[6];
    m[12] = 0.0, m[13] = 0.0, m[14] = 0.0, m[15] = 1.0;
}

double reg_squared_norm6(const double* d) {
    return ((((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3]) + d[4] * d[4]) + d[5] * d[5];
}

bool reg_solve_pass(const double* sums, double convergence, double* dx6, RegPose* estimate) {
    double jtj[36], jtr[6];
    reg_system(sums, jtj, jtr);
    reg_solve6(jtj, jtr, dx6);
    *estimate = reg_exp(dx6);
    return reg_squared_norm6(dx6) < convergence * convergence;
}

void reg_pass_ref(const HostVoxelMap& map, double* moved, uint64_t n, const RegPose* estimate, double max_distance, double kernel_scale,
                  uint8_t* flags, double* neighbours, double* dist_sq, double* sums, uint64_t* count) {
    const double bound = max_distance * max_distance;
    for (int k = 0; k < REG_SUMS; ++k) sums[k] = 0.0;
    uint64_t c = 0;
    for (uint64_t i = 0; i < n; ++i) {
        double* s = moved + 3 * i;
        if (estimate) reg_apply(*estimate, s, s);
        double q[3], d2;
        map.closest(s, bound, q, &d2);
        const bool flag = d2 < bound;
        double t[REG_SUMS];
        if (flag) reg_terms(s, q, kernel_scale, t);
        else
            for (int k = 0; k < REG_SUMS; ++k) t[k] = 0.0;
        for (int k = 0; k < REG_SUMS; ++k) sums[k] = sums[k] + t[k];
        c += flag;
        if (flags) flags[i] = flag;
        if (neighbours) neighbours[3 * i] = q[0], neighbours[3 * i + 1] = q[1], neighbours[3 * i + 2] = q[2];
        if (dist_sq) dist_sq[i] = d2;
    }
    *count = c;
}

void reg_identity(ouster_hip_registration_desc* desc) {
    reg_matrix(RegPose{}, desc->pose);
    desc->iterations = 0, desc->converged = 0, desc->correspondences = 0;
}

void reg_align_ref(const HostVoxelMap& map, const void* points, bool f32, uint64_t n, uint64_t stride, ouster_hip_registration_desc* desc) {
    reg_identity(desc);
    if (n == 0 || map.voxels() == 0 || desc->max_iterations <= 0) return;
    std::vector<double> moved(3 * n);
    for (uint64_t i = 0; i < n; ++i)
        for (int c = 0; c < 3; ++c)
            moved[3 * i + c] = f32 ? (double)static_cast<const float*>(points)[i * stride + c] : static_cast<const double*>(points)[i * stride + c];
    RegPose pose, estimate;
    for (int32_t j = 0; j < desc->max_iterations; ++j) {
        double sums[REG_SUMS], dx[6];
        uint64_t count = 0;
        reg_pass_ref(map, moved.data(), n, j ? &estimate : nullptr, desc->max_distance, desc->kernel_scale, nullptr, nullptr, nullptr, sums, &count);
        const bool stop = reg_solve_pass(sums, desc->convergence_criterion, dx, &estimate);
        pose = reg_compose(estimate, pose);
        desc->iterations = (uint32_t)(j + 1), desc->correspondences = count;
        if (stop) {
            desc->converged = 1;
            break;
        }
    }
    reg_matrix(pose, desc->pose);
}

void reg_build_linear_system(const double* sources, const double* targets, uint64_t n, double kernel_scale, double* jtj36, double* jtr6) {
    double sums[REG_SUMS] = {};
    for (uint64_t i = 0; i < n; ++i) {
        double t[REG_SUMS];
        reg_terms(sources + 3 * i, targets + 3 * i, kernel_scale, t);
        for (int k = 0; k < REG_SUMS; ++k) sums[k] = sums[k] + t[k];
    }
    reg_system(sums, jtj36, jtr6);
}

double reg_model_error(const double* d, double max_range) {
    const double m[3][3] = {{d[0], d[1], d[2]}, {d[4], d[5], d[6]}, {d[8], d[9], d[10]}};
    double t = (m[0][0] + m[1][1]) + m[2][2];
    double q[3] = {0.0, 0.0, 0.0}, w;
    if (t > 0.0) {
        t = std::sqrt(t + 1.0);
        w = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[2][1] - m[1][2]) * t, q[1] = (m[0][2] - m[2][0]) * t, q[2] = (m[1][0] - m[0][1]) * t;
    } else {
        int i = 0;
        if (m[1][1] > m[0][0]) i = 1;
        if (m[2][2] > m[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        t = std::sqrt(((m[i][i] - m[j][j]) - m[k][k]) + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        w = (m[k][j] - m[j][k]) * t;
        q[j] = (m[j][i] + m[i][j]) * t;
        q[k] = (m[k][i] + m[i][k]) * t;
    }
    const double n = std::sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
    const double theta = n != 0.0 ? 2.0 * std::atan2(n, std::fabs(w)) : 0.0;
    const double delta_rot = (2.0 * max_range) * std::sin(theta / 2.0);
    const double delta_trans = std::sqrt((d[3] * d[3] + d[7] * d[7]) + d[11] * d[11]);
    return delta_trans + delta_rot;
}

}  // namespace ouster_hip_dev
