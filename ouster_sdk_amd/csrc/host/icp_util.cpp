// icp_util.cpp -- the plain C++ half of point_to_point_align / point_to_plane_align inside libouster_hip.so: what is refused, with
// the reference's messages; the constants of a call; the solve that follows the sums of a pass (Kabsch over a one-sided Jacobi SVD
// with the determinant fix, or a 6x6 L D L^T step and the SE(3) exponential of host/pose_util.cpp) and the stop rules; and
// ouster_hip_icp_align_ref / ouster_hip_icp_step_ref, the whole algorithm on one core with the reference's left-fold sums
// (ouster_algorithm/src/align_clouds.cpp:146-235, 1590-1874, impl/spatial_hash.h).  Built with -ffp-contract=off, an object of its
// own (Makefile): it follows tests/icp_model.py operation for operation and is compared with it bit for bit.
#include <algorithm>
#include <cmath>
#include <cfloat>
#include <cstdio>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "../icp_host.h"
#include "../pose_host.h"

namespace ouster_hip_dev {

const char* icp_validate(const ouster_hip_icp_desc* d) {
    if (!std::isfinite(d->max_corr_dist) || d->max_corr_dist <= 0.0) return "max_corr_dist must be finite and greater than zero";
    if ((d->source_normals != nullptr) != (d->target_normals != nullptr)) return "normals must be given for both clouds or for neither";
    if (d->source_normals) {
        if (!std::isfinite(d->max_normal_angle_deg) || d->max_normal_angle_deg < 0.0 || d->max_normal_angle_deg > 180.0)
            return "max_normal_angle_deg must be finite and in [0, 180]";
        if (d->n_source != d->n_source_normals) return "source_points and source_normals must have the same number of rows";
        if (d->n_target != d->n_target_normals) return "target_points and target_normals must have the same number of rows";
    }
    if (d->dtype != OUSTER_HIP_F32 && d->dtype != OUSTER_HIP_F64) return "dtype must be F32 or F64";
    for (uint64_t s : {d->source_stride, d->target_stride, d->source_normal_stride, d->target_normal_stride})
        if (s && s < 3) return "a row stride is smaller than 3";
    if ((d->n_source && !d->source_points) || (d->n_target && !d->target_points)) return "NULL pointer";
    return nullptr;
}

const char* icp_msg_grid(IcpMethod m) {
    return m == ICP_PLANE ? "point_to_plane_align: target point outside the int32 cell grid"
                          : "point_to_point_align: target point outside the int32 cell grid";
}

const char* icp_target_validate(const ouster_hip_icp_target_desc* d) {
    if (!std::isfinite(d->max_corr_dist) || d->max_corr_dist <= 0.0) return "max_corr_dist must be finite and greater than zero";
    if (d->normals && d->n != d->n_normals) return "target_points and target_normals must have the same number of rows";
    if (d->dtype != OUSTER_HIP_F32 && d->dtype != OUSTER_HIP_F64) return "dtype must be F32 or F64";
    if (d->flags != 0) return "flags must be 0";
    for (uint64_t s : {d->stride, d->normal_stride})
        if (s && s < 3) return "a row stride is smaller than 3";
    if (d->n && !d->points) return "NULL pointer";
    return nullptr;
}

int icp_sources_validate(bool target_has_normals, const ouster_hip_icp_source* sources, uint32_t n_sources, int32_t dtype,
                         double max_normal_angle_deg, char* msg, size_t cap) {
    auto refuse = [&](int code, const char* text) {
        std::snprintf(msg, cap, "%s", text);
        return code;
    };
    if (target_has_normals) {
        if (!std::isfinite(max_normal_angle_deg) || max_normal_angle_deg < 0.0 || max_normal_angle_deg > 180.0)
            return refuse(OUSTER_HIP_ERR_INVALID_ARGUMENT, "max_normal_angle_deg must be finite and in [0, 180]");
        for (uint32_t k = 0; k < n_sources; ++k)
            if (sources[k].normals && sources[k].n != sources[k].n_normals)
                return refuse(OUSTER_HIP_ERR_INVALID_ARGUMENT, "source_points and source_normals must have the same number of rows");
    }
    for (uint32_t k = 0; k < n_sources; ++k)
        if ((sources[k].normals != nullptr) != target_has_normals) {
            std::snprintf(msg, cap, target_has_normals ? "icp_target: source %u has no normals and the target has them"
                                                       : "icp_target: source %u has normals and the target has none", k);
            return OUSTER_HIP_ERR_INVALID_ARGUMENT;
        }
    if (dtype != OUSTER_HIP_F32 && dtype != OUSTER_HIP_F64) return refuse(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dtype must be F32 or F64");
    uint64_t total = 0;
    for (uint32_t k = 0; k < n_sources; ++k) {
        for (uint64_t s : {sources[k].stride, sources[k].normal_stride})
            if (s && s < 3) return refuse(OUSTER_HIP_ERR_INVALID_ARGUMENT, "a row stride is smaller than 3");
        if (sources[k].n && !sources[k].points) return refuse(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    }
    if (n_sources > ICP_MAX_SOURCES) return refuse(OUSTER_HIP_ERR_UNSUPPORTED, "icp_target: more than 65535 sources");
    for (uint32_t k = 0; k < n_sources; ++k) {
        if (sources[k].n > ICP_MAX_ROWS) return refuse(OUSTER_HIP_ERR_UNSUPPORTED, "icp: more than 2^30 rows");
        total += sources[k].n;
    }
    if (total > ICP_MAX_ROWS) return refuse(OUSTER_HIP_ERR_UNSUPPORTED, "icp: more than 2^30 rows");
    return OUSTER_HIP_OK;
}

uint64_t icp_chunk_table(const uint64_t* rows, uint32_t n_sources, IcpChunk* chunks, uint64_t cap, uint64_t* first_row,
                         uint64_t* first_chunk) {
    uint64_t row = 0, at = 0;
    for (uint32_t k = 0; k < n_sources; ++k) {
        if (first_row) first_row[k] = row;
        if (first_chunk) first_chunk[k] = at;
        for (uint64_t first = 0; first < rows[k]; first += ICP_CHUNK_ROWS, ++at)
            if (at < cap) chunks[at] = IcpChunk{k, (uint32_t)first, (uint32_t)std::min<uint64_t>(ICP_CHUNK_ROWS, rows[k] - first)};
        row += rows[k];
    }
    return at;
}

double icp_cos_gate(double max_normal_angle_deg) { return std::cos(max_normal_angle_deg * M_PI / 180.0); }

double icp_huber_delta(double median, double max_corr_dist) {
    double sigma = 1.4826 * median;
    if (!std::isfinite(sigma) || sigma < 1e-4) sigma = std::max(1e-3, 0.25 * max_corr_dist);
    return 1.5 * sigma;
}

namespace {

double norm3(double a, double b, double c) { return std::sqrt((a * a + b * b) + c * c); }
bool finite3(const double* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

void matmul3(const double (&a)[3][3], const double (&b)[3][3], double (&r)[3][3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r[i][j] = (a[i][0] * b[0][j] + a[i][1] * b[1][j]) + a[i][2] * b[2][j];
}

double det3(const double (&m)[3][3]) {
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])) +
           m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}

}  // namespace

bool icp_svd3(const double (&in)[3][3], double (&u)[3][3], double (&sigma)[3], double (&v)[3][3]) {
    double a[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) a[i][j] = in[i][j], v[i][j] = i == j ? 1.0 : 0.0;
    static const int pairs[3][2] = {{0, 1}, {0, 2}, {1, 2}};
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
        for (const auto& pq : pairs) {
            const int p = pq[0], q = pq[1];
            const double alpha = (a[0][p] * a[0][p] + a[1][p] * a[1][p]) + a[2][p] * a[2][p];
            const double beta = (a[0][q] * a[0][q] + a[1][q] * a[1][q]) + a[2][q] * a[2][q];
            const double gamma = (a[0][p] * a[0][q] + a[1][p] * a[1][q]) + a[2][p] * a[2][q];
            if (gamma == 0.0 || !(std::fabs(gamma) > DBL_EPSILON * std::sqrt(alpha * beta))) continue;
            rotated = true;
            const double zeta = (beta - alpha) / (2.0 * gamma);
            const double t = std::copysign(1.0, zeta) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
            const double c = 1.0 / std::sqrt(1.0 + t * t);
            const double s = c * t;
            for (auto* m : {&a, &v})
                for (int i = 0; i < 3; ++i) {
                    const double mp = (*m)[i][p], mq = (*m)[i][q];
                    (*m)[i][p] = c * mp - s * mq;
                    (*m)[i][q] = s * mp + c * mq;
                }
        }
        if (!rotated) break;
    }
    double sg[3];
    for (int k = 0; k < 3; ++k) sg[k] = norm3(a[0][k], a[1][k], a[2][k]);
    if (!finite3(sg)) return false;
    int order[3] = {0, 1, 2};
    std::stable_sort(order, order + 3, [&](int x, int y) { return sg[x] > sg[y]; });
    if (!(sg[order[1]] > 0.0)) return false;
    double as[3][3], vs[3][3];
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) as[i][k] = a[i][order[k]], vs[i][k] = v[i][order[k]];
    for (int k = 0; k < 3; ++k) sigma[k] = sg[order[k]];
    for (int i = 0; i < 3; ++i) {
        u[i][0] = as[i][0] / sigma[0], u[i][1] = as[i][1] / sigma[1];
        for (int k = 0; k < 3; ++k) v[i][k] = vs[i][k];
    }
    u[0][2] = u[1][0] * u[2][1] - u[2][0] * u[1][1];
    u[1][2] = u[2][0] * u[0][1] - u[0][0] * u[2][1];
    u[2][2] = u[0][0] * u[1][1] - u[1][0] * u[0][1];
    if ((u[0][2] * as[0][2] + u[1][2] * as[1][2]) + u[2][2] * as[2][2] < 0.0)   // the side the third column of a lies on
        for (int i = 0; i < 3; ++i) u[i][2] = -u[i][2];
    return true;
}

bool icp_ldlt6(const double (&h)[6][6], const double (&b)[6], double (&x)[6]) {
    constexpr int n = 6;
    double low[n][n] = {}, d[n] = {}, y[n] = {};
    for (int j = 0; j < n; ++j) {
        double s = h[j][j];
        for (int k = 0; k < j; ++k) s = s - (low[j][k] * low[j][k]) * d[k];
        if (!(s > 0.0) || !std::isfinite(s)) return false;
        d[j] = s;
        low[j][j] = 1.0;
        for (int i = j + 1; i < n; ++i) {
            double t = h[i][j];
            for (int k = 0; k < j; ++k) t = t - (low[i][k] * low[j][k]) * d[k];
            low[i][j] = t / d[j];
        }
    }
    for (int i = 0; i < n; ++i) {
        double s = b[i];
        for (int k = 0; k < i; ++k) s = s - low[i][k] * y[k];
        y[i] = s;
    }
    for (int i = n - 1; i >= 0; --i) {
        double s = y[i] / d[i];
        for (int k = i + 1; k < n; ++k) s = s - low[k][i] * x[k];
        x[i] = s;
    }
    for (double v : x)
        if (!std::isfinite(v)) return false;
    return true;
}

void icp_finish_pass(IcpMethod m, uint64_t count, const double* sums, const double* cx, const double* cq, const double* pose16,
                     double* next16, bool* stop) {
    std::memcpy(next16, pose16, 16 * sizeof(double));
    *stop = true;
    if (count < ICP_MIN_POINTS) return;
    double delta[16], d_rot, d_trans;
    if (m == ICP_POINT) {
        if (!std::isfinite(sums[0]) || sums[0] <= 1e-12) return;
        double cov[3][3], u[3][3], sigma[3], v[3][3], ut[3][3], rot[3][3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) cov[i][j] = sums[7 + 3 * i + j];
        if (!icp_svd3(cov, u, sigma, v)) return;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) ut[i][j] = u[j][i];
        matmul3(v, ut, rot);
        if (det3(rot) < 0.0) {
            for (int i = 0; i < 3; ++i) v[i][2] = -v[i][2];
            matmul3(v, ut, rot);
        }
        double t[3];
        for (int i = 0; i < 3; ++i) t[i] = cq[i] - ((rot[i][0] * cx[0] + rot[i][1] * cx[1]) + rot[i][2] * cx[2]);
        for (int i = 0; i < 3; ++i)
            if (!finite3(rot[i])) return;
        if (!finite3(t)) return;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) delta[4 * i + j] = rot[i][j];
            delta[4 * i + 3] = t[i];
        }
        delta[12] = delta[13] = delta[14] = 0.0, delta[15] = 1.0;
        const double trace_term = std::max(-1.0, std::min(0.5 * (((rot[0][0] + rot[1][1]) + rot[2][2]) - 1.0), 1.0));
        d_rot = std::acos(trace_term);
        d_trans = norm3(t[0], t[1], t[2]);
    } else {
        double h[6][6], b[6], dx[6];
        int k = 0;
        for (int a = 0; a < 6; ++a)
            for (int c = a; c < 6; ++c) h[a][c] = h[c][a] = sums[k++];
        for (int a = 0; a < 6; ++a) h[a][a] = h[a][a] + 1e-10, b[a] = sums[21 + a];
        if (!icp_ldlt6(h, b, dx)) return;
        pose_exp(dx, delta);
        d_rot = norm3(dx[0], dx[1], dx[2]);
        d_trans = norm3(dx[3], dx[4], dx[5]);
    }
    pose_compose(delta, pose16, next16);
    *stop = d_rot < 1e-4 && d_trans < 1e-3;
}

namespace {

struct Cell {
    int32_t v[3];
    bool operator==(const Cell& o) const { return v[0] == o.v[0] && v[1] == o.v[1] && v[2] == o.v[2]; }
};
struct CellHash {
    size_t operator()(const Cell& k) const {
        return ((size_t)(uint32_t)k.v[0] * 73856093u) ^ ((size_t)(uint32_t)k.v[1] * 19349669u) ^ ((size_t)(uint32_t)k.v[2] * 83492791u);
    }
};

struct Cloud {
    const void* p;
    uint64_t stride;
    bool f32;
    void load(uint64_t i, double* out) const {
        if (f32) {
            const float* s = static_cast<const float*>(p) + i * stride;
            out[0] = static_cast<double>(s[0]), out[1] = static_cast<double>(s[1]), out[2] = static_cast<double>(s[2]);
        } else {
            std::memcpy(out, static_cast<const double*>(p) + i * stride, 3 * sizeof(double));
        }
    }
};

bool cell_of(const double* p, double inv, int64_t* c) {
    for (int k = 0; k < 3; ++k) {
        const double f = std::floor(p[k] * inv);
        if (!(f >= -2147483648.0 && f <= 2147483647.0)) return false;
        c[k] = static_cast<int64_t>(f);
    }
    return true;
}

struct HostIcp {
    IcpMethod method;
    Cloud src, tgt, src_n, tgt_n;
    uint64_t n_src, n_tgt;
    double max_corr_dist, inv, cos_gate;
    std::unordered_map<Cell, std::vector<uint32_t>, CellHash> grid;

    explicit HostIcp(const ouster_hip_icp_desc* d)
        : method(icp_method(d)), n_src(d->n_source), n_tgt(d->n_target), max_corr_dist(d->max_corr_dist), inv(1.0 / d->max_corr_dist),
          cos_gate(d->source_normals ? icp_cos_gate(d->max_normal_angle_deg) : 0.0) {
        const bool f32 = d->dtype == OUSTER_HIP_F32;
        src = Cloud{d->source_points, d->source_stride ? d->source_stride : 3, f32};
        tgt = Cloud{d->target_points, d->target_stride ? d->target_stride : 3, f32};
        src_n = Cloud{d->source_normals, d->source_normal_stride ? d->source_normal_stride : 3, f32};
        tgt_n = Cloud{d->target_normals, d->target_normal_stride ? d->target_normal_stride : 3, f32};
    }

    // false: a participating target row outside the int32 grid
    bool build() {
        grid.reserve(n_tgt);
        for (uint64_t j = 0; j < n_tgt; ++j) {
            double p[3], m[3];
            tgt.load(j, p);
            if (!finite3(p)) continue;
            if (method == ICP_PLANE) {
                tgt_n.load(j, m);
                if (!finite3(m) || norm3(m[0], m[1], m[2]) <= ICP_NORMAL_EPS) continue;
            }
            int64_t c[3];
            if (!cell_of(p, inv, c)) return false;
            grid[Cell{{(int32_t)c[0], (int32_t)c[1], (int32_t)c[2]}}].push_back((uint32_t)j);
        }
        return true;
    }

    int64_t nearest(const double* q, double max_d2) const {
        int64_t c[3];
        if (!finite3(q) || !cell_of(q, inv, c)) return -1;
        int64_t best = -1;
        double best_d2 = max_d2;
        for (int dx = -1; dx <= 1; ++dx)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dz = -1; dz <= 1; ++dz) {
                    const int64_t x = c[0] + dx, y = c[1] + dy, z = c[2] + dz;
                    if (x < INT32_MIN || x > INT32_MAX || y < INT32_MIN || y > INT32_MAX || z < INT32_MIN || z > INT32_MAX) continue;
                    const auto it = grid.find(Cell{{(int32_t)x, (int32_t)y, (int32_t)z}});
                    if (it == grid.end()) continue;
                    for (uint32_t j : it->second) {
                        double p[3];
                        tgt.load(j, p);
                        const double e0 = p[0] - q[0], e1 = p[1] - q[1], e2 = p[2] - q[2];
                        const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
                        if (d2 < best_d2) best_d2 = d2, best = j;
                    }
                }
        return best;
    }

    // one pass with left-fold sums in source order
    void step(const double* pose, ouster_hip_icp_step_out* o) const {
        const double d2max = max_corr_dist * max_corr_dist;
        std::vector<double> xs, qs, rs;   // the correspondences in source order: x, q or the unit target normal, r
        o->count = 0;
        for (uint64_t i = 0; i < n_src; ++i) {
            if (o->nn) o->nn[i] = -1;
            if (o->r) o->r[i] = 0.0;
            double p[3], m[3] = {0, 0, 0}, x[3];
            src.load(i, p);
            if (method == ICP_PLANE) {
                src_n.load(i, m);
                const double len = norm3(m[0], m[1], m[2]);
                if (!finite3(m) || len <= ICP_NORMAL_EPS) continue;
                m[0] = m[0] / len, m[1] = m[1] / len, m[2] = m[2] / len;
            }
            for (int k = 0; k < 3; ++k) x[k] = ((pose[4 * k] * p[0] + pose[4 * k + 1] * p[1]) + pose[4 * k + 2] * p[2]) + pose[4 * k + 3];
            const int64_t j = nearest(x, d2max);
            if (j < 0) continue;
            double q[3], second[3], r;
            tgt.load((uint64_t)j, q);
            const double e[3] = {x[0] - q[0], x[1] - q[1], x[2] - q[2]};
            if (method == ICP_PLANE) {
                double mw[3], t[3];
                for (int k = 0; k < 3; ++k) mw[k] = (pose[4 * k] * m[0] + pose[4 * k + 1] * m[1]) + pose[4 * k + 2] * m[2];
                tgt_n.load((uint64_t)j, t);
                const double len = norm3(t[0], t[1], t[2]);
                if (!finite3(t) || len <= ICP_NORMAL_EPS) continue;
                t[0] = t[0] / len, t[1] = t[1] / len, t[2] = t[2] / len;
                const double align = std::fabs((t[0] * mw[0] + t[1] * mw[1]) + t[2] * mw[2]);
                if (!std::isfinite(align) || align < cos_gate) continue;
                r = (t[0] * e[0] + t[1] * e[1]) + t[2] * e[2];
                std::memcpy(second, t, sizeof t);
            } else {
                r = norm3(e[0], e[1], e[2]);
                std::memcpy(second, q, sizeof q);
            }
            if (!std::isfinite(r)) continue;
            if (o->nn) o->nn[i] = (int32_t)j;
            if (o->r) o->r[i] = r;
            xs.insert(xs.end(), x, x + 3), qs.insert(qs.end(), second, second + 3), rs.push_back(r);
        }
        const size_t count = rs.size();
        o->count = count;
        o->median = o->huber_delta = 0.0;
        for (double& s : o->sums) s = 0.0;
        for (int k = 0; k < 3; ++k) o->centroid_x[k] = o->centroid_q[k] = 0.0;
        o->solved = count >= ICP_MIN_POINTS;
        if (o->solved) {
            std::vector<double> a(count);
            for (size_t k = 0; k < count; ++k) a[k] = std::fabs(rs[k]);
            std::sort(a.begin(), a.end());
            const size_t mid = count / 2;
            o->median = (count & 1) ? a[mid] : 0.5 * (a[mid - 1] + a[mid]);
            const double delta = o->huber_delta = icp_huber_delta(o->median, max_corr_dist);
            auto weight = [delta](double r) {
                const double ar = std::fabs(r);
                return (ar <= delta || delta <= 0.0) ? 1.0 : delta / ar;
            };
            double* s = o->sums;
            if (method == ICP_POINT) {
                for (size_t k = 0; k < count; ++k) {
                    const double w = weight(rs[k]);
                    s[0] = s[0] + w;
                    for (int c = 0; c < 3; ++c) s[1 + c] = s[1 + c] + w * xs[3 * k + c], s[4 + c] = s[4 + c] + w * qs[3 * k + c];
                }
                if (std::isfinite(s[0]) && !(s[0] <= 1e-12)) {
                    for (int c = 0; c < 3; ++c) o->centroid_x[c] = s[1 + c] / s[0], o->centroid_q[c] = s[4 + c] / s[0];
                    for (size_t k = 0; k < count; ++k) {
                        const double w = weight(rs[k]);
                        double wx[3], dq[3];
                        for (int c = 0; c < 3; ++c) wx[c] = w * (xs[3 * k + c] - o->centroid_x[c]), dq[c] = qs[3 * k + c] - o->centroid_q[c];
                        for (int a2 = 0; a2 < 3; ++a2)
                            for (int b = 0; b < 3; ++b) s[7 + 3 * a2 + b] = s[7 + 3 * a2 + b] + wx[a2] * dq[b];
                    }
                }
            } else {
                for (size_t k = 0; k < count; ++k) {
                    const double r = rs[k], w = weight(r);
                    const double *x = &xs[3 * k], *m = &qs[3 * k];
                    const double j[6] = {x[1] * m[2] - x[2] * m[1], x[2] * m[0] - x[0] * m[2], x[0] * m[1] - x[1] * m[0], m[0], m[1], m[2]};
                    int at = 0;
                    for (int a2 = 0; a2 < 6; ++a2)
                        for (int b = a2; b < 6; ++b, ++at) s[at] = s[at] + w * (j[a2] * j[b]);
                    for (int a2 = 0; a2 < 6; ++a2) s[21 + a2] = s[21 + a2] + (-w) * (j[a2] * r);
                }
            }
        }
        bool stop = true;
        icp_finish_pass(method, count, o->sums, o->centroid_x, o->centroid_q, pose, o->next_pose, &stop);
        o->stop = stop;
    }
};

}  // namespace
}  // namespace ouster_hip_dev

extern "C" int ouster_hip_icp_step_ref(const ouster_hip_icp_desc* d, const double* pose16, ouster_hip_icp_step_out* out) {
    using namespace ouster_hip_dev;
    if (!d || !pose16 || !out) return fail_msg(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (const char* msg = icp_validate(d)) return fail_msg(OUSTER_HIP_ERR_INVALID_ARGUMENT, msg);
    if (d->n_source < ICP_MIN_POINTS || d->n_target < ICP_MIN_POINTS)
        return fail_msg(OUSTER_HIP_ERR_INVALID_ARGUMENT, "icp_step: fewer than 20 rows");
    if (d->n_source > ICP_MAX_ROWS || d->n_target > ICP_MAX_ROWS) return fail_msg(OUSTER_HIP_ERR_UNSUPPORTED, "icp: more than 2^30 rows");
    HostIcp icp(d);
    if (!icp.build()) return fail_msg(OUSTER_HIP_ERR_INVALID_ARGUMENT, icp_msg_grid(icp.method));
    icp.step(pose16, out);
    return OUSTER_HIP_OK;
}

extern "C" int ouster_hip_icp_align_ref(ouster_hip_icp_desc* d) {
    using namespace ouster_hip_dev;
    if (!d) return fail_msg(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (const char* msg = icp_validate(d)) return fail_msg(OUSTER_HIP_ERR_INVALID_ARGUMENT, msg);
    if (d->n_source > ICP_MAX_ROWS || d->n_target > ICP_MAX_ROWS) return fail_msg(OUSTER_HIP_ERR_UNSUPPORTED, "icp: more than 2^30 rows");
    double pose[16];
    std::memcpy(pose, d->initial_guess, sizeof pose);
    uint32_t iterations = 0, solved = 0;
    uint64_t count = 0;
    if (d->n_source >= ICP_MIN_POINTS && d->n_target >= ICP_MIN_POINTS) {
        HostIcp icp(d);
        if (!icp.build()) return fail_msg(OUSTER_HIP_ERR_INVALID_ARGUMENT, icp_msg_grid(icp.method));
        for (uint32_t it = 0; it < ICP_MAX_ITERATIONS; ++it) {
            ouster_hip_icp_step_out o{};
            icp.step(pose, &o);
            ++iterations;
            count = o.count;
            solved |= (uint32_t)o.solved;
            std::memcpy(pose, o.next_pose, sizeof pose);
            if (o.stop) break;
        }
    }
    std::memcpy(d->pose, solved ? pose : d->initial_guess, sizeof pose);
    d->iterations = iterations, d->solved = solved, d->correspondences = count;
    return OUSTER_HIP_OK;
}

extern "C" uint64_t ouster_hip_icp_chunk_table(const uint64_t* rows, uint32_t n_sources, uint32_t* chunks, uint64_t cap) {
    using namespace ouster_hip_dev;
    static_assert(sizeof(IcpChunk) == 3 * sizeof(uint32_t), "chunks[cap][3]");
    if (!rows || (cap && !chunks)) return 0;
    return icp_chunk_table(rows, n_sources, reinterpret_cast<IcpChunk*>(chunks), cap, nullptr, nullptr);
}
