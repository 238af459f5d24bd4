// align_clouds.cpp -- algorithm::point_to_point_align / point_to_plane_align (include/ouster/algorithm/align_clouds.h) over the C
// ABI.  Parameters and shapes are refused on the host first, in the reference's order and with its messages, as
// std::invalid_argument; clouds of fewer than 20 rows return the guess without a GPU; then the GPU is asked for and
// ouster_hip_icp_align_host does the work.
#include "ouster/algorithm/align_clouds.h"

#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>

#include "host_internal.h"

namespace ouster {
namespace sdk {
namespace algorithm {
namespace impl {

AlignStats align_arrays(const double* source_points, std::size_t source_rows, const double* target_points, std::size_t target_rows,
                        const double* source_normals, std::size_t source_normal_rows, const double* target_normals,
                        std::size_t target_normal_rows, const double* initial_guess16, double max_corr_dist,
                        double max_normal_angle_deg, double* pose16) {
    const bool plane = source_normals != nullptr || target_normals != nullptr;
    // what the C ABI refuses, in its order, before a GPU is asked for
    if (!std::isfinite(max_corr_dist) || max_corr_dist <= 0.0)
        throw std::invalid_argument("max_corr_dist must be finite and greater than zero");
    if (plane) {
        if (!std::isfinite(max_normal_angle_deg) || max_normal_angle_deg < 0.0 || max_normal_angle_deg > 180.0)
            throw std::invalid_argument("max_normal_angle_deg must be finite and in [0, 180]");
        if (source_rows != source_normal_rows)
            throw std::invalid_argument("source_points and source_normals must have the same number of rows");
        if (target_rows != target_normal_rows)
            throw std::invalid_argument("target_points and target_normals must have the same number of rows");
    }
    ouster_hip_icp_desc d{};
    static const double none[3] = {0, 0, 0};   // an empty cloud still needs somewhere to point
    d.source_points = source_rows ? source_points : none, d.target_points = target_rows ? target_points : none;
    if (plane) {
        d.source_normals = source_rows ? source_normals : none, d.target_normals = target_rows ? target_normals : none;
        d.n_source_normals = source_normal_rows, d.n_target_normals = target_normal_rows;
    }
    d.n_source = source_rows, d.n_target = target_rows;
    d.dtype = OUSTER_HIP_F64;
    std::memcpy(d.initial_guess, initial_guess16, sizeof d.initial_guess);
    d.max_corr_dist = max_corr_dist, d.max_normal_angle_deg = max_normal_angle_deg;
    // fewer than 20 rows on a side: the guess, and no GPU is needed for that
    const bool small = source_rows < 20 || target_rows < 20;
    const int rc = ouster_hip_icp_align_host(small ? nullptr : hip::default_ctx() /* throws without a GPU */, &d);
    if (rc != OUSTER_HIP_OK) {
        if (rc == OUSTER_HIP_ERR_INVALID_ARGUMENT) throw std::invalid_argument(ouster_hip_last_error());
        throw std::runtime_error(ouster_hip_last_error());
    }
    std::memcpy(pose16, d.pose, sizeof d.pose);
    AlignStats s;
    s.iterations = d.iterations, s.correspondences = d.correspondences, s.solved = d.solved != 0;
    return s;
}

}  // namespace impl

core::Matrix4dR point_to_point_align(const core::ArrayX3dR& source_points, const core::ArrayX3dR& target_points,
                                     const core::Matrix4dR& initial_guess, double max_corr_dist) {
    double pose[16];
    impl::align_arrays(source_points.data(), source_points.rows(), target_points.data(), target_points.rows(), nullptr, 0, nullptr, 0,
                       initial_guess.data(), max_corr_dist, 20.0, pose);
    return core::Matrix4dR::FromRowMajor(pose);
}

core::Matrix4dR point_to_plane_align(const core::ArrayX3dR& source_points, const core::ArrayX3dR& target_points,
                                     const core::ArrayX3dR& source_normals, const core::ArrayX3dR& target_normals,
                                     const core::Matrix4dR& initial_guess, double max_corr_dist, double max_normal_angle_deg) {
    static const double none[3] = {0, 0, 0};
    double pose[16];
    // an empty normals array still selects the point-to-plane checks
    impl::align_arrays(source_points.data(), source_points.rows(), target_points.data(), target_points.rows(),
                       source_normals.rows() ? source_normals.data() : none, source_normals.rows(),
                       target_normals.rows() ? target_normals.data() : none, target_normals.rows(), initial_guess.data(), max_corr_dist,
                       max_normal_angle_deg, pose);
    return core::Matrix4dR::FromRowMajor(pose);
}

// ---- IcpTarget (a project extension): ouster_hip_icp_target_* behind a move-only handle ----
namespace {
[[noreturn]] void raise(int rc) {
    if (rc == OUSTER_HIP_ERR_INVALID_ARGUMENT) throw std::invalid_argument(ouster_hip_last_error());
    throw std::runtime_error(ouster_hip_last_error());
}

const double kNone[3] = {0, 0, 0};   // an empty cloud still needs somewhere to point; it is never read

ouster_hip_icp_target* handle_of(void* h) { return static_cast<ouster_hip_icp_target*>(h); }
}  // namespace

namespace {
// Create through `create` (the device or the _host form).  First without a context: the C ABI refuses what it refuses, in its
// order and with its messages, and makes a target of fewer than 20 rows, all before a GPU is asked for; only "ctx is NULL" -- every
// check passed and there is work for a GPU -- asks for the thread's current context (which throws without a GPU) and goes again.
template <class Create>
ouster_hip_icp_target* create_target(Create create, const ouster_hip_icp_target_desc& d, std::shared_ptr<hip::Context>& ctx) {
    ouster_hip_icp_target* h = nullptr;
    int rc = create(nullptr, &d, &h);
    if (rc == OUSTER_HIP_ERR_INVALID_ARGUMENT && std::string(ouster_hip_last_error()) == "ctx is NULL") {
        hip::default_ctx();   // throws without a GPU
        ctx = hip::Context::current();
        rc = create(ctx->handle(), &d, &h);
    }
    if (rc != OUSTER_HIP_OK) raise(rc);
    return h;
}
}  // namespace

IcpTarget IcpTarget::from_arrays(const double* points, std::size_t rows, const double* normals, std::size_t normal_rows,
                                 double max_corr_dist) {
    ouster_hip_icp_target_desc d{};
    d.points = rows ? points : kNone, d.n = rows;
    if (normals) d.normals = normal_rows ? normals : kNone, d.n_normals = normal_rows;
    d.dtype = OUSTER_HIP_F64, d.max_corr_dist = max_corr_dist;
    IcpTarget t;
    t.handle_ = create_target(ouster_hip_icp_target_create_host, d, t.ctx_);
    return t;
}

IcpTarget IcpTarget::from_device(const double* points, const double* normals, std::size_t rows, double max_corr_dist) {
    ouster_hip_icp_target_desc d{};
    d.points = rows ? points : kNone, d.n = rows;
    if (normals) d.normals = normals, d.n_normals = rows;
    d.dtype = OUSTER_HIP_F64, d.max_corr_dist = max_corr_dist;
    IcpTarget t;
    t.handle_ = create_target(ouster_hip_icp_target_create, d, t.ctx_);
    return t;
}

IcpTarget::IcpTarget(const core::ArrayX3dR& points, double max_corr_dist)
    : IcpTarget(from_arrays(points.data(), points.rows(), nullptr, 0, max_corr_dist)) {}

IcpTarget::IcpTarget(const core::ArrayX3dR& points, const core::ArrayX3dR& normals, double max_corr_dist)
    : IcpTarget(from_arrays(points.data(), points.rows(), normals.rows() ? normals.data() : kNone, normals.rows(), max_corr_dist)) {}

IcpTarget::~IcpTarget() { ouster_hip_icp_target_destroy(handle_of(handle_)); }

IcpTarget::IcpTarget(IcpTarget&& o) noexcept : handle_(o.handle_), ctx_(std::move(o.ctx_)) { o.handle_ = nullptr; }

IcpTarget& IcpTarget::operator=(IcpTarget&& o) noexcept {
    if (this != &o) {
        ouster_hip_icp_target_destroy(handle_of(handle_));
        handle_ = o.handle_, ctx_ = std::move(o.ctx_);
        o.handle_ = nullptr;
    }
    return *this;
}

namespace {
ouster_hip_icp_target_info info_of(void* h) {
    ouster_hip_icp_target_info i{};
    if (h && ouster_hip_icp_target_info_read(handle_of(h), &i) != OUSTER_HIP_OK) throw std::runtime_error(ouster_hip_last_error());
    return i;
}
}  // namespace

std::size_t IcpTarget::size() const { return info_of(handle_).rows; }
bool IcpTarget::has_normals() const { return info_of(handle_).has_normals != 0; }
std::size_t IcpTarget::device_bytes() const { return info_of(handle_).device_bytes; }
double IcpTarget::max_corr_dist() const { return info_of(handle_).max_corr_dist; }
int IcpTarget::device() const { return ctx_ ? ctx_->device() : -1; }

void IcpTarget::align_arrays(const double* const* points, const std::size_t* rows, const double* const* normals,
                             const std::size_t* normal_rows, std::size_t n_sources, const double* guesses16, double max_normal_angle_deg,
                             double* poses16, impl::AlignStats* stats) const {
    if (!handle_) throw std::runtime_error("IcpTarget: moved from");
    if (n_sources > 0xffffffffull) throw std::runtime_error("icp_target: more than 65535 sources");
    std::vector<ouster_hip_icp_source> s(n_sources);
    for (std::size_t k = 0; k < n_sources; ++k) {
        s[k].points = rows[k] ? points[k] : kNone, s[k].n = rows[k];
        if (normals && normals[k]) s[k].normals = normal_rows[k] ? normals[k] : kNone, s[k].n_normals = normal_rows[k];
        if (guesses16) std::memcpy(s[k].initial_guess, guesses16 + 16 * k, sizeof s[k].initial_guess);
        else std::memcpy(s[k].initial_guess, core::Matrix4dR::Identity().data(), sizeof s[k].initial_guess);
    }
    const int rc = ouster_hip_icp_target_align_host((ctx_ ? ctx_->handle() : nullptr), handle_of(handle_), s.data(),
                                                    static_cast<uint32_t>(n_sources), OUSTER_HIP_F64, max_normal_angle_deg);
    if (rc != OUSTER_HIP_OK) raise(rc);
    for (std::size_t k = 0; k < n_sources; ++k) {
        std::memcpy(poses16 + 16 * k, s[k].pose, sizeof s[k].pose);
        if (stats) stats[k].iterations = s[k].iterations, stats[k].correspondences = s[k].correspondences, stats[k].solved = s[k].solved != 0;
    }
}

impl::AlignStats IcpTarget::align_device(const double* points, const double* normals, std::size_t rows, const double* initial_guess16,
                                         double max_normal_angle_deg, double* pose16) const {
    if (!handle_) throw std::runtime_error("IcpTarget: moved from");
    ouster_hip_icp_source s{};
    s.points = rows ? points : kNone, s.n = rows;
    if (normals) s.normals = normals, s.n_normals = rows;
    if (initial_guess16) std::memcpy(s.initial_guess, initial_guess16, sizeof s.initial_guess);
    else std::memcpy(s.initial_guess, core::Matrix4dR::Identity().data(), sizeof s.initial_guess);
    const int rc = ouster_hip_icp_target_align((ctx_ ? ctx_->handle() : nullptr), handle_of(handle_), &s, 1, OUSTER_HIP_F64, max_normal_angle_deg);
    if (rc != OUSTER_HIP_OK) raise(rc);
    std::memcpy(pose16, s.pose, sizeof s.pose);
    impl::AlignStats st;
    st.iterations = s.iterations, st.correspondences = s.correspondences, st.solved = s.solved != 0;
    return st;
}

namespace {
std::vector<core::Matrix4dR> many(const IcpTarget& t, const std::vector<core::ArrayX3dR>& sources, const std::vector<core::ArrayX3dR>* normals,
                                  const std::vector<core::Matrix4dR>& guesses, double angle, std::vector<impl::AlignStats>* stats) {
    const std::size_t n = sources.size();
    if (!guesses.empty() && guesses.size() != n) throw std::invalid_argument("icp_target: one initial guess per source, or none");
    if (normals && normals->size() != n) throw std::invalid_argument("icp_target: one normals array per source");
    std::vector<const double*> p(n), q(n);
    std::vector<std::size_t> rows(n), nrows(n);
    std::vector<double> g(16 * guesses.size()), poses(16 * n);
    for (std::size_t k = 0; k < n; ++k) {
        p[k] = sources[k].data(), rows[k] = sources[k].rows();
        if (normals) q[k] = (*normals)[k].rows() ? (*normals)[k].data() : kNone, nrows[k] = (*normals)[k].rows();
        if (!guesses.empty()) std::memcpy(&g[16 * k], guesses[k].data(), 16 * sizeof(double));
    }
    if (stats) stats->assign(n, impl::AlignStats());
    t.align_arrays(p.data(), rows.data(), normals ? q.data() : nullptr, nrows.data(), n, guesses.empty() ? nullptr : g.data(), angle,
                   poses.data(), stats ? stats->data() : nullptr);
    std::vector<core::Matrix4dR> out(n);
    for (std::size_t k = 0; k < n; ++k) out[k] = core::Matrix4dR::FromRowMajor(&poses[16 * k]);
    return out;
}
}  // namespace

std::vector<core::Matrix4dR> IcpTarget::align_many(const std::vector<core::ArrayX3dR>& sources, const std::vector<core::Matrix4dR>& guesses,
                                                   std::vector<impl::AlignStats>* stats) const {
    return many(*this, sources, nullptr, guesses, 20.0, stats);
}

std::vector<core::Matrix4dR> IcpTarget::align_many(const std::vector<core::ArrayX3dR>& sources, const std::vector<core::ArrayX3dR>& normals,
                                                   const std::vector<core::Matrix4dR>& guesses, double max_normal_angle_deg,
                                                   std::vector<impl::AlignStats>* stats) const {
    return many(*this, sources, &normals, guesses, max_normal_angle_deg, stats);
}

core::Matrix4dR IcpTarget::align(const core::ArrayX3dR& source, const core::Matrix4dR& initial_guess) const {
    const std::vector<core::ArrayX3dR> sources(1, source);
    return many(*this, sources, nullptr, std::vector<core::Matrix4dR>(1, initial_guess), 20.0, nullptr)[0];
}

core::Matrix4dR IcpTarget::align(const core::ArrayX3dR& source, const core::ArrayX3dR& source_normals, const core::Matrix4dR& initial_guess,
                                 double max_normal_angle_deg) const {
    const std::vector<core::ArrayX3dR> sources(1, source), normals(1, source_normals);
    return many(*this, sources, &normals, std::vector<core::Matrix4dR>(1, initial_guess), max_normal_angle_deg, nullptr)[0];
}

}  // namespace algorithm
}  // namespace sdk
}  // namespace ouster
