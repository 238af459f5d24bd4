// pose_interp.cpp -- core::interp_pose / core::transform over the C ABI (include/ouster/core/pose_util.h).  Everything that can
// be refused is refused on the host first, with the reference's messages (ouster_core/include/ouster/core/pose_util.h:195-263),
// before the GPU is asked for; the per-x and per-point work runs there (ouster_hip_interp_pose_host, ouster_hip_transform_host).
#include <cfloat>
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

#include "host_internal.h"
#include "ouster/core/pose_util.h"

namespace ouster {
namespace sdk {
namespace core {
namespace impl {
namespace {
void check_increasing(const double* x, size_t n) {
    for (size_t i = 1; i < n; ++i)
        if (x[i] < x[i - 1])
            throw std::invalid_argument("x_interp values must be monotonically increasing: " + std::to_string(x[i]) + " < " +
                                        std::to_string(x[i - 1]));
}
}  // namespace

void interp_pose_device(const double* x_interp, size_t n, const double* x_known, const double* poses_known, size_t k, bool f64,
                        void* out) {
    if (k > 0xffffffffu) throw std::invalid_argument("interp_pose: too many known poses");
    hip::check(ouster_hip_pose_validate(x_known, poses_known, static_cast<uint32_t>(k), x_interp, n));
    ouster_hip_ctx* ctx = hip::default_ctx();   // throws without a GPU
    hip::check(ouster_hip_interp_pose_host(ctx, x_interp, n, x_known, poses_known, static_cast<uint32_t>(k),
                                           f64 ? OUSTER_HIP_F64 : OUSTER_HIP_F32, out));
}

void interp_pose_pair_device(const double* x_interp, size_t n, double t0, const double* x0, double t1, const double* x1,
                             double* out) {
    if (std::fabs(t1 - t0) < DBL_EPSILON) throw std::invalid_argument("Cannot interpolate with zero duration between poses");
    check_increasing(x_interp, n);
    ouster_hip_ctx* ctx = hip::default_ctx();
    hip::check(ouster_hip_interp_pose_pair_host(ctx, x_interp, n, t0, x0, t1, x1, OUSTER_HIP_F64, out));
}

void transform_device(const void* points, const double* pose16, void* out, bool f64, size_t n) {
    hip::check(ouster_hip_transform_host(hip::default_ctx(), points, pose16, out, f64 ? OUSTER_HIP_F64 : OUSTER_HIP_F32, n));
}

}  // namespace impl
}  // namespace core
}  // namespace sdk
}  // namespace ouster
