// registration_host.h -- the host half of ICPRegistration (csrc/host/registration_util.cpp): the solve, SE(3), the stop rule, the
// argument checks, AdaptiveThreshold's arithmetic and the whole algorithm on one core over HostVoxelMap with left-fold sums (the
// _ref form).  Operation for operation tests/registration_model.py.  Plain C++, no HIP: the C ABI (capi_registration.hip) calls it
// between the passes, and tests/cpp builds it alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/ouster_hip.h"
#include "voxel_map_host.h"

namespace ouster_hip_dev {

constexpr int REG_SUMS = OUSTER_HIP_REG_SUMS;
constexpr uint64_t REG_MAX_ROWS = 1ull << 30;

// a pose: (qx, qy, qz, qw, tx, ty, tz)
struct RegPose {
    double v[7] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
};

// nullptr, or why the call is refused (INVALID_ARGUMENT); *unsupported: the message is an UNSUPPORTED one
const char* reg_validate(const void* map, const void* points, int32_t dtype, uint64_t n, uint64_t row_stride, double max_distance,
                         double kernel_scale, double convergence, bool* unsupported);

// the 16 terms of one correspondence (model: terms)
void reg_terms(const double* s, const double* q, double kernel_scale, double* t);
// the 16 sums -> jtj (row-major 6 x 6, the lower triangle, the upper left zero) and jtr
void reg_system(const double* sums, double* jtj36, double* jtr6);
// dx = solve(jtj, -jtr): L D L^T without pivoting over the lower triangle; a zero pivot gives a zero component
void reg_solve6(const double* jtj36, const double* jtr6, double* dx6);
RegPose reg_exp(const double* dx6);
void reg_apply(const RegPose& p, const double* in, double* out);
RegPose reg_compose(const RegPose& a, const RegPose& b);
void reg_matrix(const RegPose& p, double* m16);
double reg_squared_norm6(const double* dx6);
// sums -> dx and exp(dx); true: dx . dx < convergence^2
bool reg_solve_pass(const double* sums, double convergence, double* dx6, RegPose* estimate);

// one pass on the host map: applies `estimate` (nullptr: nothing) to moved[n][3] in place, associates, left-fold sums.  flags,
// neighbours, dist_sq: nullptr or per-row outputs.
void reg_pass_ref(const HostVoxelMap& map, double* moved, uint64_t n, const RegPose* estimate, double max_distance, double kernel_scale,
                  uint8_t* flags, double* neighbours, double* dist_sq, double* sums, uint64_t* count);
// the whole loop on the host map over rows[n][stride] of f32 / f64 -> desc's outputs
void reg_align_ref(const HostVoxelMap& map, const void* points, bool f32, uint64_t n, uint64_t stride, ouster_hip_registration_desc* desc);
void reg_identity(ouster_hip_registration_desc* desc);

void reg_build_linear_system(const double* sources, const double* targets, uint64_t n, double kernel_scale, double* jtj36, double* jtr6);
double reg_model_error(const double* deviation16, double max_range);

}  // namespace ouster_hip_dev
