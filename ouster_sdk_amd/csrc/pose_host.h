// pose_host.h -- the host half of interp_pose (csrc/host/pose_util.cpp): validation with the reference's messages and the
// per-segment table.  Plain C++, no HIP: the C ABI (capi_pose.hip) calls it before anything touches the GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ouster_hip_dev {

constexpr uint32_t POSE_SEG_DOUBLES = 24;   // t0, a[16], scaled_twist[6] (rotation then translation), one pad

// nullptr when (x_known, k poses) may be interpolated, else the reference's message (pose_util.h:252-263)
const char* pose_validate_known(const double* x_known, const double* poses_known, uint32_t k);
// the two-pose form's check (pose_util.h:212-215)
const char* pose_validate_pair(double t0, double t1);
// nullptr, or the message of the first x_interp[i] < x_interp[i - 1] (pose_util.h:195-200) in `msg`
const char* pose_validate_interp(const double* x_interp, size_t n, char* msg, size_t msg_size);
// one row of the table: log(inv(a) b) / (t1 - t0) next to t0 and a (pose_util.h:216-222)
void pose_segment(double t0, const double* a16, double t1, const double* b16, double* seg24);
// PoseV::exp of (rotation, translation) as a row-major 4x4, and the full 4x4 product a b with every sum left to right: shared
// with the ICP step (host/icp_util.cpp)
void pose_exp(const double* twist6, double* out16);
void pose_compose(const double* a16, const double* b16, double* out16);

// the C ABI's error channel (ouster_hip_capi.hip): stores the thread's message, returns `code`
int fail_msg(int code, const char* msg);

}  // namespace ouster_hip_dev
