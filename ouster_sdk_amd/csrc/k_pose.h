// k_pose.h -- launch interface of the pose kernels (k_pose.hip): interp_pose per x / per column, transform per point.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/ouster_hip.h"
#include "pose_host.h"

namespace ouster_hip_dev {

struct PoseInterpArgs {
    const double* x;            // array form: [n] times; nullptr selects the column form
    const uint64_t* timestamp;  // column form: [n] ns, x = double(ts) * 1e-9 ...
    const uint32_t* status;     //   ... and a column with (status & 1) == 0 is skipped, its outputs left as they are
    uint64_t n;
    const double* segments;     // device [k - 1][POSE_SEG_DOUBLES]
    const double* x_known;      // device [k], strictly increasing
    uint32_t k;
    int32_t dtype;              // OUSTER_HIP_F32 / OUSTER_HIP_F64: element type of `out`
    void* out;                  // [n][16], 16-byte aligned
    float* pose_rows;           // column form, optional: [n][12] = float(pose[0..11]), 16-byte aligned
    int32_t direct_stores;      // 1: every lane stores its own row (A/B); 0: rows staged in LDS, stores lane-linear
};

struct PoseTransformArgs {
    const void* points;         // [n][3] of dtype
    void* out;                  // [n][3]; may alias points
    double pose[16];            // row-major 4x4; cast to dtype before it multiplies
    uint64_t n;
    int32_t dtype;
};

hipError_t launch_pose_interp(const PoseInterpArgs& a, hipStream_t st);
hipError_t launch_pose_transform(const PoseTransformArgs& a, hipStream_t st);

}  // namespace ouster_hip_dev
