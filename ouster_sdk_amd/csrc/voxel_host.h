// voxel_host.h -- the host half of voxel down-sampling (csrc/host/voxel_util.cpp): validation with the reference's messages, the
// choice of the GPU's reduction form, and the plain C++ restatement behind ouster_hip_voxel_downsample_ref.  Plain C++, no HIP:
// the C ABI (capi_voxel.hip) calls it before anything touches the GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/ouster_hip.h"

namespace ouster_hip_dev {

// what k_voxel_reduce / k_voxel_write do with a voxel's points (k_voxel.h)
enum VoxelForm : int32_t {
    VOXEL_FORM_AVERAGE = 0,   // AVERAGE_POINT: fold in input order, divide by the count, keep where count >= min_pts_threshold
    VOXEL_FORM_FIRST = 1,     // FIRST_N_POINT with max_points_per_voxel == 1: the voxel's first point
    VOXEL_FORM_LAST = 2,      // RANDOM with max_points_per_voxel == 1: the voxel's last point
    VOXEL_FORM_NORMALS = 3,   // voxel_downsample_with_normals
    VOXEL_FORM_HOST = -1      // FIRST_N_POINT / RANDOM with max_points_per_voxel > 1: sequential by nature, host code only
};

constexpr uint64_t VOXEL_MAX_POINTS = 1ull << 30;
constexpr const char* VOXEL_MSG_GRID = "voxel_downsample: point outside the int32 voxel grid";

// nullptr, or the message the reference (or, for a non-finite voxel_size and an unknown strategy, this project) refuses with:
// strategy, max_points_per_voxel, voxel_size in the VoxelHashMap constructor's order; the with-normals form's own two
const char* voxel_validate(const ouster_hip_voxel_desc* d);
VoxelForm voxel_form(const ouster_hip_voxel_desc* d);

// the C ABI's error channel (ouster_hip_capi.hip): stores the thread's message, returns `code`
int fail_msg(int code, const char* msg);

}  // namespace ouster_hip_dev
