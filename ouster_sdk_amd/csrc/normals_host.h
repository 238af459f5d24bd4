// normals_host.h -- the host half of algorithm::normals (csrc/host/normals_util.cpp): validation with the reference's messages
// and the per-call constants, the only place where acos and tan are evaluated (libm).  Plain C++, no HIP: the C ABI
// (capi_normals.hip) calls it before anything touches the GPU and between the two kernels.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/ouster_hip.h"

namespace ouster_hip_dev {

// nullptr, or the reference's message (ouster_algorithm/src/normals.cpp:412-417, 436-445): the clouds hold h * w points, the
// second range image has the first one's shape, there is one origin per column
const char* normals_validate_shapes(uint64_t h, uint64_t w, uint64_t xyz_rows, bool dual, uint64_t xyz2_rows, uint64_t range2_h,
                                    uint64_t range2_w, uint64_t n_origins);
// nullptr, or the message of normals.cpp:84-89, in the reference's order
const char* normals_validate_params(double min_angle_of_incidence_rad, double target_distance_m);
// compute_vertical_subtent from its acos on (normals.cpp:56-64, 75-76) and the constants of compute_unit_normals
void normals_constants(uint32_t w, uint32_t h, double min_angle_of_incidence_rad, double target_distance_m, bool has_pair,
                       double dot, uint32_t rows_apart, ouster_hip_normals_consts* out);

// the C ABI's error channel (ouster_hip_capi.hip): stores the thread's message, returns `code`
int fail_msg(int code, const char* msg);

}  // namespace ouster_hip_dev
