// normals_util.cpp -- the plain C++ half of algorithm::normals inside libouster_hip.so: what the reference refuses, with its
// messages, and the per-call constants.  Built with -ffp-contract=off, an object of its own (Makefile): the constants are compared
// bit for bit with tests/normals_model.py, which evaluates acos and tan with the same libm.
#include <algorithm>
#include <cmath>

#include "../normals_host.h"

namespace ouster_hip_dev {

const char* normals_validate_shapes(uint64_t h, uint64_t w, uint64_t xyz_rows, bool dual, uint64_t xyz2_rows, uint64_t range2_h,
                                    uint64_t range2_w, uint64_t n_origins) {
    if (xyz_rows != h * w || (dual && xyz2_rows != h * w)) return "normals: xyz dimensions mismatch";
    if (dual && (range2_h != h || range2_w != w)) return "normals: range2 dimensions mismatch";
    if (n_origins != w) return "normals: sensor_origins size must match image width";
    return nullptr;
}

const char* normals_validate_params(double min_angle_of_incidence_rad, double target_distance_m) {
    if (target_distance_m <= 0.0) return "normals: target_distance_m must be positive";
    if (min_angle_of_incidence_rad <= 0.0) return "normals: min_angle_of_incidence_rad must be positive";
    return nullptr;
}

void normals_constants(uint32_t w, uint32_t h, double min_angle_of_incidence_rad, double target_distance_m, bool has_pair,
                       double dot, uint32_t rows_apart, ouster_hip_normals_consts* out) {
    double subtent;
    if (has_pair) {
        const double clamped = std::max(-1.0, std::min(1.0, dot));   // a NaN becomes 1.0, as in the reference
        subtent = std::acos(clamped) / static_cast<double>(rows_apart);
    } else {
        const uint32_t intervals = std::max<uint32_t>(1, h > 0 ? h - 1 : 1);
        subtent = (0.5 * M_PI) / static_cast<double>(intervals);
    }
    const double horizontal_subtent = 2.0 * M_PI / static_cast<double>(w);
    out->px_res_h = (2.0 * M_PI) / horizontal_subtent;
    out->px_res_v = (2.0 * M_PI) / subtent;
    out->tan_safe = std::tan(std::max(min_angle_of_incidence_rad, 1e-6));
    out->target_sq = target_distance_m * target_distance_m;
    out->subtent = subtent;
}

}  // namespace ouster_hip_dev

extern "C" int ouster_hip_normals_constants(uint32_t w, uint32_t h, double min_angle_of_incidence_rad, double target_distance_m,
                                            int has_pair, double dot, uint32_t rows_apart, ouster_hip_normals_consts* out) {
    using namespace ouster_hip_dev;
    if (!out) return fail_msg(OUSTER_HIP_ERR_INVALID_ARGUMENT, "out is NULL");
    if (const char* msg = normals_validate_params(min_angle_of_incidence_rad, target_distance_m))
        return fail_msg(OUSTER_HIP_ERR_INVALID_ARGUMENT, msg);
    if (w == 0 || h == 0) return fail_msg(OUSTER_HIP_ERR_INVALID_ARGUMENT, "normals: empty image");
    if (has_pair && rows_apart == 0) return fail_msg(OUSTER_HIP_ERR_INVALID_ARGUMENT, "normals: a pair of rows is at least one row apart");
    normals_constants(w, h, min_angle_of_incidence_rad, target_distance_m, has_pair != 0, dot, rows_apart, out);
    return OUSTER_HIP_OK;
}
