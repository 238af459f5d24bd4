// icp_ref_main.cpp -- the host half of ICP (csrc/host/icp_util.cpp, pose_util.cpp) on its own: the reference's two published cases
// through ouster_hip_icp_align_ref and one pass through ouster_hip_icp_step_ref.  No GPU, no library: `make sanitized` in
// this directory builds it with -fsanitize=address,undefined and runs it, the way to run a sanitizer over that code.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>
#include "../../include/ouster_hip.h"
namespace ouster_hip_dev { static std::string g; int fail_msg(int code, const char* msg) { g = msg; return code; } }
int main() {
    std::vector<double> src, tgt;
    for (int x = -1; x <= 1; ++x) for (int y = -1; y <= 1; ++y) for (int z = -1; z <= 1; ++z) {
        src.insert(src.end(), {double(x), double(y), double(z)});
        tgt.insert(tgt.end(), {x + 0.1, y - 0.05, z + 0.025});
    }
    ouster_hip_icp_desc d{};
    d.source_points = src.data(), d.target_points = tgt.data(), d.n_source = d.n_target = 27, d.dtype = OUSTER_HIP_F64;
    for (int i = 0; i < 4; ++i) d.initial_guess[5 * i] = 1.0;
    d.max_corr_dist = 0.5, d.max_normal_angle_deg = 20.0;
    if (ouster_hip_icp_align_ref(&d) != 0) return 1;
    std::printf("point: t = %.12f %.12f %.12f, %u passes, %llu correspondences\n", d.pose[3], d.pose[7], d.pose[11], d.iterations, (unsigned long long)d.correspondences);
    if (std::fabs(d.pose[3] - 0.1) > 1e-10 || std::fabs(d.pose[7] + 0.05) > 1e-10 || std::fabs(d.pose[11] - 0.025) > 1e-10) return 2;
    std::vector<double> p, q, n;
    for (int x = 0; x < 5; ++x) for (int y = 0; y < 5; ++y) {
        p.insert(p.end(), {double(x), double(y), 0.0}); q.insert(q.end(), {double(x), double(y), 0.2}); n.insert(n.end(), {0.0, 0.0, 1.0});
    }
    ouster_hip_icp_desc e{};
    e.source_points = p.data(), e.target_points = q.data(), e.source_normals = n.data(), e.target_normals = n.data();
    e.n_source = e.n_target = e.n_source_normals = e.n_target_normals = 25, e.dtype = OUSTER_HIP_F64;
    for (int i = 0; i < 4; ++i) e.initial_guess[5 * i] = 1.0;
    e.max_corr_dist = 0.5, e.max_normal_angle_deg = 20.0;
    if (ouster_hip_icp_align_ref(&e) != 0) return 3;
    std::printf("plane: t = %.12f %.12f %.12f, %u passes\n", e.pose[3], e.pose[7], e.pose[11], e.iterations);
    if (std::fabs(e.pose[11] - 0.2) > 1e-9) return 4;
    std::vector<int32_t> nn(25); std::vector<double> r(25);
    ouster_hip_icp_step_out o{}; o.nn = nn.data(), o.r = r.data();
    if (ouster_hip_icp_step_ref(&e, e.initial_guess, &o) != 0) return 5;
    std::printf("ok\n");
    return 0;
}
