// registration_snippet.cpp -- a C++ caller of include/ouster/mapping/icp_registration.h and adaptive_threshold.h on host maps
// (VoxelHashMap3d::on_host: no GPU): defaults, the reference's scenarios, every refusal.  Built with -Werror by
// tests/cpp/Makefile, run by tests/test_registration_api_cpu.py.
#include <cmath>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <vector>

#include "ouster/mapping/adaptive_threshold.h"
#include "ouster/mapping/icp_registration.h"

using namespace ouster::sdk;

static int failures = 0;
#define CHECK(cond)                                                 \
    do {                                                            \
        if (!(cond)) {                                              \
            std::printf("FAIL line %d: %s\n", __LINE__, #cond);     \
            ++failures;                                             \
        }                                                           \
    } while (0)

template <class F>
static bool refused(F f) {
    try {
        f();
    } catch (const std::invalid_argument&) {
        return true;
    }
    return false;
}

int main() {
    const mapping::ICPRegistration defaults;
    CHECK(defaults.max_num_iterations_ == 50 && defaults.convergence_criterion_ == 0.0001 && defaults.max_num_threads_ > 0);
    CHECK(mapping::ICPRegistration(5, 1e-3, 3).max_num_threads_ == 3);

    const std::vector<mapping::Point3d> pts = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    core::VoxelHashMap3d empty = core::VoxelHashMap3d::on_host(0.5, 10.0);
    const mapping::ICPRegistration reg(20);
    core::Matrix4dR T = reg.align_points_to_map(pts, empty, 1.0, 0.1);
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) CHECK(T(r, c) == (r == c ? 1.0 : 0.0));

    core::VoxelHashMap3d map = core::VoxelHashMap3d::on_host(0.5, 10.0);
    map.add_points(pts);
    core::ArrayX3dR shifted(4);
    const double shift[3] = {0.05, 0.02, -0.01};
    for (size_t i = 0; i < 4; ++i)
        for (int c = 0; c < 3; ++c) shifted.data()[3 * i + c] = pts[i][c] + shift[c];
    T = reg.align_points_to_map(shifted, map, 0.5, 0.1);
    for (size_t i = 0; i < 4; ++i)
        for (int r = 0; r < 3; ++r) {
            const double* s = shifted.data() + 3 * i;
            CHECK(std::fabs(T(r, 0) * s[0] + T(r, 1) * s[1] + T(r, 2) * s[2] + T(r, 3) - pts[i][r]) < 0.05);
        }
    CHECK(T(3, 3) == 1.0);
    const core::Matrix4dR none = mapping::ICPRegistration(0).align_points_to_map(shifted, map, 0.5, 0.1);
    CHECK(none(0, 0) == 1.0 && none(0, 3) == 0.0);
    const core::Matrix4dR no_rows = reg.align_points_to_map(std::vector<mapping::Point3d>{}, map, 0.5, 0.1);
    CHECK(no_rows(1, 1) == 1.0 && no_rows(1, 3) == 0.0);

    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (double bad : {-1.0, nan, inf}) {
        CHECK(refused([&] { reg.align_points_to_map(shifted, map, bad, 0.1); }));
        CHECK(refused([&] { reg.align_points_to_map(shifted, map, 0.5, bad); }));
        CHECK(refused([&] { mapping::ICPRegistration(5, bad).align_points_to_map(shifted, map, 0.5, 0.1); }));
        CHECK(refused([&] { mapping::build_linear_system({}, bad); }));
    }

    // one correspondence on paper: s = (1, 2, 3), q = (1, 2, 2), k = 1: w = 1 / 4
    const mapping::LinearSystem ls = mapping::build_linear_system({{{1, 2, 3}, {1, 2, 2}}}, 1.0);
    CHECK(ls.first(0, 0) == 0.25 && ls.first(3, 3) == 3.25 && ls.first(4, 3) == -0.5 && ls.first(5, 1) == 0.25 && ls.first(3, 1) == -0.75);
    CHECK(ls.first(0, 4) == 0.0 && ls.first(1, 5) == 0.0);   // the upper triangle stays zero
    CHECK(ls.second(2) == 0.25 && ls.second(3) == 0.5 && ls.second(4) == -0.25 && ls.second(5) == 0.0);

    mapping::AdaptiveThreshold fresh(100.0);
    CHECK(fresh.max_range_ == 100.0 && fresh.min_motion_threshold_ == 0.01 && fresh.compute_threshold() == 2.0);
    mapping::AdaptiveThreshold at(100.0, 1.0);
    core::mat4d dev = core::mat4d::Identity();
    dev(0, 3) = 2.0;
    at.update_model_deviation(dev);
    CHECK(at.num_samples_ == 2 && at.compute_threshold() == std::sqrt(2.5));
    dev(0, 3) = 0.01;   // exactly at min_motion_threshold: not a sample
    at.update_model_deviation(dev);
    CHECK(at.num_samples_ == 2);

    if (failures) return 1;
    std::printf("registration_snippet: ok\n");
    return 0;
}
