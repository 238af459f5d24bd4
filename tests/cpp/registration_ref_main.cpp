// registration_ref_main.cpp -- the plain C++ half of ICPRegistration (csrc/host/registration_util.cpp over HostVoxelMap of
// csrc/host/voxel_map_util.cpp) in a program of its own, built with -fsanitize=address,undefined by tests/cpp/Makefile: the
// checks, the solve, SE(3), the whole loop on empty, tiny, strided and float clouds, rows no cell holds.  No GPU, no library.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../ouster_sdk_amd/csrc/registration_host.h"

using namespace ouster_hip_dev;

int ouster_hip_dev::fail_msg(int code, const char*) { return code; }

static int failures = 0;
#define CHECK(cond)                                                 \
    do {                                                            \
        if (!(cond)) {                                              \
            std::printf("FAIL line %d: %s\n", __LINE__, #cond);     \
            ++failures;                                             \
        }                                                           \
    } while (0)

static std::vector<double> cloud(size_t n, double scale, uint32_t seed) {
    std::vector<double> a(3 * n);
    uint32_t s = seed;
    for (double& v : a) {
        s = s * 1664525u + 1013904223u;
        v = scale * (static_cast<double>(s >> 8) / 16777216.0 - 0.5);
    }
    return a;
}

static ouster_hip_registration_desc desc(int iterations, double max_distance, double kernel) {
    ouster_hip_registration_desc d{};
    d.max_iterations = iterations, d.convergence_criterion = 1e-4, d.max_distance = max_distance, d.kernel_scale = kernel;
    return d;
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    bool uns = false;
    const double one[3] = {0, 0, 0};
    int map_stand_in = 0;
    CHECK(reg_validate(&map_stand_in, one, OUSTER_HIP_F64, 1, 3, 1.0, 0.1, 1e-4, &uns) == nullptr && !uns);
    CHECK(reg_validate(nullptr, one, OUSTER_HIP_F64, 1, 3, 1.0, 0.1, 1e-4, &uns) != nullptr);
    CHECK(reg_validate(&map_stand_in, one, 3, 1, 3, 1.0, 0.1, 1e-4, &uns) != nullptr);
    CHECK(reg_validate(&map_stand_in, one, OUSTER_HIP_F32, 1, 2, 1.0, 0.1, 1e-4, &uns) != nullptr);
    CHECK(reg_validate(&map_stand_in, nullptr, OUSTER_HIP_F32, 1, 0, 1.0, 0.1, 1e-4, &uns) != nullptr);
    CHECK(reg_validate(&map_stand_in, nullptr, OUSTER_HIP_F32, 0, 0, 1.0, 0.1, 1e-4, &uns) == nullptr);
    CHECK(reg_validate(&map_stand_in, one, OUSTER_HIP_F64, (1ull << 30) + 1, 3, 1.0, 0.1, 1e-4, &uns) != nullptr && uns);
    for (double bad : {-1.0, nan, inf, -inf}) {
        CHECK(reg_validate(&map_stand_in, one, OUSTER_HIP_F64, 1, 3, bad, 0.1, 1e-4, &uns) != nullptr && !uns);
        CHECK(reg_validate(&map_stand_in, one, OUSTER_HIP_F64, 1, 3, 1.0, bad, 1e-4, &uns) != nullptr);
        CHECK(reg_validate(&map_stand_in, one, OUSTER_HIP_F64, 1, 3, 1.0, 0.1, bad, &uns) != nullptr);
    }

    // the solve: a diagonal system with a zero pivot, the zero system
    double jtj[36] = {}, jtr[6] = {2, -4, 5, 8, 1, 1}, dx[6];
    const double diag[6] = {2, 4, 0, 8, 1, 0.5};
    for (int i = 0; i < 6; ++i) jtj[7 * i] = diag[i];
    jtj[5] = 123.0;   // the upper triangle is never read
    reg_solve6(jtj, jtr, dx);
    CHECK(dx[0] == -1 && dx[1] == 1 && dx[2] == 0 && dx[3] == -1 && dx[4] == -1 && dx[5] == -2);
    std::memset(jtj, 0, sizeof jtj);
    reg_solve6(jtj, jtr, dx);
    for (double v : dx) CHECK(v == 0.0);

    // SE(3)
    const double shift[6] = {1, -2, 3, 0, 0, 0};
    RegPose p = reg_exp(shift);
    CHECK(p.v[3] == 1.0 && p.v[0] == 0.0 && p.v[4] == 1 && p.v[5] == -2 && p.v[6] == 3);
    const double turn[6] = {0, 0, 0, 0, 0, 1.5707963267948966};
    p = reg_exp(turn);
    double moved[3] = {1, 0, 0};
    reg_apply(p, moved, moved);   // in place
    CHECK(std::fabs(moved[0]) < 1e-15 && std::fabs(moved[1] - 1.0) < 1e-15 && moved[2] == 0.0);
    const RegPose twice = reg_compose(p, p);
    double m16[16];
    reg_matrix(twice, m16);
    CHECK(std::fabs(m16[0] + 1.0) < 1e-15 && std::fabs(m16[5] + 1.0) < 1e-15 && m16[10] == 1.0 && m16[15] == 1.0);
    CHECK(std::fabs(reg_model_error(m16, 10.0) - 20.0) < 1e-12);   // a half turn: the branch without a positive trace
    double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    CHECK(reg_model_error(eye, 100.0) == 0.0);
    eye[3] = 2.0;
    CHECK(reg_model_error(eye, 100.0) == 2.0);

    // the loop
    ouster_hip_voxel_map_desc md{};
    md.voxel_size = 0.5, md.max_distance = 100.0, md.max_points_per_voxel = 20, md.min_pts_threshold = 1;
    HostVoxelMap map(voxel_map_params(&md));
    const std::vector<double> pts = cloud(3000, 8.0, 7);
    ouster_hip_registration_desc d = desc(20, 0.5, 0.1);
    reg_align_ref(map, pts.data(), false, 100, 3, &d);                 // an empty map
    CHECK(d.iterations == 0 && d.pose[0] == 1.0 && d.pose[3] == 0.0 && !d.converged);
    CHECK(map.add_points(pts.data(), false, 3000, 3));
    d = desc(0, 0.5, 0.1);
    reg_align_ref(map, pts.data(), false, 100, 3, &d);                 // no iterations
    CHECK(d.iterations == 0 && d.pose[5] == 1.0);
    d = desc(20, 0.5, 0.1);
    reg_align_ref(map, nullptr, false, 0, 3, &d);                      // no rows
    CHECK(d.iterations == 0);
    // the cloud itself, shifted by centimetres, as strided doubles and as floats
    for (int f32 = 0; f32 < 2; ++f32) {
        const size_t n = 1500, stride = 5;
        std::vector<double> rows64(n * stride, 7.5);
        std::vector<float> rows32(n * stride, 7.5f);
        for (size_t i = 0; i < n; ++i)
            for (int c = 0; c < 3; ++c) {
                const double v = pts[3 * i + c] + (c == 0 ? 0.03 : c == 1 ? -0.02 : 0.01);
                rows64[i * stride + c] = v, rows32[i * stride + c] = (float)v;
            }
        d = desc(50, 0.5, 0.1);
        reg_align_ref(map, f32 ? (const void*)rows32.data() : (const void*)rows64.data(), f32 != 0, n, stride, &d);
        CHECK(d.iterations >= 1 && d.iterations <= 50 && d.correspondences > n / 2);
        CHECK(std::fabs(d.pose[3] + 0.03) < 0.01 && std::fabs(d.pose[7] - 0.02) < 0.01 && std::fabs(d.pose[11] + 0.01) < 0.01);
        CHECK(std::fabs(d.pose[0] - 1.0) < 1e-3 && d.pose[15] == 1.0);
    }
    // one pass with every per-row output, rows that no cell holds among them
    {
        std::vector<double> rows = {pts[0] + 0.01, pts[1], pts[2], nan, 0, 0, 1e300, 0, 0, 500, 500, 500};
        uint8_t flags[4];
        double nb[12], d2[4], sums[REG_SUMS];
        uint64_t count = 0;
        const RegPose identity;
        reg_pass_ref(map, rows.data(), 4, &identity, 0.5, 0.1, flags, nb, d2, sums, &count);
        CHECK(count == 1 && flags[0] == 1 && !flags[1] && !flags[2] && !flags[3] && d2[1] == 0.25 && nb[3] == 0.0);
        for (double s : sums) CHECK(std::isfinite(s));
        double dx6[6];
        RegPose est;
        reg_solve_pass(sums, 1e-4, dx6, &est);
        for (double v : dx6) CHECK(std::isfinite(v));
        double j36[36], r6[6];
        reg_build_linear_system(rows.data(), nb, 1, 0.1, j36, r6);
        CHECK(j36[0] == sums[0] && j36[1] == 0.0 && r6[0] == sums[10]);
        reg_build_linear_system(nullptr, nullptr, 0, 0.1, j36, r6);
        CHECK(j36[0] == 0.0 && r6[5] == 0.0);
    }
    if (failures) {
        std::printf("registration_ref_main: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("registration_ref_main: ok\n");
    return 0;
}
