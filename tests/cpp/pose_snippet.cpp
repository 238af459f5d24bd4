// pose_snippet.cpp -- a C++ caller of interp_pose / transform / dewarp(points, pose) as the reference's users write them, compiled
// against include/ouster/core/pose_util.h by tests/test_pose_api_cpu.py.  Every validation error must arrive as
// std::invalid_argument with the reference's message, with or without a GPU; then the per-x work runs ("ok ...") or is refused
// loudly ("no-gpu").
#include <cmath>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "ouster/core/pose_util.h"
#include "ouster/hip/context.h"

using namespace ouster::sdk::core;

static int failures = 0;

static void expect_invalid(const char* what, const std::string& message, const std::function<void()>& f) {
    try {
        f();
        std::printf("FAIL %s: no exception\n", what);
        ++failures;
    } catch (const std::invalid_argument& e) {
        if (std::string(e.what()).find(message) == std::string::npos) {
            std::printf("FAIL %s: message '%s'\n", what, e.what());
            ++failures;
        }
    } catch (const std::exception& e) {
        std::printf("FAIL %s: wrong exception '%s'\n", what, e.what());
        ++failures;
    }
}

int main() {
    const mat4d eye = mat4d::Identity();
    mat4d b = eye;
    b(0, 0) = std::cos(0.5), b(0, 1) = -std::sin(0.5), b(1, 0) = std::sin(0.5), b(1, 1) = std::cos(0.5);
    b(0, 3) = 1.0, b(1, 3) = 2.0, b(2, 3) = 3.0;
    const std::vector<double> x = {0.0, 0.25, 1.0, 1.5};

    expect_invalid("one pose", "Not enough evaluation poses for interpolation", [&] { interp_pose<double>(x, {1.0}, {eye}); });
    expect_invalid("sizes", "x_known and poses_known sizes are not matching", [&] { interp_pose<double>(x, {1.0, 2.0}, {eye}); });
    expect_invalid("repeated", "input x_known values are not monotonically increasing or values repeated",
                   [&] { interp_pose<double>(x, {1.0, 1.0}, {eye, b}); });
    expect_invalid("last pair", "input x_known values are not monotonically increasing or values repeated",
                   [&] { interp_pose<double>({}, {1.0, 2.0, 3.0, 2.5}, {eye, b, eye, b}); });
    expect_invalid("duration", "Cannot interpolate with zero duration between poses",
                   [&] { interp_pose<double>(x, 1.0, eye, 1.0, b); });
    expect_invalid("x order", "x_interp values must be monotonically increasing: 1.000000 < 2.000000",
                   [&] { interp_pose<double>({0.0, 2.0, 1.0}, {0.0, 5.0}, {eye, b}); });
    expect_invalid("x order, pair", "x_interp values must be monotonically increasing",
                   [&] { interp_pose<double>({2.0, 1.0}, 0.0, eye, 1.0, b); });
    ArrayXXR<float> known_f(3, 16);
    expect_invalid("sizes, flat", "x_known and poses_known sizes are not matching",
                   [&] { interp_pose<double, float>(x, {0.0, 1.0}, known_f); });
    PointCloudXYZd pts(5);
    ArrayXXR<double> bad(5, 3), out4(4, 3);
    expect_invalid("transform rows", "transform: unexpected dimensions", [&] {
        transform<double>(ImgRef<double>(out4), ImgRef<const double>(bad), Vector16d{});
    });
    if (failures) return 1;
    std::printf("validation ok\n");

    Vector16d pose{};
    for (int i = 0; i < 16; ++i) pose[i] = b.m[i];
    for (size_t i = 0; i < pts.rows(); ++i) pts(i, 0) = 1.0 + i, pts(i, 1) = -2.0 * i, pts(i, 2) = 0.5;
    if (ouster::sdk::hip::device_count() == 0) {
        int loud = 0;
        try { interp_pose<double>(x, {0.0, 1.0}, {eye, b}); } catch (const std::runtime_error&) { ++loud; }
        try { interp_pose<double>(x, 0.0, eye, 1.0, b); } catch (const std::runtime_error&) { ++loud; }
        try { transform(pts, pose); } catch (const std::runtime_error&) { ++loud; }
        try { dewarp(pts, pose); } catch (const std::runtime_error&) { ++loud; }
        std::printf("%s: %d of 4 calls refused without a GPU\n", loud == 4 ? "no-gpu" : "FAIL", loud);
        return loud == 4 ? 0 : 1;
    }
    const auto general = interp_pose<double>(x, {0.0, 1.0}, {eye, b});
    const auto pair = interp_pose<double>(x, 0.0, eye, 1.0, b);
    ArrayXXR<double> known_d(2, 16);
    for (int i = 0; i < 16; ++i) known_d(0, i) = eye.m[i], known_d(1, i) = b.m[i];
    const auto flat = interp_pose<double, double>(x, {0.0, 1.0}, known_d);
    ArrayXXR<float> known_f2(2, 16);
    for (int i = 0; i < 16; ++i) known_f2(0, i) = static_cast<float>(eye.m[i]), known_f2(1, i) = static_cast<float>(b.m[i]);
    const auto flat_f = interp_pose<double, float>(x, {0.0, 1.0}, known_f2);
    bool ok = general.size() == 4 && pair.size() == 4 && flat.rows() == 4 && flat_f.rows() == 4;
    for (size_t i = 0; ok && i < 4; ++i) {
        ok = general[i] == pair[i];   // k == 2: the same segment, the same kernel
        for (int e = 0; e < 16; ++e)
            ok = ok && flat(i, e) == general[i].m[e] && std::fabs(flat_f(i, e) - static_cast<float>(general[i].m[e])) <= 1e-5f;
    }
    for (int e = 0; e < 16; ++e) ok = ok && std::fabs(general[2].m[e] - b.m[e]) < 1e-14 && std::fabs(general[0].m[e] - eye.m[e]) < 1e-14;
    const PointCloudXYZd moved = transform(pts, pose), dewarped = dewarp(pts, pose);
    for (size_t i = 0; i < pts.rows(); ++i)
        for (int r = 0; r < 3; ++r) {
            const double want = b(r, 0) * pts(i, 0) + b(r, 1) * pts(i, 1) + b(r, 2) * pts(i, 2) + b(r, 3);
            ok = ok && std::fabs(moved(i, r) - want) < 1e-13 && std::fabs(dewarped(i, r) - want) < 1e-13;
        }
    std::printf("%s\n", ok ? "ok interp_pose transform dewarp" : "FAIL: results");
    return ok ? 0 : 1;
}
