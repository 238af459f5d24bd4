// icp_snippet.cpp -- a C++ caller of include/ouster/algorithm/align_clouds.h, compiled with -Werror and run by
// tests/test_icp_api_cpu.py.  Every error is std::invalid_argument with the reference's message and comes before a GPU is asked for;
// clouds of fewer than 20 rows return the guess without one.  With a GPU the reference's two published cases follow, within its own
// tolerances; without one the call must throw std::runtime_error (no CPU fallback).  Last line: "ok" or "no-gpu".
#include <cmath>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>

#include "ouster/algorithm/align_clouds.h"

using namespace ouster::sdk;
using core::ArrayX3dR;
using core::Matrix4dR;

template <class F>
static bool refuses(const char* message, F f) {
    try {
        f();
    } catch (const std::invalid_argument& e) {
        if (std::string(e.what()) == message) return true;
        std::printf("wrong message: %s (want %s)\n", e.what(), message);
        return false;
    } catch (const std::exception& e) {
        std::printf("wrong exception: %s (want %s)\n", e.what(), message);
        return false;
    }
    std::printf("no exception (want %s)\n", message);
    return false;
}

static ArrayX3dR lattice(double dx, double dy, double dz) {
    ArrayX3dR a(27);
    size_t i = 0;
    for (int x = -1; x <= 1; ++x)
        for (int y = -1; y <= 1; ++y)
            for (int z = -1; z <= 1; ++z, ++i) a(i, 0) = x + dx, a(i, 1) = y + dy, a(i, 2) = z + dz;
    return a;
}

static bool near_pose(const Matrix4dR& m, double tx, double ty, double tz, double rot_tol, double t_tol) {
    bool ok = true;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) ok = ok && std::fabs(m(i, j) - (i == j ? 1.0 : 0.0)) <= rot_tol;
    return ok && std::fabs(m(0, 3) - tx) <= t_tol && std::fabs(m(1, 3) - ty) <= t_tol && std::fabs(m(2, 3) - tz) <= t_tol;
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const ArrayX3dR src = lattice(0, 0, 0), tgt = lattice(0.1, -0.05, 0.025);
    ArrayX3dR nrm(27), short_nrm(26);
    for (size_t i = 0; i < 27; ++i) nrm(i, 0) = 0, nrm(i, 1) = 0, nrm(i, 2) = 1;
    const Matrix4dR eye = Matrix4dR::Identity();
    bool ok = true;
    for (double bad : {0.0, -1.0, nan, inf}) {
        ok = ok && refuses("max_corr_dist must be finite and greater than zero", [&] { algorithm::point_to_point_align(src, tgt, eye, bad); });
        ok = ok && refuses("max_corr_dist must be finite and greater than zero",
                           [&] { algorithm::point_to_plane_align(src, tgt, short_nrm, nrm, eye, bad, -1.0); });
    }
    for (double bad : {-0.5, 180.5, nan, inf})
        ok = ok && refuses("max_normal_angle_deg must be finite and in [0, 180]",
                           [&] { algorithm::point_to_plane_align(src, tgt, short_nrm, nrm, eye, 0.25, bad); });
    ok = ok && refuses("source_points and source_normals must have the same number of rows",
                       [&] { algorithm::point_to_plane_align(src, tgt, short_nrm, short_nrm); });
    ok = ok && refuses("target_points and target_normals must have the same number of rows",
                       [&] { algorithm::point_to_plane_align(src, tgt, nrm, short_nrm); });
    if (!ok) return 1;
    std::printf("validation ok\n");

    // 19 rows: the guess, bit for bit, on any machine
    Matrix4dR guess = eye;
    guess(0, 3) = 0.5, guess(1, 2) = -0.25;
    ArrayX3dR few(19);
    for (size_t i = 0; i < 19; ++i) few(i, 0) = src(i, 0), few(i, 1) = src(i, 1), few(i, 2) = src(i, 2);
    if (!(algorithm::point_to_point_align(few, tgt, guess, 0.5) == guess) || !(algorithm::point_to_point_align(src, few, guess, 0.5) == guess))
        return 2;
    std::printf("small clouds ok\n");

    try {
        const Matrix4dR p = algorithm::point_to_point_align(src, tgt, eye, 0.5);
        if (!near_pose(p, 0.1, -0.05, 0.025, 1e-10, 1e-10)) return 3;
        ArrayX3dR plane(25), moved(25), up(25);
        for (size_t i = 0; i < 25; ++i) {
            plane(i, 0) = moved(i, 0) = static_cast<double>(i / 5), plane(i, 1) = moved(i, 1) = static_cast<double>(i % 5);
            plane(i, 2) = 0.0, moved(i, 2) = 0.2;
            up(i, 0) = 0, up(i, 1) = 0, up(i, 2) = 1;
        }
        const Matrix4dR q = algorithm::point_to_plane_align(plane, moved, up, up, eye, 0.5);
        if (!near_pose(q, 0.0, 0.0, 0.2, 1e-10, 1e-9)) return 4;
        std::printf("ok\n");
    } catch (const std::invalid_argument&) {
        return 5;
    } catch (const std::runtime_error& e) {
        std::printf("no-gpu: %s\n", e.what());
    }
    return 0;
}
