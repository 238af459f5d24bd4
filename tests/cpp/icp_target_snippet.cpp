// icp_target_snippet.cpp -- a C++ caller of algorithm::IcpTarget (include/ouster/algorithm/align_clouds.h), compiled with -Werror
// and run by tests/test_icp_target_api_cpu.py.  Every argument error is std::invalid_argument with the C ABI's message and comes
// before a GPU is asked for; a target of fewer than 20 rows needs no GPU and returns every source's guess.  With a GPU the
// reference's two published cases follow through align_many, each result equal to point_to_point_align / point_to_plane_align bit
// for bit; without one the constructor must throw std::runtime_error (no CPU fallback).  Last line: "ok" or "no-gpu".
#include <cmath>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "ouster/algorithm/align_clouds.h"

using namespace ouster::sdk;
using algorithm::IcpTarget;
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

static ArrayX3dR head(const ArrayX3dR& a, size_t n) {
    ArrayX3dR out(n);
    for (size_t i = 0; i < n; ++i) out(i, 0) = a(i, 0), out(i, 1) = a(i, 1), out(i, 2) = a(i, 2);
    return out;
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const ArrayX3dR src = lattice(0, 0, 0), tgt = lattice(0.1, -0.05, 0.025);
    ArrayX3dR nrm(27);
    for (size_t i = 0; i < 27; ++i) nrm(i, 0) = 0, nrm(i, 1) = 0, nrm(i, 2) = 1;
    const ArrayX3dR short_nrm = head(nrm, 26), few = head(tgt, 19), few_nrm = head(nrm, 19);
    const Matrix4dR eye = Matrix4dR::Identity();
    bool ok = true;
    for (double bad : {0.0, -1.0, nan, inf}) {
        ok = ok && refuses("max_corr_dist must be finite and greater than zero", [&] { IcpTarget t(tgt, bad); });
        ok = ok && refuses("max_corr_dist must be finite and greater than zero", [&] { IcpTarget t(tgt, short_nrm, bad); });
    }
    ok = ok && refuses("target_points and target_normals must have the same number of rows", [&] { IcpTarget t(tgt, short_nrm); });
    if (!ok) return 1;

    // small targets need no GPU: the method is fixed by the constructor, and align's refusals come before anything else
    Matrix4dR guess = eye;
    guess(0, 3) = 0.5, guess(1, 2) = -0.25;
    IcpTarget point(few, 0.5), plane(few, few_nrm, 0.5);
    if (point.size() != 19 || point.has_normals() || !plane.has_normals() || point.device_bytes() != 0 || plane.max_corr_dist() != 0.5) return 2;
    for (double bad : {-0.5, 180.5, nan, inf})
        ok = ok && refuses("max_normal_angle_deg must be finite and in [0, 180]", [&] { plane.align(src, nrm, eye, bad); });
    ok = ok && refuses("source_points and source_normals must have the same number of rows", [&] { plane.align(src, short_nrm); });
    ok = ok && refuses("icp_target: source 0 has normals and the target has none", [&] { point.align(src, nrm); });
    ok = ok && refuses("icp_target: source 0 has no normals and the target has them", [&] { plane.align(src, guess); });
    ok = ok && refuses("icp_target: source 1 has normals and the target has none", [&] {
        const std::vector<const double*> p{src.data(), src.data()}, q{nullptr, nrm.data()};
        const std::vector<std::size_t> rows{27, 27};
        double poses[32];
        point.align_arrays(p.data(), rows.data(), q.data(), rows.data(), 2, nullptr, 20.0, poses, nullptr);
    });
    if (!ok) return 3;
    std::printf("validation ok\n");

    std::vector<algorithm::impl::AlignStats> stats;
    const std::vector<Matrix4dR> got = point.align_many({src, tgt}, {guess, eye}, &stats);
    if (got.size() != 2 || !(got[0] == guess) || !(got[1] == eye) || stats.size() != 2 || stats[0].solved || stats[0].iterations != 0) return 4;
    if (!(plane.align(src, nrm, guess) == guess) || !point.align_many({}).empty()) return 5;
    IcpTarget moved(std::move(point));   // move-only
    point = std::move(moved);
    if (point.size() != 19) return 6;
    std::printf("small targets ok\n");

    try {
        IcpTarget t(tgt, 0.5);
        if (t.size() != 27 || t.device_bytes() == 0) return 7;
        const std::vector<Matrix4dR> poses = t.align_many({src, few, src}, {eye, guess, eye}, &stats);
        const Matrix4dR single = algorithm::point_to_point_align(src, tgt, eye, 0.5);
        if (!(poses[0] == single) || !(poses[2] == single) || !(poses[1] == guess) || !stats[0].solved || stats[1].solved) return 8;
        if (std::fabs(single(0, 3) - 0.1) > 1e-10) return 9;
        ArrayX3dR flat(25), lifted(25), up(25);
        for (size_t i = 0; i < 25; ++i) {
            flat(i, 0) = lifted(i, 0) = static_cast<double>(i / 5), flat(i, 1) = lifted(i, 1) = static_cast<double>(i % 5);
            flat(i, 2) = 0.0, lifted(i, 2) = 0.2;
            up(i, 0) = 0, up(i, 1) = 0, up(i, 2) = 1;
        }
        IcpTarget tp(lifted, up, 0.5);
        if (!(tp.align(flat, up) == algorithm::point_to_plane_align(flat, lifted, up, up, eye, 0.5))) return 10;
        std::printf("ok\n");
    } catch (const std::invalid_argument& e) {
        std::printf("unexpected: %s\n", e.what());
        return 11;
    } catch (const std::runtime_error& e) {
        std::printf("no-gpu: %s\n", e.what());
    }
    return 0;
}
