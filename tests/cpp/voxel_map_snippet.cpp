// voxel_map_snippet.cpp -- a C++ caller of core::VoxelHashMap3d as the reference's users write it, compiled against
// include/ouster/core/voxel_hash_map.h by tests/test_voxel_map_api_cpu.py (-Werror).  Every refusal must arrive as
// std::invalid_argument with its message, with or without a GPU; a host map must do every operation without one; then the same
// script runs on the GPU and must give the host map's bytes ("ok"), or the constructor is refused loudly ("no-gpu").
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "ouster/core/voxel_hash_map.h"
#include "ouster/hip/context.h"

using namespace ouster::sdk::core;

static int failures = 0;

static void expect_invalid(const char* what, const std::string& message, const std::function<void()>& f) {
    try {
        f();
        std::printf("FAIL %s: no exception\n", what);
        ++failures;
    } catch (const std::invalid_argument& e) {
        if (std::string(e.what()) != message) {
            std::printf("FAIL %s: message '%s'\n", what, e.what());
            ++failures;
        }
    } catch (const std::exception& e) {
        std::printf("FAIL %s: wrong exception '%s'\n", what, e.what());
        ++failures;
    }
}

static void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAIL %s\n", what);
        ++failures;
    }
}

static ArrayX3dR cloud(std::size_t n, double scale, double shift) {
    ArrayX3dR a(n);
    uint32_t s = 12345u;
    for (std::size_t i = 0; i < 3 * n; ++i) {
        s = s * 1664525u + 1013904223u;
        a.data()[i] = shift + scale * (static_cast<double>(s >> 8) / 16777216.0 - 0.5);
    }
    return a;
}

// every operation once; what they returned, as bytes
static std::vector<double> script(VoxelHashMap3d& m) {
    std::vector<double> out;
    auto keep = [&out](const ArrayX3dR& a) { out.insert(out.end(), a.data(), a.data() + 3 * a.rows()); };
    m.add_points(cloud(700, 8.0, 0.0));
    m.update(cloud(500, 8.0, 1.5), {1.5, 1.5, 1.5});
    keep(m.pointcloud());
    std::vector<double> d2;
    keep(m.get_closest_neighbors(cloud(129, 9.0, 1.0), d2, 2.25));
    out.insert(out.end(), d2.begin(), d2.end());
    const auto one = m.get_closest_neighbor({0.25, -0.5, 1.0});
    out.insert(out.end(), std::get<0>(one).begin(), std::get<0>(one).end());
    out.push_back(std::get<1>(one));
    keep(m.extract_voxels_far_from_location({4.0, 1.5, 1.5}));
    m.remove_voxels_far_from_location({4.5, 1.5, 1.5});
    keep(m.pointcloud());
    out.push_back(static_cast<double>(m.num_voxels()));
    out.push_back(static_cast<double>(m.num_points()));
    m.add_points(std::vector<VoxelHashMap3d::point_type>{{0.1, 0.2, 0.3}, {9.0, 9.0, 9.0}});
    keep(m.pointcloud());
    m.clear();
    out.push_back(m.empty() ? 1.0 : 0.0);
    return out;
}

int main() {
    static_assert(!std::is_copy_constructible<VoxelHashMap3d>::value && std::is_move_constructible<VoxelHashMap3d>::value, "move-only");
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const std::string grid = "voxel map: point outside the int32 voxel grid";
    // the constructor's refusals in the reference's order, before a GPU is asked for
    for (int host = 0; host < 2; ++host) {
        auto make = [host](double v, double d, std::size_t p, std::size_t a) {
            if (host) VoxelHashMap3d::on_host(v, d, p, 1, a);
            else VoxelHashMap3d(v, d, p, 1, a);
        };
        expect_invalid("max_points", "max_points_per_voxel must be greater than 0", [&] { make(0.0, -1.0, 0, 5); });
        expect_invalid("voxel_size", "voxel_size must be greater than 0", [&] { make(0.0, -1.0, 20, 5); });
        expect_invalid("voxel_size nan", "voxel_size must be greater than 0", [&] { make(nan, 100.0, 20, 0); });
        expect_invalid("max_distance", "max_distance must be greater than 0", [&] { make(1.0, 0.0, 20, 5); });
        expect_invalid("max_distance inf", "max_distance must be greater than 0", [&] { make(1.0, inf, 20, 0); });
        expect_invalid("num_attributes", "num_attributes must be 0 for a fixed-size PointType", [&] { make(1.0, 100.0, 20, 5); });
        expect_invalid("range", "voxel map: max_distance / voxel_size exceeds the int32 voxel grid", [&] { make(1e-3, 1e9, 20, 0); });
    }
    std::printf("validation ok\n");

    VoxelHashMap3d host = VoxelHashMap3d::on_host(0.5, 4.0, 3);
    expect(host.empty() && host.device() == -1 && host.max_points_per_voxel() == 3 && host.min_pts_threshold() == 1, "a fresh host map");
    expect(std::get<1>(host.get_closest_neighbor({0.5, 0.5, 0.5})) == std::numeric_limits<double>::max(), "empty map: DBL_MAX");
    ArrayX3dR bad(2);
    bad.data()[3] = nan;
    host.add_points(cloud(10, 1.0, 0.0));
    const std::size_t before = host.num_points();
    expect_invalid("add nan", grid, [&] { host.add_points(bad); });
    expect_invalid("remove inf", grid, [&] { host.remove_voxels_far_from_location({inf, 0, 0}); });
    expect_invalid("extract nan", grid, [&] { host.extract_voxels_far_from_location({0, nan, 0}); });
    expect_invalid("update 1e300", grid, [&] { host.update(cloud(5, 1.0, 0.0), {1e300, 0, 0}); });
    expect_invalid("point_to_voxel", grid, [&] { VoxelHashMap3d::point_to_voxel({nan, 0, 0}, 1.0); });
    expect(host.num_points() == before, "a refused call leaves the map unchanged");
    expect((VoxelHashMap3d::point_to_voxel({-0.5, 1.5, 2.0}, 2.0) == VoxelHashMap3d::voxel_type{-1, 3, 4}), "point_to_voxel");
    host.clear();
    const std::vector<double> want = script(host);
    expect(want.size() > 1000, "the script returns rows");
    VoxelHashMap3d moved = std::move(host);
    expect(moved.empty(), "a moved map");
    std::printf("host map ok\n");

    if (ouster::sdk::hip::device_count() == 0) {
        int loud = 0;
        try { VoxelHashMap3d m(0.5); } catch (const std::runtime_error&) { ++loud; }
        std::printf("%s: the constructor %s without a GPU\n", loud == 1 && !failures ? "no-gpu" : "FAIL", loud ? "is refused" : "succeeds");
        return loud == 1 && !failures ? 0 : 1;
    }
    VoxelHashMap3d gpu(0.5, 4.0, 3);
    expect(gpu.device() >= 0, "a GPU map has a device");
    const std::vector<double> got = script(gpu);
    expect(got.size() == want.size() && std::memcmp(got.data(), want.data(), got.size() * sizeof(double)) == 0, "GPU map == host map, bytes");
    std::printf("%s\n", failures ? "FAIL" : "ok");
    return failures ? 1 : 0;
}
