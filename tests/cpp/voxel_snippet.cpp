// voxel_snippet.cpp -- a C++ caller of core::voxel_downsample_3d / _xd and algorithm::voxel_downsample_with_normals as the
// reference's users write it, compiled against include/ouster/core/voxel_hash_map.h and include/ouster/algorithm/voxel_downsample.h
// by tests/test_voxel_api_cpu.py.  Every validation error must arrive as std::invalid_argument with the reference's message, with
// or without a GPU, and the two host-routed combinations must work without one; then the reference's recorded case runs ("ok ...")
// or is refused loudly ("no-gpu").
#include <cstdio>
#include <functional>
#include <limits>
#include <stdexcept>
#include <string>

#include "ouster/algorithm/voxel_downsample.h"
#include "ouster/core/voxel_hash_map.h"
#include "ouster/hip/context.h"

using namespace ouster::sdk::core;
using ouster::sdk::algorithm::voxel_downsample_with_normals;

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

int main() {
    const double rows[4][5] = {{0, 1, 0, 10, 100}, {0, 1, 0, 12, 102}, {0, 2, 0, 20, 200}, {0, 2, 0, 22, 202}};
    ArrayXXdR frame(4, 5);
    ArrayX3dR cloud(4), normals(4);
    for (size_t i = 0; i < 4; ++i) {
        for (size_t c = 0; c < 5; ++c) frame(i, c) = rows[i][c];
        for (size_t c = 0; c < 3; ++c) cloud(i, c) = rows[i][c];
        normals(i, 2) = 2.0;
    }
    const auto AVG = VoxelDownsampleStrategy::AVERAGE_POINT;
    const double nan = std::numeric_limits<double>::quiet_NaN();

    if (voxel_downsample_3d(ArrayX3dR(0), -1.0, 0).rows() != 0 || voxel_downsample_xd(ArrayXXdR(0, 2), -1.0, 0).cols() != 2) {
        std::printf("FAIL: an empty frame comes back empty before any check\n");
        return 1;
    }
    expect_invalid("xd columns", "voxel_downsample_xd: frame must be Nx>=3 (x,y,z + optional attributes)",
                   [&] { voxel_downsample_xd(ArrayXXdR(2, 2), 1.0); });
    expect_invalid("max points first", "max_points_per_voxel must be greater than 0", [&] { voxel_downsample_xd(frame, -1.0, 0); });
    expect_invalid("max points, 3d", "max_points_per_voxel must be greater than 0", [&] { voxel_downsample_3d(cloud, 1.0, 0, 1, AVG); });
    expect_invalid("voxel size", "voxel_size must be greater than 0", [&] { voxel_downsample_3d(cloud, 0.0); });
    expect_invalid("voxel size nan", "voxel_size must be greater than 0", [&] { voxel_downsample_xd(frame, nan, 1, 1, AVG); });
    expect_invalid("voxel size, host route", "voxel_size must be greater than 0", [&] { voxel_downsample_xd(frame, -2.0, 3); });
    expect_invalid("with normals rows", "voxel_downsample_with_normals points/normals size mismatch",
                   [&] { voxel_downsample_with_normals(cloud, ArrayX3dR(3), 1.0); });
    expect_invalid("with normals size", "voxel_downsample_with_normals voxel_size must be > 0",
                   [&] { voxel_downsample_with_normals(cloud, normals, 0.0); });
    expect_invalid("with normals, rows before size", "voxel_downsample_with_normals points/normals size mismatch",
                   [&] { voxel_downsample_with_normals(cloud, ArrayX3dR(5), -1.0); });
    {   // the host-routed combinations refuse a point outside the grid without a GPU as well
        ArrayX3dR far = cloud;
        far(2, 0) = 1e13;
        expect_invalid("grid", "voxel_downsample: point outside the int32 voxel grid",
                       [&] { voxel_downsample_3d(far, 0.5, 2, 1, VoxelDownsampleStrategy::FIRST_N_POINT); });
    }
    if (failures) return 1;
    std::printf("validation ok\n");

    // FIRST_N_POINT / RANDOM keeping several points: host code, with or without a GPU.  resolution^2 = 16 / 2: the second point
    // is the first one again (refused), the third is 1 away (refused): one row; RANDOM keeps two of the four
    const ArrayXXdR first = voxel_downsample_xd(frame, 4.0, 2, 1, VoxelDownsampleStrategy::FIRST_N_POINT);
    const ArrayX3dR random = voxel_downsample_3d(cloud, 4.0, 2, 1, VoxelDownsampleStrategy::RANDOM);
    if (first.rows() != 1 || first.cols() != 5 || first(0, 3) != 10.0 || random.rows() != 2) {
        std::printf("FAIL: host-routed combinations (%zu x %zu, %zu rows)\n", first.rows(), first.cols(), random.rows());
        return 1;
    }
    std::printf("host route ok\n");

    if (ouster::sdk::hip::device_count() == 0) {
        int loud = 0;
        try { voxel_downsample_xd(frame, 4.0, 1, 1, AVG); } catch (const std::runtime_error&) { ++loud; }
        try { voxel_downsample_3d(cloud, 4.0); } catch (const std::runtime_error&) { ++loud; }
        try { voxel_downsample_with_normals(cloud, normals, 4.0); } catch (const std::runtime_error&) { ++loud; }
        std::printf("%s: %d of 3 calls refused without a GPU\n", loud == 3 ? "no-gpu" : "FAIL", loud);
        return loud == 3 ? 0 : 1;
    }
    const ArrayXXdR two = voxel_downsample_xd(frame, 0.1, 1, 1, AVG), one = voxel_downsample_xd(frame, 4.0, 1, 1, AVG);
    const auto wn = voxel_downsample_with_normals(cloud, normals, 4.0);
    const bool ok = two.rows() == 2 && two(0, 1) == 1.0 && two(0, 3) == 11.0 && two(1, 1) == 2.0 && two(1, 4) == 201.0 &&
                    one.rows() == 1 && one(0, 1) == 1.5 && one(0, 3) == 16.0 && one(0, 4) == 151.0 &&
                    voxel_downsample_3d(cloud, 0.1).rows() == 2 && wn.first.rows() == 1 && wn.first(0, 1) == 1.5 &&
                    wn.second(0, 2) == 1.0 && wn.second(0, 0) == 0.0;
    std::printf("%s\n", ok ? "ok voxel_downsample" : "FAIL: results");
    return ok ? 0 : 1;
}
