// normals_snippet.cpp -- a C++ caller of algorithm::normals as the reference's users write it, compiled against
// include/ouster/algorithm/normals.h by tests/test_normals_api_cpu.py.  Every validation error must arrive as std::runtime_error
// with the reference's message, with or without a GPU; then the 2 x 2 case of the reference's tests runs ("ok ...") or is refused
// loudly ("no-gpu").
#include <cmath>
#include <cstdio>
#include <functional>
#include <stdexcept>
#include <string>

#include "ouster/algorithm/normals.h"
#include "ouster/hip/context.h"

using namespace ouster::sdk::core;
using ouster::sdk::algorithm::normals;

static int failures = 0;

static void expect_runtime(const char* what, const std::string& message, const std::function<void()>& f) {
    try {
        f();
        std::printf("FAIL %s: no exception\n", what);
        ++failures;
    } catch (const std::runtime_error& e) {
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
    PointCloudXYZd xyz(4);
    xyz(1, 0) = 1.0, xyz(2, 1) = 1.0, xyz(3, 0) = 1.0, xyz(3, 1) = 1.0;
    img_t<uint32_t> range(2, 2), wide(1, 4);
    range(0, 1) = range(1, 0) = range(1, 1) = 1;
    const ArrayX3dR origins(2), none(0);
    const PointCloudXYZd three(3);

    expect_runtime("xyz rows", "normals: xyz dimensions mismatch", [&] { normals(three, range, origins); });
    expect_runtime("xyz2 rows", "normals: xyz dimensions mismatch", [&] { normals(xyz, range, three, range, origins); });
    expect_runtime("range2", "normals: range2 dimensions mismatch", [&] { normals(xyz, range, xyz, wide, origins); });
    expect_runtime("origins", "normals: sensor_origins size must match image width", [&] { normals(xyz, range, none); });
    expect_runtime("origins, dual", "normals: sensor_origins size must match image width",
                   [&] { normals(xyz, range, xyz, range, none); });
    expect_runtime("target", "normals: target_distance_m must be positive", [&] { normals(xyz, range, origins, 1, 0.1, -100.0); });
    expect_runtime("target, dual", "normals: target_distance_m must be positive",
                   [&] { normals(xyz, range, xyz, range, origins, 1, 0.1, 0.0); });
    expect_runtime("angle", "normals: min_angle_of_incidence_rad must be positive", [&] { normals(xyz, range, origins, 1, -0.1, 100.0); });
    expect_runtime("angle, dual", "normals: min_angle_of_incidence_rad must be positive",
                   [&] { normals(xyz, range, xyz, range, origins, 1, 0.0, 100.0); });
    if (failures) return 1;
    std::printf("validation ok\n");

    if (ouster::sdk::hip::device_count() == 0) {
        int loud = 0;
        try { normals(xyz, range, origins, 1, 0.1, 100.0); } catch (const std::runtime_error&) { ++loud; }
        try { normals(xyz, range, xyz, range, origins, 1, 0.1, 100.0); } catch (const std::runtime_error&) { ++loud; }
        std::printf("%s: %d of 2 calls refused without a GPU\n", loud == 2 ? "no-gpu" : "FAIL", loud);
        return loud == 2 ? 0 : 1;
    }
    const ArrayX3dR n = normals(xyz, range, origins, 1, 0.1, 100.0);
    const auto both = normals(xyz, range, xyz, range, origins, 1, 0.1, 100.0);
    const double s = std::sqrt(0.5);
    const double want[4][3] = {{0, 0, 0}, {-1, 0, 0}, {0, -1, 0}, {-s, -s, 0}};
    bool ok = n.rows() == 4 && both.first.rows() == 4 && both.second.rows() == 4;
    for (size_t i = 0; ok && i < 4; ++i)
        for (size_t c = 0; c < 3; ++c)
            ok = ok && std::fabs(n(i, c) - want[i][c]) < 1e-8 && std::fabs(both.first(i, c) - want[i][c]) < 1e-8;
    std::printf("%s\n", ok ? "ok normals" : "FAIL: results");
    return ok ? 0 : 1;
}
