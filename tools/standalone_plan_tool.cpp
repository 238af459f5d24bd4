// standalone_plan_tool -- evaluates the launch plan of the standalone kernels (ouster_sdk_amd/csrc/standalone_plan.cpp) on
// the CPU: g++ only, no HIP header or library.  stdin: one query per line, every name of its form given:
//   destagger row_bytes=N aligned=0|1 rows_env=N h=N n=N
//   cartesian w=N h=N n=N vec_ok=0|1 tile=64|256
//   dewarp    w=N h=N n=N aligned=0|1 tile=64|256
// stdout: the plan of each line as one JSON object.  Driven by tests/test_standalone_plan.py and
// tests/test_gpu_standalone_routes.py (tests/standalone_plan_query.py).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../ouster_sdk_amd/csrc/standalone_plan.h"

using namespace ouster_hip_dev;

namespace {
bool answer(const std::string& kind, std::istringstream& ss) {
    long long row_bytes = -1, aligned = -1, rows_env = -2, h = -1, n = -1, w = -1, vec_ok = -1, tile = -1;
    std::string tok;
    while (ss >> tok) {
        const size_t eq = tok.find('=');
        if (eq == std::string::npos) return false;
        const std::string name = tok.substr(0, eq);
        const long long v = strtoll(tok.c_str() + eq + 1, nullptr, 0);
        if (name == "row_bytes") row_bytes = v;
        else if (name == "aligned") aligned = v;
        else if (name == "rows_env") rows_env = v;
        else if (name == "h") h = v;
        else if (name == "n") n = v;
        else if (name == "w") w = v;
        else if (name == "vec_ok") vec_ok = v;
        else if (name == "tile") tile = v;
        else return false;
    }
    if (kind == "destagger") {
        if (row_bytes < 0 || aligned < 0 || rows_env < -1 || h < 0 || n < 0 || w >= 0 || vec_ok >= 0 || tile >= 0) return false;
        const DestaggerPlan p = plan_destagger((size_t)row_bytes, aligned != 0, (int)rows_env, (uint32_t)h, (uint32_t)n);
        printf("{\"route\":\"%s\",\"rows_per_wg\":%u,\"lds_bytes\":%u,\"grid\":[%u,%u]}\n", destagger_route_name(p.route),
               p.rows_per_wg, p.lds_bytes, p.grid_x, p.grid_y);
        return true;
    }
    if (w < 0 || h < 0 || n < 0 || tile < 0 || row_bytes >= 0 || rows_env != -2) return false;
    TiledPlan p;
    if (kind == "cartesian") {
        if (vec_ok < 0 || aligned >= 0) return false;
        p = plan_cartesian((uint32_t)w, (uint32_t)h, (uint32_t)n, vec_ok != 0, (uint32_t)tile);
    } else if (kind == "dewarp") {
        if (aligned < 0 || vec_ok >= 0) return false;
        p = plan_dewarp((uint32_t)w, (uint32_t)h, (uint32_t)n, aligned != 0, (uint32_t)tile);
    } else {
        return false;
    }
    printf("{\"route\":\"%s\",\"tile_width\":%u,\"rows_per_block\":%u,\"images_per_block\":%u,\"grid\":[%u,%u]}\n",
           p.tiled ? "TILED" : "GENERIC", p.tile_width, p.rows_per_block, p.images_per_block, p.grid_x, p.grid_y);
    return true;
}
}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        std::string kind;
        ss >> kind;
        if (!answer(kind, ss)) {
            fprintf(stderr, "standalone_plan_tool: bad query '%s'\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
