// normals_lanes.cpp -- csrc/k_normals.hip compiled for the CPU (tests/cpp/host_lanes/hip/hip_runtime.h: one thread per lane) and
// driven the way ouster_hip_normals drives it: k_normals_subtent, the host's constants per (frame, return), k_normals.  Built and
// run by tests/test_normals_lanes_cpu.py, which compares the result with tests/normals_model.py bit for bit.
//   normals_lanes <case file> <result file>
// case file: u32 n_frames h w dual f32 pixel_search_range has_shifts origin_mode(0 zeros, 1 array, 2 poses) staggered_out, then
// xyz, range [, xyz2, range2] [, reduced shifts u32[h]] [, origins f64[w][3] | poses f64[n][w][16], sensor_to_body f64[16]].
#include "../../ouster_sdk_amd/csrc/k_normals.hip"

#include "host_lanes/lanes_util.h"

namespace ouster_hip_dev {
int fail_msg(int code, const char*) { return code; }
}  // namespace ouster_hip_dev
using namespace ouster_hip_dev;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    uint32_t hd[9];
    if (!f || !rd(hd, sizeof hd, f)) return 2;
    const uint32_t n = hd[0], h = hd[1], w = hd[2], dual = hd[3], f32 = hd[4], psr = hd[5], hs = hd[6], om = hd[7], so = hd[8];
    const size_t px = (size_t)n * h * w, es = f32 ? 4 : 8;
    std::vector<uint8_t> x1(px * 3 * es), x2(px * 3 * es);
    std::vector<uint32_t> r1(px), r2(px), sh(h);
    std::vector<double> org((size_t)w * 3), poses((size_t)n * w * 16), s2b(16), o1(px * 3, 7.0), o2(px * 3, 7.0);
    bool ok = rd(x1.data(), x1.size(), f) && rd(r1.data(), px * 4, f);
    if (dual) ok = ok && rd(x2.data(), x2.size(), f) && rd(r2.data(), px * 4, f);
    if (hs) ok = ok && rd(sh.data(), (size_t)h * 4, f);
    if (om == 1) ok = ok && rd(org.data(), org.size() * 8, f);
    if (om == 2) ok = ok && rd(poses.data(), poses.size() * 8, f) && rd(s2b.data(), 128, f);
    std::fclose(f);
    if (!ok) return 2;
    NormalsArgs a{};
    a.xyz[0] = x1.data(), a.range[0] = r1.data(), a.out[0] = o1.data();
    if (dual) a.xyz[1] = x2.data(), a.range[1] = r2.data(), a.out[1] = o2.data();
    a.f32 = (int32_t)f32, a.n_frames = n, a.h = h, a.w = w, a.n_ret = dual ? 2 : 1;
    a.shifts = hs ? sh.data() : nullptr;
    a.origins = om == 1 ? org.data() : nullptr;
    a.poses = om == 2 ? poses.data() : nullptr;
    double last_col[4];
    for (int r = 0; r < 4; ++r) last_col[r] = s2b[4 * r + 3];
    if (om == 2) a.s2b = last_col, a.n_s2b = 1;
    a.pixel_search_range = std::min(psr, std::max(h, w));
    a.staggered_out = hs && so;
    std::vector<NormalsPair> pairs((size_t)n * a.n_ret);
    std::vector<double> k((size_t)n * a.n_ret * 4);
    a.pairs = pairs.data(), a.consts = k.data();
    if (launch_normals_subtent(a, nullptr) != hipSuccess) return 3;
    const double angle = 1 * M_PI / 180.0, target = 0.025;   // the defaults of normals.h
    for (uint32_t fr = 0; fr < n; ++fr) {
        ouster_hip_normals_consts c0, c;
        const NormalsPair& p0 = pairs[(size_t)fr * a.n_ret];
        normals_constants(w, h, angle, target, p0.rows != 0, p0.dot, p0.rows, &c0);
        for (uint32_t r = 0; r < a.n_ret; ++r) {
            c = c0;
            if (r == 1 && !(c0.subtent > 0.0)) {
                const NormalsPair& p1 = pairs[(size_t)fr * a.n_ret + 1];
                normals_constants(w, h, angle, target, p1.rows != 0, p1.dot, p1.rows, &c);
            }
            double* row = k.data() + ((size_t)fr * a.n_ret + r) * 4;
            row[0] = c.px_res_h, row[1] = c.px_res_v, row[2] = c.tan_safe, row[3] = c.target_sq;
        }
    }
    if (launch_normals(a, nullptr) != hipSuccess) return 3;
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    std::fwrite(o1.data(), 8, px * 3, f);
    if (dual) std::fwrite(o2.data(), 8, px * 3, f);
    std::fclose(f);
    return 0;
}
