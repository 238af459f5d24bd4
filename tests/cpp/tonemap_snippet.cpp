// A reference caller's colour-camera step against the mirror: includes ouster/core/image_processing.h and calls every RGB
// overload of AutoExposure and LocalToneMapper (tests/test_tonemap_api_cpu.py compiles, links and runs it).
//   tonemap_snippet                       prints "no-gpu" when the calls refuse for lack of a GPU and leave the images untouched,
//                                         "ok" when they ran; argument errors must surface either way
//   tonemap_snippet steps <in> <out>      the host half alone (no GPU needed): feeds recorded (n, lo, hi) to step()
// steps input: u32 kind (0 LocalToneMapper / 1 AutoExposure), u32 update_every, u32 color_correct, u32 calls, f64 lo_percentile,
// hi_percentile, damping, compress_dr_max_lum; per call u32 n, u32 update_state, f64 lo, hi.
// steps output per call: the record (ouster_hip_tonemap_params / ouster_hip_image_map), f64 lo_state, hi_state.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "ouster/core/image_processing.h"
#include "ouster_hip.h"

using namespace ouster::sdk::core;

static int steps(const char* in_path, const char* out_path) {
    FILE* f = std::fopen(in_path, "rb");
    uint32_t hd[4];
    double cfg[4];
    if (!f || std::fread(hd, 4, 4, f) != 4 || std::fread(cfg, 8, 4, f) != 4) return 2;
    image::LocalToneMapper ltm(cfg[0], cfg[1], static_cast<int>(hd[1]), cfg[2], cfg[3], hd[2] != 0);
    image::AutoExposure ae(cfg[0], cfg[1], static_cast<int>(hd[1]), cfg[2]);
    FILE* o = std::fopen(out_path, "wb");
    if (!o) return 2;
    for (uint32_t i = 0; i < hd[3]; ++i) {
        uint32_t nu[2];
        double lh[2];
        if (std::fread(nu, 4, 2, f) != 2 || std::fread(lh, 8, 2, f) != 2) return 2;
        double st[2];
        if (hd[0] == 0) {
            ouster_hip_tonemap_params p;
            ltm.step(nu[0], lh[0], lh[1], nu[1] != 0, p);
            std::fwrite(&p, sizeof p, 1, o);
            st[0] = ltm.lo_state(), st[1] = ltm.hi_state();
        } else {
            ouster_hip_image_map m;
            std::memset(&m, 0, sizeof m);
            ae.step(nu[0], lh[0], lh[1], nu[1] != 0, m);
            std::fwrite(&m, sizeof m, 1, o);
            st[0] = ae.lo_state(), st[1] = ae.hi_state();
        }
        std::fwrite(st, 8, 2, o);
    }
    std::fclose(f);
    std::fclose(o);
    return 0;
}

template <typename F>
static bool refuses(F&& f) {
    try {
        f();
    } catch (const std::invalid_argument&) {
        return true;
    } catch (const std::exception&) {
    }
    return false;
}

int main(int argc, char** argv) {
    if (argc == 4 && std::strcmp(argv[1], "steps") == 0) return steps(argv[2], argv[3]);
    const size_t h = 32, w = 64;
    std::vector<float> f(h * w * 3);
    std::vector<double> d(h * w * 3);
    std::vector<float16_t> half(h * w * 3);
    for (size_t i = 0; i < f.size(); ++i) {
        f[i] = 0.01f * static_cast<float>(1 + i % 97);
        d[i] = 0.01 * static_cast<double>(1 + i % 89);
        half[i].bits = static_cast<uint16_t>(0x3000 + i % 2048);
    }
    const std::vector<float> f0 = f;
    const std::vector<double> d0 = d;
    std::vector<float> out(f.size(), -7.25f);
    image::LocalToneMapper ltm, ltm3(3), ltm_b(0.0, 0.2, 1, 0.3, true, false), ltm_d(0.0, 0.2, 1, 0.3, 0.25, true);
    image::AutoExposure ae;
    (void)ltm3; (void)ltm_b; (void)ltm_d;
    // argument errors need no GPU, and nothing is written
    if (!refuses([&] { ltm.update(RgbImgRef<float>(f.data(), 7, 64)); }) || !refuses([&] { ltm.update(RgbImgRef<double>(d.data(), 64, 7)); }) ||
        !refuses([&] { ltm.update(RgbImgRef<const float16_t>(half.data(), h, w), RgbImgRef<float>(out.data(), h, w / 2)); }) ||
        !refuses([&] { ae.update(RgbImgRef<const float16_t>(half.data(), h, w), RgbImgRef<float>(out.data(), h / 2, w)); }) ||
        f != f0 || d != d0 || out[0] != -7.25f || ltm.initialized() || ae.initialized()) {
        std::printf("an argument error did not surface\n");
        return 6;
    }
    try {
        ltm.update(RgbImgRef<float>(f.data(), h, w));
        ltm.update(RgbImgRef<float>(f.data(), h, w), false);
        ltm.update(RgbImgRef<double>(d.data(), h, w));
        ltm.update(RgbImgRef<const float16_t>(half.data(), h, w), RgbImgRef<float>(out.data(), h, w));
        ae.update(RgbImgRef<const float16_t>(half.data(), h, w), RgbImgRef<float>(out.data(), h, w));
        std::vector<float> g = f0;
        std::vector<double> e = d0;
        ae.update(RgbImgRef<float>(g.data(), h, w));
        ae.update(RgbImgRef<double>(e.data(), h, w), true);
    } catch (const std::runtime_error& e) {
        if (f != f0 || d != d0 || out[0] != -7.25f) {
            std::printf("image changed by a failed call\n");
            return 2;
        }
        std::printf("no-gpu: %s\n", e.what());
        return 0;
    }
    for (size_t i = 0; i < f.size(); ++i)
        if (!(f[i] >= 0.f && f[i] <= 1.f) || !(d[i] >= 0.0 && d[i] <= 1.0) || !(out[i] >= 0.f && out[i] <= 1.f)) {
            std::printf("value outside [0, 1]\n");
            return 3;
        }
    if (!(ltm.hi_state() > ltm.lo_state()) || !ae.initialized()) return 4;
    std::printf("ok\n");
    return 0;
}
