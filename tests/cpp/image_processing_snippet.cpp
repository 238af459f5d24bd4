// A reference caller's "lidar as a camera" step against the mirror: includes ouster/core/image_processing.h and calls both
// update overloads of both classes on img_t lvalues (tests/test_image_api_cpu.py compiles, links and runs it).
// Prints "no-gpu" when the calls refuse for lack of a GPU and leave the images untouched, "ok" when they ran.
#include <cstdio>
#include <cstring>
#include <vector>
#include <stdexcept>

#include "ouster/core/image_processing.h"

using namespace ouster::sdk::core;

int main() {
    img_t<float> f(64, 128);
    img_t<double> d(64, 128);
    for (size_t i = 0; i < f.size(); ++i) {
        f.data()[i] = static_cast<float>(1 + i % 97);
        d.data()[i] = static_cast<double>(1 + i % 89);
    }
    const img_t<float> f0 = f;
    const img_t<double> d0 = d;
    image::BeamUniformityCorrector buc;
    image::AutoExposure ae, ae3(3), ae4(0.05, 0.2, 2, 0.5), ae5(0.05, 0.2, 2);
    (void)ae3; (void)ae4; (void)ae5;
    try {
        buc.update(f);
        ae.update(f);
        ae.update(f, false);
        buc.update(d, true);
        ae.update(d);
    } catch (const std::runtime_error& e) {
        if (!(f == f0) || !(d == d0)) {
            std::printf("image changed by a failed call\n");
            return 2;
        }
        std::printf("no-gpu: %s\n", e.what());
        return 0;
    }
    for (size_t i = 0; i < f.size(); ++i)
        if (!(f.data()[i] >= 0.f && f.data()[i] <= 1.f) || !(d.data()[i] >= 0.0 && d.data()[i] <= 1.0)) {
            std::printf("value outside [0, 1]\n");
            return 3;
        }
    if (buc.dark_count().size() != 64 || !(ae.hi_state() > ae.lo_state())) return 4;
    // foreign memory (a std::vector behind an ImgRef) gives the bits of pool memory (img_t)
    std::vector<float> v(f0.data(), f0.data() + f0.size());
    img_t<float> p = f0;
    image::BeamUniformityCorrector b1, b2;
    image::AutoExposure a1, a2;
    b1.update(p);
    a1.update(p);
    b2.update(ImgRef<float>(v.data(), p.rows(), p.cols()));
    a2.update(ImgRef<float>(v.data(), p.rows(), p.cols()));
    if (std::memcmp(v.data(), p.data(), v.size() * sizeof(float)) != 0 || a1.hi_state() != a2.hi_state()) {
        std::printf("std::vector and img_t differ\n");
        return 5;
    }
    std::printf("ok\n");
    return 0;
}
