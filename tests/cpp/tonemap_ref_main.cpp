// tonemap_ref_main.cpp -- the host half of the display images (csrc/host/image_processing.cpp) on its own: the state machines of
// LocalToneMapper, AutoExposure and BeamUniformityCorrector driven through step() over a brightness sweep, and update() against a
// device half that refuses, as it does without a GPU.  No GPU, no library: the C ABI calls the file makes are stubs here.
// `make sanitized` in this directory builds it with -fsanitize=address,undefined and runs it with the others of its kind, the way to run a
// sanitizer over that code.
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "ouster/core/image_processing.h"
#include "ouster_hip.h"

// ---- the device half, absent: every call fails the way it does without a GPU ---------------------------------------------------
namespace ouster { namespace sdk { namespace hip {
void check(int rc) { if (rc != OUSTER_HIP_OK) throw std::runtime_error("no device"); }
ouster_hip_ctx* default_ctx() { throw std::runtime_error("no device"); }
}}}
extern "C" {
int ouster_hip_copy_in(ouster_hip_ctx*, void*, const void*, size_t) { return OUSTER_HIP_ERR_NO_DEVICE; }
int ouster_hip_copy_out(ouster_hip_ctx*, void*, const void*, size_t) { return OUSTER_HIP_ERR_NO_DEVICE; }
int ouster_hip_ctx_scratch(ouster_hip_ctx*, uint32_t, size_t, void**) { return OUSTER_HIP_ERR_NO_DEVICE; }
int ouster_hip_sync(ouster_hip_ctx*) { return OUSTER_HIP_ERR_NO_DEVICE; }
int ouster_hip_image_dark_rows(ouster_hip_ctx*, const void*, int, int, uint32_t, uint32_t, uint32_t, size_t, void*, uint32_t*) { return OUSTER_HIP_ERR_NO_DEVICE; }
int ouster_hip_image_percentiles(ouster_hip_ctx*, const void*, int, int, uint32_t, uint32_t, uint32_t, size_t, const void*, double, double, uint32_t*, void*) { return OUSTER_HIP_ERR_NO_DEVICE; }
int ouster_hip_image_apply(ouster_hip_ctx*, const void*, int, void*, int, uint32_t, uint32_t, uint32_t, size_t, size_t, const void*, const ouster_hip_image_map*) { return OUSTER_HIP_ERR_NO_DEVICE; }
int ouster_hip_image_dark_rows_host(ouster_hip_ctx*, const void*, int, uint32_t, uint32_t, void*, uint32_t*) { return OUSTER_HIP_ERR_NO_DEVICE; }
int ouster_hip_image_percentiles_host(ouster_hip_ctx*, const void*, int, uint32_t, uint32_t, const void*, double, double, uint32_t*, void*) { return OUSTER_HIP_ERR_NO_DEVICE; }
int ouster_hip_image_apply_host(ouster_hip_ctx*, void*, int, uint32_t, uint32_t, const void*, const ouster_hip_image_map*) { return OUSTER_HIP_ERR_NO_DEVICE; }
int ouster_hip_image_lum_percentiles(ouster_hip_ctx*, const void*, int, int, uint32_t, uint32_t, uint32_t, size_t, double, double, uint32_t*, void*) { return OUSTER_HIP_ERR_NO_DEVICE; }
int ouster_hip_image_tonemap(ouster_hip_ctx*, const void*, int, void*, int, uint32_t, uint32_t, uint32_t, size_t, size_t, const ouster_hip_tonemap_params*) { return OUSTER_HIP_ERR_NO_DEVICE; }
int ouster_hip_image_lum_percentiles_host(ouster_hip_ctx*, const void*, int, int, uint32_t, uint32_t, double, double, uint32_t*, void*) { return OUSTER_HIP_ERR_NO_DEVICE; }
int ouster_hip_image_tonemap_host(ouster_hip_ctx*, const void*, int, void*, int, uint32_t, uint32_t, const ouster_hip_tonemap_params*) { return OUSTER_HIP_ERR_NO_DEVICE; }
int ouster_hip_image_apply_rgb_host(ouster_hip_ctx*, const void*, int, void*, int, uint32_t, uint32_t, const ouster_hip_image_map*) { return OUSTER_HIP_ERR_NO_DEVICE; }
}

using namespace ouster::sdk::core;

int main() {
    const double levels[12] = {0.03, 0.08, 0.25, 0.7, 2.0, 5.0, 2.0, 0.7, 0.25, 0.08, 0.03, 0.02};
    image::LocalToneMapper mappers[4] = {image::LocalToneMapper(), image::LocalToneMapper(3), image::LocalToneMapper(0.1, 0.2, 1, 0.3, 0.2, false),
                                         image::LocalToneMapper(0.0, 0.1, 2, 0.5, false, true)};
    bool compress = false, ramp = false, full = false, zero = false, none = false, scale = false, affine = false;
    for (image::LocalToneMapper& m : mappers)
        for (int i = 0; i < 12; ++i) {
            ouster_hip_tonemap_params p;
            const bool update = i != 3 && i != 8;
            if (i == 7) m.step(60, 0.5, 0.5, update, p);                          // too few samples: the early return
            else if (i == 0) m.step(512, levels[i], levels[i], update, p);        // lo == hi: the map by hi alone
            else m.step(512, 0.15 * levels[i], 3.0 * levels[i], update, p);
            none |= p.map.mode == OUSTER_HIP_IMAGE_MAP_NONE;
            scale |= p.map.mode == OUSTER_HIP_IMAGE_MAP_SCALE;
            affine |= p.map.mode == OUSTER_HIP_IMAGE_MAP_AFFINE;
            if (p.map.mode == OUSTER_HIP_IMAGE_MAP_NONE) continue;
            if (!std::isfinite(p.map.mul) || !(p.color_ramp >= 0.0 && p.color_ramp <= 1.0)) return 1;
            compress |= p.compress != 0;
            zero |= p.color_ramp == 0.0;
            ramp |= p.color_ramp > 0.0 && p.color_ramp < 1.0;
            full |= p.color_ramp == 1.0;
        }
    if (!(compress && ramp && full && zero && none && scale && affine)) {
        std::printf("a branch of LocalToneMapper::step was not reached\n");
        return 2;
    }
    image::AutoExposure ae(0.1, 0.1, 2, 0.5);
    for (int i = 0; i < 12; ++i) {
        ouster_hip_image_map map;
        ae.step(i == 7 ? 60 : 512, 0.15 * levels[i], 3.0 * levels[i], i != 3, map);
    }
    if (!ae.initialized() || !(ae.hi_state() > ae.lo_state())) return 3;
    image::BeamUniformityCorrector buc;
    std::vector<float> med(31);
    for (int k = 0; k < 10; ++k) {
        for (size_t i = 0; i < med.size(); ++i) med[i] = 0.25f * static_cast<float>((i + k) % 5) - 0.5f;
        if (buc.wants_dark_rows(32, true)) buc.step<float>(med.data(), 64, 32, true);
        else buc.step_keep();
    }
    if (buc.dark_count().size() != 32) return 4;
    // update() without a device: the argument errors first, then the refusal, and the images as they were
    std::vector<float> img(16 * 16 * 3, 0.5f), out(16 * 16 * 3, -7.25f);
    std::vector<float16_t> half(16 * 16 * 3);
    int refused = 0, invalid = 0;
    auto attempt = [&](auto&& f) {
        try { f(); } catch (const std::invalid_argument&) { ++invalid; } catch (const std::runtime_error&) { ++refused; }
    };
    attempt([&] { mappers[0].update(RgbImgRef<float>(img.data(), 7, 16)); });
    attempt([&] { mappers[0].update(RgbImgRef<const float16_t>(half.data(), 16, 16), RgbImgRef<float>(out.data(), 16, 8)); });
    attempt([&] { mappers[0].update(RgbImgRef<float>(img.data(), 16, 16)); });
    attempt([&] { mappers[0].update(RgbImgRef<const float16_t>(half.data(), 16, 16), RgbImgRef<float>(out.data(), 16, 16)); });
    attempt([&] { ae.update(RgbImgRef<float>(img.data(), 16, 16)); });
    attempt([&] { ae.update(ImgRef<float>(img.data(), 16, 48)); });
    for (float v : img) if (v != 0.5f) return 5;
    for (float v : out) if (v != -7.25f) return 5;
    if (invalid != 2 || refused != 4) return 6;
    std::printf("ok\n");
    return 0;
}
