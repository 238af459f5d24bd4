// k_image.h -- launch interface of the display-image kernels (k_image.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/ouster_hip.h"

namespace ouster_hip_dev {

constexpr uint32_t IMAGE_MAX_W_DARK = 4096;   // k_img_dark_rows keeps one row of keys in LDS: 4096 doubles = 32 KB

// n_images images of h x w elements of in_type, image i at in + i * in_stride elements; out_type is F32 or F64 (= T)
struct ImageArgs {
    const void* in;
    void* out;                           // k_img_apply only: image i at out + i * out_stride elements of T
    size_t in_stride, out_stride;
    uint32_t n_images, h, w;
    uint32_t vec;                        // 4-element vector loads (and stores) are aligned for every image
    uint64_t* col_mask;                  // [n_images][(w + 63) / 64]: bit c set when column c holds a non-zero pixel
    void* medians;                       // k_img_dark_rows: T [n_images][h - 1]
    uint32_t* n_cols;                    // k_img_dark_rows: [n_images] (nullable)
    const void* dark;                    // T [n_images][h] dark counts (nullable)
    double lo_percentile, hi_percentile;
    uint32_t* n_positive;                // k_img_percentiles: [n_images]
    void* lo_hi;                         // k_img_percentiles: T [n_images][2]
    const ouster_hip_image_map* maps;    // k_img_apply: [n_images] (nullable: dark counts only)
};

hipError_t launch_image_dark_rows(const ImageArgs& a, int in_type, int out_type, hipStream_t st);
hipError_t launch_image_percentiles(const ImageArgs& a, int in_type, int out_type, hipStream_t st);
hipError_t launch_image_apply(const ImageArgs& a, int in_type, int out_type, hipStream_t st);

}  // namespace ouster_hip_dev
