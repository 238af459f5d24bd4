// k_tonemap.h -- launch interface of the RGB display-image kernels (k_tonemap.hip): luminance percentiles, LocalToneMapper.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/ouster_hip.h"

namespace ouster_hip_dev {

// n_images images of h x w pixels of 3 interleaved elements of in_type (F16 patterns, F32, F64), image i at in + i * in_stride
// ELEMENTS; out_type is F32 or F64 (= T)
struct TonemapArgs {
    const void* in;
    void* out;                                  // k_tm_finish: image i at out + i * out_stride elements of T (may be `in`)
    size_t in_stride, out_stride;
    uint32_t n_images, h, w;
    uint32_t vec;                               // a lane's 4 pixels are three aligned vector accesses on both sides
    const ouster_hip_tonemap_params* params;    // [n_images], device
    uint32_t* hist;                             // [n_images][64][1024] counts, zero before k_tm_hist
    float* luts;                                // [n_images][64][1024]
    uint32_t pieces;                            // k_tm_hist: workgroups per tile (bands of the tile's rows); 0: the launch chooses
    uint32_t grid_x;                            // k_tm_finish: workgroups per image (grid-stride over the pixel quads)
    double lo_percentile, hi_percentile;        // k_tm_lum_percentiles
    uint32_t* n_positive;                       //   [n_images]
    void* lo_hi;                                //   T [n_images][2]
};

constexpr int TM_WG = 256;   // lanes per workgroup of the three tone-map kernels on the device

hipError_t launch_tm_lum_percentiles(const TonemapArgs& a, int in_type, int out_type, hipStream_t st);
// hist -> luts -> finish, in this order on one stream; they fill in a.pieces / a.grid_x themselves
hipError_t launch_tm_hist(TonemapArgs a, int in_type, int out_type, hipStream_t st);
hipError_t launch_tm_luts(const TonemapArgs& a, hipStream_t st);
hipError_t launch_tm_finish(TonemapArgs a, int in_type, int out_type, hipStream_t st);

}  // namespace ouster_hip_dev
