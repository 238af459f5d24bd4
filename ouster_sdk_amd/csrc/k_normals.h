// k_normals.h -- launch interface of the surface-normal kernels (k_normals.hip): the vertical-subtent search per frame and
// algorithm::normals per destaggered pixel.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/ouster_hip.h"
#include "normals_host.h"

namespace ouster_hip_dev {

constexpr uint32_t NORMALS_TILE_W = 64;   // one wave per image row of the tile: its loads are 64 consecutive pixels
constexpr uint32_t NORMALS_TILE_H = 4;    // the rows a workgroup's waves share through L1 / L2 (no LDS halo: any search range)

// what k_normals_subtent leaves per (frame, return): the host applies clamp, acos and the division (normals_host.h)
struct NormalsPair {
    double dot;       // of the two beams, model order, unclamped
    uint32_t rows;    // top - bottom of the winning column; 0: no column has two rows with range
    uint32_t col;     // the winning column (diagnostic)
};
static_assert(sizeof(NormalsPair) == 16, "16 bytes per frame and return");

struct NormalsArgs {
    const void* xyz[2];          // [n_frames][h * w][3] of f32 / f64 per return; [1] nullptr: single return
    const uint32_t* range[2];    // [n_frames][h][w]
    int32_t f32;                 // clouds are float (widened on load) instead of double
    uint32_t n_frames, h, w, n_ret;
    const uint32_t* shifts;      // device [h], reduced to [0, w): inputs are staggered, pixel (u, v) lies at column (v - shift[u]) mod w;
                                 // nullptr: inputs are destaggered
    const double* origins;       // device [w][3], the same for every frame; nullptr: zeros, or from the poses
    const double* poses;         // device [n_frames][w][16]: origin = translation of pose[frame][v] * sensor_to_body
    const double* s2b;           // device [n_s2b][4], the last column of sensor_to_body; frame f uses row f % n_s2b.  Without poses the
    uint32_t n_s2b;              //   origin is the row's first three elements; nullptr (and no poses): zeros
    const double* consts;        // device [n_frames][n_ret][4]: px_res_h, px_res_v, tan_safe, target_sq
    uint32_t pixel_search_range;
    int32_t staggered_out;       // 1: normal (u, v) is written at the pixel's staggered index (only with shifts)
    double* out[2];              // [n_frames][h * w][3] per return; every element is written
    NormalsPair* pairs;          // k_normals_subtent: [n_frames][n_ret]
};

hipError_t launch_normals_subtent(const NormalsArgs& a, hipStream_t st);
hipError_t launch_normals(const NormalsArgs& a, hipStream_t st);

}  // namespace ouster_hip_dev
