// k_frame_ops.h -- launch interface of the frame_ops kernels (k_frame_ops.hip): clip, invalidate, select_rows.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/ouster_hip.h"

namespace ouster_hip_dev {

constexpr uint32_t FOPS_MAX_PLANES = 32;   // planes of one launch (they travel in the kernel arguments); longer lists are split
constexpr uint32_t FOPS_GROUP = 16;        // pixels per thread step: one 16-byte chunk of a u8 plane, eight of a u64 plane

struct FopsPlane {
    void* data;              // image i at data + i * stride elements
    void* twin;              // invalidate: the destaggered copy of the same images (nullable)
    size_t stride;           // elements between images
    uint64_t invalid_bits;   // bit pattern of static_cast<T>(invalid) in the low elem bytes
    uint32_t elem;           // 1, 2, 4, 8; invalidate also 12 / 24: a cloud of 3 floats / doubles per pixel, zeroed
    int32_t type;            // OUSTER_HIP_* (clip converts to double by it)
};

struct FopsClipArgs {
    FopsPlane planes[FOPS_MAX_PLANES];
    uint32_t n_planes, n_images, hw;
    double lower, upper;
};

struct FopsInvalidateArgs {
    FopsPlane planes[FOPS_MAX_PLANES];
    uint32_t n_planes, n_images, h, w;
    int32_t kind;            // OUSTER_HIP_FOPS_PRED_*
    int32_t src_type;        // KEY: element type of the key plane; XYZ: F32 / F64
    const void* src;         // KEY: [n_images] key planes; MASK: [n_masks] u8 masks; XYZ: [n_images][h * w][3]
    size_t src_stride;       // elements (XYZ: points) between images
    uint32_t n_masks, axis;
    double lower, upper;     // KEY / XYZ: the value range, inclusive
    uint32_t lo, hi;         // ROWS / COLS: the index range [lo, hi)
    const uint32_t* shifts;  // device [n_tables][h], every value already reduced to [0, w): COLS and twins
    uint32_t n_tables;       // image i uses table i % n_tables
};

struct FopsSelectArgs {
    const void* src[FOPS_MAX_PLANES];   // [n_images][h][w] elements of elem[i] bytes
    void* dst[FOPS_MAX_PLANES];         // [n_images][n_sel][w]
    uint32_t elem[FOPS_MAX_PLANES];
    uint32_t n_planes, n_images, h, w, n_sel;
    const uint32_t* indices;            // device [n_sel], every value < h
};

hipError_t launch_fops_clip(const FopsClipArgs& a, hipStream_t st);
hipError_t launch_fops_invalidate(const FopsInvalidateArgs& a, hipStream_t st);
hipError_t launch_fops_select_rows(const FopsSelectArgs& a, hipStream_t st);

}  // namespace ouster_hip_dev
