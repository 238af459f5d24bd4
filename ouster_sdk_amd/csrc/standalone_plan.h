// standalone_plan.h -- which kernel and which launch shape ouster_hip_destagger / ouster_hip_cartesian / ouster_hip_dewarp
// get: host integers in, values out.  Includes nothing but the standard library, so it compiles (and is tested) without
// HIP, like decode_plan.h.  The launchers of k_destagger.hip, k_cartesian.hip and k_dewarp.hip call these functions and only launch.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ouster_hip_dev {

// rows up to this size take k_destagger_rows (up to DESTAGGER_ROWS_ENV_MAX when OUSTER_HIP_DESTAGGER_ROWS asks for it)
constexpr size_t DESTAGGER_ROWS_MAX = 4u << 10;
constexpr size_t DESTAGGER_ROWS_ENV_MAX = 16u << 10;
// rows up to this size are staged in LDS by k_destagger
constexpr uint32_t DESTAGGER_LDS_MAX = 64u << 10;
// the tiled kernels split the rows of a small batch until the grid has this many workgroups ...
constexpr size_t STANDALONE_MIN_WGS = 1024;
// ... and k_cartesian_tiled groups images (CARTESIAN_MAX_GROUP at most) while this many workgroups are left
constexpr size_t CARTESIAN_GROUP_MIN_WGS = 2048;
constexpr uint32_t CARTESIAN_MAX_GROUP = 16;
// grid cap of the generic grid-stride kernels
constexpr size_t STANDALONE_GENERIC_MAX_WGS = 256 * 32;

enum class DestaggerRoute {
    ROWS1,   // k_destagger_rows<1>: several rows per workgroup, one 16 B chunk per lane and row
    ROWS2,   // k_destagger_rows<2>
    ROWS4,   // k_destagger_rows<4>
    LDS,     // k_destagger, the row staged in LDS
    DIRECT,  // k_destagger, aligned 16 B stores straight from global memory (row too long for LDS)
    BYTES,   // k_destagger, byte by byte (row not 16 B granular, or a pointer not 16 B aligned)
};
const char* destagger_route_name(DestaggerRoute r);

struct DestaggerPlan {
    DestaggerRoute route;
    uint32_t rows_per_wg;   // consecutive rows of one workgroup (1 outside the ROWS routes)
    uint32_t lds_bytes;     // dynamic LDS of the launch
    uint32_t grid_x, grid_y;
};

// row_bytes = w * elem; pointers_aligned: source and destination are both 16 B aligned; rows_env: the value of
// OUSTER_HIP_DESTAGGER_ROWS (-1: not set, 0: never k_destagger_rows, n > 0: n rows per workgroup, for rows up to 16 KB)
DestaggerPlan plan_destagger(size_t row_bytes, bool pointers_aligned, int rows_env, uint32_t h, uint32_t n_images);

struct TiledPlan {
    bool tiled;                 // k_*_tiled, else the generic grid-stride kernel
    uint32_t tile_width;        // columns of a tile (tiled only)
    uint32_t rows_per_block;    // rows of a tile handled by one workgroup (tiled only)
    uint32_t images_per_block;  // images that share one workgroup (k_cartesian_tiled only; 1 otherwise)
    uint32_t grid_x, grid_y;
};

// vec_ok: range and xyz 16 B aligned and h * w % 4 == 0; tile_width: 64, or 256 when OUSTER_HIP_CT_TILE asks for it
TiledPlan plan_cartesian(uint32_t w, uint32_t h, uint32_t n_images, bool vec_ok, uint32_t tile_width);
// aligned: points and output 16 B aligned
TiledPlan plan_dewarp(uint32_t w, uint32_t h, uint32_t n_images, bool aligned, uint32_t tile_width);

}  // namespace ouster_hip_dev
