// standalone_plan.cpp -- the launch plan of the standalone kernels: plain C++, no HIP header, no state.
#include "standalone_plan.h"

namespace ouster_hip_dev {

const char* destagger_route_name(DestaggerRoute r) {
    switch (r) {
        case DestaggerRoute::ROWS1: return "ROWS1";
        case DestaggerRoute::ROWS2: return "ROWS2";
        case DestaggerRoute::ROWS4: return "ROWS4";
        case DestaggerRoute::LDS: return "LDS";
        case DestaggerRoute::DIRECT: return "DIRECT";
        default: return "BYTES";
    }
}

DestaggerPlan plan_destagger(size_t row_bytes, bool pointers_aligned, int rows_env, uint32_t h, uint32_t n_images) {
    DestaggerPlan p{};
    p.rows_per_wg = 1;
    p.grid_x = h;
    p.grid_y = n_images;
    const bool al = (row_bytes % 16 == 0) && pointers_aligned;
    if (al && row_bytes <= (rows_env > 0 ? DESTAGGER_ROWS_ENV_MAX : DESTAGGER_ROWS_MAX) && rows_env != 0) {
        // rows of up to 4 KB (8 / 16-bit planes of a 2048-column frame): two rows per workgroup, pipelined -- 0.77 / 0.79 of the HBM
        // roofline on 256 images against 0.72 / 0.75 for one row per workgroup (round 6, same box); 8 KB rows (32-bit planes)
        // lose with this form (0.50 against 0.76) and stay on k_destagger
        const uint32_t rpw = rows_env > 0 ? (uint32_t)rows_env : 2u;
        const uint32_t nchunk = (uint32_t)(row_bytes >> 4), ch = (nchunk + 255) / 256;
        p.route = ch <= 1 ? DestaggerRoute::ROWS1 : ch <= 2 ? DestaggerRoute::ROWS2 : DestaggerRoute::ROWS4;
        p.rows_per_wg = rpw;
        p.lds_bytes = 2u * (uint32_t)row_bytes;
        p.grid_x = (h + rpw - 1) / rpw;
        return p;
    }
    if (!al) p.route = DestaggerRoute::BYTES;
    else if (row_bytes <= DESTAGGER_LDS_MAX) p.route = DestaggerRoute::LDS;
    else p.route = DestaggerRoute::DIRECT;
    p.lds_bytes = p.route == DestaggerRoute::LDS ? (uint32_t)row_bytes : 0u;
    return p;
}

namespace {
// enough workgroups to fill the chip: split the rows when the batch is small
uint32_t tiled_rows_per_block(uint32_t tiles, uint32_t h, uint32_t n_images) {
    uint32_t rpb = h;
    while (rpb > 16 && (size_t)tiles * n_images * ((h + rpb - 1) / rpb) < STANDALONE_MIN_WGS) rpb = (rpb + 1) / 2;
    return (rpb + 15) / 16 * 16;
}

TiledPlan generic_plan(size_t items) {
    TiledPlan p{};
    size_t blocks = (items + 255) / 256;
    if (blocks > STANDALONE_GENERIC_MAX_WGS) blocks = STANDALONE_GENERIC_MAX_WGS;
    if (blocks == 0) blocks = 1;
    p.images_per_block = 1;
    p.grid_x = (uint32_t)blocks;
    p.grid_y = 1;
    return p;
}
}  // namespace

TiledPlan plan_cartesian(uint32_t w, uint32_t h, uint32_t n_images, bool vec_ok, uint32_t tile_width) {
    if (!(vec_ok && w % 4 == 0)) return generic_plan(((size_t)w * h + 3) / 4 * n_images);   // a lane owns 4 pixels
    TiledPlan p{};
    p.tiled = true;
    p.tile_width = tile_width;
    const uint32_t tiles = (w + tile_width - 1) / tile_width;
    const uint32_t rpb = tiled_rows_per_block(tiles, h, n_images);
    p.rows_per_block = rpb;
    // as many images per workgroup as leave >= 2048 workgroups (16 at most): a full LUT's rows / the separable
    // directions of a row are fetched / computed once per group, and the group's range quads are fetched four deep
    uint32_t ipb = 1;
    const size_t per_image = (size_t)tiles * ((h + rpb - 1) / rpb);
    while (ipb < CARTESIAN_MAX_GROUP && ipb * 2 <= n_images &&
           per_image * ((n_images + ipb * 2 - 1) / (ipb * 2)) >= CARTESIAN_GROUP_MIN_WGS)
        ipb *= 2;
    p.images_per_block = ipb;
    p.grid_x = tiles * ((h + rpb - 1) / rpb);
    p.grid_y = (n_images + ipb - 1) / ipb;
    return p;
}

TiledPlan plan_dewarp(uint32_t w, uint32_t h, uint32_t n_images, bool aligned, uint32_t tile_width) {
    if (!(w % 4 == 0 && aligned)) return generic_plan((size_t)w * h * n_images);   // a lane owns one point
    TiledPlan p{};
    p.tiled = true;
    p.tile_width = tile_width;
    const uint32_t tiles = (w + tile_width - 1) / tile_width;
    const uint32_t rpb = tiled_rows_per_block(tiles, h, n_images);
    p.rows_per_block = rpb;
    p.images_per_block = 1;
    p.grid_x = tiles * ((h + rpb - 1) / rpb);
    p.grid_y = n_images;
    return p;
}

}  // namespace ouster_hip_dev
