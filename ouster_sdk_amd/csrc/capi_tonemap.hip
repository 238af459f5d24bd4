// capi_tonemap.hip -- the C ABI of the RGB display images (k_tonemap.hip): ouster_hip_image_lum_percentiles / _tonemap /
// _apply_rgb_host of include/ouster_hip.h.  Arguments are checked before the context is looked at -- in the host forms before
// anything is staged --, so every refusal is the same with and without a GPU.
#include "capi_internal.h"
#include "k_tonemap.h"
#include "tonemap_dev.h"

using namespace ouster_hip_dev;

namespace {
size_t rgb_elem(int t) { return t == OUSTER_HIP_F16 ? 2 : float_elem(t); }

// the two checks every entry point starts with, device and host forms alike
int rgb_types(int in_type, int out_type) {
    if (!float_elem(out_type)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "out_type must be F32 or F64");
    if (in_type != out_type && !(in_type == OUSTER_HIP_F16 && out_type == OUSTER_HIP_F32))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "in_type must be out_type, or F16 with out_type F32");
    return OUSTER_HIP_OK;
}
// the reference's float counts stop counting at 2^24 pixels per tile
int rgb_tile_limit(uint32_t h, uint32_t w) {
    if ((uint64_t)((h + 7) / 8) * ((w + 7) / 8) > (1ull << 24))
        return fail(OUSTER_HIP_ERR_UNSUPPORTED, "tone mapping: tiles of more than 2^24 pixels");
    return OUSTER_HIP_OK;
}

// shared argument checks; fills what every kernel needs.  Returns 1 when there is nothing to do.
int rgb_args(const void* images, int in_type, int out_type, uint32_t n_images, uint32_t h, uint32_t w, size_t image_stride,
             bool tiles, TonemapArgs& a) {
    if (const int rc = rgb_types(in_type, out_type)) return rc;
    if (n_images == 0) return 1;
    if (tiles && (h < (uint32_t)TM_TILES || w < (uint32_t)TM_TILES))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "tone mapping needs an image of at least 8 x 8 pixels (got %u x %u)", h, w);
    if (h == 0 || w == 0) return 1;
    if (n_images > 65535u) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "at most 65535 images per call");
    if ((uint64_t)h * w > (1ull << 31)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "image larger than 2^31 pixels");
    if (!images) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL image pointer");
    const size_t dense = (size_t)h * w * 3;
    if (image_stride && image_stride < dense) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "image_stride smaller than an image");
    a = TonemapArgs{};
    a.in = images;
    a.in_stride = image_stride ? image_stride : dense;
    a.n_images = n_images;
    a.h = h;
    a.w = w;
    return OUSTER_HIP_OK;
}
}  // namespace

int ouster_hip_image_lum_percentiles(ouster_hip_ctx* ctx, const void* images, int in_type, int out_type, uint32_t n_images,
                                     uint32_t h, uint32_t w, size_t image_stride, double lo_percentile, double hi_percentile,
                                     uint32_t* n, void* lo_hi) {
    TonemapArgs a;
    const int rc = rgb_args(images, in_type, out_type, n_images, h, w, image_stride, false, a);
    if (rc) return rc > 0 ? OUSTER_HIP_OK : rc;
    if (!n || !lo_hi) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL output pointer");
    if (!(lo_percentile >= 0) || !(hi_percentile >= 0) || !(lo_percentile + hi_percentile < 1))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "percentiles must be >= 0 and sum to less than 1");
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    a.lo_percentile = lo_percentile;
    a.hi_percentile = hi_percentile;
    a.n_positive = n;
    a.lo_hi = lo_hi;
    HIP_TRY(launch_tm_lum_percentiles(a, in_type, out_type, ctx->stream));
    return OUSTER_HIP_OK;
}

int ouster_hip_image_tonemap(ouster_hip_ctx* ctx, const void* images, int in_type, void* out, int out_type, uint32_t n_images,
                             uint32_t h, uint32_t w, size_t in_stride, size_t out_stride,
                             const ouster_hip_tonemap_params* params) {
    TonemapArgs a;
    const int rc = rgb_args(images, in_type, out_type, n_images, h, w, in_stride, true, a);
    if (rc) return rc > 0 ? OUSTER_HIP_OK : rc;
    if (!out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "out is NULL");
    if (!params) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "params is NULL");
    const size_t dense = (size_t)h * w * 3;
    if (out_stride && out_stride < dense) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "out_stride smaller than an image");
    a.out = out;
    a.out_stride = out_stride ? out_stride : dense;
    if (out == images && (in_type != out_type || a.out_stride != a.in_stride))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "in place needs equal types and strides");
    if (const int rc2 = rgb_tile_limit(h, w)) return rc2;
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t table = (size_t)n_images * TM_LUT_ELEMS * 4;
    if (const int rc = grow_idle(ctx, ctx->tonemap_ws, 2 * table, "tone-map tables")) return rc;
    a.hist = (uint32_t*)ctx->tonemap_ws.p;
    a.luts = (float*)((uint8_t*)ctx->tonemap_ws.p + table);
    a.params = params;
    a.pieces = (uint32_t)std::min(std::max(ctx->knobs.tonemap_bands, 0), 64);   // 0: launch_tm_hist chooses
    const size_t es_in = rgb_elem(in_type), es_out = rgb_elem(out_type), al_in = std::min<size_t>(16, 4 * es_in);
    a.vec = (uintptr_t)images % al_in == 0 && (uintptr_t)out % 16 == 0 &&
            (n_images == 1 || ((a.in_stride * es_in) % al_in == 0 && (a.out_stride * es_out) % 16 == 0));
    HIP_TRY(hipMemsetAsync(a.hist, 0, table, ctx->stream));
    HIP_TRY(launch_tm_hist(a, in_type, out_type, ctx->stream));
    HIP_TRY(launch_tm_luts(a, ctx->stream));
    HIP_TRY(launch_tm_finish(a, in_type, out_type, ctx->stream));
    return OUSTER_HIP_OK;
}

// One host image: pool memory in place, anything else through the context's scratch; the few numbers that go out or come in are
// staged whatever memory they are in.
int ouster_hip_image_lum_percentiles_host(ouster_hip_ctx* ctx, const void* image, int in_type, int out_type, uint32_t h,
                                          uint32_t w, double lo_percentile, double hi_percentile, uint32_t* n, void* lo_hi) {
    if (const int rc0 = rgb_types(in_type, out_type)) return rc0;
    const size_t es = float_elem(out_type);
    if (!image || !n || !lo_hi || h == 0 || w == 0) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "bad image arguments");
    if ((uint64_t)h * w > (1ull << 31)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "image larger than 2^31 pixels");
    if (!(lo_percentile >= 0) || !(hi_percentile >= 0) || !(lo_percentile + hi_percentile < 1))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "percentiles must be >= 0 and sum to less than 1");
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    Staging st(ctx);
    const auto in = st.input(image, (size_t)h * w * 3 * rgb_elem(in_type));
    const auto cnt = st.output(n, 4, true), lh = st.output(lo_hi, 2 * es, true);
    int rc = st.stage();
    if (rc != OUSTER_HIP_OK) return rc;
    rc = ouster_hip_image_lum_percentiles(ctx, st.dev(in), in_type, out_type, 1, h, w, 0, lo_percentile, hi_percentile,
                                          (uint32_t*)st.dev(cnt), st.dev(lh));
    if (rc != OUSTER_HIP_OK) return rc;
    return st.finish();
}

namespace {
// in -> out of one host image through `run(dev_in, dev_out, dev_record)`; out == image: one array updated in place
template <class REC, class RUN>
int rgb_host(ouster_hip_ctx* ctx, const void* image, int in_type, void* out, int out_type, uint32_t h, uint32_t w, const REC& rec, RUN&& run) {
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t px = (size_t)h * w * 3;
    Staging st(ctx);
    Staging::Ref in, o;
    if (out == image) in = o = st.inout(out, px * rgb_elem(out_type));
    else in = st.input(image, px * rgb_elem(in_type)), o = st.output(out, px * rgb_elem(out_type));
    const auto dr = st.input(&rec, sizeof rec, true);   // pageable source: staged before the call returns
    int rc = st.stage();
    if (rc != OUSTER_HIP_OK) return rc;
    rc = run(st.dev(in), st.dev(o), (const REC*)st.dev(dr));
    if (rc != OUSTER_HIP_OK) return rc;
    return st.finish();
}
int rgb_host_args(const void* image, int in_type, const void* out, int out_type) {
    if (const int rc = rgb_types(in_type, out_type)) return rc;
    if (!image || !out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL image pointer");
    if (out == image && in_type != out_type) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "in place needs equal types");
    return OUSTER_HIP_OK;
}
}  // namespace

int ouster_hip_image_tonemap_host(ouster_hip_ctx* ctx, const void* image, int in_type, void* out, int out_type, uint32_t h,
                                  uint32_t w, const ouster_hip_tonemap_params* params) {
    const int rc = rgb_host_args(image, in_type, out, out_type);
    if (rc != OUSTER_HIP_OK) return rc;
    if (h < (uint32_t)TM_TILES || w < (uint32_t)TM_TILES)
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "tone mapping needs an image of at least 8 x 8 pixels (got %u x %u)", h, w);
    if ((uint64_t)h * w > (1ull << 31)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "image larger than 2^31 pixels");
    if (!params) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "params is NULL");
    if (const int rc2 = rgb_tile_limit(h, w)) return rc2;
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (params->map.mode == OUSTER_HIP_IMAGE_MAP_NONE && out == image) return OUSTER_HIP_OK;   // the early return: nothing moves
    return rgb_host(ctx, image, in_type, out, out_type, h, w, *params, [&](const void* din, void* dout, const ouster_hip_tonemap_params* dp) {
        return ouster_hip_image_tonemap(ctx, din, in_type, dout, out_type, 1, h, w, 0, 0, dp);
    });
}

int ouster_hip_image_apply_rgb_host(ouster_hip_ctx* ctx, const void* image, int in_type, void* out, int out_type, uint32_t h,
                                    uint32_t w, const ouster_hip_image_map* map) {
    const int rc = rgb_host_args(image, in_type, out, out_type);
    if (rc != OUSTER_HIP_OK) return rc;
    if ((uint64_t)h * w * 3 > (1ull << 31)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "image larger than 2^31 elements");
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    ouster_hip_image_map m{};
    if (map) m = *map;
    m.use_dark = 0;
    if (h == 0 || w == 0 || (m.mode == OUSTER_HIP_IMAGE_MAP_NONE && out == image)) return OUSTER_HIP_OK;
    return rgb_host(ctx, image, in_type, out, out_type, h, w, m, [&](const void* din, void* dout, const ouster_hip_image_map* dm) {
        return ouster_hip_image_apply(ctx, din, in_type, dout, out_type, 1, h, 3 * w, 0, 0, nullptr, dm);
    });
}
