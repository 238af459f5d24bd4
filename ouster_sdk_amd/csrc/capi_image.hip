// capi_image.hip -- the C ABI of the display images (k_image.hip): ouster_hip_image_* of include/ouster_hip.h
#include "capi_internal.h"
#include "k_image.h"

using namespace ouster_hip_dev;

namespace {
size_t image_elem(int t) {
    switch (t) {
        case OUSTER_HIP_U8: return 1;
        case OUSTER_HIP_U16: case OUSTER_HIP_F16: return 2;
        case OUSTER_HIP_U32: case OUSTER_HIP_F32: return 4;
        case OUSTER_HIP_F64: return 8;
        default: return 0;
    }
}
// shared argument checks; fills what every image kernel needs.  Returns 1 when there is nothing to do.
// f16_ok: FLOAT16 patterns with out_type F32 pass as well (ouster_hip_image_apply alone converts them)
int image_args(ouster_hip_ctx* ctx, const void* planes, int in_type, int out_type, uint32_t n_images, uint32_t h, uint32_t w,
               size_t image_stride, ImageArgs& a, bool f16_ok = false) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (!float_elem(out_type))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "out_type must be F32 or F64");
    if (in_type != OUSTER_HIP_U8 && in_type != OUSTER_HIP_U16 && in_type != OUSTER_HIP_U32 && in_type != out_type &&
        !(f16_ok && in_type == OUSTER_HIP_F16 && out_type == OUSTER_HIP_F32))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "in_type must be U8, U16, U32 or out_type");
    if (n_images == 0 || h == 0 || w == 0) return 1;
    if (n_images > 65535u) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "at most 65535 images per call");
    if ((uint64_t)h * w > (1ull << 31)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "image larger than 2^31 elements");
    if (!planes) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL image pointer");
    if (image_stride && image_stride < (size_t)h * w) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "image_stride smaller than an image");
    a = ImageArgs{};
    a.in = planes;
    a.in_stride = image_stride ? image_stride : (size_t)h * w;
    a.n_images = n_images;
    a.h = h;
    a.w = w;
    const size_t vb = std::min<size_t>(16, 4 * image_elem(in_type));
    a.vec = ((uintptr_t)planes % vb == 0) && (a.in_stride % 4 == 0 || n_images == 1);
    return OUSTER_HIP_OK;
}
}  // namespace

int ouster_hip_image_dark_rows(ouster_hip_ctx* ctx, const void* planes, int in_type, int out_type, uint32_t n_images,
                               uint32_t h, uint32_t w, size_t image_stride, void* medians, uint32_t* n_cols) {
    ImageArgs a;
    const int rc = image_args(ctx, planes, in_type, out_type, n_images, h, w, image_stride, a);
    if (rc) return rc > 0 ? OUSTER_HIP_OK : rc;
    if (w > IMAGE_MAX_W_DARK) return fail(OUSTER_HIP_ERR_UNSUPPORTED, "dark rows: images wider than %u columns", IMAGE_MAX_W_DARK);
    HIP_TRY(hipSetDevice(ctx->device));
    if (h < 2) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dark rows need at least two rows");
    if (!medians) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "medians is NULL");
    const size_t words = (w + 63) / 64;
    if (ctx->image_mask.ensure((size_t)n_images * words * 8)) return fail(OUSTER_HIP_ERR_RUNTIME, "out of device memory (column masks)");
    a.col_mask = (uint64_t*)ctx->image_mask.p;
    a.medians = medians;
    a.n_cols = n_cols;
    a.vec = a.vec && (w % 4 == 0);
    HIP_TRY(launch_image_dark_rows(a, in_type, out_type, ctx->stream));
    return OUSTER_HIP_OK;
}

int ouster_hip_image_percentiles(ouster_hip_ctx* ctx, const void* planes, int in_type, int out_type, uint32_t n_images,
                                 uint32_t h, uint32_t w, size_t image_stride, const void* dark, double lo_percentile,
                                 double hi_percentile, uint32_t* n, void* lo_hi) {
    ImageArgs a;
    const int rc = image_args(ctx, planes, in_type, out_type, n_images, h, w, image_stride, a);
    if (rc) return rc > 0 ? OUSTER_HIP_OK : rc;
    if (!n || !lo_hi) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL output pointer");
    if (!(lo_percentile >= 0) || !(hi_percentile >= 0) || !(lo_percentile + hi_percentile < 1))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "percentiles must be >= 0 and sum to less than 1");
    HIP_TRY(hipSetDevice(ctx->device));
    a.dark = dark;
    a.lo_percentile = lo_percentile;
    a.hi_percentile = hi_percentile;
    a.n_positive = n;
    a.lo_hi = lo_hi;
    HIP_TRY(launch_image_percentiles(a, in_type, out_type, ctx->stream));
    return OUSTER_HIP_OK;
}

int ouster_hip_image_apply(ouster_hip_ctx* ctx, const void* planes, int in_type, void* out, int out_type, uint32_t n_images,
                           uint32_t h, uint32_t w, size_t in_stride, size_t out_stride, const void* dark,
                           const ouster_hip_image_map* maps) {
    ImageArgs a;
    const int rc = image_args(ctx, planes, in_type, out_type, n_images, h, w, in_stride, a, true);
    if (rc) return rc > 0 ? OUSTER_HIP_OK : rc;
    if (!out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "out is NULL");
    if (out_stride && out_stride < (size_t)h * w) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "out_stride smaller than an image");
    if (out == planes && (in_type != out_type || (out_stride ? out_stride : (size_t)h * w) != a.in_stride))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "in place needs equal types and strides");
    HIP_TRY(hipSetDevice(ctx->device));
    a.out = out;
    a.out_stride = out_stride ? out_stride : (size_t)h * w;
    a.vec = a.vec && ((uintptr_t)out % 16 == 0) && (a.out_stride % 4 == 0 || n_images == 1);
    a.dark = dark;
    a.maps = maps;
    HIP_TRY(launch_image_apply(a, in_type, out_type, ctx->stream));
    return OUSTER_HIP_OK;
}

// One host image: the few numbers that go out or come in are staged whatever memory they are in.
int ouster_hip_image_dark_rows_host(ouster_hip_ctx* ctx, const void* image, int dtype, uint32_t h, uint32_t w, void* medians,
                                    uint32_t* n_cols) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    const size_t es = float_elem(dtype);
    if (!es) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dtype must be F32 or F64");
    if (h < 2 || w == 0) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dark rows need at least two rows");
    if (!image || !medians || !n_cols) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    HIP_TRY(hipSetDevice(ctx->device));
    Staging st(ctx);
    const auto in = st.input(image, (size_t)h * w * es), cols = st.output(n_cols, 4, true), med = st.output(medians, (size_t)(h - 1) * es, true);
    int rc = st.stage();
    if (rc != OUSTER_HIP_OK) return rc;
    rc = ouster_hip_image_dark_rows(ctx, st.dev(in), dtype, dtype, 1, h, w, 0, st.dev(med), (uint32_t*)st.dev(cols));
    if (rc != OUSTER_HIP_OK) return rc;
    return st.finish();
}

int ouster_hip_image_percentiles_host(ouster_hip_ctx* ctx, const void* image, int dtype, uint32_t h, uint32_t w,
                                      const void* dark, double lo_percentile, double hi_percentile, uint32_t* n,
                                      void* lo_hi) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    const size_t es = float_elem(dtype);
    if (!es) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dtype must be F32 or F64");
    if (!image || !n || !lo_hi || h == 0 || w == 0) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "bad image arguments");
    HIP_TRY(hipSetDevice(ctx->device));
    Staging st(ctx);
    const auto in = st.input(image, (size_t)h * w * es), dk = dark ? st.input(dark, (size_t)h * es, true) : Staging::Ref{};
    const auto cnt = st.output(n, 4, true), lh = st.output(lo_hi, 2 * es, true);
    int rc = st.stage();
    if (rc != OUSTER_HIP_OK) return rc;
    rc = ouster_hip_image_percentiles(ctx, st.dev(in), dtype, dtype, 1, h, w, 0, st.dev(dk), lo_percentile, hi_percentile, (uint32_t*)st.dev(cnt), st.dev(lh));
    if (rc != OUSTER_HIP_OK) return rc;
    return st.finish();
}

int ouster_hip_image_apply_host(ouster_hip_ctx* ctx, void* image, int dtype, uint32_t h, uint32_t w, const void* dark,
                                const ouster_hip_image_map* map) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    const size_t es = float_elem(dtype);
    if (!es) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dtype must be F32 or F64");
    if (h == 0 || w == 0) return OUSTER_HIP_OK;
    if (!image) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL image pointer");
    HIP_TRY(hipSetDevice(ctx->device));
    ouster_hip_image_map m{};
    if (map) m = *map;
    else m.use_dark = 1;
    Staging st(ctx);
    const auto io = st.inout(image, (size_t)h * w * es), dk = dark ? st.input(dark, (size_t)h * es, true) : Staging::Ref{};
    const auto dm = st.input(&m, sizeof m, true);   // pageable source: staged before the call returns
    int rc = st.stage();
    if (rc != OUSTER_HIP_OK) return rc;
    rc = ouster_hip_image_apply(ctx, st.dev(io), dtype, st.dev(io), dtype, 1, h, w, 0, 0, st.dev(dk), (const ouster_hip_image_map*)st.dev(dm));
    if (rc != OUSTER_HIP_OK) return rc;
    return st.finish();
}
