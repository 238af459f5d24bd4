// capi_destagger.hip -- the C ABI of the standalone destagger (k_destagger.hip): ouster_hip_destagger / _destagger_host
#include "capi_internal.h"

using namespace ouster_hip_dev;

extern "C" {

// ---- standalone destagger -----------------------------------------------------------------
int ouster_hip_destagger(ouster_hip_ctx* ctx, const void* src, void* dst, uint32_t h, uint32_t w,
                         uint32_t elem_bytes, const int32_t* shifts, uint32_t n_shifts,
                         int inverse, uint32_t n_images) {
    if (!ctx || !shifts) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_shifts != h)
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "image height does not match shifts size");
    if (n_images == 0 || h == 0 || w == 0) return OUSTER_HIP_OK;
    if (!src || !dst || src == dst) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "bad image pointers");
    if (elem_bytes == 0) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "elem_bytes is 0");
    HIP_TRY(hipSetDevice(ctx->device));
    DestaggerArgs a{};
    if (const int rc = stage_offsets(ctx, shifts, h, w, inverse, &a.offsets)) return rc;
    a.src = src;
    a.dst = dst;
    a.h = h;
    a.w = w;
    a.elem = elem_bytes;
    HIP_TRY(launch_destagger(a, n_images, ctx->stream));
    return OUSTER_HIP_OK;
}

int ouster_hip_destagger_host(ouster_hip_ctx* ctx, const void* src, void* dst, uint32_t h, uint32_t w,
                              uint32_t elem_bytes, const int32_t* shifts, uint32_t n_shifts, int inverse) {
    if (!ctx || !shifts) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_shifts != h) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "image height does not match shifts size");
    if (h == 0 || w == 0) return OUSTER_HIP_OK;
    if (!src || !dst || elem_bytes == 0) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "bad image arguments");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)h * w * elem_bytes;
    Staging st(ctx);
    // in place (src == dst) in the reference copies rows through each other: not a supported call there either; go through scratch
    const auto in = st.input(src, bytes), out = st.output(dst, bytes, src == dst);
    int rc = st.stage();
    if (rc != OUSTER_HIP_OK) return rc;
    rc = ouster_hip_destagger(ctx, st.dev(in), st.dev(out), h, w, elem_bytes, shifts, n_shifts, inverse, 1);
    if (rc != OUSTER_HIP_OK) return rc;
    return st.finish();
}

}  // extern "C"
