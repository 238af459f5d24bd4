// capi_frame_ops.hip -- the C ABI of frame_ops (k_frame_ops.hip): ouster_hip_frame_ops_* of include/ouster_hip.h
#include "capi_internal.h"
#include "k_frame_ops.h"

using namespace ouster_hip_dev;

namespace {
size_t fops_elem(int t) {
    switch (t) {
        case OUSTER_HIP_U8: case OUSTER_HIP_I8: return 1;
        case OUSTER_HIP_U16: case OUSTER_HIP_I16: return 2;
        case OUSTER_HIP_U32: case OUSTER_HIP_I32: case OUSTER_HIP_F32: return 4;
        case OUSTER_HIP_U64: case OUSTER_HIP_I64: case OUSTER_HIP_F64: return 8;
        default: return 0;
    }
}
const char* fops_type_name(int t) {
    static const char* names[] = {"VOID", "UINT8", "UINT16", "UINT32", "UINT64", "INT8", "INT16", "INT32", "INT64", "FLOAT32", "FLOAT64"};
    return (t >= 0 && t <= 10) ? names[t] : "?";
}
// shared checks of the three entry points; returns 1 when there is nothing to do
int fops_shape(ouster_hip_ctx* ctx, uint32_t n_planes, uint32_t n_images, uint32_t h, uint32_t w) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (n_images > 65535u) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "at most 65535 images per call");
    if ((uint64_t)h * w > (1ull << 31)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "image larger than 2^31 elements");
    return (n_planes == 0 || n_images == 0 || h == 0 || w == 0) ? 1 : OUSTER_HIP_OK;
}
// the planes of one call -> the launch records; every `invalid` is checked before the first launch
int fops_planes(const ouster_hip_fops_plane* planes, uint32_t n_planes, uint32_t h, uint32_t w, std::vector<FopsPlane>& out,
                bool clouds_allowed = false) {
    if (!planes) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "planes is NULL");
    out.resize(n_planes);
    for (uint32_t i = 0; i < n_planes; ++i) {
        const ouster_hip_fops_plane& p = planes[i];
        FopsPlane& o = out[i];
        if (p.type == OUSTER_HIP_FOPS_XYZ_F32 || p.type == OUSTER_HIP_FOPS_XYZ_F64) {
            const uint32_t scalar = p.type == OUSTER_HIP_FOPS_XYZ_F64 ? 8 : 4;
            if (!clouds_allowed) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: a cloud can only be invalidated", i);
            if (p.invalid != 0 || p.twin) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: a cloud takes invalid == 0 and no twin", i);
            if (!p.data || (uintptr_t)p.data % scalar) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: NULL or misaligned pointer", i);
            if (p.image_stride && p.image_stride < (size_t)h * w) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: image_stride smaller than an image", i);
            o = FopsPlane{};
            o.data = p.data;
            o.stride = p.image_stride ? p.image_stride : (size_t)h * w;
            o.elem = 3 * scalar;
            o.type = p.type;
            continue;
        }
        o.elem = (uint32_t)fops_elem(p.type);
        if (!o.elem) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: unsupported element type %d", i, p.type);
        const int rc = ouster_hip_frame_ops_invalid_bits(p.type, p.invalid, &o.invalid_bits);
        if (rc != OUSTER_HIP_OK) return rc;
        if (!p.data || (uintptr_t)p.data % o.elem || (uintptr_t)p.twin % o.elem)
            return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: NULL or misaligned pointer", i);
        if (p.image_stride && p.image_stride < (size_t)h * w)
            return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: image_stride smaller than an image", i);
        o.data = p.data;
        o.twin = p.twin;
        o.stride = p.image_stride ? p.image_stride : (size_t)h * w;
        o.type = p.type;
    }
    return OUSTER_HIP_OK;
}
}  // namespace

int ouster_hip_frame_ops_invalid_bits(int type, double invalid, uint64_t* bits) {
    if (!bits) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "bits is NULL");
    *bits = 0;
    bool ok = true;
    const double t = std::trunc(invalid);
    auto put = [&](auto v) { std::memcpy(bits, &v, sizeof v); };
    switch (type) {
        case OUSTER_HIP_U8: ok = t >= 0 && t <= 255.0; if (ok) put((uint8_t)t); break;
        case OUSTER_HIP_U16: ok = t >= 0 && t <= 65535.0; if (ok) put((uint16_t)t); break;
        case OUSTER_HIP_U32: ok = t >= 0 && t <= 4294967295.0; if (ok) put((uint32_t)t); break;
        case OUSTER_HIP_U64: ok = t >= 0 && t < 18446744073709551616.0; if (ok) put((uint64_t)t); break;
        case OUSTER_HIP_I8: ok = t >= -128.0 && t <= 127.0; if (ok) put((int8_t)t); break;
        case OUSTER_HIP_I16: ok = t >= -32768.0 && t <= 32767.0; if (ok) put((int16_t)t); break;
        case OUSTER_HIP_I32: ok = t >= -2147483648.0 && t <= 2147483647.0; if (ok) put((int32_t)t); break;
        case OUSTER_HIP_I64: ok = t >= -9223372036854775808.0 && t < 9223372036854775808.0; if (ok) put((int64_t)t); break;
        case OUSTER_HIP_F32: ok = !std::isfinite(invalid) || std::fabs(invalid) <= 3.4028234663852886e38; if (ok) put((float)invalid); break;
        case OUSTER_HIP_F64: put(invalid); break;
        default: return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "unsupported element type %d", type);
    }
    if (!ok) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "invalid == %g does not fit a field of type %s", invalid, fops_type_name(type));
    return OUSTER_HIP_OK;
}

int ouster_hip_frame_ops_clip(ouster_hip_ctx* ctx, const ouster_hip_fops_plane* planes, uint32_t n_planes,
                              uint32_t n_images, uint32_t h, uint32_t w, double lower, double upper) {
    std::vector<FopsPlane> pl;
    int rc = fops_planes(planes, n_planes, h, w, pl);   // also when there is nothing to do: a bad `invalid` is an error
    if (rc != OUSTER_HIP_OK && n_planes) return rc;
    rc = fops_shape(ctx, n_planes, n_images, h, w);
    if (rc) return rc > 0 ? OUSTER_HIP_OK : rc;
    HIP_TRY(hipSetDevice(ctx->device));
    for (uint32_t p0 = 0; p0 < n_planes; p0 += FOPS_MAX_PLANES) {
        FopsClipArgs a{};
        a.n_planes = std::min<uint32_t>(FOPS_MAX_PLANES, n_planes - p0);
        std::copy(pl.begin() + p0, pl.begin() + p0 + a.n_planes, a.planes);
        a.n_images = n_images;
        a.hw = h * w;
        a.lower = lower;
        a.upper = upper;
        HIP_TRY(launch_fops_clip(a, ctx->stream));
    }
    return OUSTER_HIP_OK;
}

int ouster_hip_frame_ops_invalidate(ouster_hip_ctx* ctx, const ouster_hip_fops_pred* pred,
                                    const ouster_hip_fops_plane* planes, uint32_t n_planes, uint32_t n_images,
                                    uint32_t h, uint32_t w) {
    if (!pred) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "pred is NULL");
    std::vector<FopsPlane> pl;
    int rc = fops_planes(planes, n_planes, h, w, pl, true);
    if (rc != OUSTER_HIP_OK && n_planes) return rc;
    rc = fops_shape(ctx, n_planes, n_images, h, w);
    if (rc < 0) return rc;
    const bool nothing = rc > 0;
    FopsInvalidateArgs a{};
    a.kind = pred->kind;
    a.src_type = pred->src_type;
    a.src = pred->src;
    a.src_stride = pred->src_stride ? pred->src_stride : (size_t)h * w;
    a.n_masks = pred->n_masks;
    a.axis = pred->axis;
    a.lower = pred->lower;
    a.upper = pred->upper;
    a.lo = pred->lo;
    a.hi = pred->hi;
    bool need_shifts = false;
    for (const FopsPlane& p : pl) need_shifts = need_shifts || p.twin != nullptr;
    switch (pred->kind) {
        case OUSTER_HIP_FOPS_PRED_KEY:
            if (!fops_elem(pred->src_type)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "unsupported key element type %d", pred->src_type);
            if (!nothing && (!pred->src || (uintptr_t)pred->src % fops_elem(pred->src_type))) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL or misaligned key plane");
            break;
        case OUSTER_HIP_FOPS_PRED_ROWS:
        case OUSTER_HIP_FOPS_PRED_COLS: {
            const uint32_t size = pred->kind == OUSTER_HIP_FOPS_PRED_ROWS ? h : w;
            if (pred->lo > pred->hi || pred->hi > size)
                return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "index range [%u, %u) must lie in [0, %u]", pred->lo, pred->hi, size);
            need_shifts = need_shifts || pred->kind == OUSTER_HIP_FOPS_PRED_COLS;
            break;
        }
        case OUSTER_HIP_FOPS_PRED_MASK:
            if (pred->n_masks == 0 || (!nothing && !pred->src)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "mask predicate without masks");
            break;
        case OUSTER_HIP_FOPS_PRED_XYZ:
            if (!float_elem(pred->src_type)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "xyz type must be F32 or F64");
            if (pred->axis > 2) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "axis == %u must be in the range [0, 2]", pred->axis);
            if (!nothing && (!pred->src || (uintptr_t)pred->src % fops_elem(pred->src_type))) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL or misaligned point cloud");
            break;
        default:
            return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "unknown predicate kind %d", pred->kind);
    }
    if (need_shifts && (!pred->shifts || pred->n_shift_tables == 0))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "this call needs pixel_shift_by_row tables");
    if (nothing) return OUSTER_HIP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    a.n_images = n_images;
    a.h = h;
    a.w = w;
    if (need_shifts) {
        // (W + x % W) % W on the host, once per row: the kernel wraps a column with one conditional subtraction
        const size_t n = (size_t)pred->n_shift_tables * h;
        std::vector<uint32_t> red(n);
        for (size_t i = 0; i < n; ++i) red[i] = (uint32_t)((((int64_t)pred->shifts[i] % (int64_t)w) + w) % w);
        const int urc = upload_table(ctx, red.data(), n * 4);
        if (urc != OUSTER_HIP_OK) return urc;
        a.shifts = (const uint32_t*)ctx->tables.p;
        a.n_tables = pred->n_shift_tables;
    }
    // a key that is also a target must be read before it is written, for EVERY target of the pixel: where the list needs
    // more than one launch the key plane goes into the last one
    if (pred->kind == OUSTER_HIP_FOPS_PRED_KEY && n_planes > FOPS_MAX_PLANES)
        std::stable_partition(pl.begin(), pl.end(), [&](const FopsPlane& p) { return p.data != pred->src; });
    for (uint32_t p0 = 0; p0 < n_planes; p0 += FOPS_MAX_PLANES) {
        a.n_planes = std::min<uint32_t>(FOPS_MAX_PLANES, n_planes - p0);
        std::copy(pl.begin() + p0, pl.begin() + p0 + a.n_planes, a.planes);
        HIP_TRY(launch_fops_invalidate(a, ctx->stream));
    }
    return OUSTER_HIP_OK;
}

int ouster_hip_frame_ops_select_rows(ouster_hip_ctx* ctx, const void* const* src, void* const* dst,
                                     const uint32_t* elem_bytes, uint32_t n_planes, uint32_t n_images, uint32_t h,
                                     uint32_t w, const uint32_t* indices, uint32_t n_sel) {
    int rc = fops_shape(ctx, n_planes, n_images, h, w);
    if (rc < 0) return rc;
    if (n_sel > 65535u) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "at most 65535 rows per call");
    if (n_sel && !indices) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "indices is NULL");
    for (uint32_t i = 0; i < n_sel; ++i)
        if (indices[i] >= h) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "row index %u must be in the range [0, %u)", indices[i], h);
    if (rc > 0 || n_sel == 0) return OUSTER_HIP_OK;
    if (!src || !dst || !elem_bytes) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    for (uint32_t p = 0; p < n_planes; ++p) {
        const uint32_t e = elem_bytes[p];
        if (e != 1 && e != 2 && e != 4 && e != 8) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: elem_bytes must be 1, 2, 4 or 8", p);
        if (!src[p] || !dst[p] || (uintptr_t)src[p] % e || (uintptr_t)dst[p] % e) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: NULL or misaligned pointer", p);
    }
    HIP_TRY(hipSetDevice(ctx->device));
    const int urc = upload_table(ctx, indices, (size_t)n_sel * 4);
    if (urc != OUSTER_HIP_OK) return urc;
    for (uint32_t p0 = 0; p0 < n_planes; p0 += FOPS_MAX_PLANES) {
        FopsSelectArgs a{};
        a.n_planes = std::min<uint32_t>(FOPS_MAX_PLANES, n_planes - p0);
        for (uint32_t i = 0; i < a.n_planes; ++i) {
            a.src[i] = src[p0 + i];
            a.dst[i] = dst[p0 + i];
            a.elem[i] = elem_bytes[p0 + i];
        }
        a.n_images = n_images;
        a.h = h;
        a.w = w;
        a.n_sel = n_sel;
        a.indices = (const uint32_t*)ctx->tables.p;
        HIP_TRY(launch_fops_select_rows(a, ctx->stream));
    }
    return OUSTER_HIP_OK;
}

namespace {
// checks the planes of a *_host call and registers them, updated in place; 1: nothing to do.  After st.stage(): fops_dev_planes
int fops_host_planes(ouster_hip_ctx* ctx, const ouster_hip_fops_plane* planes, uint32_t n_planes, uint32_t h, uint32_t w,
                     Staging& st, std::vector<Staging::Ref>& refs) {
    if (!ctx || !planes) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    for (uint32_t i = 0; i < n_planes; ++i) {
        uint64_t bits;
        if (!fops_elem(planes[i].type)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: unsupported element type %d", i, planes[i].type);
        const int rc = ouster_hip_frame_ops_invalid_bits(planes[i].type, planes[i].invalid, &bits);
        if (rc != OUSTER_HIP_OK) return rc;
        if (planes[i].twin) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: a host call takes no twin plane", i);
    }
    if ((uint64_t)h * w == 0 || n_planes == 0) return 1;
    HIP_TRY(hipSetDevice(ctx->device));
    for (uint32_t i = 0; i < n_planes; ++i) {
        if (!planes[i].data) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: NULL pointer", i);
        refs.push_back(st.inout(planes[i].data, (size_t)h * w * fops_elem(planes[i].type)));
    }
    return OUSTER_HIP_OK;
}
std::vector<ouster_hip_fops_plane> fops_dev_planes(const ouster_hip_fops_plane* planes, const Staging& st, const std::vector<Staging::Ref>& refs) {
    std::vector<ouster_hip_fops_plane> dp(planes, planes + refs.size());
    for (size_t i = 0; i < refs.size(); ++i) dp[i].data = st.dev(refs[i]), dp[i].image_stride = 0;
    return dp;
}
}  // namespace

int ouster_hip_frame_ops_clip_host(ouster_hip_ctx* ctx, const ouster_hip_fops_plane* planes, uint32_t n_planes, uint32_t h,
                                   uint32_t w, double lower, double upper) {
    Staging st(ctx);
    std::vector<Staging::Ref> refs;
    int rc = fops_host_planes(ctx, planes, n_planes, h, w, st, refs);
    if (rc == OUSTER_HIP_OK) rc = st.stage();
    if (rc) return rc > 0 ? OUSTER_HIP_OK : rc;
    rc = ouster_hip_frame_ops_clip(ctx, fops_dev_planes(planes, st, refs).data(), n_planes, 1, h, w, lower, upper);
    if (rc != OUSTER_HIP_OK) return rc;
    return st.finish();
}

int ouster_hip_frame_ops_invalidate_host(ouster_hip_ctx* ctx, const ouster_hip_fops_pred* pred,
                                         const ouster_hip_fops_plane* planes, uint32_t n_planes, uint32_t h, uint32_t w) {
    if (!pred) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "pred is NULL");
    Staging st(ctx);
    std::vector<Staging::Ref> refs;
    int rc = fops_host_planes(ctx, planes, n_planes, h, w, st, refs);
    if (rc) return rc > 0 ? OUSTER_HIP_OK : rc;
    ouster_hip_fops_pred dpred = *pred;
    dpred.src_stride = 0;
    size_t sbytes = 0;
    switch (pred->kind) {
        case OUSTER_HIP_FOPS_PRED_KEY: sbytes = (size_t)h * w * fops_elem(pred->src_type); break;
        case OUSTER_HIP_FOPS_PRED_MASK: sbytes = (size_t)h * w; dpred.n_masks = 1; break;
        case OUSTER_HIP_FOPS_PRED_XYZ: sbytes = (size_t)h * w * 3 * (pred->src_type == OUSTER_HIP_F64 ? 8 : 4); break;
        default: break;
    }
    Staging::Ref src;
    if (sbytes) {
        if (!pred->src) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "predicate source is NULL");
        src = st.find(pred->src, sbytes);   // the key among the targets: the same device image
        if (!src) src = st.input(pred->src, sbytes);
    }
    rc = st.stage();
    if (rc != OUSTER_HIP_OK) return rc;
    if (sbytes) dpred.src = st.dev(src);
    rc = ouster_hip_frame_ops_invalidate(ctx, &dpred, fops_dev_planes(planes, st, refs).data(), n_planes, 1, h, w);
    if (rc != OUSTER_HIP_OK) return rc;
    return st.finish();
}

int ouster_hip_frame_ops_select_rows_host(ouster_hip_ctx* ctx, const void* const* src, void* const* dst,
                                          const uint32_t* elem_bytes, uint32_t n_planes, uint32_t h, uint32_t w,
                                          const uint32_t* indices, uint32_t n_sel) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (n_planes == 0 || h == 0 || w == 0 || n_sel == 0) return ouster_hip_frame_ops_select_rows(ctx, src, dst, elem_bytes, n_planes, 1, h, w, indices, n_sel);
    if (!src || !dst || !elem_bytes) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(ctx->device));
    Staging st(ctx);
    std::vector<Staging::Ref> in, out;
    for (uint32_t p = 0; p < n_planes; ++p) {
        if (!src[p] || !dst[p]) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: NULL pointer", p);
        in.push_back(st.input(src[p], (size_t)h * w * elem_bytes[p]));
        out.push_back(st.output(dst[p], (size_t)n_sel * w * elem_bytes[p]));
    }
    int rc = st.stage();
    if (rc != OUSTER_HIP_OK) return rc;
    std::vector<const void*> s(n_planes);
    std::vector<void*> d(n_planes);
    for (uint32_t p = 0; p < n_planes; ++p) s[p] = st.dev(in[p]), d[p] = st.dev(out[p]);
    rc = ouster_hip_frame_ops_select_rows(ctx, s.data(), d.data(), elem_bytes, n_planes, 1, h, w, indices, n_sel);
    if (rc != OUSTER_HIP_OK) return rc;
    return st.finish();
}
