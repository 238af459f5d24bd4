// capi_voxel.hip -- the C ABI of voxel down-sampling (k_voxel.hip, host/voxel_util.cpp): ouster_hip_voxel_*
#include "capi_internal.h"
#include "carve.h"
#include "k_voxel.h"

using namespace ouster_hip_dev;

void ouster_hip_dev::carve_voxel_grid(Carver& c, VoxelArgs& v) {
    const size_t n = v.n;
    v.keys = c.take<VoxelKey>(n), v.table = c.take<int32_t>((size_t)v.table_mask + 1);
    v.slot = c.take<uint32_t>(n), v.first = c.take<uint32_t>(n), v.first_id = c.take<uint32_t>(n);
    v.vid = c.take<uint32_t>(n), v.idx = c.take<uint32_t>(n), v.svid = c.take<uint32_t>(n), v.sidx = c.take<uint32_t>(n);
    v.seg_begin = c.take<uint32_t>(n), v.seg_end = c.take<uint32_t>(n);
}

namespace {
// the workspace of a call: the header, the grid, what the folding forms add, the sort's temporaries
size_t voxel_layout(void* base, VoxelArgs& a, size_t temp_bytes, void** temp) {
    const size_t folds = a.form == VOXEL_FORM_AVERAGE || a.form == VOXEL_FORM_NORMALS ? a.n : 0;
    Carver c(base);
    a.hdr = c.take<VoxelHeader>(1);
    carve_voxel_grid(c, a);
    a.keep = c.take<uint32_t>(folds), a.pos = c.take<uint32_t>(folds);
    a.rows = c.take<double>(folds * (a.form == VOXEL_FORM_NORMALS ? 6 : a.cols));
    *temp = c.take<uint8_t>(temp_bytes);
    return c.total;
}

// everything but the device: NULL / dtype / stride / table_log2; 1: nothing to do (n == 0)
int voxel_validate_call(const ouster_hip_voxel_desc* d, uint64_t* n_out) {
    if (!d || !n_out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    *n_out = 0;
    if (d->n == 0 && !d->normals) return 1;
    if (const char* msg = voxel_validate(d)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", msg);
    if (!float_elem(d->dtype)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dtype must be F32 or F64");
    if (d->row_stride && d->row_stride < d->cols) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "row_stride is smaller than cols");
    if (d->table_log2 && (d->table_log2 > 31 || (1ull << d->table_log2) <= d->n))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "voxel_downsample: 2^table_log2 must exceed n (table_log2 <= 31)");
    if (d->n == 0) return 1;
    if (!d->points || (d->out_capacity && (!d->out || (d->normals && !d->out_normals)))) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    return OUSTER_HIP_OK;
}

// d: every array in device memory, validated, a form the GPU takes
int voxel_device(ouster_hip_ctx* ctx, const ouster_hip_voxel_desc* d, uint64_t* n_out) {
    if (d->n > VOXEL_MAX_POINTS) return fail(OUSTER_HIP_ERR_UNSUPPORTED, "voxel_downsample: more than 2^30 points");
    HIP_TRY(hipSetDevice(ctx->device));
    VoxelArgs a{};
    a.points = d->points, a.normals = d->normals;
    a.n = (uint32_t)d->n, a.cols = d->cols;
    a.stride = d->row_stride ? d->row_stride : d->cols;
    a.f32 = d->dtype == OUSTER_HIP_F32;
    a.form = voxel_form(d);
    a.inv = 1.0 / d->voxel_size;
    a.min_pts = d->min_pts_threshold;
    a.out = d->out, a.out_normals = d->out_normals, a.out_capacity = d->out_capacity;
    uint32_t log2 = d->table_log2;
    if (!log2)
        for (log2 = 1; (1ull << log2) < 2 * d->n; ++log2) {}
    a.table_mask = (uint32_t)((1ull << log2) - 1);
    size_t temp_bytes = 0;
    HIP_TRY(voxel_temp_bytes(a.n, &temp_bytes));
    void* temp = nullptr;
    const size_t total = voxel_layout(nullptr, a, temp_bytes, &temp);
    if (const int rc = grow_idle(ctx, ctx->voxel_ws, total, "voxel workspace", true)) return rc;
    voxel_layout(ctx->voxel_ws.p, a, temp_bytes, &temp);
    ctx->voxel_timer.timed = false;
    HIP_TRY(voxel_run(a, temp, temp_bytes, ctx->stream, ctx->voxel_timer.on ? ctx->voxel_timer.ev : nullptr));
    VoxelHeader hdr{};
    HIP_TRY(hipMemcpyAsync(&hdr, a.hdr, sizeof hdr, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->voxel_timer.timed = ctx->voxel_timer.on;
    if (hdr.status == VOXEL_STATUS_TABLE) return fail(OUSTER_HIP_ERR_RUNTIME, "voxel_downsample: hash table exhausted");
    if (hdr.status) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", VOXEL_MSG_GRID);
    *n_out = hdr.n_out;
    if (hdr.n_out > d->out_capacity) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "voxel_downsample: out_capacity is too small");
    return OUSTER_HIP_OK;
}
}  // namespace

int ouster_hip_voxel_timing(ouster_hip_ctx* ctx, int on) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    return ctx->voxel_timer.enable(ctx->device, on != 0);
}

int ouster_hip_voxel_phase_ms(ouster_hip_ctx* ctx, float* ms) {
    if (!ctx || !ms) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!ctx->voxel_timer.timed) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "voxel_downsample: no timed call (ouster_hip_voxel_timing)");
    for (int k = 0; k < OUSTER_HIP_VOXEL_PHASES; ++k) HIP_TRY(hipEventElapsedTime(&ms[k], ctx->voxel_timer.ev[k], ctx->voxel_timer.ev[k + 1]));
    return OUSTER_HIP_OK;
}

int ouster_hip_voxel_downsample(ouster_hip_ctx* ctx, const ouster_hip_voxel_desc* desc, uint64_t* n_out) {
    const int rc = voxel_validate_call(desc, n_out);
    if (rc != OUSTER_HIP_OK) return rc == 1 ? OUSTER_HIP_OK : rc;
    if (voxel_form(desc) == VOXEL_FORM_HOST)
        return fail(OUSTER_HIP_ERR_UNSUPPORTED, "voxel_downsample: FIRST_N_POINT / RANDOM with max_points_per_voxel > 1 run on the host (the _host form)");
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    return voxel_device(ctx, desc, n_out);
}

int ouster_hip_voxel_downsample_host(ouster_hip_ctx* ctx, const ouster_hip_voxel_desc* desc, uint64_t* n_out) {
    int rc = voxel_validate_call(desc, n_out);
    if (rc != OUSTER_HIP_OK) return rc == 1 ? OUSTER_HIP_OK : rc;
    if (voxel_form(desc) == VOXEL_FORM_HOST) return ouster_hip_voxel_downsample_ref(desc, n_out);
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (desc->n > VOXEL_MAX_POINTS) return fail(OUSTER_HIP_ERR_UNSUPPORTED, "voxel_downsample: more than 2^30 points");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t es = float_elem(desc->dtype), stride = desc->row_stride ? desc->row_stride : desc->cols;
    const bool wn = desc->normals != nullptr;
    using Ref = Staging::Ref;
    Staging st(ctx);
    const Ref in = st.input(desc->points, ((size_t)(desc->n - 1) * stride + desc->cols) * es);
    const Ref in_n = wn ? st.input(desc->normals, (size_t)desc->n * 24) : Ref{};
    // foreign output memory gets scratch that is copied back only after success: a call that refuses leaves the caller's array
    // alone.  A result of no rows still needs somewhere to point
    static double none[3];
    const Ref out = st.output(desc->out_capacity ? (void*)desc->out : (void*)none, (size_t)desc->out_capacity * desc->cols * 8);
    const Ref out_n = wn ? st.output(desc->out_capacity ? (void*)desc->out_normals : (void*)none, (size_t)desc->out_capacity * 24) : Ref{};
    rc = st.stage();
    if (rc != OUSTER_HIP_OK) return rc;
    ouster_hip_voxel_desc d = *desc;
    d.points = st.dev(in), d.out = (double*)st.dev(out);
    if (wn) d.normals = (const double*)st.dev(in_n), d.out_normals = (double*)st.dev(out_n);
    rc = voxel_device(ctx, &d, n_out);
    if (rc != OUSTER_HIP_OK) return rc;
    // only the rows of the result travel back
    st.set_bytes(out, (size_t)*n_out * desc->cols * 8);
    if (wn) st.set_bytes(out_n, (size_t)*n_out * 24);
    return st.finish();
}
