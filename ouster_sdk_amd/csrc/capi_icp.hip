// capi_icp.hip -- the C ABI of ICP, point_to_point_align / point_to_plane_align (k_icp.hip, host/icp_util.cpp): ouster_hip_icp_*
#include "capi_internal.h"
#include "carve.h"
#include "k_icp.h"

using namespace ouster_hip_dev;

namespace {
struct IcpCall {
    IcpArgs a{};
    VoxelArgs va{};
    uint8_t* temp = nullptr;
    size_t temp_bytes = 0;
    IcpMethod method = ICP_POINT;
};

// the workspace of a call: the read-back, the target grid as the launchers of k_voxel.h see it (c.va), ICP's own view of it,
// the per-row outputs of a pass, partial sums, the sorts' temporaries
size_t icp_layout(void* base, IcpCall& c) {
    IcpArgs& a = c.a;
    VoxelArgs& v = c.va;
    const size_t nt = a.n_tgt, ns = a.n_src, slots = (size_t)a.table_mask + 1;
    Carver k(base);
    a.rb = k.take<IcpReadback>(1);
    v.n = a.n_tgt, v.table_mask = a.table_mask, v.hdr = a.rb ? &a.rb->grid : nullptr;
    carve_voxel_grid(k, v);
    a.keys = v.keys, a.table = v.table, a.first_id = v.first_id, a.svid = v.svid, a.sidx = v.sidx;
    a.seg_begin = v.seg_begin, a.seg_end = v.seg_end;
    a.slots = k.take<IcpSlot>(slots), a.slot_end = k.take<uint32_t>(slots), a.rows = k.take<double>(nt * (a.plane ? 6 : 3));
    a.nn = k.take<int32_t>(ns), a.r = k.take<double>(ns), a.key = k.take<uint64_t>(ns), a.key_sorted = k.take<uint64_t>(ns);
    a.flag = k.take<uint32_t>(ns), a.xq = k.take<double>(ns * 6);
    a.partials = k.take<double>((size_t)icp_chunks(a.n_src) * OUSTER_HIP_ICP_SUMS);
    c.temp = k.take<uint8_t>(c.temp_bytes);
    return k.total;
}

// what every entry point refuses before a GPU is looked at; 1: fewer than 20 rows on a side (the guess is the answer)
int icp_validate_call(const ouster_hip_icp_desc* d) {
    if (!d) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (const char* msg = icp_validate(d)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", msg);
    if (d->n_source > ICP_MAX_ROWS || d->n_target > ICP_MAX_ROWS) return fail(OUSTER_HIP_ERR_UNSUPPORTED, "icp: more than 2^30 rows");
    return d->n_source < ICP_MIN_POINTS || d->n_target < ICP_MIN_POINTS ? 1 : OUSTER_HIP_OK;
}

void icp_guess_is_the_answer(ouster_hip_icp_desc* d) {
    memcpy(d->pose, d->initial_guess, sizeof d->pose);
    d->iterations = 0, d->solved = 0, d->correspondences = 0;
}

// d: every array in device memory, validated, at least 20 rows a side.  Lays the workspace out; launches nothing
int icp_prepare(ouster_hip_ctx* ctx, const ouster_hip_icp_desc* d, IcpCall& c) {
    HIP_TRY(hipSetDevice(ctx->device));
    IcpArgs& a = c.a;
    c.method = icp_method(d);
    a.src = d->source_points, a.tgt = d->target_points, a.src_n = d->source_normals, a.tgt_n = d->target_normals;
    a.src_stride = d->source_stride ? d->source_stride : 3, a.tgt_stride = d->target_stride ? d->target_stride : 3;
    a.src_n_stride = d->source_normal_stride ? d->source_normal_stride : 3, a.tgt_n_stride = d->target_normal_stride ? d->target_normal_stride : 3;
    a.n_src = (uint32_t)d->n_source, a.n_tgt = (uint32_t)d->n_target;
    a.f32 = d->dtype == OUSTER_HIP_F32, a.plane = c.method == ICP_PLANE;
    a.inv = 1.0 / d->max_corr_dist;
    a.max_d2 = d->max_corr_dist * d->max_corr_dist;
    a.max_corr_dist = d->max_corr_dist;
    a.cos_gate = a.plane ? icp_cos_gate(d->max_normal_angle_deg) : 0.0;
    uint32_t log2 = 1;
    while ((1ull << log2) < 2 * d->n_target) ++log2;
    a.table_mask = (uint32_t)((1ull << log2) - 1);
    HIP_TRY(icp_temp_bytes(a.n_src, a.n_tgt, &c.temp_bytes));
    const size_t total = icp_layout(nullptr, c);
    if (ctx->icp_ws.cap < total) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (ctx->icp_ws.ensure(total)) return fail(OUSTER_HIP_ERR_RUNTIME, "out of device memory (icp workspace, %zu bytes)", total);
    }
    icp_layout(ctx->icp_ws.p, c);
    return OUSTER_HIP_OK;
}

// one pass from `pose` and its read-back; the grid's refusals come with the first one
int icp_pass(ouster_hip_ctx* ctx, IcpCall& c, const double* pose, IcpReadback& rb, hipEvent_t* ev) {
    memcpy(c.a.pose, pose, sizeof c.a.pose);
    if (ev) HIP_TRY(hipEventRecord(ev[0], ctx->stream));
    HIP_TRY(icp_pass_run(c.a, c.temp, c.temp_bytes, ctx->stream, ev ? ev + 1 : nullptr));
    HIP_TRY(hipMemcpyAsync(&rb, c.a.rb, sizeof rb, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (rb.grid.status) return fail(OUSTER_HIP_ERR_RUNTIME, "icp: hash table exhausted");
    if (rb.pass.status) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", icp_msg_grid(c.method));
    return OUSTER_HIP_OK;
}

// d: every array in device memory, validated, at least 20 rows a side
int icp_device(ouster_hip_ctx* ctx, ouster_hip_icp_desc* d) {
    IcpCall c;
    int rc = icp_prepare(ctx, d, c);
    if (rc != OUSTER_HIP_OK) return rc;
    const bool timing = ctx->icp_timer.on;
    hipEvent_t* ev = ctx->icp_timer.ev;
    ctx->icp_timer.timed = false;
    if (timing) HIP_TRY(hipEventRecord(ev[0], ctx->stream));
    HIP_TRY(icp_grid_run(c.a, c.va, c.temp, c.temp_bytes, ctx->stream));
    if (timing) HIP_TRY(hipEventRecord(ev[1], ctx->stream));
    double pose[16];
    memcpy(pose, d->initial_guess, sizeof pose);
    uint32_t iterations = 0, solved = 0;
    uint64_t count = 0;
    for (uint32_t it = 0; it < ICP_MAX_ITERATIONS; ++it) {
        IcpReadback rb{};
        rc = icp_pass(ctx, c, pose, rb, timing ? ev + 2 + 4 * it : nullptr);
        if (rc != OUSTER_HIP_OK) return rc;
        ++iterations;
        count = rb.pass.count;
        solved |= count >= ICP_MIN_POINTS;
        double next[16];
        bool stop = true;
        icp_finish_pass(c.method, count, rb.pass.sums, rb.pass.centroid_x, rb.pass.centroid_q, pose, next, &stop);
        memcpy(pose, next, sizeof pose);
        if (stop) break;
    }
    memcpy(d->pose, solved ? pose : d->initial_guess, sizeof pose);
    d->iterations = iterations, d->solved = solved, d->correspondences = count;
    ctx->icp_timer.timed = timing;
    ctx->icp_timed_passes = iterations;
    return OUSTER_HIP_OK;
}
}  // namespace

uint32_t ouster_hip_icp_chunk_rows(void) { return ICP_CHUNK; }

int ouster_hip_icp_timing(ouster_hip_ctx* ctx, int on) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    return ctx->icp_timer.enable(ctx->device, on != 0);
}

int ouster_hip_icp_phase_ms(ouster_hip_ctx* ctx, float* ms) {
    if (!ctx || !ms) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!ctx->icp_timer.timed) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "icp: no timed call (ouster_hip_icp_timing)");
    const hipEvent_t* ev = ctx->icp_timer.ev;
    for (int k = 0; k < OUSTER_HIP_ICP_PHASES; ++k) ms[k] = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms[0], ev[0], ev[1]));
    for (uint32_t it = 0; it < ctx->icp_timed_passes; ++it)
        for (int k = 0; k < 3; ++k) {
            float t = 0.0f;
            HIP_TRY(hipEventElapsedTime(&t, ev[2 + 4 * it + k], ev[2 + 4 * it + k + 1]));
            ms[1 + k] += t;
        }
    return OUSTER_HIP_OK;
}

int ouster_hip_icp_align(ouster_hip_ctx* ctx, ouster_hip_icp_desc* desc) {
    const int rc = icp_validate_call(desc);
    if (rc < 0) return rc;
    if (rc == 1) return icp_guess_is_the_answer(desc), OUSTER_HIP_OK;
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    return icp_device(ctx, desc);
}

int ouster_hip_icp_step(ouster_hip_ctx* ctx, const ouster_hip_icp_desc* desc, const double* pose16, ouster_hip_icp_step_out* out) {
    if (!pose16 || !out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    int rc = icp_validate_call(desc);
    if (rc < 0) return rc;
    if (rc == 1) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "icp_step: fewer than 20 rows");
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    IcpCall c;
    rc = icp_prepare(ctx, desc, c);
    if (rc != OUSTER_HIP_OK) return rc;
    HIP_TRY(icp_grid_run(c.a, c.va, c.temp, c.temp_bytes, ctx->stream));
    IcpReadback rb{};
    rc = icp_pass(ctx, c, pose16, rb, nullptr);
    if (rc != OUSTER_HIP_OK) return rc;
    if (out->nn) HIP_TRY(hipMemcpyAsync(out->nn, c.a.nn, (size_t)c.a.n_src * 4, hipMemcpyDeviceToDevice, ctx->stream));
    if (out->r) HIP_TRY(hipMemcpyAsync(out->r, c.a.r, (size_t)c.a.n_src * 8, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const bool solved = rb.pass.count >= ICP_MIN_POINTS;
    out->count = rb.pass.count;
    out->median = rb.pass.median, out->huber_delta = rb.pass.huber_delta;
    for (int k = 0; k < OUSTER_HIP_ICP_SUMS; ++k) out->sums[k] = solved ? rb.pass.sums[k] : 0.0;
    for (int k = 0; k < 3; ++k) {
        out->centroid_x[k] = solved && c.method == ICP_POINT ? rb.pass.centroid_x[k] : 0.0;
        out->centroid_q[k] = solved && c.method == ICP_POINT ? rb.pass.centroid_q[k] : 0.0;
    }
    bool stop = true;
    icp_finish_pass(c.method, rb.pass.count, rb.pass.sums, rb.pass.centroid_x, rb.pass.centroid_q, pose16, out->next_pose, &stop);
    out->stop = stop, out->solved = solved;
    return OUSTER_HIP_OK;
}

int ouster_hip_icp_align_host(ouster_hip_ctx* ctx, ouster_hip_icp_desc* desc) {
    int rc = icp_validate_call(desc);
    if (rc < 0) return rc;
    if (rc == 1) return icp_guess_is_the_answer(desc), OUSTER_HIP_OK;
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t es = float_elem(desc->dtype);
    auto bytes = [es](uint64_t n, uint64_t stride) { return ((size_t)(n - 1) * (stride ? stride : 3) + 3) * es; };
    using Ref = Staging::Ref;
    Staging st(ctx);   // inputs only: the result is a pose
    const bool wn = desc->source_normals != nullptr;
    const Ref src = st.input(desc->source_points, bytes(desc->n_source, desc->source_stride));
    const Ref tgt = st.input(desc->target_points, bytes(desc->n_target, desc->target_stride));
    const Ref src_n = wn ? st.input(desc->source_normals, bytes(desc->n_source, desc->source_normal_stride)) : Ref{};
    const Ref tgt_n = wn ? st.input(desc->target_normals, bytes(desc->n_target, desc->target_normal_stride)) : Ref{};
    rc = st.stage();
    if (rc != OUSTER_HIP_OK) return rc;
    ouster_hip_icp_desc d = *desc;
    d.source_points = st.dev(src), d.target_points = st.dev(tgt);
    if (wn) d.source_normals = st.dev(src_n), d.target_normals = st.dev(tgt_n);
    rc = icp_device(ctx, &d);
    if (rc != OUSTER_HIP_OK) return rc;
    memcpy(desc->pose, d.pose, sizeof d.pose);
    desc->iterations = d.iterations, desc->solved = d.solved, desc->correspondences = d.correspondences;
    return OUSTER_HIP_OK;
}
