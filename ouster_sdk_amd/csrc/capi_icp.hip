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
    if (const int rc = grow_idle(ctx, ctx->icp_ws, total, "icp workspace", true)) return rc;
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

// the passes of one source from d->initial_guess over the grid c.a holds, the reference's loop: a launch sequence, one read-back
// and the host solve per pass.  timing: events of the context's timer around the phases (ev[2] on)
int icp_loop(ouster_hip_ctx* ctx, IcpCall& c, ouster_hip_icp_desc* d, bool timing) {
    hipEvent_t* ev = ctx->icp_timer.ev;
    double pose[16];
    memcpy(pose, d->initial_guess, sizeof pose);
    uint32_t iterations = 0, solved = 0;
    uint64_t count = 0;
    for (uint32_t it = 0; it < ICP_MAX_ITERATIONS; ++it) {
        IcpReadback rb{};
        const int rc = icp_pass(ctx, c, pose, rb, timing ? ev + 2 + 4 * it : nullptr);
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
    rc = icp_loop(ctx, c, d, timing);
    if (rc != OUSTER_HIP_OK) return rc;
    ctx->icp_timer.timed = timing;
    ctx->icp_timed_passes = d->iterations;
    return OUSTER_HIP_OK;
}
}  // namespace

// ---- IcpTarget: the grid of a target kept in device memory of its own, and many sources per call ----
struct ouster_hip_icp_target {
    ouster_hip_ctx* ctx = nullptr;   // whose stream and workspace built it and serve it; NULL: fewer than 20 rows, made without one
    int device = 0;
    void* mem = nullptr;             // slots, slot_end, sidx, rows: what a query reads
    size_t bytes = 0;
    IcpSlot* slots = nullptr;
    uint32_t *slot_end = nullptr, *sidx = nullptr;
    double* rows = nullptr;
    uint32_t table_mask = 0, n_tgt = 0;
    bool plane = false;
    double max_corr_dist = 0.0, inv = 0.0, max_d2 = 0.0;
    uint64_t rows_given = 0, rows_used = 0, cells = 0;
};

namespace {
size_t icp_target_layout(void* base, ouster_hip_icp_target& t) {
    const size_t slots = (size_t)t.table_mask + 1;
    Carver k(base);
    t.slots = k.take<IcpSlot>(slots), t.slot_end = k.take<uint32_t>(slots), t.sidx = k.take<uint32_t>(t.n_tgt);
    t.rows = k.take<double>((size_t)t.n_tgt * (t.plane ? 6 : 3));
    return k.total;
}

void icp_target_free(ouster_hip_icp_target* t) {
    if (!t) return;
    if (t->mem) {   // on the handle's device, and back: a destroy leaves the caller's thread where it was
        int before = -1;
        const bool known = hipGetDevice(&before) == hipSuccess;
        (void)hipSetDevice(t->device);
        counted_free(t->mem);
        if (known && before != t->device) (void)hipSetDevice(before);
    }
    delete t;
}

// what create refuses before a GPU is looked at; 1: fewer than 20 rows
int icp_target_validate_call(const ouster_hip_icp_target_desc* d, ouster_hip_icp_target** out) {
    if (out) *out = nullptr;
    if (!d || !out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (const char* msg = icp_target_validate(d)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", msg);
    if (d->n > ICP_MAX_ROWS) return fail(OUSTER_HIP_ERR_UNSUPPORTED, "icp: more than 2^30 rows");
    return d->n < ICP_MIN_POINTS ? 1 : OUSTER_HIP_OK;
}

ouster_hip_icp_target* icp_target_new(ouster_hip_ctx* ctx, const ouster_hip_icp_target_desc* d) {
    ouster_hip_icp_target* t = new ouster_hip_icp_target;
    t->ctx = ctx, t->device = ctx ? ctx->device : 0;
    t->plane = d->normals != nullptr;
    t->max_corr_dist = d->max_corr_dist, t->inv = 1.0 / d->max_corr_dist, t->max_d2 = d->max_corr_dist * d->max_corr_dist;
    t->rows_given = d->n;
    return t;
}

// d: arrays in device memory, validated, at least 20 rows.  The handle's allocation first; then, all on the stream, the grid of
// ouster_hip_icp_align in the context's workspace, the count of the rows that take part, what a query reads copied into the handle,
// and the read-back; one synchronisation, after which the grid's refusals surface
int icp_target_build(ouster_hip_ctx* ctx, const ouster_hip_icp_target_desc* d, ouster_hip_icp_target* t) {
    ouster_hip_icp_desc sd{};   // the target side of a single call; no source row is ever read
    sd.source_points = sd.target_points = d->points, sd.source_normals = sd.target_normals = d->normals;
    sd.n_source = sd.n_source_normals = ICP_MIN_POINTS, sd.n_target = sd.n_target_normals = d->n;
    sd.target_stride = d->stride, sd.target_normal_stride = d->normal_stride;
    sd.dtype = d->dtype, sd.max_corr_dist = d->max_corr_dist;
    IcpCall c;
    int rc = icp_prepare(ctx, &sd, c);
    if (rc != OUSTER_HIP_OK) return rc;
    t->table_mask = c.a.table_mask, t->n_tgt = c.a.n_tgt;
    t->bytes = icp_target_layout(nullptr, *t);
    if (counted_malloc(&t->mem, t->bytes) != hipSuccess) {
        t->mem = nullptr;
        return fail(OUSTER_HIP_ERR_RUNTIME, "out of device memory (icp target, %zu bytes)", t->bytes);
    }
    icp_target_layout(t->mem, *t);
    HIP_TRY(icp_grid_run(c.a, c.va, c.temp, c.temp_bytes, ctx->stream));
    HIP_TRY(launch_icp_rows_used(c.a, ctx->stream));   // -> rb.pass.count
    const size_t slots = (size_t)t->table_mask + 1, nt = t->n_tgt;
    HIP_TRY(hipMemcpyAsync(t->slots, c.a.slots, slots * sizeof(IcpSlot), hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(t->slot_end, c.a.slot_end, slots * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(t->sidx, c.a.sidx, nt * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(t->rows, c.a.rows, nt * (t->plane ? 6 : 3) * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    IcpReadback rb{};
    HIP_TRY(hipMemcpyAsync(&rb, c.a.rb, sizeof rb, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (rb.grid.status) return fail(OUSTER_HIP_ERR_RUNTIME, "icp: hash table exhausted");
    if (rb.pass.status) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", icp_msg_grid(c.method));
    if (rb.grid.n_vox > c.a.n_tgt) return fail(OUSTER_HIP_ERR_RUNTIME, "icp_target: %u cells of %u rows", rb.grid.n_vox, c.a.n_tgt);
    t->cells = rb.grid.n_vox, t->rows_used = rb.pass.count;
    return OUSTER_HIP_OK;
}

int icp_target_create(ouster_hip_ctx* ctx, const ouster_hip_icp_target_desc* d, ouster_hip_icp_target** out) {
    ouster_hip_icp_target* t = icp_target_new(ctx, d);
    const int rc = icp_target_build(ctx, d, t);
    if (rc != OUSTER_HIP_OK) return icp_target_free(t), rc;
    *out = t;
    return OUSTER_HIP_OK;
}

// the many-source call: the host's tables, the workspace and the state of every source across the passes
struct IcpManyCall {
    IcpManyArgs m{};
    uint8_t* temp = nullptr;
    size_t temp_bytes = 0;
    IcpMethod method = ICP_POINT;
    std::vector<uint8_t> table;         // what goes up: sources, seg_begin, seg_end (again once per pass), then the chunks
    size_t per_pass_bytes = 0;          //   ... the bytes of the first three
    std::vector<IcpHeader> hdr;         // the read-back of a pass
    IcpSource* sources() { return reinterpret_cast<IcpSource*>(table.data()); }
    uint32_t* seg_begin() { return reinterpret_cast<uint32_t*>(table.data() + sizeof(IcpSource) * m.n_sources); }
    uint32_t* seg_end() { return seg_begin() + m.n_sources; }
};

size_t icp_many_layout(void* base, IcpManyCall& c) {
    IcpManyArgs& m = c.m;
    const size_t ns = m.n_rows;
    Carver k(base);
    m.hdr = k.take<IcpHeader>(m.n_sources), m.counts = k.take<uint32_t>(m.n_sources);
    m.q.nn = k.take<int32_t>(ns), m.q.r = k.take<double>(ns), m.q.key = k.take<uint64_t>(ns), m.key_sorted = k.take<uint64_t>(ns);
    m.q.flag = k.take<uint32_t>(ns), m.q.xq = k.take<double>(ns * 6);
    m.partials = k.take<double>((size_t)m.n_chunks * OUSTER_HIP_ICP_SUMS);
    c.temp = k.take<uint8_t>(c.temp_bytes);
    return k.total;
}

// sources: device arrays, validated; take[k]: source k takes part (20 rows or more).  Builds both tables and lays the workspace
// out; launches nothing
int icp_many_prepare(ouster_hip_ctx* ctx, const ouster_hip_icp_target* t, const ouster_hip_icp_source* sources, uint32_t n_sources,
                     int32_t dtype, double angle, IcpManyCall& c) {
    HIP_TRY(hipSetDevice(ctx->device));
    IcpManyArgs& m = c.m;
    c.method = t->plane ? ICP_PLANE : ICP_POINT;
    m.q = IcpQuery{t->plane, t->table_mask, t->n_tgt, t->inv, t->max_d2, t->plane ? icp_cos_gate(angle) : 0.0,
                   t->slots, t->slot_end, t->sidx, t->rows, nullptr, nullptr, nullptr, nullptr, nullptr};
    m.n_sources = n_sources, m.f32 = dtype == OUSTER_HIP_F32, m.max_corr_dist = t->max_corr_dist;
    std::vector<uint64_t> rows(n_sources), first_row(n_sources), first_chunk(n_sources);
    for (uint32_t k = 0; k < n_sources; ++k) rows[k] = sources[k].n >= ICP_MIN_POINTS ? sources[k].n : 0;
    const uint64_t n_chunks = icp_chunk_table(rows.data(), n_sources, nullptr, 0, first_row.data(), first_chunk.data());
    m.n_chunks = (uint32_t)n_chunks;
    m.n_rows = (uint32_t)(first_row[n_sources - 1] + rows[n_sources - 1]);
    c.per_pass_bytes = (sizeof(IcpSource) * n_sources + 2 * sizeof(uint32_t) * n_sources + 15) & ~(size_t)15;
    c.table.assign(c.per_pass_bytes + sizeof(IcpChunk) * n_chunks, 0);
    icp_chunk_table(rows.data(), n_sources, reinterpret_cast<IcpChunk*>(c.table.data() + c.per_pass_bytes), n_chunks, nullptr, nullptr);
    for (uint32_t k = 0; k < n_sources; ++k) {
        IcpSource& s = c.sources()[k];
        s.src = sources[k].points, s.src_n = sources[k].normals;
        s.src_stride = sources[k].stride ? sources[k].stride : 3, s.src_n_stride = sources[k].normal_stride ? sources[k].normal_stride : 3;
        s.n = (uint32_t)rows[k], s.first = (uint32_t)first_row[k];
        s.first_chunk = (uint32_t)first_chunk[k], s.chunks = icp_chunks(s.n);
        s.active = rows[k] != 0;
        c.seg_begin()[k] = s.first;
    }
    c.hdr.assign(n_sources, IcpHeader{});
    HIP_TRY(icp_many_temp_bytes(m.n_rows, m.n_sources, &c.temp_bytes));
    const size_t total = icp_many_layout(nullptr, c);
    if (const int rc = grow_idle(ctx, ctx->icp_ws, total, "icp workspace", true)) return rc;
    icp_many_layout(ctx->icp_ws.p, c);
    return OUSTER_HIP_OK;
}

// one pass of every active source from the poses of the source table, and the read-back of the headers.  first: the chunk table
// goes up too; later passes send the sources (poses, flags) and their segments again
int icp_many_pass(ouster_hip_ctx* ctx, IcpManyCall& c, bool first) {
    IcpManyArgs& m = c.m;
    for (uint32_t k = 0; k < m.n_sources; ++k) {
        const IcpSource& s = c.sources()[k];
        c.seg_end()[k] = s.active ? s.first + s.n : s.first;
    }
    const int rc = upload_table(ctx, c.table.data(), first ? c.table.size() : c.per_pass_bytes);
    if (rc != OUSTER_HIP_OK) return rc;
    const uint8_t* dev = static_cast<const uint8_t*>(ctx->tables.p);
    m.sources = reinterpret_cast<const IcpSource*>(dev);
    m.seg_begin = reinterpret_cast<const uint32_t*>(dev + sizeof(IcpSource) * m.n_sources), m.seg_end = m.seg_begin + m.n_sources;
    m.chunks = reinterpret_cast<const IcpChunk*>(dev + c.per_pass_bytes);
    // every call starts from clean headers, like the single call: the sums a method does not write read as zero
    if (first) HIP_TRY(hipMemsetAsync(m.hdr, 0, sizeof(IcpHeader) * m.n_sources, ctx->stream));
    HIP_TRY(icp_many_pass_run(m, c.temp, c.temp_bytes, ctx->stream));
    HIP_TRY(hipMemcpyAsync(c.hdr.data(), m.hdr, sizeof(IcpHeader) * m.n_sources, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return OUSTER_HIP_OK;
}

void icp_source_guess_is_the_answer(ouster_hip_icp_source* s) {
    memcpy(s->pose, s->initial_guess, sizeof s->pose);
    s->iterations = 0, s->solved = 0, s->correspondences = 0;
}

// what align and step refuse before a GPU is looked at
int icp_many_validate_call(ouster_hip_ctx* ctx, const ouster_hip_icp_target* t, const ouster_hip_icp_source* sources, uint32_t n_sources,
                           int32_t dtype, double angle) {
    if (!t || (n_sources && !sources)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (t->ctx != ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "icp_target: made by another context");
    char msg[160];
    const int rc = icp_sources_validate(t->plane, sources, n_sources, dtype, angle, msg, sizeof msg);
    return rc == OUSTER_HIP_OK ? rc : fail(rc, "%s", msg);
}

// sources: every array in device memory, validated; results into `results` (the caller's sources, or copies of them)
int icp_many_device(ouster_hip_ctx* ctx, const ouster_hip_icp_target* t, ouster_hip_icp_source* sources, uint32_t n_sources, int32_t dtype,
                    double angle) {
    struct State {
        double pose[16];
        uint32_t iterations = 0, solved = 0;
        uint64_t count = 0;
    };
    IcpManyCall c;
    int rc = icp_many_prepare(ctx, t, sources, n_sources, dtype, angle, c);
    if (rc != OUSTER_HIP_OK) return rc;
    std::vector<State> st(n_sources);
    uint32_t active = 0;
    for (uint32_t k = 0; k < n_sources; ++k) {
        memcpy(st[k].pose, sources[k].initial_guess, sizeof st[k].pose);
        memcpy(c.sources()[k].pose, st[k].pose, sizeof st[k].pose);
        active += c.sources()[k].active != 0;
    }
    for (uint32_t it = 0; it < ICP_MAX_ITERATIONS && active; ++it) {
        rc = icp_many_pass(ctx, c, it == 0);
        if (rc != OUSTER_HIP_OK) return rc;
        for (uint32_t k = 0; k < n_sources; ++k) {
            IcpSource& s = c.sources()[k];
            if (!s.active) continue;
            const IcpHeader& h = c.hdr[k];
            State& v = st[k];
            ++v.iterations;
            v.count = h.count;
            v.solved |= v.count >= ICP_MIN_POINTS;
            double next[16];
            bool stop = true;
            icp_finish_pass(c.method, v.count, h.sums, h.centroid_x, h.centroid_q, v.pose, next, &stop);
            memcpy(v.pose, next, sizeof v.pose);
            memcpy(s.pose, next, sizeof s.pose);
            if (stop || it + 1 == ICP_MAX_ITERATIONS) s.active = 0, --active;
        }
    }
    for (uint32_t k = 0; k < n_sources; ++k) {
        memcpy(sources[k].pose, st[k].solved ? st[k].pose : sources[k].initial_guess, sizeof st[k].pose);
        sources[k].iterations = st[k].iterations, sources[k].solved = st[k].solved, sources[k].correspondences = st[k].count;
    }
    return OUSTER_HIP_OK;
}

// One source of at least 20 rows, arrays in device memory, validated: the pass sequence of ouster_hip_icp_align itself (icp_pass_run:
// a row per thread, the pose as a kernel argument, no table) over the handle's grid.  A lone source then costs what the single call
// costs less the grid; the kernels are the single call's, so are the bits.
int icp_one_device(ouster_hip_ctx* ctx, const ouster_hip_icp_target* t, ouster_hip_icp_source* s, int32_t dtype, double angle) {
    HIP_TRY(hipSetDevice(ctx->device));
    IcpCall c;
    IcpArgs& a = c.a;
    c.method = t->plane ? ICP_PLANE : ICP_POINT;
    a.src = s->points, a.src_n = s->normals;
    a.src_stride = s->stride ? s->stride : 3, a.src_n_stride = s->normal_stride ? s->normal_stride : 3;
    a.n_src = (uint32_t)s->n, a.n_tgt = t->n_tgt;
    a.f32 = dtype == OUSTER_HIP_F32, a.plane = t->plane;
    a.inv = t->inv, a.max_d2 = t->max_d2, a.max_corr_dist = t->max_corr_dist;
    a.cos_gate = t->plane ? icp_cos_gate(angle) : 0.0;
    a.table_mask = t->table_mask;
    HIP_TRY(icp_temp_bytes(a.n_src, t->n_tgt, &c.temp_bytes));
    auto layout = [&](void* base) {   // the source side of icp_layout; the target side is the handle's
        const size_t ns = a.n_src;
        Carver k(base);
        a.rb = k.take<IcpReadback>(1);
        a.nn = k.take<int32_t>(ns), a.r = k.take<double>(ns), a.key = k.take<uint64_t>(ns), a.key_sorted = k.take<uint64_t>(ns);
        a.flag = k.take<uint32_t>(ns), a.xq = k.take<double>(ns * 6);
        a.partials = k.take<double>((size_t)icp_chunks(a.n_src) * OUSTER_HIP_ICP_SUMS);
        c.temp = k.take<uint8_t>(c.temp_bytes);
        return k.total;
    };
    const size_t total = layout(nullptr);
    if (const int rc = grow_idle(ctx, ctx->icp_ws, total, "icp workspace", true)) return rc;
    layout(ctx->icp_ws.p);
    a.slots = t->slots, a.slot_end = t->slot_end, a.sidx = t->sidx, a.rows = t->rows;
    HIP_TRY(hipMemsetAsync(a.rb, 0, sizeof(IcpReadback), ctx->stream));   // a clean header, as after the grid of a single call
    ouster_hip_icp_desc d{};
    memcpy(d.initial_guess, s->initial_guess, sizeof d.initial_guess);
    const int rc = icp_loop(ctx, c, &d, false);
    if (rc != OUSTER_HIP_OK) return rc;
    memcpy(s->pose, d.pose, sizeof d.pose);
    s->iterations = d.iterations, s->solved = d.solved, s->correspondences = d.correspondences;
    return OUSTER_HIP_OK;
}

// true: nothing can be launched (a target or every source of fewer than 20 rows): every source gets its guess
bool icp_many_is_trivial(const ouster_hip_icp_target* t, const ouster_hip_icp_source* sources, uint32_t n_sources) {
    if (t->rows_given < ICP_MIN_POINTS) return true;
    for (uint32_t k = 0; k < n_sources; ++k)
        if (sources[k].n >= ICP_MIN_POINTS) return false;
    return true;
}
}  // namespace

int ouster_hip_icp_target_create(ouster_hip_ctx* ctx, const ouster_hip_icp_target_desc* desc, ouster_hip_icp_target** out) {
    const int rc = icp_target_validate_call(desc, out);
    if (rc < 0) return rc;
    if (rc == 1) return *out = icp_target_new(ctx, desc), OUSTER_HIP_OK;
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    return icp_target_create(ctx, desc, out);
}

int ouster_hip_icp_target_create_host(ouster_hip_ctx* ctx, const ouster_hip_icp_target_desc* desc, ouster_hip_icp_target** out) {
    int rc = icp_target_validate_call(desc, out);
    if (rc < 0) return rc;
    if (rc == 1) return *out = icp_target_new(ctx, desc), OUSTER_HIP_OK;
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t es = float_elem(desc->dtype);
    auto bytes = [es](uint64_t n, uint64_t stride) { return ((size_t)(n - 1) * (stride ? stride : 3) + 3) * es; };
    Staging st(ctx);   // inputs only; the build synchronises before it returns
    const Staging::Ref pts = st.input(desc->points, bytes(desc->n, desc->stride));
    const Staging::Ref nrm = desc->normals ? st.input(desc->normals, bytes(desc->n, desc->normal_stride)) : Staging::Ref{};
    rc = st.stage();
    if (rc != OUSTER_HIP_OK) return rc;
    ouster_hip_icp_target_desc d = *desc;
    d.points = st.dev(pts);
    if (desc->normals) d.normals = st.dev(nrm);
    return icp_target_create(ctx, &d, out);
}

void ouster_hip_icp_target_destroy(ouster_hip_icp_target* target) { icp_target_free(target); }

int ouster_hip_icp_target_info_read(const ouster_hip_icp_target* t, ouster_hip_icp_target_info* info) {
    if (!t || !info) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    *info = ouster_hip_icp_target_info{t->rows_given, t->rows_used, t->cells, t->bytes, t->plane ? 1 : 0, 0, t->max_corr_dist};
    return OUSTER_HIP_OK;
}

int ouster_hip_icp_target_align(ouster_hip_ctx* ctx, const ouster_hip_icp_target* t, ouster_hip_icp_source* sources, uint32_t n_sources,
                                int32_t dtype, double max_normal_angle_deg) {
    const int rc = icp_many_validate_call(ctx, t, sources, n_sources, dtype, max_normal_angle_deg);
    if (rc != OUSTER_HIP_OK) return rc;
    if (icp_many_is_trivial(t, sources, n_sources)) {
        for (uint32_t k = 0; k < n_sources; ++k) icp_source_guess_is_the_answer(sources + k);
        return OUSTER_HIP_OK;
    }
    if (n_sources == 1) return icp_one_device(ctx, t, sources, dtype, max_normal_angle_deg);
    return icp_many_device(ctx, t, sources, n_sources, dtype, max_normal_angle_deg);
}

int ouster_hip_icp_target_align_host(ouster_hip_ctx* ctx, const ouster_hip_icp_target* t, ouster_hip_icp_source* sources, uint32_t n_sources,
                                     int32_t dtype, double max_normal_angle_deg) {
    int rc = icp_many_validate_call(ctx, t, sources, n_sources, dtype, max_normal_angle_deg);
    if (rc != OUSTER_HIP_OK) return rc;
    if (icp_many_is_trivial(t, sources, n_sources)) {
        for (uint32_t k = 0; k < n_sources; ++k) icp_source_guess_is_the_answer(sources + k);
        return OUSTER_HIP_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t es = float_elem(dtype);
    auto bytes = [es](uint64_t n, uint64_t stride) { return ((size_t)(n - 1) * (stride ? stride : 3) + 3) * es; };
    Staging st(ctx);   // inputs only: the results are poses
    std::vector<ouster_hip_icp_source> dev(sources, sources + n_sources);
    std::vector<Staging::Ref> pts(n_sources), nrm(n_sources);
    for (uint32_t k = 0; k < n_sources; ++k) {
        if (sources[k].n < ICP_MIN_POINTS) continue;   // takes no part: nothing of it is read
        pts[k] = st.input(sources[k].points, bytes(sources[k].n, sources[k].stride));
        if (sources[k].normals) nrm[k] = st.input(sources[k].normals, bytes(sources[k].n, sources[k].normal_stride));
    }
    rc = st.stage();
    if (rc != OUSTER_HIP_OK) return rc;
    for (uint32_t k = 0; k < n_sources; ++k) {
        if (sources[k].n < ICP_MIN_POINTS) continue;
        dev[k].points = st.dev(pts[k]);
        if (sources[k].normals) dev[k].normals = st.dev(nrm[k]);
    }
    rc = n_sources == 1 ? icp_one_device(ctx, t, dev.data(), dtype, max_normal_angle_deg)
                        : icp_many_device(ctx, t, dev.data(), n_sources, dtype, max_normal_angle_deg);
    if (rc != OUSTER_HIP_OK) return rc;
    for (uint32_t k = 0; k < n_sources; ++k) {
        memcpy(sources[k].pose, dev[k].pose, sizeof dev[k].pose);
        sources[k].iterations = dev[k].iterations, sources[k].solved = dev[k].solved, sources[k].correspondences = dev[k].correspondences;
    }
    return OUSTER_HIP_OK;
}

int ouster_hip_icp_target_step(ouster_hip_ctx* ctx, const ouster_hip_icp_target* t, const ouster_hip_icp_source* sources, uint32_t n_sources,
                               int32_t dtype, double max_normal_angle_deg, const double* poses, ouster_hip_icp_step_out* outs) {
    if (n_sources && (!poses || !outs)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    int rc = icp_many_validate_call(ctx, t, sources, n_sources, dtype, max_normal_angle_deg);
    if (rc != OUSTER_HIP_OK) return rc;
    if (n_sources == 0) return OUSTER_HIP_OK;
    bool small = t->rows_given < ICP_MIN_POINTS;
    for (uint32_t k = 0; k < n_sources; ++k) small |= sources[k].n < ICP_MIN_POINTS;
    if (small) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "icp_step: fewer than 20 rows");
    IcpManyCall c;
    rc = icp_many_prepare(ctx, t, sources, n_sources, dtype, max_normal_angle_deg, c);
    if (rc != OUSTER_HIP_OK) return rc;
    for (uint32_t k = 0; k < n_sources; ++k) memcpy(c.sources()[k].pose, poses + 16 * (size_t)k, sizeof c.sources()[k].pose);
    rc = icp_many_pass(ctx, c, true);
    if (rc != OUSTER_HIP_OK) return rc;
    for (uint32_t k = 0; k < n_sources; ++k) {
        const IcpSource& s = c.sources()[k];
        if (outs[k].nn) HIP_TRY(hipMemcpyAsync(outs[k].nn, c.m.q.nn + s.first, (size_t)s.n * 4, hipMemcpyDeviceToDevice, ctx->stream));
        if (outs[k].r) HIP_TRY(hipMemcpyAsync(outs[k].r, c.m.q.r + s.first, (size_t)s.n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (uint32_t k = 0; k < n_sources; ++k) {
        const IcpHeader& h = c.hdr[k];
        ouster_hip_icp_step_out* out = outs + k;
        const bool solved = h.count >= ICP_MIN_POINTS;
        out->count = h.count;
        out->median = h.median, out->huber_delta = h.huber_delta;
        for (int i = 0; i < OUSTER_HIP_ICP_SUMS; ++i) out->sums[i] = solved ? h.sums[i] : 0.0;
        for (int i = 0; i < 3; ++i) {
            out->centroid_x[i] = solved && c.method == ICP_POINT ? h.centroid_x[i] : 0.0;
            out->centroid_q[i] = solved && c.method == ICP_POINT ? h.centroid_q[i] : 0.0;
        }
        bool stop = true;
        icp_finish_pass(c.method, h.count, h.sums, h.centroid_x, h.centroid_q, poses + 16 * (size_t)k, out->next_pose, &stop);
        out->stop = stop, out->solved = solved;
    }
    return OUSTER_HIP_OK;
}

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
