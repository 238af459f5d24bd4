// capi_voxel_map.hip -- the C ABI of the resident voxel map (k_voxel_map.hip, host/voxel_map_util.cpp): ouster_hip_voxel_map_*
#include "capi_internal.h"
#include "capi_voxel_map.h"
#include "carve.h"
#include "k_voxel_map.h"
#include "voxel_map_host.h"

#include <exception>

using namespace ouster_hip_dev;

namespace {

constexpr uint64_t VMAP_MAX_SLOTS = 1ull << 32;   // cap * P stays below: positions in a cloud are 32-bit

void free_set(VMapSet& s) {
    counted_free(s.cell), counted_free(s.count), counted_free(s.pts);
    s = VMapSet{};
}

int alloc_set(VMapSet& s, uint64_t cap, uint64_t P) {
    if (counted_malloc((void**)&s.cell, cap * sizeof(VoxelKey)) != hipSuccess || counted_malloc((void**)&s.count, cap * sizeof(uint32_t)) != hipSuccess ||
        counted_malloc((void**)&s.pts, cap * P * 3 * sizeof(double)) != hipSuccess) {
        free_set(s);
        return -1;
    }
    return 0;
}

// the pieces `carve` takes, in the context's grow-only voxel workspace: run once to measure, once over the buffer
template <class F>
int workspace(ouster_hip_ctx* ctx, F&& carve) {
    Carver measure(nullptr);
    carve(measure);
    if (const int rc = grow_idle(ctx, ctx->voxel_ws, measure.total, "voxel workspace", true)) return rc;
    Carver c(ctx->voxel_ws.p);
    carve(c);
    return OUSTER_HIP_OK;
}

// room for `want` voxels: new arrays, the old contents copied, the table rebuilt.  Ids do not change.
int ensure_capacity(ouster_hip_voxel_map* m, uint64_t want, bool exact) {
    if (want <= m->cap) return OUSTER_HIP_OK;
    const uint64_t P = m->p.max_points;
    if (want >= (1ull << 31) || P >= VMAP_MAX_SLOTS || want * P >= VMAP_MAX_SLOTS)
        return fail(OUSTER_HIP_ERR_UNSUPPORTED, "voxel map: more than 2^32 point slots (voxels x max_points_per_voxel)");
    uint64_t cap = exact ? want : std::max<uint64_t>(std::max<uint64_t>(want, 2 * m->cap), 16);
    if (cap >= (1ull << 31) || cap * P >= VMAP_MAX_SLOTS) cap = want;
    uint64_t slots = 2;
    while (slots < 2 * cap) slots <<= 1;
    ouster_hip_ctx* ctx = m->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    VMapSet fresh[2];
    int32_t* table = nullptr;
    if (alloc_set(fresh[0], cap, P) || alloc_set(fresh[1], cap, P) || counted_malloc((void**)&table, slots * sizeof(int32_t)) != hipSuccess) {
        free_set(fresh[0]), free_set(fresh[1]);
        return fail(OUSTER_HIP_ERR_RUNTIME, "out of device memory (voxel map of %llu voxels)", (unsigned long long)cap);
    }
    VMapHeader* hdr = nullptr;
    int rc = workspace(ctx, [&](Carver& c) { hdr = c.take<VMapHeader>(1); });
    hipError_t e = hipSuccess;
    VMapHeader got{};
    if (rc == OUSTER_HIP_OK) {
        const VMapSet& old = m->set[m->cur];
        if (m->n_vox) {
            e = hipMemcpyAsync(fresh[0].cell, old.cell, (size_t)m->n_vox * sizeof(VoxelKey), hipMemcpyDeviceToDevice, ctx->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(fresh[0].count, old.count, (size_t)m->n_vox * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(fresh[0].pts, old.pts, (size_t)m->n_vox * P * 3 * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream);
        }
        VMapDev d = dev_of(m);
        d.s = fresh[0], d.table = table, d.table_mask = (uint32_t)(slots - 1), d.cap = (uint32_t)cap;
        if (e == hipSuccess) e = hipMemsetAsync(hdr, 0, sizeof(VMapHeader), ctx->stream);
        if (e == hipSuccess) e = vmap_rebuild(d, hdr, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&got, hdr, sizeof got, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    if (rc != OUSTER_HIP_OK || e != hipSuccess || got.status) {
        free_set(fresh[0]), free_set(fresh[1]), counted_free(table);
        if (rc != OUSTER_HIP_OK) return rc;
        if (e != hipSuccess) return fail(OUSTER_HIP_ERR_RUNTIME, "voxel map: growing failed: %s", hipGetErrorString(e));
        return fail(OUSTER_HIP_ERR_RUNTIME, "voxel map: hash table exhausted");
    }
    free_set(m->set[0]), free_set(m->set[1]), counted_free(m->table);
    m->set[0] = fresh[0], m->set[1] = fresh[1], m->cur = 0;
    m->table = table, m->table_mask = (uint32_t)(slots - 1), m->cap = cap;
    m->bytes = 2 * (cap * sizeof(VoxelKey) + cap * sizeof(uint32_t) + cap * P * 3 * sizeof(double)) + slots * sizeof(int32_t);
    return OUSTER_HIP_OK;
}

int validate_rows(const ouster_hip_voxel_map* m, const void* rows, int32_t dtype, uint64_t n, uint64_t stride, const char* what) {
    if (!m) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "map is NULL");
    if (!float_elem(dtype)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dtype must be F32 or F64");
    if (stride && stride < 3) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "row_stride is smaller than 3");
    if (n && !rows) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    if (n > VOXEL_MAP_MAX_ROWS) return fail(OUSTER_HIP_ERR_UNSUPPORTED, "voxel map: more than 2^30 %s", what);
    return OUSTER_HIP_OK;
}

int origin_cell(const ouster_hip_voxel_map* m, const double* origin, int32_t* cell) {
    if (!m || !origin) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!voxel_map_cell(origin, m->p.inv, cell)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", VOXEL_MAP_MSG_GRID);
    return OUSTER_HIP_OK;
}

// rows in device memory, validated, n > 0
int add_device(ouster_hip_voxel_map* m, const void* points, int32_t dtype, uint64_t n, uint64_t stride) {
    ouster_hip_ctx* ctx = m->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    VoxelArgs a{};
    a.points = points;
    a.n = (uint32_t)n, a.cols = 3;
    a.stride = stride ? stride : 3;
    a.f32 = dtype == OUSTER_HIP_F32;
    a.form = VOXEL_FORM_FIRST;
    a.inv = m->p.inv;
    uint32_t log2 = 1;
    while ((1ull << log2) < 2 * n) ++log2;
    a.table_mask = (uint32_t)((1ull << log2) - 1);
    size_t temp_bytes = 0;
    HIP_TRY(voxel_temp_bytes(a.n, &temp_bytes));
    VMapAddArgs x{};
    void* temp = nullptr;
    int rc = workspace(ctx, [&](Carver& c) {
        x.hdr = c.take<VMapHeader>(1);
        a.hdr = c.take<VoxelHeader>(1);
        carve_voxel_grid(c, a);
        x.found = c.take<uint32_t>(n), x.is_new = c.take<uint32_t>(n), x.new_pos = c.take<uint32_t>(n);
        temp = c.take<uint8_t>(temp_bytes);
    });
    if (rc != OUSTER_HIP_OK) return rc;
    HIP_TRY(vmap_add_prepare(a, dev_of(m), x, temp, temp_bytes, ctx->stream));
    VoxelHeader vh{};
    VMapHeader mh{};
    HIP_TRY(hipMemcpyAsync(&vh, a.hdr, sizeof vh, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(&mh, x.hdr, sizeof mh, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (vh.status == VOXEL_STATUS_TABLE) return fail(OUSTER_HIP_ERR_RUNTIME, "voxel map: hash table exhausted");
    if (vh.status) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", VOXEL_MAP_MSG_GRID);
    // nothing is published yet: a call that cannot get its room leaves the map as it was.  (Growing reuses the header: keep n_new)
    const uint32_t n_new = mh.n_new;
    rc = ensure_capacity(m, (uint64_t)m->n_vox + n_new, false);
    if (rc != OUSTER_HIP_OK) return rc;
    HIP_TRY(vmap_add_commit(a, dev_of(m), x, ctx->stream));
    HIP_TRY(hipMemcpyAsync(&mh, x.hdr, sizeof mh, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (mh.status) return fail(OUSTER_HIP_ERR_RUNTIME, "voxel map: hash table exhausted");
    m->n_vox += n_new;
    m->n_pts += mh.n_admitted;
    return OUSTER_HIP_OK;
}

// out: device memory or NULL (remove)
int far_device(ouster_hip_voxel_map* m, const int32_t* origin, double* out, uint64_t out_capacity, uint64_t* n_out, bool extract) {
    if (n_out) *n_out = 0;
    if (m->n_vox == 0) return OUSTER_HIP_OK;
    ouster_hip_ctx* ctx = m->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    size_t temp_bytes = 0;
    HIP_TRY(vmap_temp_bytes(m->n_vox, &temp_bytes));
    VMapFarArgs f{};
    void* temp = nullptr;
    const size_t nv = m->n_vox;
    int rc = workspace(ctx, [&](Carver& c) {
        f.hdr = c.take<VMapHeader>(1);
        f.keep = c.take<uint32_t>(nv), f.keep_pos = c.take<uint32_t>(nv), f.gone = c.take<uint32_t>(nv), f.gone_pos = c.take<uint32_t>(nv);
        temp = c.take<uint8_t>(temp_bytes);
    });
    if (rc != OUSTER_HIP_OK) return rc;
    std::memcpy(f.origin, origin, sizeof f.origin);
    f.max_voxel_dist = m->p.max_voxel_dist;
    f.out = extract ? out : nullptr;
    const VMapDev d = dev_of(m);
    HIP_TRY(vmap_far_prepare(d, f, temp, temp_bytes, ctx->stream));
    VMapHeader mh{};
    HIP_TRY(hipMemcpyAsync(&mh, f.hdr, sizeof mh, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (extract) {
        *n_out = mh.n_evicted;
        if (mh.n_evicted > out_capacity) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", VOXEL_MAP_MSG_CAPACITY);
    }
    if (mh.n_keep == m->n_vox) return OUSTER_HIP_OK;
    HIP_TRY(vmap_far_commit(d, m->set[1 - m->cur], f, ctx->stream));
    m->cur = 1 - m->cur;
    m->n_vox = mh.n_keep;
    m->n_pts -= mh.n_evicted;
    HIP_TRY(vmap_rebuild(dev_of(m), f.hdr, ctx->stream));
    HIP_TRY(hipMemcpyAsync(&mh, f.hdr, sizeof mh, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (mh.status) return fail(OUSTER_HIP_ERR_RUNTIME, "voxel map: hash table exhausted");
    return OUSTER_HIP_OK;
}

int cloud_device(const ouster_hip_voxel_map* m, double* out) {
    if (m->n_vox == 0 || m->n_pts == 0) return OUSTER_HIP_OK;
    ouster_hip_ctx* ctx = m->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    size_t temp_bytes = 0;
    HIP_TRY(vmap_temp_bytes(m->n_vox, &temp_bytes));
    uint32_t* pos = nullptr;
    void* temp = nullptr;
    int rc = workspace(ctx, [&](Carver& c) {
        pos = c.take<uint32_t>(m->n_vox);
        temp = c.take<uint8_t>(temp_bytes);
    });
    if (rc != OUSTER_HIP_OK) return rc;
    HIP_TRY(vmap_cloud(dev_of(m), pos, out, temp, temp_bytes, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return OUSTER_HIP_OK;
}

int closest_device(const ouster_hip_voxel_map* m, const void* queries, int32_t dtype, uint64_t q, uint64_t stride, double max_distance_sq,
                   double* out_points, double* out_dist_sq) {
    ouster_hip_ctx* ctx = m->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    VMapClosestArgs c{};
    c.queries = queries, c.stride = stride ? stride : 3, c.q = (uint32_t)q, c.f32 = dtype == OUSTER_HIP_F32;
    c.max_distance_sq = max_distance_sq, c.out_points = out_points, c.out_dist_sq = out_dist_sq;
    HIP_TRY(vmap_closest(dev_of(m), c, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return OUSTER_HIP_OK;
}

int validate_closest(const ouster_hip_voxel_map* m, const void* queries, int32_t dtype, uint64_t q, uint64_t stride, const double* out_points,
                     const double* out_dist_sq) {
    const int rc = validate_rows(m, queries, dtype, q, stride, "queries");
    if (rc != OUSTER_HIP_OK) return rc;
    if (q && (!out_points || !out_dist_sq)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    return OUSTER_HIP_OK;
}

// the host map's halves of the calls
// (no exception leaves the C ABI: a host map that cannot get its memory reports it)
int host_add(ouster_hip_voxel_map* m, const void* points, int32_t dtype, uint64_t n, uint64_t stride) {
    try {
        if (!m->host->add_points(points, dtype == OUSTER_HIP_F32, n, stride ? stride : 3)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", VOXEL_MAP_MSG_GRID);
    } catch (const std::exception&) {
        return fail(OUSTER_HIP_ERR_RUNTIME, "voxel map: out of host memory");
    }
    return OUSTER_HIP_OK;
}

int host_far(ouster_hip_voxel_map* m, const int32_t* origin, double* out, uint64_t out_capacity, uint64_t* n_out, bool extract) {
    if (extract) {
        *n_out = m->host->count_far(origin);
        if (*n_out > out_capacity) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", VOXEL_MAP_MSG_CAPACITY);
    }
    m->host->remove_far(origin, extract ? out : nullptr);
    return OUSTER_HIP_OK;
}

int add_any(ouster_hip_voxel_map* m, const void* points, int32_t dtype, uint64_t n, uint64_t stride, bool host_rows) {
    if (n == 0) return OUSTER_HIP_OK;
    if (m->host) return host_add(m, points, dtype, n, stride);
    if (!host_rows) return add_device(m, points, dtype, n, stride);
    HIP_TRY(hipSetDevice(m->ctx->device));
    Staging st(m->ctx);
    const Staging::Ref in = st.input(points, ((size_t)(n - 1) * (stride ? stride : 3) + 3) * float_elem(dtype));
    const int rc = st.stage();
    if (rc != OUSTER_HIP_OK) return rc;
    return add_device(m, st.dev(in), dtype, n, stride);   // synchronises: the staged rows are read before the scratch is reused
}

int extract_any(ouster_hip_voxel_map* m, const double* origin, double* out, uint64_t out_capacity, uint64_t* n_out, bool host_rows) {
    if (!n_out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    *n_out = 0;
    int32_t cell[3];
    int rc = origin_cell(m, origin, cell);
    if (rc != OUSTER_HIP_OK) return rc;
    if (out_capacity && !out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    if (m->host) return host_far(m, cell, out, out_capacity, n_out, true);
    if (!host_rows) return far_device(m, cell, out, out_capacity, n_out, true);
    HIP_TRY(hipSetDevice(m->ctx->device));
    // no more rows than the map holds can come back: the scratch is sized by that, not by a generous out_capacity
    const uint64_t room = std::min<uint64_t>(out_capacity, m->n_pts);
    static double none[3];
    Staging st(m->ctx);
    const Staging::Ref o = st.output(room ? (void*)out : (void*)none, (size_t)room * 24);
    rc = st.stage();
    if (rc != OUSTER_HIP_OK) return rc;
    rc = far_device(m, cell, (double*)st.dev(o), out_capacity, n_out, true);
    if (rc != OUSTER_HIP_OK) return rc;
    st.set_bytes(o, (size_t)*n_out * 24);
    return st.finish();
}

}  // namespace

int ouster_hip_voxel_map_create(ouster_hip_ctx* ctx, const ouster_hip_voxel_map_desc* desc, ouster_hip_voxel_map** out) {
    if (out) *out = nullptr;
    if (!desc || !out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (const char* msg = voxel_map_validate(desc)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", msg);
    if (desc->flags & ~OUSTER_HIP_VOXEL_MAP_HOST) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "voxel map: unknown flags");
    const bool host = (desc->flags & OUSTER_HIP_VOXEL_MAP_HOST) != 0;
    if (!host && !ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    ouster_hip_voxel_map* m = new ouster_hip_voxel_map();
    m->p = voxel_map_params(desc);
    if (host) m->host = new HostVoxelMap(m->p);
    else m->ctx = ctx;
    *out = m;
    return OUSTER_HIP_OK;
}

void ouster_hip_voxel_map_destroy(ouster_hip_voxel_map* m) {
    if (!m) return;
    if (m->ctx && m->cap) {
        (void)hipSetDevice(m->ctx->device);
        (void)hipStreamSynchronize(m->ctx->stream);
    }
    free_set(m->set[0]), free_set(m->set[1]), counted_free(m->table);
    delete m->host;
    delete m;
}

int ouster_hip_voxel_map_clear(ouster_hip_voxel_map* m) {
    if (!m) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "map is NULL");
    if (m->host) {
        m->host->clear();
        return OUSTER_HIP_OK;
    }
    m->n_vox = 0, m->n_pts = 0;
    if (m->table) {
        HIP_TRY(hipSetDevice(m->ctx->device));
        HIP_TRY(hipMemsetAsync(m->table, 0xff, ((size_t)m->table_mask + 1) * sizeof(int32_t), m->ctx->stream));
        HIP_TRY(hipStreamSynchronize(m->ctx->stream));
    }
    return OUSTER_HIP_OK;
}

int ouster_hip_voxel_map_reserve(ouster_hip_voxel_map* m, uint64_t voxels) {
    if (!m) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "map is NULL");
    if (m->host) {
        if (voxels > VOXEL_MAP_MAX_ROWS * 2) return fail(OUSTER_HIP_ERR_UNSUPPORTED, "voxel map: more than 2^31 voxels");
        try {
            m->host->reserve(voxels);
        } catch (const std::exception&) {
            return fail(OUSTER_HIP_ERR_RUNTIME, "voxel map: out of host memory");
        }
        return OUSTER_HIP_OK;
    }
    return ensure_capacity(m, voxels, true);
}

int ouster_hip_voxel_map_info_read(const ouster_hip_voxel_map* m, ouster_hip_voxel_map_info* info) {
    if (!m || !info) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    info->voxels = m->host ? m->host->voxels() : m->n_vox;
    info->points = m->host ? m->host->points() : m->n_pts;
    info->voxel_capacity = m->host ? m->host->capacity() : m->cap;
    info->points_per_voxel = m->p.max_points;
    info->device_bytes = m->bytes;
    return OUSTER_HIP_OK;
}

int ouster_hip_voxel_map_add_points(ouster_hip_voxel_map* m, const void* points, int32_t dtype, uint64_t n, uint64_t row_stride) {
    const int rc = validate_rows(m, points, dtype, n, row_stride, "rows");
    return rc != OUSTER_HIP_OK ? rc : add_any(m, points, dtype, n, row_stride, false);
}

int ouster_hip_voxel_map_add_points_host(ouster_hip_voxel_map* m, const void* points, int32_t dtype, uint64_t n, uint64_t row_stride) {
    const int rc = validate_rows(m, points, dtype, n, row_stride, "rows");
    return rc != OUSTER_HIP_OK ? rc : add_any(m, points, dtype, n, row_stride, true);
}

int ouster_hip_voxel_map_remove_far(ouster_hip_voxel_map* m, const double* origin) {
    int32_t cell[3];
    const int rc = origin_cell(m, origin, cell);
    if (rc != OUSTER_HIP_OK) return rc;
    return m->host ? host_far(m, cell, nullptr, 0, nullptr, false) : far_device(m, cell, nullptr, 0, nullptr, false);
}

int ouster_hip_voxel_map_extract_far(ouster_hip_voxel_map* m, const double* origin, double* out, uint64_t out_capacity, uint64_t* n_out) {
    return extract_any(m, origin, out, out_capacity, n_out, false);
}

int ouster_hip_voxel_map_extract_far_host(ouster_hip_voxel_map* m, const double* origin, double* out, uint64_t out_capacity, uint64_t* n_out) {
    return extract_any(m, origin, out, out_capacity, n_out, true);
}

int ouster_hip_voxel_map_update(ouster_hip_voxel_map* m, const void* points, int32_t dtype, uint64_t n, uint64_t row_stride, const double* position) {
    int rc = validate_rows(m, points, dtype, n, row_stride, "rows");
    if (rc != OUSTER_HIP_OK) return rc;
    int32_t cell[3];
    rc = origin_cell(m, position, cell);
    if (rc != OUSTER_HIP_OK) return rc;
    rc = add_any(m, points, dtype, n, row_stride, false);
    return rc != OUSTER_HIP_OK ? rc : ouster_hip_voxel_map_remove_far(m, position);
}

int ouster_hip_voxel_map_update_host(ouster_hip_voxel_map* m, const void* points, int32_t dtype, uint64_t n, uint64_t row_stride,
                                     const double* position) {
    int rc = validate_rows(m, points, dtype, n, row_stride, "rows");
    if (rc != OUSTER_HIP_OK) return rc;
    int32_t cell[3];
    rc = origin_cell(m, position, cell);
    if (rc != OUSTER_HIP_OK) return rc;
    rc = add_any(m, points, dtype, n, row_stride, true);
    return rc != OUSTER_HIP_OK ? rc : ouster_hip_voxel_map_remove_far(m, position);
}

int ouster_hip_voxel_map_pointcloud(const ouster_hip_voxel_map* m, double* out, uint64_t out_capacity, uint64_t* n_out) {
    if (!m || !n_out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    *n_out = m->host ? m->host->points() : m->n_pts;
    if (*n_out > out_capacity) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", VOXEL_MAP_MSG_CAPACITY);
    if (*n_out && !out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    if (m->host) {
        m->host->pointcloud(out);
        return OUSTER_HIP_OK;
    }
    return cloud_device(m, out);
}

int ouster_hip_voxel_map_pointcloud_host(const ouster_hip_voxel_map* m, double* out, uint64_t out_capacity, uint64_t* n_out) {
    if (!m || !n_out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (m->host) return ouster_hip_voxel_map_pointcloud(m, out, out_capacity, n_out);
    *n_out = m->n_pts;
    if (*n_out > out_capacity) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", VOXEL_MAP_MSG_CAPACITY);
    if (*n_out == 0) return OUSTER_HIP_OK;
    if (!out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    HIP_TRY(hipSetDevice(m->ctx->device));
    Staging st(m->ctx);
    const Staging::Ref o = st.output(out, (size_t)*n_out * 24);
    int rc = st.stage();
    if (rc != OUSTER_HIP_OK) return rc;
    rc = cloud_device(m, (double*)st.dev(o));
    return rc != OUSTER_HIP_OK ? rc : st.finish();
}

int ouster_hip_voxel_map_closest(const ouster_hip_voxel_map* m, const void* queries, int32_t dtype, uint64_t q, uint64_t row_stride,
                                 double max_distance_sq, double* out_points, double* out_dist_sq) {
    const int rc = validate_closest(m, queries, dtype, q, row_stride, out_points, out_dist_sq);
    if (rc != OUSTER_HIP_OK || q == 0) return rc;
    if (m->host) {
        const uint64_t stride = row_stride ? row_stride : 3;
        for (uint64_t i = 0; i < q; ++i) {
            double query[3];
            for (int c = 0; c < 3; ++c)
                query[c] = dtype == OUSTER_HIP_F32 ? (double)((const float*)queries)[i * stride + c] : ((const double*)queries)[i * stride + c];
            m->host->closest(query, max_distance_sq, out_points + 3 * i, out_dist_sq + i);
        }
        return OUSTER_HIP_OK;
    }
    return closest_device(m, queries, dtype, q, row_stride, max_distance_sq, out_points, out_dist_sq);
}

int ouster_hip_voxel_map_closest_host(const ouster_hip_voxel_map* m, const void* queries, int32_t dtype, uint64_t q, uint64_t row_stride,
                                      double max_distance_sq, double* out_points, double* out_dist_sq) {
    int rc = validate_closest(m, queries, dtype, q, row_stride, out_points, out_dist_sq);
    if (rc != OUSTER_HIP_OK || q == 0) return rc;
    if (m->host) return ouster_hip_voxel_map_closest(m, queries, dtype, q, row_stride, max_distance_sq, out_points, out_dist_sq);
    HIP_TRY(hipSetDevice(m->ctx->device));
    Staging st(m->ctx);
    const Staging::Ref in = st.input(queries, ((size_t)(q - 1) * (row_stride ? row_stride : 3) + 3) * float_elem(dtype));
    const Staging::Ref op = st.output(out_points, (size_t)q * 24);
    const Staging::Ref od = st.output(out_dist_sq, (size_t)q * 8);
    rc = st.stage();
    if (rc != OUSTER_HIP_OK) return rc;
    rc = closest_device(m, st.dev(in), dtype, q, row_stride, max_distance_sq, (double*)st.dev(op), (double*)st.dev(od));
    return rc != OUSTER_HIP_OK ? rc : st.finish();
}
