// capi_pose.hip -- the C ABI of interp_pose / transform (k_pose.hip, host/pose_util.cpp): ouster_hip_interp_pose* / _transform*
#include "capi_internal.h"
#include "k_pose.h"

using namespace ouster_hip_dev;

namespace {
// validated known poses -> the table and the known times on the device, [k - 1][24] + [k] doubles in ctx->tables
int pose_tables(ouster_hip_ctx* ctx, const std::vector<double>& host, uint32_t k, PoseInterpArgs& a) {
    const int rc = upload_table(ctx, host.data(), host.size() * 8);
    if (rc != OUSTER_HIP_OK) return rc;
    a.segments = (const double*)ctx->tables.p;
    a.x_known = a.segments + (size_t)(k - 1) * POSE_SEG_DOUBLES;
    a.k = k;
    return OUSTER_HIP_OK;
}
int pose_known_host(const double* x_known, const double* poses_known, uint32_t k, std::vector<double>& host) {
    if (const char* msg = pose_validate_known(x_known, poses_known, k)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", msg);
    host.resize((size_t)(k - 1) * POSE_SEG_DOUBLES + k);
    for (uint32_t i = 0; i + 1 < k; ++i)
        pose_segment(x_known[i], poses_known + 16 * (size_t)i, x_known[i + 1], poses_known + 16 * (size_t)(i + 1),
                     host.data() + (size_t)POSE_SEG_DOUBLES * i);
    std::copy(x_known, x_known + k, host.begin() + (size_t)(k - 1) * POSE_SEG_DOUBLES);
    return OUSTER_HIP_OK;
}
int pose_pair_host(double t0, const double* x0, double t1, const double* x1, std::vector<double>& host) {
    if (const char* msg = pose_validate_pair(t0, t1)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", msg);
    if (!x0 || !x1) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pose");
    host.assign(POSE_SEG_DOUBLES + 2, 0.0);   // one segment; with k == 2 the known times select nothing
    pose_segment(t0, x0, t1, x1, host.data());
    host[POSE_SEG_DOUBLES] = t0;
    host[POSE_SEG_DOUBLES + 1] = t1;
    return OUSTER_HIP_OK;
}
int pose_interp_launch(ouster_hip_ctx* ctx, const std::vector<double>& host, uint32_t k, PoseInterpArgs& a) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (a.dtype != OUSTER_HIP_F32 && a.dtype != OUSTER_HIP_F64) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dtype must be F32 or F64");
    if (a.n == 0) return OUSTER_HIP_OK;
    if (a.n > (1ull << 38)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "at most 2^38 poses per call");
    if (!a.out || (!a.x && (!a.timestamp || !a.status))) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    if (((uintptr_t)a.out | (uintptr_t)a.pose_rows) & 15) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "pose output is not 16-byte aligned");
    HIP_TRY(hipSetDevice(ctx->device));
    const int rc = pose_tables(ctx, host, k, a);
    if (rc != OUSTER_HIP_OK) return rc;
    a.direct_stores = ctx->knobs.pose_direct ? 1 : 0;
    HIP_TRY(launch_pose_interp(a, ctx->stream));
    return OUSTER_HIP_OK;
}
int pose_interp_host(ouster_hip_ctx* ctx, const double* x_interp, uint64_t n, const std::vector<double>& table, uint32_t k,
                     int dtype, void* poses_out) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (!float_elem(dtype)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dtype must be F32 or F64");
    if (n == 0) return OUSTER_HIP_OK;
    if (!x_interp || !poses_out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    char msg[160];
    if (pose_validate_interp(x_interp, n, msg, sizeof msg)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", msg);
    HIP_TRY(hipSetDevice(ctx->device));
    Staging st(ctx);
    const auto in = st.input(x_interp, n * 8), out = st.output(poses_out, n * 16 * float_elem(dtype));
    int rc = st.stage();
    if (rc != OUSTER_HIP_OK) return rc;
    PoseInterpArgs a{};
    a.x = (const double*)st.dev(in);
    a.n = n;
    a.dtype = dtype;
    a.out = st.dev(out);
    rc = pose_interp_launch(ctx, table, k, a);
    if (rc != OUSTER_HIP_OK) return rc;
    return st.finish();
}
int pose_columns(ouster_hip_ctx* ctx, const uint64_t* timestamp, const uint32_t* status, uint32_t n_frames, uint32_t w,
                 const std::vector<double>& table, uint32_t k, double* poses, float* pose_rows) {
    PoseInterpArgs a{};
    a.timestamp = timestamp;
    a.status = status;
    a.n = (uint64_t)n_frames * w;
    a.dtype = OUSTER_HIP_F64;
    a.out = poses;
    a.pose_rows = pose_rows;
    return pose_interp_launch(ctx, table, k, a);
}
}  // namespace

int ouster_hip_pose_validate(const double* x_known, const double* poses_known, uint32_t k, const double* x_interp, uint64_t n) {
    if (const char* msg = pose_validate_known(x_known, poses_known, k)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", msg);
    char msg[160];
    if (x_interp && pose_validate_interp(x_interp, n, msg, sizeof msg)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", msg);
    return OUSTER_HIP_OK;
}

int ouster_hip_interp_pose(ouster_hip_ctx* ctx, const double* x_interp_dev, uint64_t n, const double* x_known,
                           const double* poses_known, uint32_t k, int dtype, void* poses_out_dev) {
    std::vector<double> table;
    const int rc = pose_known_host(x_known, poses_known, k, table);
    if (rc != OUSTER_HIP_OK) return rc;
    PoseInterpArgs a{};
    a.x = x_interp_dev;
    a.n = n;
    a.dtype = dtype;
    a.out = poses_out_dev;
    if (n && !x_interp_dev) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    return pose_interp_launch(ctx, table, k, a);
}

int ouster_hip_interp_pose_host(ouster_hip_ctx* ctx, const double* x_interp, uint64_t n, const double* x_known,
                                const double* poses_known, uint32_t k, int dtype, void* poses_out) {
    std::vector<double> table;
    const int rc = pose_known_host(x_known, poses_known, k, table);
    if (rc != OUSTER_HIP_OK) return rc;
    return pose_interp_host(ctx, x_interp, n, table, k, dtype, poses_out);
}

int ouster_hip_interp_pose_pair_host(ouster_hip_ctx* ctx, const double* x_interp, uint64_t n, double t0, const double* x0,
                                     double t1, const double* x1, int dtype, void* poses_out) {
    std::vector<double> table;
    const int rc = pose_pair_host(t0, x0, t1, x1, table);
    if (rc != OUSTER_HIP_OK) return rc;
    return pose_interp_host(ctx, x_interp, n, table, 2, dtype, poses_out);
}

int ouster_hip_interp_pose_columns(ouster_hip_ctx* ctx, const uint64_t* timestamp_dev, const uint32_t* status_dev,
                                   uint32_t n_frames, uint32_t w, const double* x_known, const double* poses_known,
                                   uint32_t k, double* poses_dev, float* pose_rows_dev) {
    std::vector<double> table;
    const int rc = pose_known_host(x_known, poses_known, k, table);
    if (rc != OUSTER_HIP_OK) return rc;
    return pose_columns(ctx, timestamp_dev, status_dev, n_frames, w, table, k, poses_dev, pose_rows_dev);
}

int ouster_hip_interp_pose_pair_columns(ouster_hip_ctx* ctx, const uint64_t* timestamp_dev, const uint32_t* status_dev,
                                        uint32_t n_frames, uint32_t w, double t0, const double* x0, double t1,
                                        const double* x1, double* poses_dev, float* pose_rows_dev) {
    std::vector<double> table;
    const int rc = pose_pair_host(t0, x0, t1, x1, table);
    if (rc != OUSTER_HIP_OK) return rc;
    return pose_columns(ctx, timestamp_dev, status_dev, n_frames, w, table, 2, poses_dev, pose_rows_dev);
}

int ouster_hip_transform(ouster_hip_ctx* ctx, const void* points_dev, const double* pose16, void* out_dev, int dtype,
                         uint64_t n) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (!float_elem(dtype)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dtype must be F32 or F64");
    if (!pose16) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "pose is NULL");
    if (n == 0) return OUSTER_HIP_OK;
    if (n > (1ull << 38)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "at most 2^38 points per call");
    if (!points_dev || !out_dev) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    HIP_TRY(hipSetDevice(ctx->device));
    PoseTransformArgs a{};
    a.points = points_dev;
    a.out = out_dev;
    std::copy(pose16, pose16 + 16, a.pose);
    a.n = n;
    a.dtype = dtype;
    HIP_TRY(launch_pose_transform(a, ctx->stream));
    return OUSTER_HIP_OK;
}

int ouster_hip_transform_host(ouster_hip_ctx* ctx, const void* points, const double* pose16, void* out, int dtype, uint64_t n) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (!float_elem(dtype)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dtype must be F32 or F64");
    if (!pose16) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "pose is NULL");
    if (n == 0) return OUSTER_HIP_OK;
    if (!points || !out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)n * 3 * float_elem(dtype);
    Staging st(ctx);
    const auto in = st.input(points, bytes), o = st.output(out, bytes);
    int rc = st.stage();
    if (rc != OUSTER_HIP_OK) return rc;
    rc = ouster_hip_transform(ctx, st.dev(in), pose16, st.dev(o), dtype, n);
    if (rc != OUSTER_HIP_OK) return rc;
    return st.finish();
}
