// capi_registration.hip -- the C ABI of ICPRegistration (k_registration.hip, host/registration_util.cpp): ouster_hip_registration_*,
// ouster_hip_build_linear_system_ref
#include "capi_internal.h"
#include "capi_voxel_map.h"
#include "carve.h"
#include "k_registration.h"
#include "registration_host.h"

#include <exception>

using namespace ouster_hip_dev;

namespace {

int refuse(const char* msg, bool unsupported) {
    return fail_msg(unsupported ? OUSTER_HIP_ERR_UNSUPPORTED : OUSTER_HIP_ERR_INVALID_ARGUMENT, msg);
}

// the pieces of a pass over n rows, in the context's grow-only voxel workspace (the map's own calls lay theirs out afresh)
int carve_pass(ouster_hip_ctx* ctx, RegPassArgs& a) {
    const uint32_t chunks = reg_chunks(a.n);
    auto lay = [&](Carver& c) {
        a.hdr = c.take<RegHeader>(1);
        a.partials = c.take<double>((size_t)chunks * REG_NS);
        a.counts = c.take<uint32_t>(chunks);
        a.moved = c.take<double>((size_t)a.n * 3);
    };
    Carver measure(nullptr);
    lay(measure);
    if (const int rc = grow_idle(ctx, ctx->voxel_ws, measure.total, "registration workspace", true)) return rc;
    Carver c(ctx->voxel_ws.p);
    lay(c);
    return OUSTER_HIP_OK;
}

void set_estimate(RegPassArgs& a, const RegPose* e) {
    a.apply = e != nullptr;
    for (int k = 0; k < 4; ++k) a.q[k] = e ? e->v[k] : (k == 3 ? 1.0 : 0.0);
    for (int k = 0; k < 3; ++k) a.t[k] = e ? e->v[4 + k] : 0.0;
}

// launches one pass and reads its header back: one copy, one synchronisation
int run_pass(const ouster_hip_voxel_map* m, const RegPassArgs& a, bool from_f32, RegHeader* got) {
    ouster_hip_ctx* ctx = m->ctx;
    HIP_TRY(reg_pass_run(dev_of(m), a, from_f32, ctx->stream));
    HIP_TRY(hipMemcpyAsync(got, a.hdr, sizeof *got, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return OUSTER_HIP_OK;
}

// rows in device memory, validated, n > 0, a device map that holds voxels, max_iterations > 0
int align_device(const ouster_hip_voxel_map* m, const void* points, int32_t dtype, uint64_t n, uint64_t stride, ouster_hip_registration_desc* d) {
    ouster_hip_ctx* ctx = m->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    RegPassArgs a{};
    a.n = (uint32_t)n;
    a.max_d2 = d->max_distance * d->max_distance;
    a.k = d->kernel_scale;
    if (const int rc = carve_pass(ctx, a)) return rc;
    RegPose pose, estimate;
    for (int32_t j = 0; j < d->max_iterations; ++j) {
        // pass 0 reads the caller's rows; a later pass the moved rows, and applies the estimate of the pass before
        a.src = j ? (const void*)a.moved : points;
        a.stride = j ? 3 : (stride ? stride : 3);
        set_estimate(a, j ? &estimate : nullptr);
        RegHeader got{};
        if (const int rc = run_pass(m, a, j == 0 && dtype == OUSTER_HIP_F32, &got)) return rc;
        double dx[6];
        const bool stop = reg_solve_pass(got.sums, d->convergence_criterion, dx, &estimate);
        pose = reg_compose(estimate, pose);
        d->iterations = (uint32_t)(j + 1), d->correspondences = got.count;
        if (stop) {
            d->converged = 1;
            break;
        }
    }
    reg_matrix(pose, d->pose);
    return OUSTER_HIP_OK;
}

int align_any(const ouster_hip_voxel_map* m, const void* points, int32_t dtype, uint64_t n, uint64_t stride, ouster_hip_registration_desc* d,
              bool host_rows) {
    if (!d) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "desc is NULL");
    bool unsupported = false;
    if (const char* msg = reg_validate(m, points, dtype, n, stride, d->max_distance, d->kernel_scale, d->convergence_criterion, &unsupported))
        return refuse(msg, unsupported);
    if (d->flags) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "registration: unknown flags");
    reg_identity(d);
    if (m->host) {
        try {
            reg_align_ref(*m->host, points, dtype == OUSTER_HIP_F32, n, stride ? stride : 3, d);
        } catch (const std::exception&) {
            return fail(OUSTER_HIP_ERR_RUNTIME, "registration: out of host memory");
        }
        return OUSTER_HIP_OK;
    }
    if (n == 0 || m->n_vox == 0 || d->max_iterations <= 0) return OUSTER_HIP_OK;
    if (!host_rows) return align_device(m, points, dtype, n, stride, d);
    HIP_TRY(hipSetDevice(m->ctx->device));
    Staging st(m->ctx);
    const Staging::Ref in = st.input(points, ((size_t)(n - 1) * (stride ? stride : 3) + 3) * float_elem(dtype));
    const int rc = st.stage();
    if (rc != OUSTER_HIP_OK) return rc;
    return align_device(m, st.dev(in), dtype, n, stride, d);   // synchronises after every pass: the staged rows are read by then
}

int validate_step(const ouster_hip_voxel_map* m, const ouster_hip_registration_step_io* io) {
    if (!io) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "io is NULL");
    bool unsupported = false;
    if (const char* msg = reg_validate(m, io->points, io->dtype, io->n, io->row_stride, io->max_distance, io->kernel_scale, 0.0, &unsupported))
        return refuse(msg, unsupported);
    if (io->n == 0) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "registration_step: no rows");
    if (!io->moved || !io->flags || !io->neighbours || !io->dist_sq) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    return OUSTER_HIP_OK;
}

void finish_step(ouster_hip_registration_step_io* io) {
    RegPose next;
    reg_solve_pass(io->sums, 0.0, io->dx, &next);
    std::memcpy(io->next_estimate, next.v, sizeof next.v);
}

}  // namespace

int ouster_hip_registration_align(const ouster_hip_voxel_map* map, const void* points, int32_t dtype, uint64_t n, uint64_t row_stride,
                                  ouster_hip_registration_desc* desc) {
    return align_any(map, points, dtype, n, row_stride, desc, false);
}

int ouster_hip_registration_align_host(const ouster_hip_voxel_map* map, const void* points, int32_t dtype, uint64_t n, uint64_t row_stride,
                                       ouster_hip_registration_desc* desc) {
    return align_any(map, points, dtype, n, row_stride, desc, true);
}

int ouster_hip_registration_step(const ouster_hip_voxel_map* m, ouster_hip_registration_step_io* io) {
    if (const int rc = validate_step(m, io)) return rc;
    if (m->host) return ouster_hip_registration_step_ref(m, io);
    ouster_hip_ctx* ctx = m->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    RegPassArgs a{};
    a.n = (uint32_t)io->n;
    a.max_d2 = io->max_distance * io->max_distance;
    a.k = io->kernel_scale;
    if (const int rc = carve_pass(ctx, a)) return rc;
    a.src = io->points;
    a.stride = io->row_stride ? io->row_stride : 3;
    RegPose e;
    std::memcpy(e.v, io->estimate, sizeof e.v);
    set_estimate(a, io->has_estimate ? &e : nullptr);
    a.flags = io->flags, a.neighbours = io->neighbours, a.dist_sq = io->dist_sq;
    RegHeader got{};
    if (const int rc = run_pass(m, a, io->dtype == OUSTER_HIP_F32, &got)) return rc;
    HIP_TRY(hipMemcpyAsync(io->moved, a.moved, (size_t)io->n * 24, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::memcpy(io->sums, got.sums, sizeof got.sums);
    io->count = got.count;
    finish_step(io);
    return OUSTER_HIP_OK;
}

int ouster_hip_registration_step_ref(const ouster_hip_voxel_map* m, ouster_hip_registration_step_io* io) {
    if (const int rc = validate_step(m, io)) return rc;
    if (!m->host) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "registration_step_ref: the map is not a host map");
    const uint64_t stride = io->row_stride ? io->row_stride : 3;
    for (uint64_t i = 0; i < io->n; ++i)
        for (int c = 0; c < 3; ++c)
            io->moved[3 * i + c] = io->dtype == OUSTER_HIP_F32 ? (double)static_cast<const float*>(io->points)[i * stride + c]
                                                               : static_cast<const double*>(io->points)[i * stride + c];
    RegPose e;
    std::memcpy(e.v, io->estimate, sizeof e.v);
    reg_pass_ref(*m->host, io->moved, io->n, io->has_estimate ? &e : nullptr, io->max_distance, io->kernel_scale, io->flags, io->neighbours,
                 io->dist_sq, io->sums, &io->count);
    finish_step(io);
    return OUSTER_HIP_OK;
}

int ouster_hip_build_linear_system_ref(const double* sources, const double* targets, uint64_t n, double kernel_scale, double* jtj36, double* jtr6) {
    if (!jtj36 || !jtr6 || (n && (!sources || !targets))) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    if (!std::isfinite(kernel_scale) || kernel_scale < 0.0)
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "registration: kernel_scale must be finite and not negative");
    reg_build_linear_system(sources, targets, n, kernel_scale, jtj36, jtr6);
    return OUSTER_HIP_OK;
}

double ouster_hip_registration_model_error(const double* deviation16, double max_range) {
    return deviation16 ? reg_model_error(deviation16, max_range) : 0.0;
}
