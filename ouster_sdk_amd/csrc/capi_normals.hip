// capi_normals.hip -- the C ABI of algorithm::normals (k_normals.hip, host/normals_util.cpp): ouster_hip_normals*
#include "capi_internal.h"
#include "k_normals.h"

using namespace ouster_hip_dev;

namespace {
int normals_validate(const ouster_hip_normals_desc* d) {
    if (!d) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "desc is NULL");
    const bool dual = d->xyz2 || d->range2;
    if (const char* msg = normals_validate_shapes(d->h, d->w, d->xyz_rows, dual, d->xyz2_rows, d->range2_h, d->range2_w,
                                                  d->sensor_origins ? d->n_origins : d->w))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", msg);
    if (const char* msg = normals_validate_params(d->min_angle_of_incidence_rad, d->target_distance_m))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", msg);
    if (!float_elem(d->xyz_dtype)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "xyz_dtype must be F32 or F64");
    return OUSTER_HIP_OK;
}

// d: every array in device memory
int normals_device(ouster_hip_ctx* ctx, const ouster_hip_normals_desc* d) {
    const bool dual = d->xyz2 || d->range2;
    if (!d->xyz || !d->range || !d->normals || (dual && (!d->xyz2 || !d->range2 || !d->normals2)))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    const uint32_t n_ret = dual ? 2 : 1;
    const uint64_t rows = (uint64_t)d->n_frames * n_ret;
    if (rows > 65535) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "at most 65535 frames x returns per call");
    if ((uint64_t)d->n_frames * d->h * d->w > (1ull << 40)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "at most 2^40 pixels per call");
    if ((d->h + NORMALS_TILE_H - 1) / NORMALS_TILE_H > 65535) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "at most 262140 rows");
    HIP_TRY(hipSetDevice(ctx->device));
    NormalsArgs a{};
    a.xyz[0] = d->xyz, a.xyz[1] = d->xyz2;
    a.range[0] = d->range, a.range[1] = d->range2;
    a.out[0] = d->normals, a.out[1] = d->normals2;
    a.f32 = d->xyz_dtype == OUSTER_HIP_F32;
    a.n_frames = d->n_frames, a.h = d->h, a.w = d->w, a.n_ret = n_ret;
    a.origins = d->sensor_origins;
    a.poses = d->sensor_origins ? nullptr : d->poses;
    // the last column of every sensor_to_body; with poses and no matrix: identity's
    const bool with_s2b = !d->sensor_origins && (d->poses || d->sensor_to_body);
    a.n_s2b = with_s2b ? (d->sensor_to_body ? std::max(d->n_sensor_to_body, 1u) : 1u) : 0u;
    // Radii beyond the image are cut off at max(h, w), with the same result.  Vertical: the loop leaves at the first radius above
    // both max_up and max_down, which are below h, so a range of h or more never reaches its last radius.  Horizontal: by radius w
    // every pixel of the row has been visited with both signs; later radii revisit them at equal error, which never replaces the
    // best one (strict <), and the thin flag can only have been cleared already, so best, thin and good are constant from radius
    // w on -- and the reference's last-radius rule (accept the closest candidate under the threshold at radius ==
    // pixel_search_range) tests that constant state, whichever radius at or beyond w is the last.
    a.pixel_search_range = std::min(d->pixel_search_range, std::max(d->h, d->w));
    a.staggered_out = d->pixel_shift_by_row && d->staggered_output;
    // table: the constants [rows][4] f64, the sensor_to_body columns [n_s2b][4] f64, then the shifts reduced to [0, w); the first
    // upload carries the constants as zeros
    const size_t cbytes = (size_t)rows * 4 * 8, mbytes = (size_t)a.n_s2b * 4 * 8, sbytes = d->pixel_shift_by_row ? (size_t)d->h * 4 : 0;
    std::vector<uint8_t> table(cbytes + mbytes + sbytes, 0);
    for (uint32_t m = 0; m < a.n_s2b; ++m) {
        double* col = reinterpret_cast<double*>(table.data() + cbytes) + 4 * (size_t)m;
        col[3] = 1.0;
        if (d->sensor_to_body)
            for (int r = 0; r < 4; ++r) col[r] = d->sensor_to_body[16 * (size_t)m + 4 * r + 3];
    }
    if (sbytes) {
        uint32_t* red = reinterpret_cast<uint32_t*>(table.data() + cbytes + mbytes);
        const int64_t w = d->w;
        for (uint32_t u = 0; u < d->h; ++u) red[u] = (uint32_t)(((int64_t)d->pixel_shift_by_row[u] % w + w) % w);
    }
    int rc = upload_table(ctx, table.data(), table.size());
    if (rc != OUSTER_HIP_OK) return rc;
    a.consts = (const double*)ctx->tables.p;
    a.s2b = mbytes ? (const double*)((const uint8_t*)ctx->tables.p + cbytes) : nullptr;
    a.shifts = sbytes ? (const uint32_t*)((const uint8_t*)ctx->tables.p + cbytes + mbytes) : nullptr;
    if (const int rc = grow_idle(ctx, ctx->normals_pairs, rows * sizeof(NormalsPair), "normals")) return rc;
    a.pairs = (NormalsPair*)ctx->normals_pairs.p;
    HIP_TRY(launch_normals_subtent(a, ctx->stream));
    std::vector<NormalsPair> pairs(rows);
    HIP_TRY(hipMemcpyAsync(pairs.data(), a.pairs, rows * sizeof(NormalsPair), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    double* k = reinterpret_cast<double*>(table.data());
    for (uint32_t f = 0; f < d->n_frames; ++f) {
        ouster_hip_normals_consts c0, c;
        const NormalsPair& p0 = pairs[(size_t)f * n_ret];
        normals_constants(d->w, d->h, d->min_angle_of_incidence_rad, d->target_distance_m, p0.rows != 0, p0.dot, p0.rows, &c0);
        for (uint32_t r = 0; r < n_ret; ++r) {
            c = c0;
            if (r == 1 && !(c0.subtent > 0.0)) {   // the override of the dual form is not taken: the second return's own columns
                const NormalsPair& p1 = pairs[(size_t)f * n_ret + 1];
                normals_constants(d->w, d->h, d->min_angle_of_incidence_rad, d->target_distance_m, p1.rows != 0, p1.dot, p1.rows, &c);
            }
            double* row = k + ((size_t)f * n_ret + r) * 4;
            row[0] = c.px_res_h, row[1] = c.px_res_v, row[2] = c.tan_safe, row[3] = c.target_sq;
        }
    }
    rc = upload_table(ctx, table.data(), table.size());
    if (rc != OUSTER_HIP_OK) return rc;
    a.consts = (const double*)ctx->tables.p;
    a.s2b = mbytes ? (const double*)((const uint8_t*)ctx->tables.p + cbytes) : nullptr;
    a.shifts = sbytes ? (const uint32_t*)((const uint8_t*)ctx->tables.p + cbytes + mbytes) : nullptr;
    HIP_TRY(launch_normals(a, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return OUSTER_HIP_OK;
}
}  // namespace

int ouster_hip_normals(ouster_hip_ctx* ctx, const ouster_hip_normals_desc* desc) {
    const int rc = normals_validate(desc);
    if (rc != OUSTER_HIP_OK) return rc;
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if ((uint64_t)desc->n_frames * desc->h * desc->w == 0) return OUSTER_HIP_OK;
    return normals_device(ctx, desc);
}

int ouster_hip_normals_host(ouster_hip_ctx* ctx, const ouster_hip_normals_desc* desc) {
    int rc = normals_validate(desc);
    if (rc != OUSTER_HIP_OK) return rc;
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    const size_t px = (size_t)desc->n_frames * desc->h * desc->w;
    if (px == 0) return OUSTER_HIP_OK;
    const bool dual = desc->xyz2 || desc->range2;
    if (!desc->xyz || !desc->range || !desc->normals || (dual && (!desc->xyz2 || !desc->range2 || !desc->normals2)))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t es = float_elem(desc->xyz_dtype);
    const bool with_poses = !desc->sensor_origins && desc->poses;
    using Ref = Staging::Ref;
    Staging st(ctx);
    const Ref xyz = st.input(desc->xyz, px * 3 * es), range = st.input(desc->range, px * 4);
    const Ref xyz2 = dual ? st.input(desc->xyz2, px * 3 * es) : Ref{}, range2 = dual ? st.input(desc->range2, px * 4) : Ref{};
    const Ref origins = desc->sensor_origins ? st.input(desc->sensor_origins, (size_t)desc->w * 24) : Ref{};
    const Ref poses = with_poses ? st.input(desc->poses, (size_t)desc->n_frames * desc->w * 128) : Ref{};
    const Ref out = st.output(desc->normals, px * 24), out2 = dual ? st.output(desc->normals2, px * 24) : Ref{};
    rc = st.stage();
    if (rc != OUSTER_HIP_OK) return rc;
    ouster_hip_normals_desc d = *desc;
    d.xyz = st.dev(xyz), d.range = (const uint32_t*)st.dev(range), d.normals = (double*)st.dev(out);
    if (dual) d.xyz2 = st.dev(xyz2), d.range2 = (const uint32_t*)st.dev(range2), d.normals2 = (double*)st.dev(out2);
    if (origins) d.sensor_origins = (const double*)st.dev(origins);
    if (poses) d.poses = (const double*)st.dev(poses);
    rc = normals_device(ctx, &d);
    if (rc != OUSTER_HIP_OK) return rc;
    return st.finish();
}
