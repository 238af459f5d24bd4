// capi_cartesian.hip -- the C ABI of the XYZ lookup tables and the standalone cartesian projection (k_cartesian.hip):
// ouster_hip_lut_* / ouster_hip_cartesian / _cartesian_host.  The one-off table construction is the only compute on the host
// (make_xyz_lut is a one-off in the reference too: ouster_core/src/xyzlut.cpp:11-89, cached per sensor in sensor_info.cpp:260-275).
#include <new>

#include "capi_internal.h"

using namespace ouster_hip_dev;

// ---------------------------------------------------------------------------------------
// host math: impl::make_xyz_lut (ouster_core/src/xyzlut.cpp:11-89), full LUT in double
// ---------------------------------------------------------------------------------------
static void host_full_lut(const ouster_hip_calib& c, std::vector<double>& direction,
                          std::vector<double>& offset) {
    const size_t w = c.w, h = c.h;
    direction.assign(w * h * 3, 0.0);
    offset.assign(w * h * 3, 0.0);
    const double* b2l = c.beam_to_lidar_transform;
    const double* tf = c.transform;
    const double bx = b2l[3], bz = b2l[11];
    double n = bx;
    if (bz != 0) n = std::sqrt(std::pow(bx, 2) + std::pow(bz, 2));
    const bool per_beam = (c.n_angles == h);
    const double step = M_PI * 2.0 / static_cast<double>(w);
    for (size_t row = 0; row < h; ++row) {
        for (size_t col = 0; col < w; ++col) {
            const size_t i = row * w + col;
            double enc, azi, alt;
            if (per_beam) {
                enc = 2.0 * M_PI - static_cast<double>(col) * step;
                azi = -c.azimuth_angles_deg[row] * M_PI / 180.0;
                alt = c.altitude_angles_deg[row] * M_PI / 180.0;
            } else {
                enc = 0;
                azi = c.azimuth_angles_deg[i] * M_PI / 180.0;
                alt = c.altitude_angles_deg[i] * M_PI / 180.0;
            }
            const double d[3] = {std::cos(enc + azi) * std::cos(alt),
                                 std::sin(enc + azi) * std::cos(alt), std::sin(alt)};
            const double o[3] = {std::cos(enc) * bx - d[0] * n, std::sin(enc) * bx - d[1] * n,
                                 -d[2] * n + bz};
            for (int r = 0; r < 3; ++r) {
                double dd = 0, oo = 0;
                for (int k = 0; k < 3; ++k) {
                    dd += d[k] * tf[r * 4 + k];
                    oo += o[k] * tf[r * 4 + k];
                }
                oo += tf[r * 4 + 3];
                direction[i * 3 + r] = dd * c.range_unit;
                offset[i * 3 + r] = oo * c.range_unit;
            }
        }
    }
}

// separable form of the same table: see the derivation in DESIGN.md ("XYZ tables")
static void host_separable_tables(const ouster_hip_calib& c, std::vector<double>& beam,
                                  std::vector<double>& col, double& n_out) {
    const size_t w = c.w, h = c.h;
    const double* b2l = c.beam_to_lidar_transform;
    const double* tf = c.transform;
    const double ru = c.range_unit;
    const double bx = b2l[3], bz = b2l[11];
    double n = bx;
    if (bz != 0) n = std::sqrt(std::pow(bx, 2) + std::pow(bz, 2));
    n_out = n;
    auto rot = [&](const double v[3], double out[3]) {
        for (int r = 0; r < 3; ++r)
            out[r] = v[0] * tf[r * 4 + 0] + v[1] * tf[r * 4 + 1] + v[2] * tf[r * 4 + 2];
    };
    beam.assign(h * 9, 0.0);
    for (size_t row = 0; row < h; ++row) {
        const double azi = -c.azimuth_angles_deg[row] * M_PI / 180.0;
        const double alt = c.altitude_angles_deg[row] * M_PI / 180.0;
        const double A = std::cos(azi) * std::cos(alt), B = std::sin(azi) * std::cos(alt),
                     Cc = std::sin(alt);
        const double u[3] = {A, B, 0}, v[3] = {-B, A, 0}, wv[3] = {0, 0, Cc};
        double ru_[3];
        rot(u, ru_);
        for (int k = 0; k < 3; ++k) beam[row * 9 + k] = ru_[k] * ru;
        rot(v, ru_);
        for (int k = 0; k < 3; ++k) beam[row * 9 + 3 + k] = ru_[k] * ru;
        rot(wv, ru_);
        for (int k = 0; k < 3; ++k) beam[row * 9 + 6 + k] = ru_[k] * ru;
    }
    col.assign(w * 5, 0.0);
    const double step = M_PI * 2.0 / static_cast<double>(w);
    for (size_t cc = 0; cc < w; ++cc) {
        const double enc = 2.0 * M_PI - static_cast<double>(cc) * step;
        const double cx = std::cos(enc), sx = std::sin(enc);
        const double o[3] = {cx * bx, sx * bx, bz};
        double ro[3];
        rot(o, ro);
        col[cc * 5 + 0] = cx;
        col[cc * 5 + 1] = sx;
        for (int k = 0; k < 3; ++k) col[cc * 5 + 2 + k] = (ro[k] + tf[k * 4 + 3]) * ru;
    }
}

static int upload(void** dptr, const void* src, size_t bytes, hipStream_t st) {
    if (counted_malloc(dptr, bytes) != hipSuccess) return -1;
    if (hipMemcpyAsync(*dptr, src, bytes, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    return hipStreamSynchronize(st) == hipSuccess ? 0 : -1;
}

extern "C" {

// ---- lut -------------------------------------------------------------------------------
int ouster_hip_lut_create(ouster_hip_ctx* ctx, const ouster_hip_calib* c, ouster_hip_lut** out) {
    if (!ctx || !c || !out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (c->w == 0 || c->h == 0)
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "lut dimensions must be greater than zero");
    const size_t hw = (size_t)c->w * c->h;
    if ((c->n_angles != c->h && c->n_angles != hw) || !c->azimuth_angles_deg ||
        !c->altitude_angles_deg)
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "unexpected frame dimensions");
    HIP_TRY(hipSetDevice(ctx->device));
    ouster_hip_lut* L = new (std::nothrow) ouster_hip_lut();
    if (!L) return fail(OUSTER_HIP_ERR_RUNTIME, "out of memory");
    L->device = ctx->device;
    L->w = c->w;
    L->h = c->h;
    host_full_lut(*c, L->direction, L->offset);
    int rc = 0;
    if (c->n_angles == c->h) {
        std::vector<double> beam, col;
        double n;
        host_separable_tables(*c, beam, col, n);
        L->separable = true;
        rc |= upload(&L->d_beam, beam.data(), beam.size() * 8, ctx->stream);
        rc |= upload(&L->d_col, col.data(), col.size() * 8, ctx->stream);
        L->dev.beam_tab = (const double*)L->d_beam;
        L->dev.col_tab = (const double*)L->d_col;
        L->dev.n = n;
        L->dev.full_dtype = 0;
    } else {
        rc |= upload(&L->d_dir, L->direction.data(), hw * 24, ctx->stream);
        rc |= upload(&L->d_ofs, L->offset.data(), hw * 24, ctx->stream);
        L->dev.full_dir = L->d_dir;
        L->dev.full_ofs = L->d_ofs;
        L->dev.full_dtype = OUSTER_HIP_F64;
    }
    if (rc) {
        ouster_hip_lut_destroy(L);
        return fail(OUSTER_HIP_ERR_RUNTIME, "LUT upload failed");
    }
    *out = L;
    return OUSTER_HIP_OK;
}

int ouster_hip_lut_create_from_arrays(ouster_hip_ctx* ctx, const void* direction,
                                      const void* offset, uint32_t h, uint32_t w, int dtype,
                                      ouster_hip_lut** out) {
    if (!ctx || !direction || !offset || !out)
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (w == 0 || h == 0)
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "lut dimensions must be greater than zero");
    if (!float_elem(dtype))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "LUT dtype must be F32 or F64");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t hw = (size_t)w * h, es = float_elem(dtype);
    ouster_hip_lut* L = new (std::nothrow) ouster_hip_lut();
    if (!L) return fail(OUSTER_HIP_ERR_RUNTIME, "out of memory");
    L->device = ctx->device;
    L->w = w;
    L->h = h;
    L->direction.resize(hw * 3);
    L->offset.resize(hw * 3);
    for (size_t i = 0; i < hw * 3; ++i) {
        L->direction[i] = es == 4 ? (double)((const float*)direction)[i] : ((const double*)direction)[i];
        L->offset[i] = es == 4 ? (double)((const float*)offset)[i] : ((const double*)offset)[i];
    }
    int rc = upload(&L->d_dir, direction, hw * 3 * es, ctx->stream);
    rc |= upload(&L->d_ofs, offset, hw * 3 * es, ctx->stream);
    if (rc) {
        ouster_hip_lut_destroy(L);
        return fail(OUSTER_HIP_ERR_RUNTIME, "LUT upload failed");
    }
    L->dev.full_dir = L->d_dir;
    L->dev.full_ofs = L->d_ofs;
    L->dev.full_dtype = dtype;
    *out = L;
    return OUSTER_HIP_OK;
}

int ouster_hip_lut_export(const ouster_hip_lut* L, double* direction, double* offset) {
    if (!L || !direction || !offset) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    memcpy(direction, L->direction.data(), L->direction.size() * 8);
    memcpy(offset, L->offset.data(), L->offset.size() * 8);
    return OUSTER_HIP_OK;
}

void ouster_hip_lut_destroy(ouster_hip_lut* L) {
    if (!L) return;
    (void)hipSetDevice(L->device);
    counted_free((void*)L->d_beam);
    counted_free((void*)L->d_col);
    counted_free((void*)L->d_dir);
    counted_free((void*)L->d_ofs);
    delete L;
}

// ---- standalone cartesian -------------------------------------------------------------------
int ouster_hip_cartesian(ouster_hip_ctx* ctx, const ouster_hip_lut* lut, const uint32_t* range,
                         void* xyz, int xyz_dtype, uint32_t n_images) {
    if (!ctx || !lut) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!float_elem(xyz_dtype))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "xyz_dtype must be F32 or F64");
    if (n_images == 0) return OUSTER_HIP_OK;
    if (!range || !xyz) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL image pointer");
    HIP_TRY(hipSetDevice(ctx->device));
    CartesianArgs a{};
    a.lut = lut->dev;
    a.range = range;
    a.xyz = xyz;
    a.w = lut->w;
    a.h = lut->h;
    a.n_images = n_images;
    a.xyz_dtype = xyz_dtype;
    const size_t npx = (size_t)lut->w * lut->h;
    a.vec_ok = al16(range) && al16(xyz) && (npx % 4 == 0);
    const int mode = lut->separable ? (xyz_dtype == OUSTER_HIP_F32 ? 1 : 2) : 3;
    HIP_TRY(launch_cartesian(a, mode, ctx->stream));
    return OUSTER_HIP_OK;
}

int ouster_hip_cartesian_host(ouster_hip_ctx* ctx, const ouster_hip_lut* lut, const uint32_t* range, void* xyz,
                              int xyz_dtype) {
    if (!ctx || !lut) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!float_elem(xyz_dtype))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "xyz_dtype must be F32 or F64");
    const size_t npx = (size_t)lut->w * lut->h;
    if (npx == 0) return OUSTER_HIP_OK;
    if (!range || !xyz) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL image pointer");
    HIP_TRY(hipSetDevice(ctx->device));
    Staging st(ctx);
    const auto in = st.input(range, npx * 4), out = st.output(xyz, npx * 3 * float_elem(xyz_dtype));
    int rc = st.stage();
    if (rc != OUSTER_HIP_OK) return rc;
    rc = ouster_hip_cartesian(ctx, lut, (const uint32_t*)st.dev(in), st.dev(out), xyz_dtype, 1);
    if (rc != OUSTER_HIP_OK) return rc;
    return st.finish();
}

}  // extern "C"
