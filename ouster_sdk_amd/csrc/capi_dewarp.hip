// capi_dewarp.hip -- the C ABI of the dense dewarp and the range-gated frame dewarp (k_dewarp.hip): ouster_hip_dewarp /
// _dewarp_host / ouster_hip_range_gate / ouster_hip_dewarp_frames / _counted / _rows
#include "capi_internal.h"

using namespace ouster_hip_dev;

extern "C" {

// ---- dense dewarp -----------------------------------------------------------------------------
int ouster_hip_dewarp(ouster_hip_ctx* ctx, const void* points, const double* poses, void* dewarped,
                      int dtype, uint32_t h, uint32_t w, uint32_t n_images) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (!float_elem(dtype))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dtype must be F32 or F64");
    if (n_images == 0 || h == 0 || w == 0) return OUSTER_HIP_OK;
    if (!points || !poses || !dewarped) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    HIP_TRY(hipSetDevice(ctx->device));
    DewarpArgs a{};
    a.points = points;
    a.out = dewarped;
    a.poses = poses;
    a.w = w;
    a.h = h;
    a.n_images = n_images;
    a.dtype = dtype;
    HIP_TRY(launch_dewarp(a, ctx->stream));
    return OUSTER_HIP_OK;
}

int ouster_hip_dewarp_host(ouster_hip_ctx* ctx, const void* points, const double* poses, void* dewarped, int dtype,
                           uint32_t h, uint32_t w) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (!float_elem(dtype)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dtype must be F32 or F64");
    if (h == 0 || w == 0) return OUSTER_HIP_OK;
    if (!points || !poses || !dewarped) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t pbytes = (size_t)h * w * 3 * float_elem(dtype);
    Staging st(ctx);
    const auto in = st.input(points, pbytes), po = st.input(poses, (size_t)w * 128), out = st.output(dewarped, pbytes);
    int rc = st.stage();
    if (rc != OUSTER_HIP_OK) return rc;
    rc = ouster_hip_dewarp(ctx, st.dev(in), (const double*)st.dev(po), st.dev(out), dtype, h, w, 1);
    if (rc != OUSTER_HIP_OK) return rc;
    return st.finish();
}

// ---- range-gated, compacting frame dewarp ------------------------------------------------------
int ouster_hip_range_gate(double min_range, double max_range, uint32_t* min_r, uint32_t* max_r, int* empty) {
    // uint32_t min_r = ceil(min_range * 1e3), max_r = floor(max_range * 1e3): dewarp_impl.h:33-34
    const double lo = std::ceil(min_range * 1e3), hi = std::floor(max_range * 1e3);
    const bool none = !(hi >= 0) || !(lo <= 4294967295.0) || hi < lo;   // nothing can pass the gate
    if (empty) *empty = none ? 1 : 0;
    if (min_r) *min_r = (none || lo <= 0) ? 0u : (uint32_t)lo;
    if (max_r) *max_r = none ? 0u : (hi >= 4294967295.0 ? 0xffffffffu : (uint32_t)hi);
    return OUSTER_HIP_OK;
}

int ouster_hip_dewarp_frames(ouster_hip_ctx* ctx, const ouster_hip_lut* const* luts, uint32_t n_luts,
                             const uint32_t* range, const uint32_t* status,
                             const uint64_t* timestamp, const double* poses, uint32_t n_frames,
                             double min_range, double max_range, int dtype, void* points,
                             uint32_t* frame_idxs, uint32_t* col_idxs, uint64_t* timestamps_ns,
                             uint64_t capacity, uint64_t* frame_offsets) {
    return ouster_hip_dewarp_frames_counted(ctx, luts, n_luts, range, status, timestamp, poses, n_frames, min_range,
                                            max_range, dtype, points, frame_idxs, col_idxs, timestamps_ns, capacity,
                                            frame_offsets, nullptr);
}

static int dewarp_frames_impl(ouster_hip_ctx* ctx, const ouster_hip_lut* const* luts, uint32_t n_luts,
                              const uint32_t* range, const uint32_t* status,
                              const uint64_t* timestamp, const double* poses, const float* pose_rows, uint32_t n_frames,
                              double min_range, double max_range, int dtype, void* points,
                              uint32_t* frame_idxs, uint32_t* col_idxs, uint64_t* timestamps_ns,
                              uint64_t capacity, uint64_t* frame_offsets, const uint16_t* gate_counts) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (!float_elem(dtype))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dtype must be F32 or F64");
    if (!luts || n_luts == 0) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "at least one LUT is required");
    for (uint32_t i = 0; i < n_luts; ++i) {
        if (!luts[i]) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL LUT handle");
        if (luts[i]->w != luts[0]->w || luts[i]->h != luts[0]->h)
            return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "all LUTs of a batch must have the same dimensions");
        if (luts[i]->separable != luts[0]->separable)
            return fail(OUSTER_HIP_ERR_UNSUPPORTED, "cannot mix separable and full LUTs in one batch");
    }
    if (!frame_offsets) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "frame_offsets is NULL");
    if (timestamps_ns && !timestamp)
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "timestamps_ns requested without column timestamps");
    HIP_TRY(hipSetDevice(ctx->device));
    if (n_frames == 0) {
        HIP_TRY(hipMemsetAsync(frame_offsets, 0, sizeof(uint64_t), ctx->stream));
        return OUSTER_HIP_OK;
    }
    if (pose_rows && (((uintptr_t)pose_rows) & 15u))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "pose_rows must be 16-byte aligned");
    if (!range || !status || (!poses && !pose_rows) || (!points && capacity))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    const uint32_t w = luts[0]->w, h = luts[0]->h;
    DewarpFramesArgs a{};
    int gate_empty = 0;
    ouster_hip_range_gate(min_range, max_range, &a.min_r, &a.max_r, &gate_empty);
    if (gate_empty) {
        HIP_TRY(hipMemsetAsync(frame_offsets, 0, sizeof(uint64_t) * ((size_t)n_frames + 1), ctx->stream));
        return OUSTER_HIP_OK;
    }
    std::vector<LutDev> l(n_luts);
    for (uint32_t i = 0; i < n_luts; ++i) l[i] = luts[i]->dev;
    if (ensure_luts(ctx, l)) return fail(OUSTER_HIP_ERR_RUNTIME, "LUT descriptor upload failed");
    // scratch: the three-kernel path's per-column offsets, then the single-pass path's tile words
    const size_t col_off_bytes = ((size_t)n_frames * (w + 1) * sizeof(uint32_t) + 15) & ~(size_t)15;
    const size_t tile_words = (size_t)n_frames * ((w + 63) / 64) + 128;
    if (ctx->scratch.ensure(col_off_bytes + tile_words * 8))
        return fail(OUSTER_HIP_ERR_RUNTIME, "scratch allocation failed");
    a.range = range;
    a.status = status;
    a.timestamp = timestamp;
    a.poses = poses;
    a.pose_rows = pose_rows;
    a.luts = (const LutDev*)ctx->luts.p;
    a.n_luts = n_luts;
    a.w = w;
    a.h = h;
    a.n_frames = n_frames;
    a.dtype = dtype;
    a.col_off = (uint32_t*)ctx->scratch.p;
    a.gate_counts = gate_counts;
#ifdef OUSTER_EXPERIMENTS
    a.tile_state = (ctx->knobs.dewarp_single_pass && !gate_counts && !pose_rows) ? (uint64_t*)((uint8_t*)ctx->scratch.p + col_off_bytes) : nullptr;
#else
    a.tile_state = nullptr;   // the single-pass kernels are not in a default build (knob "dewarp_single_pass" is then without effect)
#endif
    a.frame_off = frame_offsets;
    a.points = points;
    a.frame_idxs = frame_idxs;
    a.col_idxs = col_idxs;
    a.timestamps_ns = timestamps_ns;
    a.capacity = capacity;
    HIP_TRY(launch_dewarp_frames(a, luts[0]->separable, ctx->stream, ctx->knobs.dwf_stream));
    return OUSTER_HIP_OK;
}

int ouster_hip_dewarp_frames_counted(ouster_hip_ctx* ctx, const ouster_hip_lut* const* luts, uint32_t n_luts,
                                     const uint32_t* range, const uint32_t* status,
                                     const uint64_t* timestamp, const double* poses, uint32_t n_frames,
                                     double min_range, double max_range, int dtype, void* points,
                                     uint32_t* frame_idxs, uint32_t* col_idxs, uint64_t* timestamps_ns,
                                     uint64_t capacity, uint64_t* frame_offsets, const uint16_t* gate_counts) {
    return dewarp_frames_impl(ctx, luts, n_luts, range, status, timestamp, poses, nullptr, n_frames, min_range, max_range, dtype,
                              points, frame_idxs, col_idxs, timestamps_ns, capacity, frame_offsets, gate_counts);
}

int ouster_hip_dewarp_frames_rows(ouster_hip_ctx* ctx, const ouster_hip_lut* const* luts, uint32_t n_luts,
                                  const uint32_t* range, const uint32_t* status, const uint64_t* timestamp,
                                  const float* pose_rows, uint32_t n_frames, double min_range, double max_range,
                                  void* points, uint32_t* frame_idxs, uint32_t* col_idxs, uint64_t* timestamps_ns,
                                  uint64_t capacity, uint64_t* frame_offsets, const uint16_t* gate_counts) {
    if (!pose_rows && n_frames) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    return dewarp_frames_impl(ctx, luts, n_luts, range, status, timestamp, nullptr, pose_rows, n_frames, min_range, max_range,
                              OUSTER_HIP_F32, points, frame_idxs, col_idxs, timestamps_ns, capacity, frame_offsets, gate_counts);
}

}  // extern "C"
