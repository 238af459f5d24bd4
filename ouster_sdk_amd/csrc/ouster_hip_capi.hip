// ouster_hip_capi.hip -- host side of the C ABI declared in include/ouster_hip.h.
// Owns the error channel and the context (stream, scratch, knobs), turns format descriptions into the decode's tables, and
// runs the fused decode: the variant tuner's choice (decode_tuner.h; here only the events of the launches it wants timed), the
// launch plan (decode_plan.cpp) and the launches of k_decode*.hip.
// Every other entry point is in capi_<feature>.hip, next to the feature's kernels (destagger, cartesian and the LUTs, dewarp,
// OSF, images, frame_ops, pose, normals, voxel, ICP).
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <new>

#include "capi_internal.h"

using namespace ouster_hip_dev;

static thread_local std::string g_err;

namespace ouster_hip_dev {
int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
// the error channel of the plain C++ parts of the library (csrc/pose_host.h)
int fail_msg(int code, const char* msg) { return fail(code, "%s", msg); }
}  // namespace ouster_hip_dev

static void fill_geometry(const ouster_hip_format_desc& d, Geometry& g) {
    g.pixels_per_column = d.pixels_per_column;
    g.columns_per_packet = d.columns_per_packet;
    g.columns_per_frame = d.columns_per_frame;
    g.packet_header_size = d.packet_header_size;
    g.col_header_size = d.col_header_size;
    g.channel_data_size = d.channel_data_size;
    g.col_footer_size = d.col_footer_size;
    g.packet_footer_size = d.packet_footer_size;
    g.col_size = d.col_size;
    g.lidar_packet_size = d.lidar_packet_size;
    g.col_timestamp = d.col_timestamp;
    g.col_measurement_id = d.col_measurement_id;
    g.col_status = d.col_status;
    g.frame_id = d.frame_id;
    g.alert_flags = d.alert_flags;
    g.thermal_shutdown = d.thermal_shutdown;
    g.shot_limiting = d.shot_limiting;
    g.countdown_thermal_shutdown = d.countdown_thermal_shutdown;
    g.countdown_shot_limiting = d.countdown_shot_limiting;
}

extern "C" {

const char* ouster_hip_last_error(void) { return g_err.c_str(); }
#ifdef OUSTER_EXPERIMENTS
const char* ouster_hip_version(void) { return "ouster_hip 0.4 (gfx950) +experiments"; }
#else
const char* ouster_hip_version(void) { return "ouster_hip 0.4 (gfx950)"; }
#endif

int ouster_hip_ctx_create(int device, void* stream, ouster_hip_ctx** out) {
    if (!out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "out is NULL");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(OUSTER_HIP_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n)
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "device %d out of range [0,%d)", device, n);
    HIP_TRY(hipSetDevice(device));
    ouster_hip_ctx* c = new (std::nothrow) ouster_hip_ctx();
    if (!c) return fail(OUSTER_HIP_ERR_RUNTIME, "out of memory");
    c->device = device;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
            c->resident_wgs = 2u * (uint32_t)cus, c->cus = (uint32_t)cus;
    }
    for (int i = 0; i < knob_count; ++i) {   // the only place the environment is read
        const KnobDef& k = knob_table[i];
        if (const char* e = k.env ? getenv(k.env) : nullptr) c->knobs.*k.member = atoi(e);
    }
    if (const char* e = getenv("OUSTER_HIP_TUNING_CACHE")) (void)ouster_hip_ctx_set_tuning_cache(c, e);
    if (stream == OUSTER_HIP_STREAM_NULL) {
        c->stream = nullptr;  // the null stream
    } else if (stream) {
        c->stream = (hipStream_t)stream;
    } else {
        hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete c;
            return fail(OUSTER_HIP_ERR_RUNTIME, "hipStreamCreate: %s", hipGetErrorString(e));
        }
        c->own_stream = true;
    }
    *out = c;
    return OUSTER_HIP_OK;
}

void ouster_hip_ctx_destroy(ouster_hip_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;   // every member frees what it owns (capi_internal.h), the device still current
}

void* ouster_hip_ctx_stream(ouster_hip_ctx* c) { return c ? (void*)c->stream : nullptr; }

int ouster_hip_ctx_device(ouster_hip_ctx* c) { return c ? c->device : -1; }

int ouster_hip_ctx_set_knob(ouster_hip_ctx* c, const char* name, int value) {
    if (!c || !name) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!strcmp(name, "retune")) {   // forget what the variant tuner learnt (the caller moved its buffers: pick_placement)
        if (value) {
            (void)hipStreamSynchronize(c->stream);
            c->tuner.forget();   // what this context read from the cache file is void as well: it re-measures and appends anew
        }
        return OUSTER_HIP_OK;
    }
    const KnobDef* k = find_knob(name);
    if (!k) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "unknown knob '%s'", name);
    c->knobs.*k->member = value;
    return OUSTER_HIP_OK;
}

// persisted verdicts of the variant tuner (decode_tuner.h), under the id of this device and library
int ouster_hip_ctx_set_tuning_cache(ouster_hip_ctx* c, const char* path) {
    if (!c) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    std::string id;
    if (path && *path) {
        hipDeviceProp_t prop{};
        if (hipGetDeviceProperties(&prop, c->device) != hipSuccess) {
            (void)hipGetLastError();
            c->tuner.set_cache("", "");
            return fail(OUSTER_HIP_ERR_RUNTIME, "hipGetDeviceProperties failed");
        }
        id = tune_cache_id(prop.gcnArchName, prop.multiProcessorCount, prop.name, ouster_hip_version());
    }
    c->tuner.set_cache(path ? path : "", id);
    return OUSTER_HIP_OK;
}
const char* ouster_hip_last_decode_tuner(ouster_hip_ctx* c) { return c ? c->last_tuner : ""; }

int ouster_hip_sync(ouster_hip_ctx* c) {
    if (!c) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return OUSTER_HIP_OK;
}

// ---- format ----------------------------------------------------------------------------
int ouster_hip_format_create(ouster_hip_ctx* ctx, const ouster_hip_format_desc* d,
                             ouster_hip_format** out) {
    if (!ctx || !d || !out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (d->pixels_per_column == 0)
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "unexpected pixels_per_column: 0");
    if (d->columns_per_packet == 0)
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "unexpected columns_per_packet: 0");
    if (d->columns_per_frame == 0)
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "unexpected columns_per_frame: 0");
    if (d->n_fields > OUSTER_HIP_MAX_FIELDS)
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "too many fields (%u)", d->n_fields);
    if (d->col_size != d->col_header_size + d->pixels_per_column * d->channel_data_size +
                           d->col_footer_size ||
        d->lidar_packet_size != d->packet_header_size + d->columns_per_packet * d->col_size +
                                    d->packet_footer_size)
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "inconsistent packet geometry");
    if (d->lidar_packet_size > 65535)
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "lidar_packet_size cannot exceed 65535");
    if ((d->col_size & 3) || (d->packet_header_size & 3) || (d->lidar_packet_size & 3) ||
        (d->col_header_size & 3))
        return fail(OUSTER_HIP_ERR_UNSUPPORTED, "packet geometry must be 4-byte granular");
    for (uint32_t i = 0; i < d->n_fields; ++i) {
        const uint32_t e = d->fields[i].dst_elem_size;
        if (!(e == 1 || e == 2 || e == 4 || e == 6 || e == 8))
            return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "field %u: unsupported element size %u", i, e);
    }
    ouster_hip_format* f = new (std::nothrow) ouster_hip_format();
    if (!f) return fail(OUSTER_HIP_ERR_RUNTIME, "out of memory");
    f->desc = *d;
    fill_geometry(*d, f->g);
    // match against the compile-time specialisations
    f->spec_id = SPEC_GENERIC;
    for (int sid = SPEC_DUAL_LB; sid <= SPEC_LEGACY && f->spec_id == SPEC_GENERIC; ++sid) {
        int nf, r1, r2;
        uint32_t chan;
        const FieldC* sf = spec_fields(sid, &nf, &chan, &r1, &r2);
        if (chan != d->channel_data_size || (d->col_header_size & 3) || d->n_fields == 0) continue;
        bool ok = true;
        int8_t map[OUSTER_HIP_MAX_FIELDS];
        uint32_t used = 0;
        for (uint32_t i = 0; i < d->n_fields && ok; ++i) {
            const auto& fd = d->fields[i];
            int hit = -1;
            for (int k = 0; k < nf; ++k)
                if (!(used & (1u << k)) && sf[k].offset == fd.bits.offset &&
                    sf[k].mask == fd.bits.mask && sf[k].shift == fd.bits.shift &&
                    sf[k].elem == fd.dst_elem_size && !fd.f16_nan_fill) {
                    hit = k;
                    break;
                }
            if (hit < 0) ok = false;
            else { used |= 1u << hit; map[i] = (int8_t)hit; }
        }
        if (ok) {
            f->spec_id = sid;
            memcpy(f->spec_of_desc, map, sizeof map);
            f->spec_nf = nf;
            f->spec_r1 = r1;
            f->spec_r2 = r2;
        }
    }
    *out = f;
    return OUSTER_HIP_OK;
}

void ouster_hip_format_destroy(ouster_hip_format* f) { delete f; }

}  // extern "C"

// ---- helpers for per-call device tables -------------------------------------------------
// destination column offset per row with the reference's exact arithmetic:
//   offset = (w + sign*shift % w) % w   with w a size_t, i.e. `sign*shift` is converted to
//   an unsigned 64-bit value BEFORE the modulo (impl/lidar_frame_impl.h:737-756).
static void dest_offsets(const int32_t* shifts, uint32_t h, uint32_t w, int inverse,
                         std::vector<int32_t>& out) {
    out.resize(h);
    const int sign = inverse ? -1 : +1;
    const size_t ws = w;
    for (uint32_t u = 0; u < h; ++u) {
        const size_t x = (size_t)(long long)(sign * shifts[u]);
        out[u] = (int32_t)((ws + x % ws) % ws);
    }
}

static int ensure_offsets(ouster_hip_ctx* c, const std::vector<int32_t>& off) {
    if (off == c->offsets_host && c->offsets.p) return 0;
    if (c->offsets.ensure(off.size() * 4)) return -1;
    if (hipMemcpyAsync(c->offsets.p, off.data(), off.size() * 4, hipMemcpyHostToDevice,
                       c->stream) != hipSuccess)
        return -1;
    // the source vector must outlive the (possibly staged) copy
    if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
    c->offsets_host = off;
    return 0;
}

// what the standalone destagger and the OSF stagger launch with (capi_internal.h)
int ouster_hip_dev::stage_offsets(ouster_hip_ctx* c, const int32_t* shifts, uint32_t h, uint32_t w, int inverse, const int32_t** out) {
    std::vector<int32_t> off;
    dest_offsets(shifts, h, w, inverse, off);
    if (ensure_offsets(c, off)) return fail(OUSTER_HIP_ERR_RUNTIME, "offset upload failed");
    c->shifts_host.clear();  // ouster_hip_decode's cache key no longer describes `offsets`
    *out = (const int32_t*)c->offsets.p;
    return OUSTER_HIP_OK;
}

int ouster_hip_dev::ensure_luts(ouster_hip_ctx* c, const std::vector<LutDev>& l) {
    bool same = c->luts.p && l.size() == c->luts_host.size() &&
                memcmp(l.data(), c->luts_host.data(), l.size() * sizeof(LutDev)) == 0;
    if (same) return 0;
    if (c->luts.ensure(l.size() * sizeof(LutDev))) return -1;
    if (hipMemcpyAsync(c->luts.p, l.data(), l.size() * sizeof(LutDev), hipMemcpyHostToDevice,
                       c->stream) != hipSuccess)
        return -1;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
    c->luts_host = l;
    return 0;
}

extern "C" {

// ---- decode ------------------------------------------------------------------------------
// packet_counts may live anywhere: device memory is used in place; host memory is copied with the
// stream (pinned: directly; pageable: through the context's pinned ring) -- never a stream sync
static int stage_counts(ouster_hip_ctx* ctx, const uint32_t* packet_counts, uint32_t n_frames,
                        uint32_t slots_per_frame, const uint32_t** d_counts) {
    hipPointerAttribute_t attr{};
    const hipError_t pe = hipPointerGetAttributes(&attr, packet_counts);
    if (pe != hipSuccess) (void)hipGetLastError();  // an unregistered host pointer is not an error
    if (pe == hipSuccess && (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged)) {
        *d_counts = packet_counts;  // values above slots_per_frame are clamped by the kernels
        return OUSTER_HIP_OK;
    }
    for (uint32_t f = 0; f < n_frames; ++f)
        if (packet_counts[f] > slots_per_frame)
            return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "packet_counts[%u] > slots_per_frame", f);
    const size_t bytes = (size_t)n_frames * 4;
    if (ctx->counts.ensure(bytes)) return fail(OUSTER_HIP_ERR_RUNTIME, "hipMalloc(counts) failed");
    const void* src = packet_counts;
    const bool pinned = pe == hipSuccess && attr.type == hipMemoryTypeHost;
    int slot = -1;
    if (!pinned) {
        slot = ctx->ring_next;
        ctx->ring_next = (slot + 1) % ouster_hip_ctx::RING;
        if (!ctx->ring_ev[slot].e) HIP_TRY(ctx->ring_ev[slot].create(hipEventDisableTiming));
        else HIP_TRY(hipEventSynchronize(ctx->ring_ev[slot].e));  // RING calls ago: long done
        HIP_TRY(ctx->ring_buf[slot].ensure(bytes, bytes + bytes / 2));
        memcpy(ctx->ring_buf[slot].p, packet_counts, bytes);
        src = ctx->ring_buf[slot].p;
    }
    HIP_TRY(hipMemcpyAsync(ctx->counts.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (slot >= 0) HIP_TRY(hipEventRecord(ctx->ring_ev[slot].e, ctx->stream));
    *d_counts = (const uint32_t*)ctx->counts.p;
    return OUSTER_HIP_OK;
}

static bool fast_possible(const Knobs& kn, uint32_t slots_per_frame, const Geometry& g) {
    return kn.fast && (uint64_t)slots_per_frame * g.columns_per_packet == g.columns_per_frame;
}

// ---- decode: the steps of ouster_hip_decode, in its order -----------------------------------------------------------------
// argument checks; also makes the context's device current
static int check_decode_call(ouster_hip_ctx* ctx, const ouster_hip_format* fmt, const uint8_t* packets, size_t packet_stride,
                             uint32_t slots_per_frame, const ouster_hip_frame_out* out, const int32_t* pixel_shift_by_row,
                             const ouster_hip_lut* const* luts, uint32_t n_luts, bool any_dst, bool any_xyz) {
    if (!packets) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "packets is NULL");
    const Geometry& g = fmt->g;
    const uint32_t W = g.columns_per_frame, H = g.pixels_per_column, nf = fmt->desc.n_fields;
    if (packet_stride < g.lidar_packet_size || (packet_stride & 3) || ((uintptr_t)packets & 3))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT,
                    "packet_stride must be >= lidar_packet_size and 4-byte granular");
    if ((uint64_t)slots_per_frame * g.columns_per_packet > 0x7fffffffull || slots_per_frame == 0)
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "bad slots_per_frame");
    if ((uint64_t)slots_per_frame * packet_stride > 0xffffffffull)
        return fail(OUSTER_HIP_ERR_UNSUPPORTED, "a frame's packet buffer cannot exceed 4 GiB");
    if (W > 65536 || W / g.columns_per_packet > 8192)
        return fail(OUSTER_HIP_ERR_UNSUPPORTED, "more than 65536 columns or 8192 packets per frame");
    HIP_TRY(hipSetDevice(ctx->device));
    if (any_dst && !pixel_shift_by_row)
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "image height does not match shifts size");
    if (out->gate_counts) {
        const int gf = out->gate_field;
        if (gf < 0 || (uint32_t)gf >= nf || fmt->desc.fields[gf].dst_elem_size != 4)
            return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "gate_field must name a 32-bit range field");
        if (H > 65535) return fail(OUSTER_HIP_ERR_UNSUPPORTED, "gate counts are 16-bit: more than 65535 rows");
    }
    if (any_xyz) {
        if (!luts || n_luts == 0) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "xyz output needs a LUT");
        if (out->xyz_dtype != OUSTER_HIP_F32 && out->xyz_dtype != OUSTER_HIP_F64)
            return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "xyz_dtype must be F32 or F64");
        for (int k = 0; k < 2; ++k) {
            if (!out->xyz[k]) continue;
            const int xf = out->xyz_field[k];
            if (xf < 0 || (uint32_t)xf >= nf || fmt->desc.fields[xf].dst_elem_size != 4)
                return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT,
                            "xyz_field[%d] must name a 32-bit range field", k);
        }
        for (uint32_t i = 0; i < n_luts; ++i)
            if (!luts[i] || luts[i]->w != W || luts[i]->h != H)
                return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "unexpected image dimensions");
            else if (luts[i]->device != ctx->device)
                return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "LUT %u lives on GPU %d, the context on GPU %d", i,
                            luts[i]->device, ctx->device);
    }
    return OUSTER_HIP_OK;
}

// scratch: per-frame state words (all-zero between calls: the fix-up pass cleans up after itself), packet counts,
// destagger offsets, LUT descriptors.  xyzm: 0 no xyz | 1 / 2 separable tables, f32 / f64 output | 3 full LUT
static int stage_decode_tables(ouster_hip_ctx* ctx, const ouster_hip_format* fmt, uint32_t slots_per_frame,
                               const uint32_t* packet_counts, uint32_t n_frames, const ouster_hip_frame_out* out,
                               const int32_t* pixel_shift_by_row, const ouster_hip_lut* const* luts, uint32_t n_luts,
                               bool any_dst, bool any_xyz, const uint32_t** d_counts, int* xyzm) {
    const Geometry& g = fmt->g;
    const uint32_t W = g.columns_per_frame, H = g.pixels_per_column;
    {
        const void* before = ctx->state.p;
        if (ctx->state.ensure(((size_t)2 * n_frames + FS_WORDS) * 8)) return fail(OUSTER_HIP_ERR_RUNTIME, "hipMalloc(state) failed");
        if (ctx->state.p != before || ctx->state_dirty) HIP_TRY(hipMemsetAsync(ctx->state.p, 0, ctx->state.cap, ctx->stream));
        ctx->state_dirty = fast_possible(ctx->knobs, slots_per_frame, g);  // until the fix-up pass has been queued
    }
    if (out->frame_meta && ctx->tile_valid.ensure((size_t)n_frames * ((W + 15) / 16) * 2))
        return fail(OUSTER_HIP_ERR_RUNTIME, "hipMalloc(tile_valid) failed");
    *d_counts = nullptr;
    if (packet_counts) {
        const int rc = stage_counts(ctx, packet_counts, n_frames, slots_per_frame, d_counts);
        if (rc) return rc;
    }
    if (any_dst) {
        // the offsets only change with the sensor: key the cache on the shifts themselves
        if (!(ctx->offsets.p && ctx->shifts_host.size() == H && ctx->shifts_w == W &&
              memcmp(ctx->shifts_host.data(), pixel_shift_by_row, (size_t)H * 4) == 0 &&
              ctx->offsets_host.size() == H)) {
            std::vector<int32_t> off;
            dest_offsets(pixel_shift_by_row, H, W, 0, off);
            if (ensure_offsets(ctx, off)) return fail(OUSTER_HIP_ERR_RUNTIME, "offset upload failed");
            ctx->shifts_host.assign(pixel_shift_by_row, pixel_shift_by_row + H);
            ctx->shifts_w = W;
        }
    }
    *xyzm = 0;
    if (any_xyz) {
        bool all_sep = true, none_sep = true;
        bool same = ctx->luts.p && ctx->luts_host.size() == n_luts;
        for (uint32_t i = 0; i < n_luts; ++i) {
            all_sep &= luts[i]->separable;
            none_sep &= !luts[i]->separable;
            same = same && memcmp(&luts[i]->dev, &ctx->luts_host[i], sizeof(LutDev)) == 0;
        }
        if (!all_sep && !none_sep)
            return fail(OUSTER_HIP_ERR_UNSUPPORTED, "cannot mix separable and full LUTs in one batch");
        if (!same) {
            std::vector<LutDev> l(n_luts);
            for (uint32_t i = 0; i < n_luts; ++i) l[i] = luts[i]->dev;
            if (ensure_luts(ctx, l)) return fail(OUSTER_HIP_ERR_RUNTIME, "LUT descriptor upload failed");
        }
        *xyzm = all_sep ? (out->xyz_dtype == OUSTER_HIP_F32 ? 1 : 2) : 3;
    }
    return OUSTER_HIP_OK;
}

// the kernel arguments that follow from the call's arguments alone (tile shape, mode and scratch come from the plan).
// Returns the specialisation the kernels run with.
static int fill_decode_args(DecodeArgs& da, ouster_hip_ctx* ctx, const ouster_hip_format* fmt, const uint8_t* packets,
                            size_t packet_stride, uint32_t slots_per_frame, const uint32_t* d_counts, uint32_t n_frames,
                            const uint64_t* host_timestamps, const ouster_hip_frame_out* out, uint32_t n_luts, bool any_dst, int xyzm) {
    const Geometry& g = fmt->g;
    const uint32_t W = g.columns_per_frame, H = g.pixels_per_column, nf = fmt->desc.n_fields;
    da.g = g;
    da.packets = packets;
    da.packet_stride = packet_stride;
    da.slots_per_frame = slots_per_frame;
    da.n_frames = n_frames;
    da.n_packets_out = W / g.columns_per_packet;
    da.packet_counts = d_counts;
    da.host_timestamps = host_timestamps;
    da.frame_state = (uint64_t*)ctx->state.p;
    da.ready_off = FS_WORDS + (uint32_t)((ctx->state.cap / 8 - FS_WORDS) / 2);   // the second half of the buffer: moves only when it is reallocated (and zeroed)
    da.xyz_poses = xyzm ? out->xyz_poses : nullptr;
    da.gate_counts = out->gate_counts;
    da.gate_min = out->gate_min_r;
    da.gate_max = out->gate_max_r;
    da.gate_field = out->gate_counts ? out->gate_field : -1;
    da.tile_valid = (uint16_t*)ctx->tile_valid.p;
    da.dst_offsets = (const int32_t*)ctx->offsets.p;
    da.luts = (const LutDev*)ctx->luts.p;
    da.n_luts = n_luts ? n_luts : 1;
    da.n_fields = nf;
    da.any_destagger = any_dst;
    da.timestamp = out->timestamp;
    da.measurement_id = out->measurement_id;
    da.status = out->status;
    da.packet_timestamp = out->packet_timestamp;
    da.alert_flags = out->alert_flags;
    da.frame_meta = out->frame_meta;
    da.xyz[0] = out->xyz[0];
    da.xyz[1] = out->xyz[1];
    da.xyz_field[0] = out->xyz[0] ? out->xyz_field[0] : -1;
    da.xyz_field[1] = out->xyz[1] ? out->xyz_field[1] : -1;
    da.xyz_dtype = out->xyz_dtype;
    bool vec_ok = (W % 4 == 0);
    const size_t npx = (size_t)H * W;
    for (uint32_t i = 0; i < nf; ++i) {
        da.planes[i] = out->planes[i];
        da.destaggered[i] = out->destaggered[i];
        da.bits[i] = fmt->desc.fields[i].bits;
        da.elem[i] = (uint8_t)fmt->desc.fields[i].dst_elem_size;
        da.f16_nan_mask |= fmt->desc.fields[i].f16_nan_fill ? (1u << i) : 0u;
        const size_t fstride = npx * da.elem[i];
        if (out->planes[i]) vec_ok &= al16(out->planes[i]) && (fstride % 16 == 0);
        // destaggered stores are unaligned-capable; only 4-byte stores of sub-dword
        // elements need the element alignment the caller already guarantees
    }
    const size_t xes = out->xyz_dtype == OUSTER_HIP_F64 ? 8 : 4;
    for (int k = 0; k < 2; ++k)
        if (out->xyz[k]) vec_ok &= al16(out->xyz[k]) && ((npx * 3 * xes) % 16 == 0);
    da.vec_ok = vec_ok;

    int spec = fmt->spec_id;
    if (spec != SPEC_GENERIC) {
        for (int k = 0; k < 16; ++k) da.desc_of_spec[k] = -1;
        for (uint32_t i = 0; i < nf; ++i) da.desc_of_spec[fmt->spec_of_desc[i]] = (int8_t)i;
        // the compile-time kernels take the xyz ranges from their RANGE / RANGE2 slots
        if (out->xyz[0] && fmt->spec_of_desc[out->xyz_field[0]] != fmt->spec_r1) spec = SPEC_GENERIC;
        if (out->xyz[1] && fmt->spec_of_desc[out->xyz_field[1]] != fmt->spec_r2) spec = SPEC_GENERIC;
    }
    return spec;
}

// what the launch plan (decode_plan.h) is a function of
static PlanInput fill_plan_input(const DecodeArgs& da, const ouster_hip_ctx* ctx, int spec, int xyzm) {
    PlanInput in{};
    in.g = da.g;
    in.kn = ctx->knobs;
    in.n_frames = da.n_frames;
    in.slots_per_frame = da.slots_per_frame;
    in.packet_stride = da.packet_stride;
    in.packets = (uintptr_t)da.packets;
    in.xyz_poses = (uintptr_t)da.xyz_poses;
    in.spec = spec;
    in.xyzm = xyzm;
    in.vec_ok = da.vec_ok;
    in.n_fields = da.n_fields;
    for (uint32_t i = 0; i < da.n_fields; ++i) {
        in.plane_mask |= da.planes[i] ? (1ull << i) : 0;
        in.destagger_mask |= da.destaggered[i] ? (1ull << i) : 0;
    }
    in.xyz_mask = (da.xyz[0] ? 1u : 0u) | (da.xyz[1] ? 2u : 0u);
    in.gate_counts = da.gate_counts != nullptr;
    in.host_ts = da.host_timestamps && da.packet_timestamp;
    in.cus = ctx->cus;
    in.resident_wgs = ctx->resident_wgs;
#ifdef OUSTER_EXPERIMENTS
    in.may_resolve = true;
#else
    in.may_resolve = false;   // k_decode_wide_resolved is not compiled
#endif
    return in;
}

// The variant this call launches (decode_tuner.h).  The tuner stands down with tune = 0, for a shape with nothing to choose
// (or a choice forced by a knob) and while the stream is being captured: the default variant runs.
using Tuner = decltype(ouster_hip_ctx::tuner);
static Tuner::Step tune_step(ouster_hip_ctx* ctx, const PlanInput& in, const Candidates& cand) {
    Tuner::Step ts;
    if (cand.n && in.kn.tune) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(ctx->stream, &cap);
        if (cap == hipStreamCaptureStatusNone) ts = ctx->tuner.step(tuner_key(in, cand), cand.variant, cand.n);
    }
    ctx->last_tuner = ts.source;
    return ts;
}

static void set_shape(DecodeArgs& da, const TileShape& s) {
    da.rows_per_tile = s.rows_per_tile;
    da.row_chunks = s.row_chunks;
    da.lds_col_slot = s.lds_col_slot;
    da.tiles_per_frame = s.tiles_per_frame;
    da.fix_rows_small = s.fix_rows_small;
}

int ouster_hip_decode(ouster_hip_ctx* ctx, const ouster_hip_format* fmt, const uint8_t* packets,
                      size_t packet_stride, uint32_t slots_per_frame,
                      const uint32_t* packet_counts, uint32_t n_frames,
                      const uint64_t* host_timestamps, const ouster_hip_frame_out* out,
                      const int32_t* pixel_shift_by_row, const ouster_hip_lut* const* luts,
                      uint32_t n_luts) {
    if (!ctx || !fmt || !out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_frames == 0) return OUSTER_HIP_OK;
    const Geometry& g = fmt->g;
    const uint32_t W = g.columns_per_frame, H = g.pixels_per_column, nf = fmt->desc.n_fields;
    bool any_dst = false;
    const bool any_xyz = (out->xyz[0] || out->xyz[1]);
    for (uint32_t i = 0; i < nf; ++i) any_dst |= out->destaggered[i] != nullptr;
    if (const int rc = check_decode_call(ctx, fmt, packets, packet_stride, slots_per_frame, out, pixel_shift_by_row, luts, n_luts, any_dst, any_xyz))
        return rc;
    hipStream_t st = ctx->stream;

    const uint32_t* d_counts = nullptr;
    int xyzm = 0;
    if (const int rc = stage_decode_tables(ctx, fmt, slots_per_frame, packet_counts, n_frames, out, pixel_shift_by_row, luts, n_luts, any_dst,
                                           any_xyz, &d_counts, &xyzm))
        return rc;
    if (out->xyz_poses && xyzm == 3)
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "xyz_poses need LUTs with separable tables (ouster_hip_lut_create)");

    DecodeArgs da{};
    const int spec = fill_decode_args(da, ctx, fmt, packets, packet_stride, slots_per_frame, d_counts, n_frames, host_timestamps, out, n_luts,
                                      any_dst, xyzm);
#ifdef OUSTER_PHASE_TIMING
    {   // experiment builds only: the tool passes a device buffer's address through the environment
        const char* e = getenv("OUSTER_HIP_PHASE_BUF");
        da.phase_times = e ? (uint64_t*)strtoull(e, nullptr, 0) : nullptr;
    }
    uint64_t* const phase_times_all = da.phase_times;
    if (getenv("OUSTER_HIP_PHASE_FIXUP_ONLY")) da.phase_times = nullptr;   // only the fix-up pass stamps
#endif

    // ---- the plan (decode_plan.h): which kernel, which tiles, which scratch
    const PlanInput in = fill_plan_input(da, ctx, spec, xyzm);
    const bool fast = fast_possible(in.kn, slots_per_frame, g);
    const Candidates cand = plan_candidates(in);
    const Tuner::Step ts = tune_step(ctx, in, cand);
    DecodePlan plan = plan_decode(in, cand, ts.variant);
    if (!plan.ok)   // the general mapping keeps resolve_frame's scratch ((2 + cpp) words per buffer slot) in LDS next to the tile
        return fail(OUSTER_HIP_ERR_UNSUPPORTED,
                    fast ? "column of %u bytes does not fit in LDS"
                         : "column of %u bytes + the column maps of %u buffer slots per frame do not fit in LDS (general mapping: at most "
                           "about 2000 slots of 16 columns; hand the frame over in fewer slots or in home slots)",
                    g.col_size, slots_per_frame);

    // ---- every allocation of the call is settled here, before the first launch
    if (plan.hdr_words_bytes) {
        if (ctx->hdrw.ensure(plan.hdr_words_bytes)) return fail(OUSTER_HIP_ERR_RUNTIME, "out of device memory (header words)");
        da.hdr_words = (uint32_t*)ctx->hdrw.p;
    }
    if (plan.fixup == Fixup::WIDE && ctx->slotmap.ensure(plan.slotmap_bytes)) demote_fixup(in, plan);   // the 64-column fix-up needs no maps
    if (plan.slotmap) {
        if (ctx->slotmap.ensure(plan.slotmap_bytes)) return fail(OUSTER_HIP_ERR_RUNTIME, "out of device memory (slot map)");
        da.slot_map = (int32_t*)ctx->slotmap.p;
        da.hdr_map = da.slot_map + (size_t)n_frames * W;
    }
    set_shape(da, plan.shape);
    da.beam_lds = plan.beam_lds;
    da.xcd_map = plan.xcd_map;
    da.mode = plan.mode;
    da.fast_tiles = plan.fast_tiles;
    if (plan.mode == MODE_RESOLVED) ctx->state_dirty = false;   // this call leaves the frame words alone

    // ---- the optimistic (or only) pass
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (ctx->timing && (ctx->timing_calls++ % ctx->timing_every) == 0) {
        if (ctx->ev_used == ctx->ev_pool.size()) ctx->ev_pool.emplace_back();
        auto& pair = ctx->ev_pool[ctx->ev_used];
        for (Event& e : pair) HIP_TRY(e.create());
        e0 = pair[0].e;
        e1 = pair[1].e;
        ctx->ev_used++;
        HIP_TRY(hipEventRecord(e0, st));
    }
    Event* const sample = ts.record ? ts.record->ev[ts.slot] : nullptr;   // the tuner wants this launch timed
    if (sample) {
        for (int k = 0; k < 2; ++k) HIP_TRY(sample[k].create());
        HIP_TRY(hipEventRecord(sample[0].e, st));
    }
    if (plan.slotmap) HIP_TRY(launch_slotmap(da, ctx->device, st));
    switch (plan.kernel) {
        case Kernel::STREAM:
        case Kernel::STREAM2:
            HIP_TRY(launch_decode_stream(da, plan.sa, spec, plan.cols, xyzm, ctx->device, st));
            ctx->last_tile_rows = (int)plan.sa.tr;
            break;
        case Kernel::WIDE:
        case Kernel::WIDE_RESOLVED:
            HIP_TRY(launch_decode_wide(da, spec, plan.cols, xyzm, ctx->device, st));
            ctx->last_tile_rows = (int)plan.shape.rows_per_tile;
            break;
        case Kernel::DECODE:
            HIP_TRY(launch_decode(da, spec, plan.narrow_tile, xyzm, ctx->device, st));
            ctx->last_tile_rows = (int)H;
            break;
    }
    ctx->last_tile_cols = plan.cols;
    ctx->last_kernel = kernel_name(plan.kernel);
    if (sample) HIP_TRY(hipEventRecord(sample[1].e, st));
    if (e1) HIP_TRY(hipEventRecord(e1, st));

    // ---- the fix-up pass: always launched behind an optimistic kernel; the workgroups of a clean batch leave after two
    // scalar loads (FS_ANY)
    if (plan.fixup != Fixup::NONE) {
        da.mode = MODE_FIXUP;
#ifdef OUSTER_PHASE_TIMING
        da.phase_times = phase_times_all;
#endif
        set_shape(da, plan.fix_shape);
        if (plan.fixup == Fixup::WIDE) {
            da.slot_map = (int32_t*)ctx->slotmap.p;
            da.hdr_map = da.slot_map + (size_t)n_frames * W;
            HIP_TRY(launch_decode_wide(da, spec, plan.fix_cols, xyzm, ctx->device, st, ctx->resident_wgs));
        } else {
            HIP_TRY(launch_decode(da, spec, plan.narrow_tile, xyzm, ctx->device, st));
        }
        ctx->state_dirty = false;
    }
    return OUSTER_HIP_OK;
}

// ---- host containers (include/ouster_hip.h, "host containers") -----------------------------------
int ouster_hip_device_alloc(ouster_hip_ctx* ctx, size_t bytes, void** out) {
    if (!ctx || !out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(ctx->device));
    *out = nullptr;
    const hipError_t e = counted_malloc(out, bytes ? bytes : 1);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(OUSTER_HIP_ERR_RUNTIME, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    }
    return OUSTER_HIP_OK;
}
void ouster_hip_device_free(void* p) { counted_free(p); }

int ouster_hip_ctx_scratch(ouster_hip_ctx* ctx, uint32_t slot, size_t bytes, void** out) {
    if (!ctx || !out || slot >= 8) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "bad scratch request");
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->user_scratch[slot].ensure(bytes ? bytes : 1)) return fail(OUSTER_HIP_ERR_RUNTIME, "out of device memory (scratch %u, %zu bytes)", slot, bytes);
    *out = ctx->user_scratch[slot].p;
    return OUSTER_HIP_OK;
}

int ouster_hip_copy_in(ouster_hip_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes) {
    if (!ctx || (bytes && (!dev_dst || !host_src))) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (bytes) HIP_TRY(hipMemcpyAsync(dev_dst, host_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return OUSTER_HIP_OK;
}
int ouster_hip_copy_out(ouster_hip_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes) {
    if (!ctx || (bytes && (!host_dst || !dev_src))) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (bytes) HIP_TRY(hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return OUSTER_HIP_OK;
}

const char* ouster_hip_last_decode_kernel(ouster_hip_ctx* ctx) { return ctx ? ctx->last_kernel : ""; }

int ouster_hip_last_decode_tile(ouster_hip_ctx* ctx, int* tile_cols, int* tile_rows) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (tile_cols) *tile_cols = ctx->last_tile_cols;
    if (tile_rows) *tile_rows = ctx->last_tile_rows;
    return OUSTER_HIP_OK;
}

// ---- timing ------------------------------------------------------------------------------------
int ouster_hip_timing_enable(ouster_hip_ctx* ctx, int on) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    // on > 1: sample every on-th launch (the event pair around a kernel costs the stream 2 - 3 us: a timed region that wants the
    // kernel's duration without paying that on every step samples)
    ctx->timing = on != 0;
    ctx->timing_every = on > 1 ? (uint32_t)on : 1u;
    ctx->timing_calls = 0;
    ctx->ev_used = 0;
    return OUSTER_HIP_OK;
}

int ouster_hip_timing_read(ouster_hip_ctx* ctx, double* avg_ms, uint32_t* n_launches) {
    if (!ctx || !avg_ms) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    double total = 0;
    for (size_t i = 0; i < ctx->ev_used; ++i) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ctx->ev_pool[i][0].e, ctx->ev_pool[i][1].e));
        total += ms;
    }
    *avg_ms = ctx->ev_used ? total / (double)ctx->ev_used : 0.0;
    if (n_launches) *n_launches = (uint32_t)ctx->ev_used;
    ctx->ev_used = 0;
    return OUSTER_HIP_OK;
}

}  // extern "C"
