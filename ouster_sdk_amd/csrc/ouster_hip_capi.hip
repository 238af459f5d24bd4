// ouster_hip_capi.hip -- host side of the C ABI declared in include/ouster_hip.h.
// Owns the context (stream, scratch), turns format / calibration descriptions into
// device tables and launches the kernels of ouster_hip_kernels.hip.  No compute happens
// on the host except the one-off XYZ table construction (make_xyz_lut is a one-off in the
// reference too: ouster_core/src/xyzlut.cpp:11-89, cached per sensor in sensor_info.cpp:260-275).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <map>
#include <new>
#include <string>
#include <unistd.h>
#include <vector>

#include "host_pool.h"
#include "k_frame_ops.h"
#include "k_image.h"
#include "k_normals.h"
#include "k_pose.h"
#include "k_voxel.h"
#include "k_icp.h"
#include "ouster_hip_dev.h"

using namespace ouster_hip_dev;

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return fail(OUSTER_HIP_ERR_RUNTIME, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t n) {
        if (n <= cap) return 0;
        counted_free(p);
        p = nullptr;
        cap = 0;
        size_t want = n + n / 2;
        if (counted_malloc(&p, want) != hipSuccess) {
            p = nullptr;
            return -1;
        }
        cap = want;
        return 0;
    }
    void release() {
        counted_free(p);
        p = nullptr;
        cap = 0;
    }
};

}  // namespace

// the error channel of the plain C++ parts of the library (csrc/pose_host.h)
namespace ouster_hip_dev {
int fail_msg(int code, const char* msg) { return fail(code, "%s", msg); }
}  // namespace ouster_hip_dev

// k_decode variant (64-column tiles / wide tiles of 128 or 256 columns / the persistent kernel) per workload, picked by
// timing each candidate on the first calls: which one is faster depends on how the output planes happen to be placed
// in HBM
struct Tune {
    int best = -2;  // -2: still measuring; 0: narrow; 128 / 256: wide; 1000 + tile width: the persistent kernel
    int calls = 0;
    bool from_cache = false;   // `best` was read from the tuning cache file, not timed by this context
    static constexpr int ROUNDS = 4, NCAND = 5, SAMPLES = NCAND * ROUNDS;
    hipEvent_t ev[SAMPLES][2] = {};  // up to five candidates x ROUNDS consecutive launches
    float ms[NCAND] = {0, 0, 0, 0, 0};  // fastest warm sample of each candidate
    void destroy() {
        for (auto& pr : ev)
            for (hipEvent_t& e : pr)
                if (e) (void)hipEventDestroy(e), e = nullptr;
    }
};

struct ouster_hip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    DevBuf state, tile_valid, offsets, luts, counts, scratch, slotmap, hdrw, osf_pixels;
    DevBuf image_mask;                   // ouster_hip_image_dark_rows: the column masks of a batch
    void* fops_pin = nullptr;            //   ... their page-locked staging, and the event behind its last copy
    size_t fops_pin_cap = 0;
    hipEvent_t fops_ev = nullptr;
    DevBuf fops_tables;                  // ouster_hip_frame_ops_*: shift tables reduced to [0, w) / row indices of the call in flight
    DevBuf normals_pairs;                // ouster_hip_normals: what k_normals_subtent leaves, 16 bytes per frame and return
    bool voxel_timing = false, voxel_timed = false;   // ouster_hip_voxel_timing: events around the phases of a call
    hipEvent_t voxel_ev[OUSTER_HIP_VOXEL_PHASES + 1] = {};
    DevBuf voxel_ws;                     // ouster_hip_voxel_downsample: keys, table, ids, sorted indices, gathered rows, sort temporaries
    bool icp_timing = false;             // ouster_hip_icp_timing: events around the phases of a call; icp_timed_passes: of the last one
    uint32_t icp_timed_passes = 0;
    bool icp_timed = false;
    hipEvent_t icp_ev[2 + 4 * 10] = {};  //   start, after the grid, then per pass: start, after correspond, after median, after sums
    DevBuf icp_ws;                       // ouster_hip_icp_*: the target grid, the per-row outputs of a pass, partial sums, sort temporaries
    DevBuf user_scratch[8];              // ouster_hip_ctx_scratch: what the *_host calls and bindings stage through
    uint32_t resident_wgs = 512;         // 2 workgroups (80 KB LDS each) per CU
    uint32_t cus = 256;                  // compute units (k_decode_stream: one persistent workgroup each)
    const char* last_kernel = "";        // name of the decode kernel the last ouster_hip_decode launched
    bool state_dirty = false;            // `state` may hold leftovers (fix-up pass skipped / a failed launch)
    std::vector<int32_t> offsets_host;   // cache key of `offsets`
    std::vector<int32_t> shifts_host;    // pixel_shift_by_row the cached offsets were derived from
    uint32_t shifts_w = 0;               //   ... and the frame width (the offsets are (W + x % W) % W)
    std::vector<LutDev> luts_host;       // cache key of `luts`
    // pageable host packet_counts go through a small pinned ring (no stream synchronisation)
    static constexpr int RING = 4;
    uint32_t* ring_buf[RING] = {nullptr, nullptr, nullptr, nullptr};
    size_t ring_cap[RING] = {0, 0, 0, 0};
    hipEvent_t ring_ev[RING] = {nullptr, nullptr, nullptr, nullptr};
    int ring_next = 0;
    Knobs knobs;
    bool timing = false;
    uint32_t timing_every = 1, timing_calls = 0;   // HIP events around every timing_every-th decode kernel (an event record costs the stream 2 - 3 us)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    size_t ev_used = 0;
    std::map<uint64_t, Tune> tune;       // the variant tuner, by workload key (decode_plan.h)
    // verdicts of earlier processes (ouster_hip_ctx_set_tuning_cache): workload key -> chosen variant, for THIS device and library
    std::string tune_cache_path, tune_cache_id;
    std::map<uint64_t, int> tune_cache;
    const char* last_tuner = "none";     // how the last ouster_hip_decode chose its variant
    int last_tile_cols = 0, last_tile_rows = 0;  // tile of the last k_decode launch
};

static void tune_forget(ouster_hip_ctx* c) {   // the one place the tuner's events are destroyed
    for (auto& kv : c->tune) kv.second.destroy();
    c->tune.clear();
}

struct ouster_hip_format {
    ouster_hip_format_desc desc;
    Geometry g;
    int spec_id = SPEC_GENERIC;
    int8_t spec_of_desc[OUSTER_HIP_MAX_FIELDS];
    int spec_nf = 0, spec_r1 = -1, spec_r2 = -1;
};

struct ouster_hip_lut {
    int device = 0;  // the tables outlive the context that uploaded them
    uint32_t w = 0, h = 0;
    bool separable = false;
    LutDev dev{};
    void *d_beam = nullptr, *d_col = nullptr, *d_dir = nullptr, *d_ofs = nullptr;
    // host copy of the full double LUT for ouster_hip_lut_export
    std::vector<double> direction, offset;
};

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
const char* ouster_hip_version(void) { return "ouster_hip 0.3 (gfx950) +experiments"; }
#else
const char* ouster_hip_version(void) { return "ouster_hip 0.3 (gfx950)"; }
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
    c->state.release();
    c->tile_valid.release();
    for (int i = 0; i < ouster_hip_ctx::RING; ++i) {
        if (c->ring_buf[i]) (void)hipHostFree(c->ring_buf[i]);
        if (c->ring_ev[i]) (void)hipEventDestroy(c->ring_ev[i]);
    }
    c->offsets.release();
    c->luts.release();
    c->counts.release();
    c->scratch.release();
    c->slotmap.release();
    c->hdrw.release();
    c->osf_pixels.release();
    c->image_mask.release();
    c->fops_tables.release();
    c->normals_pairs.release();
    c->voxel_ws.release();
    c->icp_ws.release();
    for (hipEvent_t& e : c->icp_ev)
        if (e) (void)hipEventDestroy(e), e = nullptr;
    for (hipEvent_t& e : c->voxel_ev)
        if (e) (void)hipEventDestroy(e), e = nullptr;
    if (c->fops_ev) (void)hipEventDestroy(c->fops_ev);
    if (c->fops_pin) (void)hipHostFree(c->fops_pin);
    for (auto& b : c->user_scratch) b.release();
    for (auto& p : c->ev_pool) {
        (void)hipEventDestroy(p.first);
        (void)hipEventDestroy(p.second);
    }
    tune_forget(c);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

void* ouster_hip_ctx_stream(ouster_hip_ctx* c) { return c ? (void*)c->stream : nullptr; }

int ouster_hip_ctx_device(ouster_hip_ctx* c) { return c ? c->device : -1; }

int ouster_hip_ctx_set_knob(ouster_hip_ctx* c, const char* name, int value) {
    if (!c || !name) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!strcmp(name, "retune")) {   // forget what the variant tuner learnt (the caller moved its buffers: pick_placement)
        if (value) {
            (void)hipStreamSynchronize(c->stream);
            tune_forget(c);
            c->tune_cache.clear();   // what this context read from the cache file is void as well: it re-measures and appends anew
        }
        return OUSTER_HIP_OK;
    }
    const KnobDef* k = find_knob(name);
    if (!k) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "unknown knob '%s'", name);
    c->knobs.*k->member = value;
    return OUSTER_HIP_OK;
}

// ---- persisted verdicts of the variant tuner -----------------------------------------------------------------------------
// One text line per verdict: "v1 <device and library id> <workload key, hex> <variant> <its fastest sample, ms>".  Lines are
// appended with one write() each (O_APPEND: ranks of one job may share the file), the last line of a key wins at load.
int ouster_hip_ctx_set_tuning_cache(ouster_hip_ctx* c, const char* path) {
    if (!c) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    c->tune_cache.clear();
    c->tune_cache_path = path ? path : "";
    if (c->tune_cache_path.empty()) return OUSTER_HIP_OK;
    hipDeviceProp_t prop{};
    if (hipGetDeviceProperties(&prop, c->device) != hipSuccess) {
        (void)hipGetLastError();
        c->tune_cache_path.clear();
        return fail(OUSTER_HIP_ERR_RUNTIME, "hipGetDeviceProperties failed");
    }
    std::string id = std::string(prop.gcnArchName) + ":" + std::to_string(prop.multiProcessorCount) + ":" + prop.name + ":" + ouster_hip_version();
    for (char& ch : id) if (ch == ' ' || ch == '\t') ch = '_';
    c->tune_cache_id = id;
    if (FILE* f = fopen(c->tune_cache_path.c_str(), "r")) {
        char line[512], ver[8], dev[320];
        unsigned long long key = 0;
        int best = 0;
        float ms = 0;
        while (fgets(line, sizeof line, f))
            if (sscanf(line, "%7s %319s %llx %d %f", ver, dev, &key, &best, &ms) == 5 && !strcmp(ver, "v1") && id == dev)
                c->tune_cache[(uint64_t)key] = best;
        fclose(f);
    }
    return OUSTER_HIP_OK;
}
static void tune_cache_append(ouster_hip_ctx* c, uint64_t key, int best, float ms) {
    if (c->tune_cache_path.empty()) return;
    c->tune_cache[key] = best;
    char line[512];
    const int n = snprintf(line, sizeof line, "v1 %s %016llx %d %.4f\n", c->tune_cache_id.c_str(), (unsigned long long)key, best, ms);
    if (n <= 0 || n >= (int)sizeof line) return;
    const int fd = open(c->tune_cache_path.c_str(), O_WRONLY | O_APPEND | O_CREAT, 0644);
    if (fd < 0) return;   // a cache that cannot be written is not an error of the decode
    (void)!write(fd, line, (size_t)n);
    close(fd);
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

// ---- lut -------------------------------------------------------------------------------
static int upload(void** dptr, const void* src, size_t bytes, hipStream_t st) {
    if (counted_malloc(dptr, bytes) != hipSuccess) return -1;
    if (hipMemcpyAsync(*dptr, src, bytes, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    return hipStreamSynchronize(st) == hipSuccess ? 0 : -1;
}

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
    if (dtype != OUSTER_HIP_F32 && dtype != OUSTER_HIP_F64)
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "LUT dtype must be F32 or F64");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t hw = (size_t)w * h, es = dtype == OUSTER_HIP_F32 ? 4 : 8;
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

static int ensure_luts(ouster_hip_ctx* c, const std::vector<LutDev>& l) {
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

static bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

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
        if (!ctx->ring_ev[slot]) HIP_TRY(hipEventCreateWithFlags(&ctx->ring_ev[slot], hipEventDisableTiming));
        else HIP_TRY(hipEventSynchronize(ctx->ring_ev[slot]));  // RING calls ago: long done
        if (ctx->ring_cap[slot] < bytes) {
            if (ctx->ring_buf[slot]) (void)hipHostFree(ctx->ring_buf[slot]);
            ctx->ring_buf[slot] = nullptr;
            ctx->ring_cap[slot] = 0;
            HIP_TRY(hipHostMalloc((void**)&ctx->ring_buf[slot], bytes + bytes / 2, hipHostMallocDefault));
            ctx->ring_cap[slot] = bytes + bytes / 2;
        }
        memcpy(ctx->ring_buf[slot], packet_counts, bytes);
        src = ctx->ring_buf[slot];
    }
    HIP_TRY(hipMemcpyAsync(ctx->counts.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (slot >= 0) HIP_TRY(hipEventRecord(ctx->ring_ev[slot], ctx->stream));
    *d_counts = (const uint32_t*)ctx->counts.p;
    return OUSTER_HIP_OK;
}

static bool fast_possible(const Knobs& kn, uint32_t slots_per_frame, const Geometry& g) {
    return kn.fast && (uint64_t)slots_per_frame * g.columns_per_packet == g.columns_per_frame;
}

// ---- the variant tuner ----------------------------------------------------------------------------
// Four launches of each candidate, back to back (a launch that follows a different variant is not representative of the
// steady state: alternating the candidates made the 64-column kernel look 8 % faster than it then ran).  Single launches
// vary by ~10 %, mostly upwards, and the candidates can be within 1-5 % of each other: each candidate's fastest sample
// counts, its first one (cold code, cold TLB, another variant's write-backs still draining) only when nothing else landed.
// The clocks are polled, never waited for: until all samples have landed the default variant runs.
// every sample of `t` is queued: once all have landed, the fastest candidate becomes the verdict (and goes to the cache file)
static void tune_collect(ouster_hip_ctx* c, uint64_t key, Tune& t, const int* cand, int nc) {
    constexpr int R = Tune::ROUNDS;
    const int NS = nc * R;
    for (int i = 0; i < NS; ++i)
        if (hipEventQuery(t.ev[i][1]) != hipSuccess) {
            (void)hipGetLastError();
            return;
        }
    float cold[Tune::NCAND] = {0, 0, 0, 0, 0};
    for (int i = 0; i < NS; ++i) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, t.ev[i][0], t.ev[i][1]) != hipSuccess || ms <= 0) continue;
        float& slot = (i % R == 0) ? cold[i / R] : t.ms[i / R];
        if (slot == 0 || ms < slot) slot = ms;
    }
    for (int k = 0; k < nc; ++k)
        if (t.ms[k] == 0) t.ms[k] = cold[k];
    t.best = 256;
    float best_ms = 0;
    for (int k = 0; k < nc; ++k)
        if (t.ms[k] > 0 && (best_ms == 0 || t.ms[k] < best_ms)) { t.best = cand[k]; best_ms = t.ms[k]; }
    tune_cache_append(c, key, t.best, best_ms);
}

// What this call launches: a verdict (measured, or an earlier process's from the cache file), the next sample of a
// candidate (then `record` / `slot` say where its two events go), or the default variant while samples are in flight.
struct TuneStep {
    int variant;
    Tune* record;
    int slot;
};
static TuneStep tune_step(ouster_hip_ctx* c, uint64_t key, const int* cand, int nc) {
    if (c->tune.size() > 64 && !c->tune.count(key)) tune_forget(c);   // bounded: forget everything, re-learn
    const bool fresh = !c->tune.count(key);
    Tune& t = c->tune[key];
    if (fresh) {   // an earlier process (or rank) has timed this workload on this device: launch its choice from call 1
        auto hit = c->tune_cache.find(key);
        if (hit != c->tune_cache.end() && std::find(cand, cand + nc, hit->second) != cand + nc) {
            t.best = hit->second;
            t.from_cache = true;
        }
    }
    const int NS = nc * Tune::ROUNDS;
    if (t.best == -2 && t.calls >= NS) tune_collect(c, key, t, cand, nc);
    if (t.best != -2) {
        c->last_tuner = t.from_cache ? "cache" : "measured";
        return {t.best, nullptr, -1};
    }
    c->last_tuner = "measuring";
    if (t.calls >= NS) return {256, nullptr, -1};   // every sample is queued, not all have landed
    const int slot = t.calls++;
    return {cand[slot / Tune::ROUNDS], &t, slot};
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
    PlanInput in{};
    in.g = g;
    in.kn = ctx->knobs;
    in.n_frames = n_frames;
    in.slots_per_frame = slots_per_frame;
    in.packet_stride = packet_stride;
    in.packets = (uintptr_t)packets;
    in.xyz_poses = (uintptr_t)da.xyz_poses;
    in.spec = spec;
    in.xyzm = xyzm;
    in.vec_ok = da.vec_ok;
    in.n_fields = nf;
    for (uint32_t i = 0; i < nf; ++i) {
        in.plane_mask |= da.planes[i] ? (1ull << i) : 0;
        in.destagger_mask |= da.destaggered[i] ? (1ull << i) : 0;
    }
    in.xyz_mask = (da.xyz[0] ? 1u : 0u) | (da.xyz[1] ? 2u : 0u);
    in.gate_counts = out->gate_counts != nullptr;
    in.cus = ctx->cus;
    in.resident_wgs = ctx->resident_wgs;
#ifdef OUSTER_EXPERIMENTS
    in.may_resolve = true;
#else
    in.may_resolve = false;   // k_decode_wide_resolved is not compiled
#endif
    const bool fast = fast_possible(in.kn, slots_per_frame, g);
    const Candidates cand = plan_candidates(in);
    // the tuner stands down with tune = 0 and while the stream is being captured: the default variant runs
    TuneStep ts{256, nullptr, -1};
    ctx->last_tuner = "none";   // forced by a knob, or a shape with nothing to choose
    if (cand.n && in.kn.tune) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(st, &cap);
        if (cap == hipStreamCaptureStatusNone) ts = tune_step(ctx, tuner_key(in, cand), cand.variant, cand.n);
    }
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
        if (ctx->ev_used == ctx->ev_pool.size()) {
            hipEvent_t a, b;
            HIP_TRY(hipEventCreate(&a));
            HIP_TRY(hipEventCreate(&b));
            ctx->ev_pool.emplace_back(a, b);
        }
        e0 = ctx->ev_pool[ctx->ev_used].first;
        e1 = ctx->ev_pool[ctx->ev_used].second;
        ctx->ev_used++;
        HIP_TRY(hipEventRecord(e0, st));
    }
    if (ts.record) {
        for (int k = 0; k < 2; ++k)
            if (!ts.record->ev[ts.slot][k]) HIP_TRY(hipEventCreate(&ts.record->ev[ts.slot][k]));
        HIP_TRY(hipEventRecord(ts.record->ev[ts.slot][0], st));
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
    if (ts.record) HIP_TRY(hipEventRecord(ts.record->ev[ts.slot][1], st));
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

// ---- standalone destagger -----------------------------------------------------------------
int ouster_hip_destagger(ouster_hip_ctx* ctx, const void* src, void* dst, uint32_t h, uint32_t w,
                         uint32_t elem_bytes, const int32_t* shifts, uint32_t n_shifts,
                         int inverse, uint32_t n_images) {
    if (!ctx || !shifts) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_shifts != h)
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "image height does not match shifts size");
    if (n_images == 0 || h == 0 || w == 0) return OUSTER_HIP_OK;
    if (!src || !dst || src == dst) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "bad image pointers");
    if (elem_bytes == 0) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "elem_bytes is 0");
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<int32_t> off;
    dest_offsets(shifts, h, w, inverse, off);
    if (ensure_offsets(ctx, off)) return fail(OUSTER_HIP_ERR_RUNTIME, "offset upload failed");
    ctx->shifts_host.clear();  // ouster_hip_decode's cache key no longer describes `offsets`
    DestaggerArgs a{};
    a.src = src;
    a.dst = dst;
    a.h = h;
    a.w = w;
    a.elem = elem_bytes;
    a.offsets = (const int32_t*)ctx->offsets.p;
    HIP_TRY(launch_destagger(a, n_images, ctx->stream));
    return OUSTER_HIP_OK;
}

// ---- standalone cartesian -------------------------------------------------------------------
int ouster_hip_cartesian(ouster_hip_ctx* ctx, const ouster_hip_lut* lut, const uint32_t* range,
                         void* xyz, int xyz_dtype, uint32_t n_images) {
    if (!ctx || !lut) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (xyz_dtype != OUSTER_HIP_F32 && xyz_dtype != OUSTER_HIP_F64)
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

// ---- dense dewarp -----------------------------------------------------------------------------
int ouster_hip_dewarp(ouster_hip_ctx* ctx, const void* points, const double* poses, void* dewarped,
                      int dtype, uint32_t h, uint32_t w, uint32_t n_images) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (dtype != OUSTER_HIP_F32 && dtype != OUSTER_HIP_F64)
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

namespace {
// One host array of a *_host call: pool memory is handed to the kernel as it is, anything else gets a slot of the context's
// grow-only scratch (inputs copied in now, outputs copied out by finish()).
struct HostArg {
    void* dev = nullptr;
    void* host = nullptr;
    size_t bytes = 0;
    bool staged = false;
};
int host_arg(ouster_hip_ctx* ctx, const void* host, size_t bytes, uint32_t slot, bool is_input, HostArg& a) {
    a.host = const_cast<void*>(host);
    a.bytes = bytes;
    if (ouster_hip_host_is_pinned(host, bytes)) {
        a.dev = a.host;
        return OUSTER_HIP_OK;
    }
    a.staged = true;
    if (ctx->user_scratch[slot].ensure(bytes)) return fail(OUSTER_HIP_ERR_RUNTIME, "out of device memory (scratch %u, %zu bytes)", slot, bytes);
    a.dev = ctx->user_scratch[slot].p;
    if (is_input) HIP_TRY(hipMemcpyAsync(a.dev, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    return OUSTER_HIP_OK;
}
int host_finish(ouster_hip_ctx* ctx, const HostArg& out) {
    if (out.staged) HIP_TRY(hipMemcpyAsync(out.host, out.dev, out.bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return OUSTER_HIP_OK;
}
}  // namespace

int ouster_hip_destagger_host(ouster_hip_ctx* ctx, const void* src, void* dst, uint32_t h, uint32_t w,
                              uint32_t elem_bytes, const int32_t* shifts, uint32_t n_shifts, int inverse) {
    if (!ctx || !shifts) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_shifts != h) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "image height does not match shifts size");
    if (h == 0 || w == 0) return OUSTER_HIP_OK;
    if (!src || !dst || elem_bytes == 0) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "bad image arguments");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)h * w * elem_bytes;
    HostArg in, out;
    int rc = host_arg(ctx, src, bytes, 0, true, in);
    if (rc == OUSTER_HIP_OK) rc = host_arg(ctx, dst, bytes, 1, false, out);
    if (rc != OUSTER_HIP_OK) return rc;
    // in place (src == dst) in the reference copies rows through each other: not a supported call there either; go through scratch
    if (in.dev == out.dev) {
        if (ctx->user_scratch[1].ensure(bytes)) return fail(OUSTER_HIP_ERR_RUNTIME, "out of device memory (scratch)");
        out.dev = ctx->user_scratch[1].p;
        out.staged = true;
    }
    rc = ouster_hip_destagger(ctx, in.dev, out.dev, h, w, elem_bytes, shifts, n_shifts, inverse, 1);
    if (rc != OUSTER_HIP_OK) return rc;
    return host_finish(ctx, out);
}

int ouster_hip_cartesian_host(ouster_hip_ctx* ctx, const ouster_hip_lut* lut, const uint32_t* range, void* xyz,
                              int xyz_dtype) {
    if (!ctx || !lut) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (xyz_dtype != OUSTER_HIP_F32 && xyz_dtype != OUSTER_HIP_F64)
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "xyz_dtype must be F32 or F64");
    const size_t npx = (size_t)lut->w * lut->h;
    if (npx == 0) return OUSTER_HIP_OK;
    if (!range || !xyz) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL image pointer");
    HIP_TRY(hipSetDevice(ctx->device));
    HostArg in, out;
    int rc = host_arg(ctx, range, npx * 4, 0, true, in);
    if (rc == OUSTER_HIP_OK) rc = host_arg(ctx, xyz, npx * 3 * (xyz_dtype == OUSTER_HIP_F64 ? 8 : 4), 1, false, out);
    if (rc != OUSTER_HIP_OK) return rc;
    rc = ouster_hip_cartesian(ctx, lut, (const uint32_t*)in.dev, out.dev, xyz_dtype, 1);
    if (rc != OUSTER_HIP_OK) return rc;
    return host_finish(ctx, out);
}

int ouster_hip_dewarp_host(ouster_hip_ctx* ctx, const void* points, const double* poses, void* dewarped, int dtype,
                           uint32_t h, uint32_t w) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (dtype != OUSTER_HIP_F32 && dtype != OUSTER_HIP_F64) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dtype must be F32 or F64");
    if (h == 0 || w == 0) return OUSTER_HIP_OK;
    if (!points || !poses || !dewarped) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t pbytes = (size_t)h * w * 3 * (dtype == OUSTER_HIP_F64 ? 8 : 4);
    HostArg in, po, out;
    int rc = host_arg(ctx, points, pbytes, 0, true, in);
    if (rc == OUSTER_HIP_OK) rc = host_arg(ctx, poses, (size_t)w * 128, 2, true, po);
    if (rc == OUSTER_HIP_OK) rc = host_arg(ctx, dewarped, pbytes, 1, false, out);
    if (rc != OUSTER_HIP_OK) return rc;
    rc = ouster_hip_dewarp(ctx, in.dev, (const double*)po.dev, out.dev, dtype, h, w, 1);
    if (rc != OUSTER_HIP_OK) return rc;
    return host_finish(ctx, out);
}

// ---- display images (k_image.hip) ----------------------------------------------------------------
namespace {
size_t image_elem(int t) {
    switch (t) {
        case OUSTER_HIP_U8: return 1;
        case OUSTER_HIP_U16: return 2;
        case OUSTER_HIP_U32: case OUSTER_HIP_F32: return 4;
        case OUSTER_HIP_F64: return 8;
        default: return 0;
    }
}
// shared argument checks; fills what every image kernel needs.  Returns 1 when there is nothing to do.
int image_args(ouster_hip_ctx* ctx, const void* planes, int in_type, int out_type, uint32_t n_images, uint32_t h, uint32_t w,
               size_t image_stride, ImageArgs& a) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (out_type != OUSTER_HIP_F32 && out_type != OUSTER_HIP_F64)
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "out_type must be F32 or F64");
    if (in_type != OUSTER_HIP_U8 && in_type != OUSTER_HIP_U16 && in_type != OUSTER_HIP_U32 && in_type != out_type)
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "in_type must be U8, U16, U32 or out_type");
    if (n_images == 0 || h == 0 || w == 0) return 1;
    if (n_images > 65535u) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "at most 65535 images per call");
    if ((uint64_t)h * w > (1ull << 31)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "image larger than 2^31 elements");
    if (!planes) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL image pointer");
    if (image_stride && image_stride < (size_t)h * w) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "image_stride smaller than an image");
    a = ImageArgs{};
    a.in = planes;
    a.in_stride = image_stride ? image_stride : (size_t)h * w;
    a.n_images = n_images;
    a.h = h;
    a.w = w;
    const size_t vb = std::min<size_t>(16, 4 * image_elem(in_type));
    a.vec = ((uintptr_t)planes % vb == 0) && (a.in_stride % 4 == 0 || n_images == 1);
    return OUSTER_HIP_OK;
}
}  // namespace

int ouster_hip_image_dark_rows(ouster_hip_ctx* ctx, const void* planes, int in_type, int out_type, uint32_t n_images,
                               uint32_t h, uint32_t w, size_t image_stride, void* medians, uint32_t* n_cols) {
    ImageArgs a;
    const int rc = image_args(ctx, planes, in_type, out_type, n_images, h, w, image_stride, a);
    if (rc) return rc > 0 ? OUSTER_HIP_OK : rc;
    if (w > IMAGE_MAX_W_DARK) return fail(OUSTER_HIP_ERR_UNSUPPORTED, "dark rows: images wider than %u columns", IMAGE_MAX_W_DARK);
    HIP_TRY(hipSetDevice(ctx->device));
    if (h < 2) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dark rows need at least two rows");
    if (!medians) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "medians is NULL");
    const size_t words = (w + 63) / 64;
    if (ctx->image_mask.ensure((size_t)n_images * words * 8)) return fail(OUSTER_HIP_ERR_RUNTIME, "out of device memory (column masks)");
    a.col_mask = (uint64_t*)ctx->image_mask.p;
    a.medians = medians;
    a.n_cols = n_cols;
    a.vec = a.vec && (w % 4 == 0);
    HIP_TRY(launch_image_dark_rows(a, in_type, out_type, ctx->stream));
    return OUSTER_HIP_OK;
}

int ouster_hip_image_percentiles(ouster_hip_ctx* ctx, const void* planes, int in_type, int out_type, uint32_t n_images,
                                 uint32_t h, uint32_t w, size_t image_stride, const void* dark, double lo_percentile,
                                 double hi_percentile, uint32_t* n, void* lo_hi) {
    ImageArgs a;
    const int rc = image_args(ctx, planes, in_type, out_type, n_images, h, w, image_stride, a);
    if (rc) return rc > 0 ? OUSTER_HIP_OK : rc;
    if (!n || !lo_hi) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL output pointer");
    if (!(lo_percentile >= 0) || !(hi_percentile >= 0) || !(lo_percentile + hi_percentile < 1))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "percentiles must be >= 0 and sum to less than 1");
    HIP_TRY(hipSetDevice(ctx->device));
    a.dark = dark;
    a.lo_percentile = lo_percentile;
    a.hi_percentile = hi_percentile;
    a.n_positive = n;
    a.lo_hi = lo_hi;
    HIP_TRY(launch_image_percentiles(a, in_type, out_type, ctx->stream));
    return OUSTER_HIP_OK;
}

int ouster_hip_image_apply(ouster_hip_ctx* ctx, const void* planes, int in_type, void* out, int out_type, uint32_t n_images,
                           uint32_t h, uint32_t w, size_t in_stride, size_t out_stride, const void* dark,
                           const ouster_hip_image_map* maps) {
    ImageArgs a;
    const int rc = image_args(ctx, planes, in_type, out_type, n_images, h, w, in_stride, a);
    if (rc) return rc > 0 ? OUSTER_HIP_OK : rc;
    if (!out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "out is NULL");
    if (out_stride && out_stride < (size_t)h * w) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "out_stride smaller than an image");
    if (out == planes && (in_type != out_type || (out_stride ? out_stride : (size_t)h * w) != a.in_stride))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "in place needs equal types and strides");
    HIP_TRY(hipSetDevice(ctx->device));
    a.out = out;
    a.out_stride = out_stride ? out_stride : (size_t)h * w;
    a.vec = a.vec && ((uintptr_t)out % 16 == 0) && (a.out_stride % 4 == 0 || n_images == 1);
    a.dark = dark;
    a.maps = maps;
    HIP_TRY(launch_image_apply(a, in_type, out_type, ctx->stream));
    return OUSTER_HIP_OK;
}

// One host image: scratch slot 0 holds a foreign image, slot 2 the few numbers that go out, slot 3 those that come in.
int ouster_hip_image_dark_rows_host(ouster_hip_ctx* ctx, const void* image, int dtype, uint32_t h, uint32_t w, void* medians,
                                    uint32_t* n_cols) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    const size_t es = (dtype == OUSTER_HIP_F32 || dtype == OUSTER_HIP_F64) ? image_elem(dtype) : 0;
    if (!es) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dtype must be F32 or F64");
    if (h < 2 || w == 0) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dark rows need at least two rows");
    if (!image || !medians || !n_cols) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    HIP_TRY(hipSetDevice(ctx->device));
    HostArg in;
    int rc = host_arg(ctx, image, (size_t)h * w * es, 0, true, in);
    if (rc != OUSTER_HIP_OK) return rc;
    const size_t mbytes = (size_t)(h - 1) * es;
    if (ctx->user_scratch[2].ensure(mbytes + 8)) return fail(OUSTER_HIP_ERR_RUNTIME, "out of device memory (scratch)");
    uint8_t* d = (uint8_t*)ctx->user_scratch[2].p;
    rc = ouster_hip_image_dark_rows(ctx, in.dev, dtype, dtype, 1, h, w, 0, d + 8, (uint32_t*)d);
    if (rc != OUSTER_HIP_OK) return rc;
    HIP_TRY(hipMemcpyAsync(medians, d + 8, mbytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(n_cols, d, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return OUSTER_HIP_OK;
}

int ouster_hip_image_percentiles_host(ouster_hip_ctx* ctx, const void* image, int dtype, uint32_t h, uint32_t w,
                                      const void* dark, double lo_percentile, double hi_percentile, uint32_t* n,
                                      void* lo_hi) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    const size_t es = (dtype == OUSTER_HIP_F32 || dtype == OUSTER_HIP_F64) ? image_elem(dtype) : 0;
    if (!es) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dtype must be F32 or F64");
    if (!image || !n || !lo_hi || h == 0 || w == 0) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "bad image arguments");
    HIP_TRY(hipSetDevice(ctx->device));
    HostArg in;
    int rc = host_arg(ctx, image, (size_t)h * w * es, 0, true, in);
    if (rc != OUSTER_HIP_OK) return rc;
    if (ctx->user_scratch[2].ensure(8 + 2 * es)) return fail(OUSTER_HIP_ERR_RUNTIME, "out of device memory (scratch)");
    uint8_t* d = (uint8_t*)ctx->user_scratch[2].p;
    void* d_dark = nullptr;
    if (dark) {
        if (ctx->user_scratch[3].ensure((size_t)h * es)) return fail(OUSTER_HIP_ERR_RUNTIME, "out of device memory (scratch)");
        d_dark = ctx->user_scratch[3].p;
        HIP_TRY(hipMemcpyAsync(d_dark, dark, (size_t)h * es, hipMemcpyHostToDevice, ctx->stream));
    }
    rc = ouster_hip_image_percentiles(ctx, in.dev, dtype, dtype, 1, h, w, 0, d_dark, lo_percentile, hi_percentile, (uint32_t*)d, d + 8);
    if (rc != OUSTER_HIP_OK) return rc;
    HIP_TRY(hipMemcpyAsync(n, d, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(lo_hi, d + 8, 2 * es, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return OUSTER_HIP_OK;
}

int ouster_hip_image_apply_host(ouster_hip_ctx* ctx, void* image, int dtype, uint32_t h, uint32_t w, const void* dark,
                                const ouster_hip_image_map* map) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    const size_t es = (dtype == OUSTER_HIP_F32 || dtype == OUSTER_HIP_F64) ? image_elem(dtype) : 0;
    if (!es) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dtype must be F32 or F64");
    if (h == 0 || w == 0) return OUSTER_HIP_OK;
    if (!image) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL image pointer");
    HIP_TRY(hipSetDevice(ctx->device));
    HostArg io;
    int rc = host_arg(ctx, image, (size_t)h * w * es, 0, true, io);
    if (rc != OUSTER_HIP_OK) return rc;
    const size_t dbytes = dark ? (size_t)h * es : 0, doff = sizeof(ouster_hip_image_map);
    if (ctx->user_scratch[3].ensure(doff + dbytes)) return fail(OUSTER_HIP_ERR_RUNTIME, "out of device memory (scratch)");
    uint8_t* d = (uint8_t*)ctx->user_scratch[3].p;
    ouster_hip_image_map m{};
    if (map) m = *map;
    else m.use_dark = 1;
    HIP_TRY(hipMemcpyAsync(d, &m, sizeof m, hipMemcpyHostToDevice, ctx->stream));   // pageable source: staged before the call returns
    if (dark) HIP_TRY(hipMemcpyAsync(d + doff, dark, dbytes, hipMemcpyHostToDevice, ctx->stream));
    rc = ouster_hip_image_apply(ctx, io.dev, dtype, io.dev, dtype, 1, h, w, 0, 0, dark ? d + doff : nullptr,
                                (const ouster_hip_image_map*)d);
    if (rc != OUSTER_HIP_OK) return rc;
    return host_finish(ctx, io);
}

// ---- frame_ops (k_frame_ops.hip) ------------------------------------------------------------------
namespace {
// A small host table (reduced shifts, row indices) -> ctx->fops_tables, safe by construction for back-to-back asynchronous
// calls: the source is copied into page-locked staging owned by the context, the staging is reused only after the event behind
// its last copy has completed, and the device buffer grows only on an idle stream.
int fops_upload(ouster_hip_ctx* ctx, const void* src, size_t bytes) {
    if (ctx->fops_ev) HIP_TRY(hipEventSynchronize(ctx->fops_ev));
    else HIP_TRY(hipEventCreateWithFlags(&ctx->fops_ev, hipEventDisableTiming));
    if (bytes > ctx->fops_pin_cap) {
        if (ctx->fops_pin) (void)hipHostFree(ctx->fops_pin);
        ctx->fops_pin = nullptr;
        ctx->fops_pin_cap = 0;
        HIP_TRY(hipHostMalloc(&ctx->fops_pin, bytes * 2, hipHostMallocDefault));
        ctx->fops_pin_cap = bytes * 2;
    }
    if (bytes > ctx->fops_tables.cap) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));   // a kernel in flight may still read the old table
        if (ctx->fops_tables.ensure(bytes)) return fail(OUSTER_HIP_ERR_RUNTIME, "out of device memory (frame_ops tables)");
    }
    std::memcpy(ctx->fops_pin, src, bytes);
    HIP_TRY(hipMemcpyAsync(ctx->fops_tables.p, ctx->fops_pin, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->fops_ev, ctx->stream));
    return OUSTER_HIP_OK;
}

size_t fops_elem(int t) {
    switch (t) {
        case OUSTER_HIP_U8: case OUSTER_HIP_I8: return 1;
        case OUSTER_HIP_U16: case OUSTER_HIP_I16: return 2;
        case OUSTER_HIP_U32: case OUSTER_HIP_I32: case OUSTER_HIP_F32: return 4;
        case OUSTER_HIP_U64: case OUSTER_HIP_I64: case OUSTER_HIP_F64: return 8;
        default: return 0;
    }
}
const char* fops_type_name(int t) {
    static const char* names[] = {"VOID", "UINT8", "UINT16", "UINT32", "UINT64", "INT8", "INT16", "INT32", "INT64", "FLOAT32", "FLOAT64"};
    return (t >= 0 && t <= 10) ? names[t] : "?";
}
// shared checks of the three entry points; returns 1 when there is nothing to do
int fops_shape(ouster_hip_ctx* ctx, uint32_t n_planes, uint32_t n_images, uint32_t h, uint32_t w) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (n_images > 65535u) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "at most 65535 images per call");
    if ((uint64_t)h * w > (1ull << 31)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "image larger than 2^31 elements");
    return (n_planes == 0 || n_images == 0 || h == 0 || w == 0) ? 1 : OUSTER_HIP_OK;
}
// the planes of one call -> the launch records; every `invalid` is checked before the first launch
int fops_planes(const ouster_hip_fops_plane* planes, uint32_t n_planes, uint32_t h, uint32_t w, std::vector<FopsPlane>& out,
                bool clouds_allowed = false) {
    if (!planes) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "planes is NULL");
    out.resize(n_planes);
    for (uint32_t i = 0; i < n_planes; ++i) {
        const ouster_hip_fops_plane& p = planes[i];
        FopsPlane& o = out[i];
        if (p.type == OUSTER_HIP_FOPS_XYZ_F32 || p.type == OUSTER_HIP_FOPS_XYZ_F64) {
            const uint32_t scalar = p.type == OUSTER_HIP_FOPS_XYZ_F64 ? 8 : 4;
            if (!clouds_allowed) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: a cloud can only be invalidated", i);
            if (p.invalid != 0 || p.twin) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: a cloud takes invalid == 0 and no twin", i);
            if (!p.data || (uintptr_t)p.data % scalar) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: NULL or misaligned pointer", i);
            if (p.image_stride && p.image_stride < (size_t)h * w) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: image_stride smaller than an image", i);
            o = FopsPlane{};
            o.data = p.data;
            o.stride = p.image_stride ? p.image_stride : (size_t)h * w;
            o.elem = 3 * scalar;
            o.type = p.type;
            continue;
        }
        o.elem = (uint32_t)fops_elem(p.type);
        if (!o.elem) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: unsupported element type %d", i, p.type);
        const int rc = ouster_hip_frame_ops_invalid_bits(p.type, p.invalid, &o.invalid_bits);
        if (rc != OUSTER_HIP_OK) return rc;
        if (!p.data || (uintptr_t)p.data % o.elem || (uintptr_t)p.twin % o.elem)
            return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: NULL or misaligned pointer", i);
        if (p.image_stride && p.image_stride < (size_t)h * w)
            return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: image_stride smaller than an image", i);
        o.data = p.data;
        o.twin = p.twin;
        o.stride = p.image_stride ? p.image_stride : (size_t)h * w;
        o.type = p.type;
    }
    return OUSTER_HIP_OK;
}
}  // namespace

int ouster_hip_frame_ops_invalid_bits(int type, double invalid, uint64_t* bits) {
    if (!bits) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "bits is NULL");
    *bits = 0;
    bool ok = true;
    const double t = std::trunc(invalid);
    auto put = [&](auto v) { std::memcpy(bits, &v, sizeof v); };
    switch (type) {
        case OUSTER_HIP_U8: ok = t >= 0 && t <= 255.0; if (ok) put((uint8_t)t); break;
        case OUSTER_HIP_U16: ok = t >= 0 && t <= 65535.0; if (ok) put((uint16_t)t); break;
        case OUSTER_HIP_U32: ok = t >= 0 && t <= 4294967295.0; if (ok) put((uint32_t)t); break;
        case OUSTER_HIP_U64: ok = t >= 0 && t < 18446744073709551616.0; if (ok) put((uint64_t)t); break;
        case OUSTER_HIP_I8: ok = t >= -128.0 && t <= 127.0; if (ok) put((int8_t)t); break;
        case OUSTER_HIP_I16: ok = t >= -32768.0 && t <= 32767.0; if (ok) put((int16_t)t); break;
        case OUSTER_HIP_I32: ok = t >= -2147483648.0 && t <= 2147483647.0; if (ok) put((int32_t)t); break;
        case OUSTER_HIP_I64: ok = t >= -9223372036854775808.0 && t < 9223372036854775808.0; if (ok) put((int64_t)t); break;
        case OUSTER_HIP_F32: ok = !std::isfinite(invalid) || std::fabs(invalid) <= 3.4028234663852886e38; if (ok) put((float)invalid); break;
        case OUSTER_HIP_F64: put(invalid); break;
        default: return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "unsupported element type %d", type);
    }
    if (!ok) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "invalid == %g does not fit a field of type %s", invalid, fops_type_name(type));
    return OUSTER_HIP_OK;
}

int ouster_hip_frame_ops_clip(ouster_hip_ctx* ctx, const ouster_hip_fops_plane* planes, uint32_t n_planes,
                              uint32_t n_images, uint32_t h, uint32_t w, double lower, double upper) {
    std::vector<FopsPlane> pl;
    int rc = fops_planes(planes, n_planes, h, w, pl);   // also when there is nothing to do: a bad `invalid` is an error
    if (rc != OUSTER_HIP_OK && n_planes) return rc;
    rc = fops_shape(ctx, n_planes, n_images, h, w);
    if (rc) return rc > 0 ? OUSTER_HIP_OK : rc;
    HIP_TRY(hipSetDevice(ctx->device));
    for (uint32_t p0 = 0; p0 < n_planes; p0 += FOPS_MAX_PLANES) {
        FopsClipArgs a{};
        a.n_planes = std::min<uint32_t>(FOPS_MAX_PLANES, n_planes - p0);
        std::copy(pl.begin() + p0, pl.begin() + p0 + a.n_planes, a.planes);
        a.n_images = n_images;
        a.hw = h * w;
        a.lower = lower;
        a.upper = upper;
        HIP_TRY(launch_fops_clip(a, ctx->stream));
    }
    return OUSTER_HIP_OK;
}

int ouster_hip_frame_ops_invalidate(ouster_hip_ctx* ctx, const ouster_hip_fops_pred* pred,
                                    const ouster_hip_fops_plane* planes, uint32_t n_planes, uint32_t n_images,
                                    uint32_t h, uint32_t w) {
    if (!pred) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "pred is NULL");
    std::vector<FopsPlane> pl;
    int rc = fops_planes(planes, n_planes, h, w, pl, true);
    if (rc != OUSTER_HIP_OK && n_planes) return rc;
    rc = fops_shape(ctx, n_planes, n_images, h, w);
    if (rc < 0) return rc;
    const bool nothing = rc > 0;
    FopsInvalidateArgs a{};
    a.kind = pred->kind;
    a.src_type = pred->src_type;
    a.src = pred->src;
    a.src_stride = pred->src_stride ? pred->src_stride : (size_t)h * w;
    a.n_masks = pred->n_masks;
    a.axis = pred->axis;
    a.lower = pred->lower;
    a.upper = pred->upper;
    a.lo = pred->lo;
    a.hi = pred->hi;
    bool need_shifts = false;
    for (const FopsPlane& p : pl) need_shifts = need_shifts || p.twin != nullptr;
    switch (pred->kind) {
        case OUSTER_HIP_FOPS_PRED_KEY:
            if (!fops_elem(pred->src_type)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "unsupported key element type %d", pred->src_type);
            if (!nothing && (!pred->src || (uintptr_t)pred->src % fops_elem(pred->src_type))) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL or misaligned key plane");
            break;
        case OUSTER_HIP_FOPS_PRED_ROWS:
        case OUSTER_HIP_FOPS_PRED_COLS: {
            const uint32_t size = pred->kind == OUSTER_HIP_FOPS_PRED_ROWS ? h : w;
            if (pred->lo > pred->hi || pred->hi > size)
                return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "index range [%u, %u) must lie in [0, %u]", pred->lo, pred->hi, size);
            need_shifts = need_shifts || pred->kind == OUSTER_HIP_FOPS_PRED_COLS;
            break;
        }
        case OUSTER_HIP_FOPS_PRED_MASK:
            if (pred->n_masks == 0 || (!nothing && !pred->src)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "mask predicate without masks");
            break;
        case OUSTER_HIP_FOPS_PRED_XYZ:
            if (pred->src_type != OUSTER_HIP_F32 && pred->src_type != OUSTER_HIP_F64) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "xyz type must be F32 or F64");
            if (pred->axis > 2) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "axis == %u must be in the range [0, 2]", pred->axis);
            if (!nothing && (!pred->src || (uintptr_t)pred->src % fops_elem(pred->src_type))) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL or misaligned point cloud");
            break;
        default:
            return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "unknown predicate kind %d", pred->kind);
    }
    if (need_shifts && (!pred->shifts || pred->n_shift_tables == 0))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "this call needs pixel_shift_by_row tables");
    if (nothing) return OUSTER_HIP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    a.n_images = n_images;
    a.h = h;
    a.w = w;
    if (need_shifts) {
        // (W + x % W) % W on the host, once per row: the kernel wraps a column with one conditional subtraction
        const size_t n = (size_t)pred->n_shift_tables * h;
        std::vector<uint32_t> red(n);
        for (size_t i = 0; i < n; ++i) red[i] = (uint32_t)((((int64_t)pred->shifts[i] % (int64_t)w) + w) % w);
        const int urc = fops_upload(ctx, red.data(), n * 4);
        if (urc != OUSTER_HIP_OK) return urc;
        a.shifts = (const uint32_t*)ctx->fops_tables.p;
        a.n_tables = pred->n_shift_tables;
    }
    // a key that is also a target must be read before it is written, for EVERY target of the pixel: where the list needs
    // more than one launch the key plane goes into the last one
    if (pred->kind == OUSTER_HIP_FOPS_PRED_KEY && n_planes > FOPS_MAX_PLANES)
        std::stable_partition(pl.begin(), pl.end(), [&](const FopsPlane& p) { return p.data != pred->src; });
    for (uint32_t p0 = 0; p0 < n_planes; p0 += FOPS_MAX_PLANES) {
        a.n_planes = std::min<uint32_t>(FOPS_MAX_PLANES, n_planes - p0);
        std::copy(pl.begin() + p0, pl.begin() + p0 + a.n_planes, a.planes);
        HIP_TRY(launch_fops_invalidate(a, ctx->stream));
    }
    return OUSTER_HIP_OK;
}

int ouster_hip_frame_ops_select_rows(ouster_hip_ctx* ctx, const void* const* src, void* const* dst,
                                     const uint32_t* elem_bytes, uint32_t n_planes, uint32_t n_images, uint32_t h,
                                     uint32_t w, const uint32_t* indices, uint32_t n_sel) {
    int rc = fops_shape(ctx, n_planes, n_images, h, w);
    if (rc < 0) return rc;
    if (n_sel > 65535u) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "at most 65535 rows per call");
    if (n_sel && !indices) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "indices is NULL");
    for (uint32_t i = 0; i < n_sel; ++i)
        if (indices[i] >= h) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "row index %u must be in the range [0, %u)", indices[i], h);
    if (rc > 0 || n_sel == 0) return OUSTER_HIP_OK;
    if (!src || !dst || !elem_bytes) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    for (uint32_t p = 0; p < n_planes; ++p) {
        const uint32_t e = elem_bytes[p];
        if (e != 1 && e != 2 && e != 4 && e != 8) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: elem_bytes must be 1, 2, 4 or 8", p);
        if (!src[p] || !dst[p] || (uintptr_t)src[p] % e || (uintptr_t)dst[p] % e) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: NULL or misaligned pointer", p);
    }
    HIP_TRY(hipSetDevice(ctx->device));
    const int urc = fops_upload(ctx, indices, (size_t)n_sel * 4);
    if (urc != OUSTER_HIP_OK) return urc;
    for (uint32_t p0 = 0; p0 < n_planes; p0 += FOPS_MAX_PLANES) {
        FopsSelectArgs a{};
        a.n_planes = std::min<uint32_t>(FOPS_MAX_PLANES, n_planes - p0);
        for (uint32_t i = 0; i < a.n_planes; ++i) {
            a.src[i] = src[p0 + i];
            a.dst[i] = dst[p0 + i];
            a.elem[i] = elem_bytes[p0 + i];
        }
        a.n_images = n_images;
        a.h = h;
        a.w = w;
        a.n_sel = n_sel;
        a.indices = (const uint32_t*)ctx->fops_tables.p;
        HIP_TRY(launch_fops_select_rows(a, ctx->stream));
    }
    return OUSTER_HIP_OK;
}

namespace {
// The planes of a *_host call: pool memory stays where it is, every other plane gets a 16-byte aligned piece of scratch `slot`.
struct HostPlanes {
    std::vector<void*> dev;
    std::vector<size_t> bytes;
    std::vector<bool> staged;
    int stage(ouster_hip_ctx* ctx, const void* const* host, const size_t* nbytes, uint32_t n, uint32_t slot, bool copy_in) {
        dev.assign(n, nullptr);
        bytes.assign(nbytes, nbytes + n);
        staged.assign(n, false);
        size_t total = 0;
        std::vector<size_t> off(n, 0);
        for (uint32_t i = 0; i < n; ++i) {
            if (!host[i]) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: NULL pointer", i);
            if (ouster_hip_host_is_pinned(host[i], nbytes[i])) {
                dev[i] = const_cast<void*>(host[i]);
                continue;
            }
            staged[i] = true;
            off[i] = total;
            total += (nbytes[i] + 15) & ~(size_t)15;
        }
        if (total && ctx->user_scratch[slot].ensure(total)) return fail(OUSTER_HIP_ERR_RUNTIME, "out of device memory (scratch %u, %zu bytes)", slot, total);
        for (uint32_t i = 0; i < n; ++i) {
            if (!staged[i]) continue;
            dev[i] = (uint8_t*)ctx->user_scratch[slot].p + off[i];
            if (copy_in) HIP_TRY(hipMemcpyAsync(dev[i], host[i], nbytes[i], hipMemcpyHostToDevice, ctx->stream));
        }
        return OUSTER_HIP_OK;
    }
    int finish(ouster_hip_ctx* ctx, void* const* host) {
        for (size_t i = 0; i < dev.size(); ++i)
            if (staged[i]) HIP_TRY(hipMemcpyAsync(host[i], dev[i], bytes[i], hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return OUSTER_HIP_OK;
    }
};
int fops_host_planes(ouster_hip_ctx* ctx, const ouster_hip_fops_plane* planes, uint32_t n_planes, uint32_t h, uint32_t w,
                     std::vector<ouster_hip_fops_plane>& dev_planes, std::vector<void*>& host, HostPlanes& hp) {
    if (!ctx || !planes) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    std::vector<size_t> nbytes(n_planes);
    host.resize(n_planes);
    for (uint32_t i = 0; i < n_planes; ++i) {
        uint64_t bits;
        if (!fops_elem(planes[i].type)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: unsupported element type %d", i, planes[i].type);
        const int rc = ouster_hip_frame_ops_invalid_bits(planes[i].type, planes[i].invalid, &bits);
        if (rc != OUSTER_HIP_OK) return rc;
        if (planes[i].twin) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: a host call takes no twin plane", i);
        nbytes[i] = (size_t)h * w * fops_elem(planes[i].type);
        host[i] = planes[i].data;
    }
    if ((uint64_t)h * w == 0 || n_planes == 0) return 1;
    HIP_TRY(hipSetDevice(ctx->device));
    const int rc = hp.stage(ctx, host.data(), nbytes.data(), n_planes, 0, true);
    if (rc != OUSTER_HIP_OK) return rc;
    dev_planes.assign(planes, planes + n_planes);
    for (uint32_t i = 0; i < n_planes; ++i) {
        dev_planes[i].data = hp.dev[i];
        dev_planes[i].image_stride = 0;
    }
    return OUSTER_HIP_OK;
}
}  // namespace

int ouster_hip_frame_ops_clip_host(ouster_hip_ctx* ctx, const ouster_hip_fops_plane* planes, uint32_t n_planes, uint32_t h,
                                   uint32_t w, double lower, double upper) {
    std::vector<ouster_hip_fops_plane> dp;
    std::vector<void*> host;
    HostPlanes hp;
    int rc = fops_host_planes(ctx, planes, n_planes, h, w, dp, host, hp);
    if (rc) return rc > 0 ? OUSTER_HIP_OK : rc;
    rc = ouster_hip_frame_ops_clip(ctx, dp.data(), n_planes, 1, h, w, lower, upper);
    if (rc != OUSTER_HIP_OK) return rc;
    return hp.finish(ctx, host.data());
}

int ouster_hip_frame_ops_invalidate_host(ouster_hip_ctx* ctx, const ouster_hip_fops_pred* pred,
                                         const ouster_hip_fops_plane* planes, uint32_t n_planes, uint32_t h, uint32_t w) {
    if (!pred) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "pred is NULL");
    std::vector<ouster_hip_fops_plane> dp;
    std::vector<void*> host;
    HostPlanes hp;
    int rc = fops_host_planes(ctx, planes, n_planes, h, w, dp, host, hp);
    if (rc) return rc > 0 ? OUSTER_HIP_OK : rc;
    ouster_hip_fops_pred dpred = *pred;
    dpred.src_stride = 0;
    size_t sbytes = 0;
    switch (pred->kind) {
        case OUSTER_HIP_FOPS_PRED_KEY: sbytes = (size_t)h * w * fops_elem(pred->src_type); break;
        case OUSTER_HIP_FOPS_PRED_MASK: sbytes = (size_t)h * w; dpred.n_masks = 1; break;
        case OUSTER_HIP_FOPS_PRED_XYZ: sbytes = (size_t)h * w * 3 * (pred->src_type == OUSTER_HIP_F64 ? 8 : 4); break;
        default: break;
    }
    if (sbytes) {
        if (!pred->src) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "predicate source is NULL");
        dpred.src = nullptr;
        for (uint32_t i = 0; i < n_planes; ++i)   // the key among the targets: the same device image
            if (host[i] == pred->src && hp.bytes[i] == sbytes) dpred.src = hp.dev[i];
        if (!dpred.src) {
            HostArg src;
            rc = host_arg(ctx, pred->src, sbytes, 1, true, src);
            if (rc != OUSTER_HIP_OK) return rc;
            dpred.src = src.dev;
        }
    }
    rc = ouster_hip_frame_ops_invalidate(ctx, &dpred, dp.data(), n_planes, 1, h, w);
    if (rc != OUSTER_HIP_OK) return rc;
    return hp.finish(ctx, host.data());
}

int ouster_hip_frame_ops_select_rows_host(ouster_hip_ctx* ctx, const void* const* src, void* const* dst,
                                          const uint32_t* elem_bytes, uint32_t n_planes, uint32_t h, uint32_t w,
                                          const uint32_t* indices, uint32_t n_sel) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (n_planes == 0 || h == 0 || w == 0 || n_sel == 0) return ouster_hip_frame_ops_select_rows(ctx, src, dst, elem_bytes, n_planes, 1, h, w, indices, n_sel);
    if (!src || !dst || !elem_bytes) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<size_t> sb(n_planes), db(n_planes);
    for (uint32_t p = 0; p < n_planes; ++p) {
        sb[p] = (size_t)h * w * elem_bytes[p];
        db[p] = (size_t)n_sel * w * elem_bytes[p];
    }
    HostPlanes in, out;
    int rc = in.stage(ctx, src, sb.data(), n_planes, 0, true);
    if (rc == OUSTER_HIP_OK) rc = out.stage(ctx, dst, db.data(), n_planes, 1, false);
    if (rc != OUSTER_HIP_OK) return rc;
    rc = ouster_hip_frame_ops_select_rows(ctx, in.dev.data(), out.dev.data(), elem_bytes, n_planes, 1, h, w, indices, n_sel);
    if (rc != OUSTER_HIP_OK) return rc;
    return out.finish(ctx, dst);
}

// ---- range-gated, compacting frame dewarp ------------------------------------------------------
int ouster_hip_range_gate(double min_range, double max_range, uint32_t* min_r, uint32_t* max_r, int* empty) {
    // uint32_t min_r = ceil(min_range * 1e3), max_r = floor(max_range * 1e3): dewarp_impl.h:33-34
    const double lo = std::ceil(min_range * 1e3), hi = std::floor(max_range * 1e3);
    const bool none = !(hi >= 0) || !(lo <= 4294967295.0) || hi < lo;
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
    if (dtype != OUSTER_HIP_F32 && dtype != OUSTER_HIP_F64)
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
    // uint32_t min_r = ceil(min_range * 1e3), max_r = floor(max_range * 1e3): dewarp_impl.h:33-34
    const double lo = std::ceil(min_range * 1e3), hi = std::floor(max_range * 1e3);
    if (!(hi >= 0) || !(lo <= 4294967295.0) || hi < lo) {  // nothing can pass the gate
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
    DewarpFramesArgs a{};
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
    a.min_r = lo <= 0 ? 0u : (uint32_t)lo;
    a.max_r = hi >= 4294967295.0 ? 0xffffffffu : (uint32_t)hi;
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

// ---- OSF field planes ---------------------------------------------------------------------------
int ouster_hip_osf_unpack(ouster_hip_ctx* ctx, const ouster_hip_osf_plane* planes, uint32_t n_planes,
                          uint32_t h, uint32_t w, const int32_t* pixel_shift_by_row) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (n_planes == 0 || h == 0 || w == 0) return OUSTER_HIP_OK;
    if (!planes) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "planes is NULL");
    bool any_png = false;
    size_t unfiltered_bytes = 0;          // device scratch for the planes that arrive as filtered PNG scanlines
    uint32_t n_filtered = 0, max_row_bytes = 0;
    for (uint32_t i = 0; i < n_planes; ++i) {
        const ouster_hip_osf_plane& p = planes[i];
        if (!p.src || !p.dst) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: NULL pointer", i);
        const uint32_t e = p.dst_elem_size;
        if (!(e == 1 || e == 2 || e == 4 || e == 8))
            return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: unsupported element size %u", i, e);
        if (p.flags & ~OUSTER_HIP_OSF_FLAG_FILTERED) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: unknown flags", i);
        static const uint32_t want[6] = {0, 1, 2, 3, 4, 8};
        if (p.encoding >= OUSTER_HIP_OSF_PNG_GRAY8 && p.encoding <= OUSTER_HIP_OSF_PNG_RGBA16) {
            if (p.src_pixel_bytes != want[p.encoding])
                return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: pixel size does not match its PNG type", i);
            any_png = true;
            if (p.flags & OUSTER_HIP_OSF_FLAG_FILTERED) {
                ++n_filtered;
                unfiltered_bytes += ((size_t)h * w * p.src_pixel_bytes + 15) & ~(size_t)15;
                max_row_bytes = std::max(max_row_bytes, w * p.src_pixel_bytes);
            }
        } else if (p.encoding == OUSTER_HIP_OSF_ZPNG) {
            if (p.src_pixel_bytes == 0 || p.src_pixel_bytes > 8)
                return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: ZPNG pixels are 1..8 bytes", i);
            if (p.flags) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: ZPNG planes carry no PNG filters", i);
        } else {
            return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "plane %u: unknown encoding %u", i, p.encoding);
        }
    }
    if (n_filtered && osf_png_unfilter_lds_bytes(w, max_row_bytes) > 160u * 1024u)   // the launcher's own figure
        return fail(OUSTER_HIP_ERR_UNSUPPORTED, "a PNG scanline of %u bytes needs %zu bytes of LDS for the device filters (160 KB per workgroup): "
                    "hand the planes over unfiltered (flags = 0)", max_row_bytes, osf_png_unfilter_lds_bytes(w, max_row_bytes));
    HIP_TRY(hipSetDevice(ctx->device));
    OsfUnpackArgs a{};
    a.h = h;
    a.w = w;
    if (any_png && pixel_shift_by_row) {  // stagger(img, px_offset) = destagger with inverse offsets
        std::vector<int32_t> off;
        dest_offsets(pixel_shift_by_row, h, w, 1, off);
        if (ensure_offsets(ctx, off)) return fail(OUSTER_HIP_ERR_RUNTIME, "offset upload failed");
        ctx->shifts_host.clear();
        a.offsets = (const int32_t*)ctx->offsets.p;
    }
    // the job arrays: the unpack jobs (filtered planes read the device-side unfiltered copy), then the unfilter jobs
    std::vector<ouster_hip_osf_plane> jobs(planes, planes + n_planes);
    std::vector<OsfUnfilterJob> unf;
    if (n_filtered) {
        if (ctx->osf_pixels.ensure(unfiltered_bytes)) return fail(OUSTER_HIP_ERR_RUNTIME, "scratch allocation failed");
        size_t at = 0;
        for (uint32_t i = 0; i < n_planes; ++i) {
            if (!(jobs[i].flags & OUSTER_HIP_OSF_FLAG_FILTERED)) continue;
            OsfUnfilterJob j{};
            j.raw = (const uint8_t*)jobs[i].src;
            j.out = (uint8_t*)ctx->osf_pixels.p + at;
            j.bpp = jobs[i].src_pixel_bytes;
            unf.push_back(j);
            jobs[i].src = j.out;
            jobs[i].flags = 0;
            at += ((size_t)h * w * j.bpp + 15) & ~(size_t)15;
        }
    }
    const size_t bytes = (size_t)n_planes * sizeof(ouster_hip_osf_plane), ubytes = unf.size() * sizeof(OsfUnfilterJob);
    if (ctx->scratch.ensure(bytes + ubytes)) return fail(OUSTER_HIP_ERR_RUNTIME, "scratch allocation failed");
    HIP_TRY(hipMemcpyAsync(ctx->scratch.p, jobs.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
    if (ubytes) HIP_TRY(hipMemcpyAsync((uint8_t*)ctx->scratch.p + bytes, unf.data(), ubytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // the job arrays are this call's memory
    if (n_filtered) {
        OsfUnfilterArgs u{};
        u.jobs = (const OsfUnfilterJob*)((uint8_t*)ctx->scratch.p + bytes);
        u.h = h;
        u.w = w;
        HIP_TRY(launch_osf_png_unfilter(u, n_filtered, max_row_bytes, ctx->stream));
    }
    a.planes = (const ouster_hip_osf_plane*)ctx->scratch.p;
    HIP_TRY(launch_osf_unpack(a, n_planes, ctx->stream));
    return OUSTER_HIP_OK;
}

const char* ouster_hip_last_decode_kernel(ouster_hip_ctx* ctx) { return ctx ? ctx->last_kernel : ""; }

int ouster_hip_last_decode_tile(ouster_hip_ctx* ctx, int* tile_cols, int* tile_rows) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (tile_cols) *tile_cols = ctx->last_tile_cols;
    if (tile_rows) *tile_rows = ctx->last_tile_rows;
    return OUSTER_HIP_OK;
}

// ---- interp_pose / transform (k_pose.hip, host/pose_util.cpp) --------------------------------------
namespace {
// validated known poses -> the table and the known times on the device, [k - 1][24] + [k] doubles in ctx->fops_tables
int pose_tables(ouster_hip_ctx* ctx, const std::vector<double>& host, uint32_t k, PoseInterpArgs& a) {
    const int rc = fops_upload(ctx, host.data(), host.size() * 8);
    if (rc != OUSTER_HIP_OK) return rc;
    a.segments = (const double*)ctx->fops_tables.p;
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
    if (dtype != OUSTER_HIP_F32 && dtype != OUSTER_HIP_F64) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dtype must be F32 or F64");
    if (n == 0) return OUSTER_HIP_OK;
    if (!x_interp || !poses_out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    char msg[160];
    if (pose_validate_interp(x_interp, n, msg, sizeof msg)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", msg);
    HIP_TRY(hipSetDevice(ctx->device));
    HostArg in, out;
    int rc = host_arg(ctx, x_interp, n * 8, 0, true, in);
    if (rc == OUSTER_HIP_OK) rc = host_arg(ctx, poses_out, n * 16 * (dtype == OUSTER_HIP_F64 ? 8 : 4), 1, false, out);
    if (rc != OUSTER_HIP_OK) return rc;
    PoseInterpArgs a{};
    a.x = (const double*)in.dev;
    a.n = n;
    a.dtype = dtype;
    a.out = out.dev;
    rc = pose_interp_launch(ctx, table, k, a);
    if (rc != OUSTER_HIP_OK) return rc;
    return host_finish(ctx, out);
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
    if (dtype != OUSTER_HIP_F32 && dtype != OUSTER_HIP_F64) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dtype must be F32 or F64");
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
    if (dtype != OUSTER_HIP_F32 && dtype != OUSTER_HIP_F64) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dtype must be F32 or F64");
    if (!pose16) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "pose is NULL");
    if (n == 0) return OUSTER_HIP_OK;
    if (!points || !out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)n * 3 * (dtype == OUSTER_HIP_F64 ? 8 : 4);
    HostArg in, o;
    int rc = host_arg(ctx, points, bytes, 0, true, in);
    if (rc == OUSTER_HIP_OK) rc = host_arg(ctx, out, bytes, 1, false, o);
    if (rc != OUSTER_HIP_OK) return rc;
    rc = ouster_hip_transform(ctx, in.dev, pose16, o.dev, dtype, n);
    if (rc != OUSTER_HIP_OK) return rc;
    return host_finish(ctx, o);
}

// ---- algorithm::normals (k_normals.hip, host/normals_util.cpp) -------------------------------------
namespace {
int normals_validate(const ouster_hip_normals_desc* d) {
    if (!d) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "desc is NULL");
    const bool dual = d->xyz2 || d->range2;
    if (const char* msg = normals_validate_shapes(d->h, d->w, d->xyz_rows, dual, d->xyz2_rows, d->range2_h, d->range2_w,
                                                  d->sensor_origins ? d->n_origins : d->w))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", msg);
    if (const char* msg = normals_validate_params(d->min_angle_of_incidence_rad, d->target_distance_m))
        return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", msg);
    if (d->xyz_dtype != OUSTER_HIP_F32 && d->xyz_dtype != OUSTER_HIP_F64) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "xyz_dtype must be F32 or F64");
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
    int rc = fops_upload(ctx, table.data(), table.size());
    if (rc != OUSTER_HIP_OK) return rc;
    a.consts = (const double*)ctx->fops_tables.p;
    a.s2b = mbytes ? (const double*)((const uint8_t*)ctx->fops_tables.p + cbytes) : nullptr;
    a.shifts = sbytes ? (const uint32_t*)((const uint8_t*)ctx->fops_tables.p + cbytes + mbytes) : nullptr;
    if (ctx->normals_pairs.cap < rows * sizeof(NormalsPair)) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (ctx->normals_pairs.ensure(rows * sizeof(NormalsPair))) return fail(OUSTER_HIP_ERR_RUNTIME, "out of device memory (normals)");
    }
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
    rc = fops_upload(ctx, table.data(), table.size());
    if (rc != OUSTER_HIP_OK) return rc;
    a.consts = (const double*)ctx->fops_tables.p;
    a.s2b = mbytes ? (const double*)((const uint8_t*)ctx->fops_tables.p + cbytes) : nullptr;
    a.shifts = sbytes ? (const uint32_t*)((const uint8_t*)ctx->fops_tables.p + cbytes + mbytes) : nullptr;
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
    const size_t es = desc->xyz_dtype == OUSTER_HIP_F32 ? 4 : 8;
    std::vector<const void*> in = {desc->xyz, desc->range};
    std::vector<size_t> in_bytes = {px * 3 * es, px * 4};
    if (dual) in.push_back(desc->xyz2), in_bytes.push_back(px * 3 * es), in.push_back(desc->range2), in_bytes.push_back(px * 4);
    const bool with_poses = !desc->sensor_origins && desc->poses;
    if (desc->sensor_origins) in.push_back(desc->sensor_origins), in_bytes.push_back((size_t)desc->w * 24);
    if (with_poses) in.push_back(desc->poses), in_bytes.push_back((size_t)desc->n_frames * desc->w * 128);
    std::vector<void*> out = {desc->normals};
    std::vector<size_t> out_bytes = {px * 24};
    if (dual) out.push_back(desc->normals2), out_bytes.push_back(px * 24);
    HostPlanes hin, hout;
    rc = hin.stage(ctx, in.data(), in_bytes.data(), (uint32_t)in.size(), 0, true);
    if (rc == OUSTER_HIP_OK) rc = hout.stage(ctx, out.data(), out_bytes.data(), (uint32_t)out.size(), 1, false);
    if (rc != OUSTER_HIP_OK) return rc;
    ouster_hip_normals_desc d = *desc;
    size_t i = 0;
    d.xyz = hin.dev[i++], d.range = (const uint32_t*)hin.dev[i++];
    if (dual) d.xyz2 = hin.dev[i++], d.range2 = (const uint32_t*)hin.dev[i++];
    if (desc->sensor_origins) d.sensor_origins = (const double*)hin.dev[i++];
    if (with_poses) d.poses = (const double*)hin.dev[i++];
    d.normals = (double*)hout.dev[0];
    if (dual) d.normals2 = (double*)hout.dev[1];
    rc = normals_device(ctx, &d);
    if (rc != OUSTER_HIP_OK) return rc;
    return hout.finish(ctx, out.data());
}

// ---- voxel down-sampling (k_voxel.hip, host/voxel_util.cpp) ------------------------------------------
namespace {
// everything but the device: NULL / dtype / stride / table_log2; 1: nothing to do (n == 0)
int voxel_validate_call(const ouster_hip_voxel_desc* d, uint64_t* n_out) {
    if (!d || !n_out) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    *n_out = 0;
    if (d->n == 0 && !d->normals) return 1;
    if (const char* msg = voxel_validate(d)) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", msg);
    if (d->dtype != OUSTER_HIP_F32 && d->dtype != OUSTER_HIP_F64) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dtype must be F32 or F64");
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
    const bool folds = a.form == VOXEL_FORM_AVERAGE || a.form == VOXEL_FORM_NORMALS;
    size_t temp_bytes = 0;
    HIP_TRY(voxel_temp_bytes(a.n, &temp_bytes));
    // the workspace, every piece 256-byte aligned
    const size_t n = a.n;
    size_t total = 0;
    auto take = [&total](size_t bytes) {
        const size_t at = total;
        total += (bytes + 255) & ~(size_t)255;
        return at;
    };
    const size_t o_hdr = take(sizeof(VoxelHeader)), o_keys = take(n * sizeof(VoxelKey)), o_table = take(((size_t)a.table_mask + 1) * 4),
                 o_slot = take(n * 4), o_first = take(n * 4), o_first_id = take(n * 4), o_vid = take(n * 4), o_idx = take(n * 4),
                 o_svid = take(n * 4), o_sidx = take(n * 4), o_begin = take(n * 4), o_end = take(n * 4),
                 o_keep = take(folds ? n * 4 : 0), o_pos = take(folds ? n * 4 : 0),
                 o_rows = take(folds ? n * 8 * (a.form == VOXEL_FORM_NORMALS ? 6 : a.cols) : 0), o_temp = take(temp_bytes);
    if (ctx->voxel_ws.cap < total) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (ctx->voxel_ws.ensure(total)) return fail(OUSTER_HIP_ERR_RUNTIME, "out of device memory (voxel workspace, %zu bytes)", total);
    }
    uint8_t* ws = (uint8_t*)ctx->voxel_ws.p;
    a.hdr = (VoxelHeader*)(ws + o_hdr), a.keys = (VoxelKey*)(ws + o_keys), a.table = (int32_t*)(ws + o_table);
    a.slot = (uint32_t*)(ws + o_slot), a.first = (uint32_t*)(ws + o_first), a.first_id = (uint32_t*)(ws + o_first_id);
    a.vid = (uint32_t*)(ws + o_vid), a.idx = (uint32_t*)(ws + o_idx), a.svid = (uint32_t*)(ws + o_svid), a.sidx = (uint32_t*)(ws + o_sidx);
    a.seg_begin = (uint32_t*)(ws + o_begin), a.seg_end = (uint32_t*)(ws + o_end);
    a.keep = (uint32_t*)(ws + o_keep), a.pos = (uint32_t*)(ws + o_pos), a.rows = (double*)(ws + o_rows);
    ctx->voxel_timed = false;
    HIP_TRY(voxel_run(a, ws + o_temp, temp_bytes, ctx->stream, ctx->voxel_timing ? ctx->voxel_ev : nullptr));
    VoxelHeader hdr{};
    HIP_TRY(hipMemcpyAsync(&hdr, a.hdr, sizeof hdr, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->voxel_timed = ctx->voxel_timing;
    if (hdr.status == VOXEL_STATUS_TABLE) return fail(OUSTER_HIP_ERR_RUNTIME, "voxel_downsample: hash table exhausted");
    if (hdr.status) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "%s", VOXEL_MSG_GRID);
    *n_out = hdr.n_out;
    if (hdr.n_out > d->out_capacity) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "voxel_downsample: out_capacity is too small");
    return OUSTER_HIP_OK;
}
}  // namespace

int ouster_hip_voxel_timing(ouster_hip_ctx* ctx, int on) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    if (on)
        for (hipEvent_t& e : ctx->voxel_ev)
            if (!e) HIP_TRY(hipEventCreate(&e));
    ctx->voxel_timing = on != 0;
    ctx->voxel_timed = false;
    return OUSTER_HIP_OK;
}

int ouster_hip_voxel_phase_ms(ouster_hip_ctx* ctx, float* ms) {
    if (!ctx || !ms) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!ctx->voxel_timed) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "voxel_downsample: no timed call (ouster_hip_voxel_timing)");
    for (int k = 0; k < OUSTER_HIP_VOXEL_PHASES; ++k) HIP_TRY(hipEventElapsedTime(&ms[k], ctx->voxel_ev[k], ctx->voxel_ev[k + 1]));
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
    const size_t es = desc->dtype == OUSTER_HIP_F32 ? 4 : 8, stride = desc->row_stride ? desc->row_stride : desc->cols;
    const bool wn = desc->normals != nullptr;
    std::vector<const void*> in = {desc->points};
    std::vector<size_t> in_bytes = {((size_t)(desc->n - 1) * stride + desc->cols) * es};
    if (wn) in.push_back(desc->normals), in_bytes.push_back((size_t)desc->n * 24);
    // a result of no rows still needs somewhere to point
    static double none[3];
    std::vector<void*> out = {desc->out_capacity ? (void*)desc->out : (void*)none};
    std::vector<size_t> out_bytes = {(size_t)desc->out_capacity * desc->cols * 8};
    if (wn) out.push_back(desc->out_capacity ? (void*)desc->out_normals : (void*)none), out_bytes.push_back((size_t)desc->out_capacity * 24);
    HostPlanes hin, hout;
    rc = hin.stage(ctx, in.data(), in_bytes.data(), (uint32_t)in.size(), 0, true);
    // foreign output memory gets scratch that is copied back only after success: a call that refuses leaves the caller's array alone
    if (rc == OUSTER_HIP_OK) rc = hout.stage(ctx, out.data(), out_bytes.data(), (uint32_t)out.size(), 1, false);
    if (rc != OUSTER_HIP_OK) return rc;
    ouster_hip_voxel_desc d = *desc;
    d.points = hin.dev[0];
    if (wn) d.normals = (const double*)hin.dev[1];
    d.out = (double*)hout.dev[0];
    if (wn) d.out_normals = (double*)hout.dev[1];
    rc = voxel_device(ctx, &d, n_out);
    if (rc != OUSTER_HIP_OK) return rc;
    // only the rows of the result travel back
    hout.bytes[0] = (size_t)*n_out * desc->cols * 8;
    if (wn) hout.bytes[1] = (size_t)*n_out * 24;
    return hout.finish(ctx, out.data());
}

// ---- ICP: point_to_point_align / point_to_plane_align (k_icp.hip, host/icp_util.cpp) -------------------
namespace {
struct IcpCall {
    IcpArgs a{};
    VoxelArgs va{};
    uint8_t* temp = nullptr;
    size_t temp_bytes = 0;
    IcpMethod method = ICP_POINT;
};

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
    const size_t nt = a.n_tgt, ns = a.n_src, slots = (size_t)a.table_mask + 1;
    size_t total = 0;
    auto take = [&total](size_t bytes) {
        const size_t at = total;
        total += (bytes + 255) & ~(size_t)255;
        return at;
    };
    const size_t o_rb = take(sizeof(IcpReadback)), o_keys = take(nt * sizeof(VoxelKey)), o_table = take(slots * 4), o_slot = take(nt * 4),
                 o_first = take(nt * 4), o_first_id = take(nt * 4), o_vid = take(nt * 4), o_idx = take(nt * 4), o_svid = take(nt * 4),
                 o_sidx = take(nt * 4), o_begin = take(nt * 4), o_end = take(nt * 4), o_slots = take(slots * sizeof(IcpSlot)),
                 o_slot_end = take(slots * 4), o_rows = take(nt * 8 * (a.plane ? 6 : 3)), o_nn = take(ns * 4), o_r = take(ns * 8),
                 o_key = take(ns * 8), o_key_sorted = take(ns * 8), o_flag = take(ns * 4), o_xq = take(ns * 48),
                 o_partials = take((size_t)icp_chunks(a.n_src) * OUSTER_HIP_ICP_SUMS * 8), o_temp = take(c.temp_bytes);
    if (ctx->icp_ws.cap < total) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (ctx->icp_ws.ensure(total)) return fail(OUSTER_HIP_ERR_RUNTIME, "out of device memory (icp workspace, %zu bytes)", total);
    }
    uint8_t* ws = (uint8_t*)ctx->icp_ws.p;
    a.rb = (IcpReadback*)(ws + o_rb), a.keys = (VoxelKey*)(ws + o_keys), a.table = (int32_t*)(ws + o_table);
    a.first_id = (uint32_t*)(ws + o_first_id), a.svid = (uint32_t*)(ws + o_svid), a.sidx = (uint32_t*)(ws + o_sidx);
    a.seg_begin = (uint32_t*)(ws + o_begin), a.seg_end = (uint32_t*)(ws + o_end);
    a.slots = (IcpSlot*)(ws + o_slots), a.slot_end = (uint32_t*)(ws + o_slot_end), a.rows = (double*)(ws + o_rows);
    a.nn = (int32_t*)(ws + o_nn), a.r = (double*)(ws + o_r), a.key = (uint64_t*)(ws + o_key), a.key_sorted = (uint64_t*)(ws + o_key_sorted);
    a.flag = (uint32_t*)(ws + o_flag), a.xq = (double*)(ws + o_xq), a.partials = (double*)(ws + o_partials);
    c.temp = ws + o_temp;
    // the target side as the launchers of k_voxel.h see it
    VoxelArgs& v = c.va;
    v.n = a.n_tgt, v.hdr = &a.rb->grid, v.keys = a.keys, v.table = a.table, v.table_mask = a.table_mask;
    v.slot = (uint32_t*)(ws + o_slot), v.first = (uint32_t*)(ws + o_first), v.first_id = a.first_id;
    v.vid = (uint32_t*)(ws + o_vid), v.idx = (uint32_t*)(ws + o_idx), v.svid = a.svid, v.sidx = a.sidx;
    v.seg_begin = a.seg_begin, v.seg_end = a.seg_end;
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
    const bool timing = ctx->icp_timing;
    ctx->icp_timed = false;
    if (timing) HIP_TRY(hipEventRecord(ctx->icp_ev[0], ctx->stream));
    HIP_TRY(icp_grid_run(c.a, c.va, c.temp, c.temp_bytes, ctx->stream));
    if (timing) HIP_TRY(hipEventRecord(ctx->icp_ev[1], ctx->stream));
    double pose[16];
    memcpy(pose, d->initial_guess, sizeof pose);
    uint32_t iterations = 0, solved = 0;
    uint64_t count = 0;
    for (uint32_t it = 0; it < ICP_MAX_ITERATIONS; ++it) {
        IcpReadback rb{};
        rc = icp_pass(ctx, c, pose, rb, timing ? ctx->icp_ev + 2 + 4 * it : nullptr);
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
    ctx->icp_timed = timing;
    ctx->icp_timed_passes = iterations;
    return OUSTER_HIP_OK;
}
}  // namespace

uint32_t ouster_hip_icp_chunk_rows(void) { return ICP_CHUNK; }

int ouster_hip_icp_timing(ouster_hip_ctx* ctx, int on) {
    if (!ctx) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    if (on)
        for (hipEvent_t& e : ctx->icp_ev)
            if (!e) HIP_TRY(hipEventCreate(&e));
    ctx->icp_timing = on != 0;
    ctx->icp_timed = false;
    return OUSTER_HIP_OK;
}

int ouster_hip_icp_phase_ms(ouster_hip_ctx* ctx, float* ms) {
    if (!ctx || !ms) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!ctx->icp_timed) return fail(OUSTER_HIP_ERR_INVALID_ARGUMENT, "icp: no timed call (ouster_hip_icp_timing)");
    for (int k = 0; k < OUSTER_HIP_ICP_PHASES; ++k) ms[k] = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms[0], ctx->icp_ev[0], ctx->icp_ev[1]));
    for (uint32_t it = 0; it < ctx->icp_timed_passes; ++it)
        for (int k = 0; k < 3; ++k) {
            float t = 0.0f;
            HIP_TRY(hipEventElapsedTime(&t, ctx->icp_ev[2 + 4 * it + k], ctx->icp_ev[2 + 4 * it + k + 1]));
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
    const size_t es = desc->dtype == OUSTER_HIP_F32 ? 4 : 8;
    auto bytes = [es](uint64_t n, uint64_t stride) { return ((size_t)(n - 1) * (stride ? stride : 3) + 3) * es; };
    std::vector<const void*> in = {desc->source_points, desc->target_points};
    std::vector<size_t> in_bytes = {bytes(desc->n_source, desc->source_stride), bytes(desc->n_target, desc->target_stride)};
    if (desc->source_normals) {
        in.push_back(desc->source_normals), in_bytes.push_back(bytes(desc->n_source, desc->source_normal_stride));
        in.push_back(desc->target_normals), in_bytes.push_back(bytes(desc->n_target, desc->target_normal_stride));
    }
    HostPlanes hin;
    rc = hin.stage(ctx, in.data(), in_bytes.data(), (uint32_t)in.size(), 0, true);
    if (rc != OUSTER_HIP_OK) return rc;
    ouster_hip_icp_desc d = *desc;
    d.source_points = hin.dev[0], d.target_points = hin.dev[1];
    if (desc->source_normals) d.source_normals = hin.dev[2], d.target_normals = hin.dev[3];
    rc = icp_device(ctx, &d);
    if (rc != OUSTER_HIP_OK) return rc;
    memcpy(desc->pose, d.pose, sizeof d.pose);
    desc->iterations = d.iterations, desc->solved = d.solved, desc->correspondences = d.correspondences;
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
        HIP_TRY(hipEventElapsedTime(&ms, ctx->ev_pool[i].first, ctx->ev_pool[i].second));
        total += ms;
    }
    *avg_ms = ctx->ev_used ? total / (double)ctx->ev_used : 0.0;
    if (n_launches) *n_launches = (uint32_t)ctx->ev_used;
    ctx->ev_used = 0;
    return OUSTER_HIP_OK;
}

}  // extern "C"
