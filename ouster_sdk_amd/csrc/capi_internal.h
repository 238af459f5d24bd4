// capi_internal.h -- what the translation units of the C ABI share: ouster_hip_capi.hip (context, formats, decode) and one
// capi_<feature>.hip next to each feature's kernels.  Internal to libouster_hip.so, not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "host_pool.h"
#include "ouster_hip_dev.h"

namespace ouster_hip_dev {

// the C ABI's error channel (ouster_hip_capi.hip): stores the thread's message, returns `code`
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail_msg(int code, const char* msg);

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return fail(OUSTER_HIP_ERR_RUNTIME, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// bytes of an F32 / F64 element; 0: `dtype` is neither
inline size_t float_elem(int dtype) { return dtype == OUSTER_HIP_F32 ? 4 : dtype == OUSTER_HIP_F64 ? 8 : 0; }
inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

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

// events around the phases of a call (ouster_hip_voxel_timing / _icp_timing): `on` asks for them, `timed`: the last call has them
template <int N>
struct PhaseTimer {
    bool on = false, timed = false;
    hipEvent_t ev[N] = {};
    int enable(int device, bool want) {
        HIP_TRY(hipSetDevice(device));
        if (want)
            for (hipEvent_t& e : ev)
                if (!e) HIP_TRY(hipEventCreate(&e));
        on = want;
        timed = false;
        return OUSTER_HIP_OK;
    }
    void destroy() {
        for (hipEvent_t& e : ev)
            if (e) (void)hipEventDestroy(e), e = nullptr;
    }
};

}  // namespace ouster_hip_dev

struct ouster_hip_ctx {
    using DevBuf = ouster_hip_dev::DevBuf;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    DevBuf state, tile_valid, offsets, luts, counts, scratch, slotmap, hdrw, osf_pixels;
    DevBuf image_mask;                   // ouster_hip_image_dark_rows: the column masks of a batch
    DevBuf tonemap_ws;                   // ouster_hip_image_tonemap: tile histograms and look-up tables, 2 x 256 KB per image
    DevBuf tables;                       // upload_table: the small host table of the call in flight (shifts, row indices, pose segments, ...)
    void* table_pin = nullptr;           //   ... its page-locked staging, and the event behind its last copy
    size_t table_pin_cap = 0;
    hipEvent_t table_ev = nullptr;
    DevBuf normals_pairs;                // ouster_hip_normals: what k_normals_subtent leaves, 16 bytes per frame and return
    ouster_hip_dev::PhaseTimer<OUSTER_HIP_VOXEL_PHASES + 1> voxel_timer;
    DevBuf voxel_ws;                     // ouster_hip_voxel_downsample: keys, table, ids, sorted indices, gathered rows, sort temporaries
    ouster_hip_dev::PhaseTimer<2 + 4 * 10> icp_timer;   // start, after the grid, then per pass: start, after correspond, after median, after sums
    uint32_t icp_timed_passes = 0;       //   ... passes of the last timed call
    DevBuf icp_ws;                       // ouster_hip_icp_*: the target grid, the per-row outputs of a pass, partial sums, sort temporaries
    DevBuf user_scratch[8];              // ouster_hip_ctx_scratch: what the *_host calls and bindings stage through
    uint32_t resident_wgs = 512;         // 2 workgroups (80 KB LDS each) per CU
    uint32_t cus = 256;                  // compute units (k_decode_stream: one persistent workgroup each)
    const char* last_kernel = "";        // name of the decode kernel the last ouster_hip_decode launched
    bool state_dirty = false;            // `state` may hold leftovers (fix-up pass skipped / a failed launch)
    std::vector<int32_t> offsets_host;   // cache key of `offsets`
    std::vector<int32_t> shifts_host;    // pixel_shift_by_row the cached offsets were derived from
    uint32_t shifts_w = 0;               //   ... and the frame width (the offsets are (W + x % W) % W)
    std::vector<ouster_hip_dev::LutDev> luts_host;   // cache key of `luts`
    // pageable host packet_counts go through a small pinned ring (no stream synchronisation)
    static constexpr int RING = 4;
    uint32_t* ring_buf[RING] = {nullptr, nullptr, nullptr, nullptr};
    size_t ring_cap[RING] = {0, 0, 0, 0};
    hipEvent_t ring_ev[RING] = {nullptr, nullptr, nullptr, nullptr};
    int ring_next = 0;
    ouster_hip_dev::Knobs knobs;
    bool timing = false;
    uint32_t timing_every = 1, timing_calls = 0;   // HIP events around every timing_every-th decode kernel (an event record costs the stream 2 - 3 us)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    size_t ev_used = 0;
    std::map<uint64_t, ouster_hip_dev::Tune> tune;   // the variant tuner, by workload key (decode_plan.h)
    // verdicts of earlier processes (ouster_hip_ctx_set_tuning_cache): workload key -> chosen variant, for THIS device and library
    std::string tune_cache_path, tune_cache_id;
    std::map<uint64_t, int> tune_cache;
    const char* last_tuner = "none";     // how the last ouster_hip_decode chose its variant
    int last_tile_cols = 0, last_tile_rows = 0;  // tile of the last k_decode launch
};

struct ouster_hip_format {
    ouster_hip_format_desc desc;
    ouster_hip_dev::Geometry g;
    int spec_id = ouster_hip_dev::SPEC_GENERIC;
    int8_t spec_of_desc[OUSTER_HIP_MAX_FIELDS];
    int spec_nf = 0, spec_r1 = -1, spec_r2 = -1;
};

struct ouster_hip_lut {
    int device = 0;  // the tables outlive the context that uploaded them
    uint32_t w = 0, h = 0;
    bool separable = false;
    ouster_hip_dev::LutDev dev{};
    void *d_beam = nullptr, *d_col = nullptr, *d_dir = nullptr, *d_ofs = nullptr;
    // host copy of the full double LUT for ouster_hip_lut_export
    std::vector<double> direction, offset;
};

namespace ouster_hip_dev {

// per-call device tables of the context (ouster_hip_capi.hip).  Both synchronise the stream when they upload and not otherwise.
//   ensure_luts     `l` -> ctx->luts, unless it is there already; 0 or -1
//   stage_offsets   the destination column offsets of `shifts` (destagger; inverse: stagger) -> ctx->offsets; *out is the device
//                   array.  Voids ouster_hip_decode's cache key for ctx->offsets.  OUSTER_HIP_OK, or the code fail() returned.
// (Hidden: the library's dynamic symbols stay what they were.)
__attribute__((visibility("hidden"))) int ensure_luts(ouster_hip_ctx* c, const std::vector<LutDev>& l);
__attribute__((visibility("hidden"))) int stage_offsets(ouster_hip_ctx* c, const int32_t* shifts, uint32_t h, uint32_t w, int inverse, const int32_t** out);

// A small host table -> ctx->tables, safe by construction for back-to-back asynchronous calls: the source is copied into
// page-locked staging owned by the context, the staging is reused only after the event behind its last copy has completed,
// and the device buffer grows only on an idle stream.
inline int upload_table(ouster_hip_ctx* ctx, const void* src, size_t bytes) {
    if (ctx->table_ev) HIP_TRY(hipEventSynchronize(ctx->table_ev));
    else HIP_TRY(hipEventCreateWithFlags(&ctx->table_ev, hipEventDisableTiming));
    if (bytes > ctx->table_pin_cap) {
        if (ctx->table_pin) (void)hipHostFree(ctx->table_pin);
        ctx->table_pin = nullptr;
        ctx->table_pin_cap = 0;
        HIP_TRY(hipHostMalloc(&ctx->table_pin, bytes * 2, hipHostMallocDefault));
        ctx->table_pin_cap = bytes * 2;
    }
    if (bytes > ctx->tables.cap) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));   // a kernel in flight may still read the old table
        if (ctx->tables.ensure(bytes)) return fail(OUSTER_HIP_ERR_RUNTIME, "out of device memory (frame_ops tables)");
    }
    std::memcpy(ctx->table_pin, src, bytes);
    HIP_TRY(hipMemcpyAsync(ctx->tables.p, ctx->table_pin, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->table_ev, ctx->stream));
    return OUSTER_HIP_OK;
}

// The host arrays of one *_host call.  Register each with input() / output() / inout(), then stage(): pool memory
// (ouster_hip_host_is_pinned) is handed to the kernel as it is, anything else -- and whatever is registered `always` -- gets a
// 256-byte aligned piece of the context's grow-only scratch, inputs in slot 0, outputs and arrays updated in place in slot 1
// (slots 4 to 7 belong to bindings: include/ouster_hip.h).  dev() is valid from stage() on; finish() copies the staged outputs
// back and synchronises.  Nothing is allocated on the host for up to INLINE arrays.
class Staging {
public:
    struct Ref { int i = -1; explicit operator bool() const { return i >= 0; } };   // default: no array, dev() is NULL
    explicit Staging(ouster_hip_ctx* c) : ctx(c) {}
    Ref input(const void* host, size_t bytes, bool always = false) { return add(const_cast<void*>(host), bytes, 0, true, false, always); }
    Ref output(void* host, size_t bytes, bool always = false) { return add(host, bytes, 1, false, true, always); }
    Ref inout(void* host, size_t bytes) { return add(host, bytes, 1, true, true, false); }
    Ref find(const void* host, size_t bytes) const {   // the array last registered with this address and size
        for (int i = n - 1; i >= 0; --i)
            if (at(i).host == host && at(i).bytes == bytes) return Ref{i};
        return Ref{};
    }
    int stage() {
        for (uint32_t s = 0; s < 2; ++s)
            if (total[s] && ctx->user_scratch[s].ensure(total[s])) return fail(OUSTER_HIP_ERR_RUNTIME, "out of device memory (scratch %u, %zu bytes)", s, total[s]);
        for (int i = 0; i < n; ++i) {
            Arg& a = at(i);
            if (!a.staged) continue;
            a.dev = (uint8_t*)ctx->user_scratch[a.slot].p + a.off;
            if (a.in && a.bytes) HIP_TRY(hipMemcpyAsync(a.dev, a.host, a.bytes, hipMemcpyHostToDevice, ctx->stream));
        }
        return OUSTER_HIP_OK;
    }
    void* dev(Ref r) const { return r ? at(r.i).dev : nullptr; }
    void set_bytes(Ref r, size_t bytes) { at(r.i).bytes = bytes; }   // what finish() copies back of an output: no more than was staged
    int finish() {
        for (int i = 0; i < n; ++i)
            if (const Arg& a = at(i); a.staged && a.out && a.bytes) HIP_TRY(hipMemcpyAsync(a.host, a.dev, a.bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return OUSTER_HIP_OK;
    }
private:
    struct Arg {
        void *host, *dev;   // dev: the host address itself where the kernel works in place
        size_t bytes, off;
        uint8_t slot;
        bool in, out, staged;
    };
    static constexpr int INLINE = 8;
    Arg& at(int i) { return i < INLINE ? first[i] : more[i - INLINE]; }
    const Arg& at(int i) const { return i < INLINE ? first[i] : more[i - INLINE]; }
    Ref add(void* host, size_t bytes, uint8_t slot, bool in, bool out, bool always) {
        const bool staged = always || !ouster_hip_host_is_pinned(host, bytes);
        const size_t off = (total[slot] + 255) & ~(size_t)255;
        if (staged) total[slot] = off + bytes;
        const Arg a{host, staged ? nullptr : host, bytes, off, slot, in, out, staged};
        if (n < INLINE) first[n] = a;
        else more.push_back(a);
        return Ref{n++};
    }
    ouster_hip_ctx* ctx;
    int n = 0;
    size_t total[2] = {0, 0};   // bytes of scratch slot 0 / 1 this call needs
    Arg first[INLINE];
    std::vector<Arg> more;      // frame_ops with many planes
};

// the eleven pieces of a voxel grid over v.n rows and v.table_mask + 1 slots, in the order voxel_downsample and ICP's target
// side both keep them (capi_voxel.hip)
struct Carver;
struct VoxelArgs;
void carve_voxel_grid(Carver& c, VoxelArgs& v);

}  // namespace ouster_hip_dev
