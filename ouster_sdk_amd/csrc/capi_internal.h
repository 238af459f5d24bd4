// capi_internal.h -- what the translation units of the C ABI share: ouster_hip_capi.hip (context, formats, decode) and one
// capi_<feature>.hip next to each feature's kernels.  Internal to libouster_hip.so, not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <deque>
#include <string>
#include <utility>
#include <vector>

#include "decode_tuner.h"
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

// What the context owns frees itself: ouster_hip_ctx_destroy makes the device current, waits for the stream and deletes.
// (HIDDEN on what is new here: the library's dynamic symbols stay what they were.)
#define HIDDEN __attribute__((visibility("hidden")))
struct DevBuf {   // a grow-only block of device memory
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    HIDDEN ~DevBuf() { counted_free(p); }
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
};

struct HIDDEN PinnedBuf {   // a grow-only block of page-locked host memory: at least `n` bytes, `want` of them when it grows
    void* p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    hipError_t ensure(size_t n, size_t want) {
        if (n <= cap) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        const hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) cap = want;
        return e;
    }
};

struct HIDDEN Event {   // an event, created on first use
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t create(unsigned flags = hipEventDefault) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
};

// The variant tuner's samples of one workload (decode_tuner.h): a pair of events around each timed launch, polled, never
// waited for.  ouster_hip_decode creates and records the pair of the slot the tuner hands out.
struct HIDDEN TuneEvents {
    Event ev[TUNE_SAMPLES][2];
    bool landed(int n) const {
        for (int i = 0; i < n; ++i)
            if (hipEventQuery(ev[i][1].e) != hipSuccess) {
                (void)hipGetLastError();
                return false;
            }
        return true;
    }
    float ms(int i) const {
        float t = 0;
        return hipEventElapsedTime(&t, ev[i][0].e, ev[i][1].e) == hipSuccess ? t : 0.f;
    }
};

// events around the phases of a call (ouster_hip_voxel_timing / _icp_timing): `on` asks for them, `timed`: the last call has them
template <int N>
struct PhaseTimer {
    bool on = false, timed = false;
    hipEvent_t ev[N] = {};
    PhaseTimer() = default;
    PhaseTimer(const PhaseTimer&) = delete;
    PhaseTimer& operator=(const PhaseTimer&) = delete;
    HIDDEN ~PhaseTimer() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    int enable(int device, bool want) {
        HIP_TRY(hipSetDevice(device));
        if (want)
            for (hipEvent_t& e : ev)
                if (!e) HIP_TRY(hipEventCreate(&e));
        on = want;
        timed = false;
        return OUSTER_HIP_OK;
    }
};

}  // namespace ouster_hip_dev

struct ouster_hip_ctx {
    using DevBuf = ouster_hip_dev::DevBuf;
    HIDDEN ouster_hip_ctx() = default;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    DevBuf state, tile_valid, offsets, luts, counts, scratch, slotmap, hdrw, osf_pixels;
    DevBuf image_mask;                   // ouster_hip_image_dark_rows: the column masks of a batch
    DevBuf tonemap_ws;                   // ouster_hip_image_tonemap: tile histograms and look-up tables, 2 x 256 KB per image
    DevBuf tables;                       // upload_table: the small host table of the call in flight (shifts, row indices, pose segments, ...)
    ouster_hip_dev::PinnedBuf table_pin; //   ... its page-locked staging, and the event behind its last copy
    ouster_hip_dev::Event table_ev;
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
    ouster_hip_dev::PinnedBuf ring_buf[RING];
    ouster_hip_dev::Event ring_ev[RING];   // behind the last copy out of each
    int ring_next = 0;
    ouster_hip_dev::Knobs knobs;
    bool timing = false;
    uint32_t timing_every = 1, timing_calls = 0;   // HIP events around every timing_every-th decode kernel (an event record costs the stream 2 - 3 us)
    std::deque<std::array<ouster_hip_dev::Event, 2>> ev_pool;   // (a deque: the events stay where they are)
    size_t ev_used = 0;
    ouster_hip_dev::DecodeTuner<ouster_hip_dev::TuneEvents> tuner;   // the variant tuner and its cache file (decode_tuner.h)
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

// `buf` holds at least `bytes`, growing only on an idle stream: a call in flight may still use the old block.  `what` is the
// noun of the error message, which names the size too where `say_bytes`.
HIDDEN inline int grow_idle(ouster_hip_ctx* ctx, DevBuf& buf, size_t bytes, const char* what, bool say_bytes = false) {
    if (bytes <= buf.cap) return OUSTER_HIP_OK;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (!buf.ensure(bytes)) return OUSTER_HIP_OK;
    return say_bytes ? fail(OUSTER_HIP_ERR_RUNTIME, "out of device memory (%s, %zu bytes)", what, bytes)
                     : fail(OUSTER_HIP_ERR_RUNTIME, "out of device memory (%s)", what);
}

// A small host table -> ctx->tables, safe by construction for back-to-back asynchronous calls: the source is copied into
// page-locked staging owned by the context, the staging is reused only after the event behind its last copy has completed,
// and the device buffer grows only on an idle stream.
inline int upload_table(ouster_hip_ctx* ctx, const void* src, size_t bytes) {
    if (ctx->table_ev.e) HIP_TRY(hipEventSynchronize(ctx->table_ev.e));
    else HIP_TRY(ctx->table_ev.create(hipEventDisableTiming));
    HIP_TRY(ctx->table_pin.ensure(bytes, bytes * 2));
    if (const int rc = grow_idle(ctx, ctx->tables, bytes, "frame_ops tables")) return rc;
    std::memcpy(ctx->table_pin.p, src, bytes);
    HIP_TRY(hipMemcpyAsync(ctx->tables.p, ctx->table_pin.p, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->table_ev.e, ctx->stream));
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
