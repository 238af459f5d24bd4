// decode_plan.h -- which kernel and which tile shape an ouster_hip_decode call gets: host integers in, values out.
// Includes nothing but the C ABI header and the standard library, so it compiles (and is tested) without HIP.
// ouster_hip_dev.h includes it: the kernel files see Geometry, StreamArgs and the constants here as before.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <optional>

#include "../../include/ouster_hip.h"

// 1: the f32 xyz transpose of the fused kernels goes through ds_bpermute (no LDS scratch);
// 0: through a 12 KB wave-private LDS scratch (the r01 form, kept for A/B builds)
#ifndef OUSTER_XYZ_PERMUTE
#define OUSTER_XYZ_PERMUTE 1
#endif

#ifdef __HIPCC__
#define OUSTER_HOST_DEVICE __host__ __device__
#else
#define OUSTER_HOST_DEVICE
#endif

namespace ouster_hip_dev {

enum SpecId { SPEC_GENERIC = 0, SPEC_DUAL_LB, SPEC_LB, SPEC_SINGLE, SPEC_DUAL, SPEC_LEGACY };

struct Geometry {
    uint32_t pixels_per_column, columns_per_packet, columns_per_frame;
    uint32_t packet_header_size, col_header_size, channel_data_size, col_footer_size,
        packet_footer_size, col_size, lidar_packet_size;
    ouster_hip_bits col_timestamp, col_measurement_id, col_status;
    ouster_hip_bits frame_id, alert_flags, thermal_shutdown, shot_limiting,
        countdown_thermal_shutdown, countdown_shot_limiting;
};

// how a decode launch finds the source column of a destination column
enum DecodeMode : uint32_t {
    MODE_FAST = 0,     // optimistic: slot s holds column s; verified against the staged headers, strays
                       //   flag their frame in frame_state
    MODE_FIXUP = 1,    // second pass: redo the frames the fast pass flagged (the others return at once)
    MODE_GENERAL = 2,  // every frame through the scan-the-frame path (slots_per_frame*cpp != W)
    MODE_RESOLVED = 3, // small batches, one launch: every wide tile resolves its frame's column maps itself (k_decode_wide_resolved)
};

// frame_state words (kernels_common.h): sequence, tag, 2 x 8 ticket counters, the launch-wide "a frame was flagged" word
// (its own cache line: only ever touched by atomics), then one word per frame (from a line boundary on)
constexpr uint32_t FS_SEQ = 0, FS_TAG = 1, FS_TICKET = 2, FS_ANY = 20, FS_WORDS = 32;

constexpr size_t XYZ_SCRATCH_BYTES = OUSTER_XYZ_PERMUTE ? 0 : 4 * 192 * 16;

// k_decode_stream (persistent, a ring of tile contexts filled by LDS-DMA): what the host works out
// once per launch.  A tile context in LDS = the pixel image (TW column blocks of `ncell` 16 B cells, block of column j at
// index j/4 + (TW/4)*(j%4)), then the column-header dwords [n_hdr][TW], the packet-level dwords [n_pkt + 2][64], the
// destagger offsets of the tile's rows and their per-beam xyz constants.
struct FieldPlan {   // a 64-bit field window assembled from fetched dwords: window dword k comes from slot[k] (-1: not needed)
    int8_t slot[3];
    uint8_t sh;      // bit position of the window inside window dword 0
};
struct StreamArgs {
    uint32_t tr, nch;          // rows per tile, row chunks per frame
    uint32_t ncell;            // 16 B cells per column block (the piece of tr rows plus its 16 B phase)
    uint32_t npix_instr;       // 1 KB wave-instructions that fill the pixel image
    uint32_t hdr_off, pkt_off, off_off, beam_off, ctx_bytes;  // byte offsets inside a tile context / its size
    uint32_t fixed_off;        // byte offset of the per-workgroup tables behind the contexts (nslot * ctx_bytes)
    uint32_t n_hdr, n_pkt;     // dwords fetched per column / per packet
    uint32_t hdr_dw[8];        //   their dword offsets from the column start
    uint32_t pkt_dw[4];        //   ... from the packet start
    FieldPlan mid, st, ts, alert;
    uint32_t groups;           // workgroups per (XCD, column tile)
    uint32_t wait0;            // 1: vmcnt(0) before a prefetched tile is used; 0: rely on the in-order counter (>= 63 stores since)
    uint32_t lds_bytes;
    uint32_t order;            // how a group walks the XCD's (frame, row chunk) items, see the kernel
    uint32_t loader;           // > 0: k_decode_stream2 with that many loader waves behind the eight decoding ones (1..4)
    uint32_t nslot;            // tile contexts in LDS (2: double-buffered; k_decode_stream2 takes up to STREAM_MAX_SLOTS and fetches nslot - 1 tiles ahead)
    uint32_t dma_per_tile[4];  // k_decode_stream2: LDS-DMA instructions loader wave l issues per tile (what its vmcnt waits count in)
};
constexpr uint32_t STREAM_MAX_SLOTS = 6;
// k_decode_stream2's loader waves wait for "tile i has landed" with s_waitcnt vmcnt(k), k = the DMA instructions the wave has issued
// for newer tiles: their queue holds nothing else and retires in order.  The counter has 6 bits.
constexpr uint32_t STREAM_MAX_VMCNT = 63;

// ---- LDS sizes ---------------------------------------------------------------------------------------------------------
// resolve_frame's scratch (kernels_common.h), in words
OUSTER_HOST_DEVICE inline size_t resolve_lds_words(uint32_t W, uint32_t npo, uint32_t slots_per_frame, uint32_t cpp) {
    return (size_t)3 * W + npo + 2 * (size_t)slots_per_frame + (size_t)slots_per_frame * cpp + 4;
}
// LDS of one k_decode workgroup (the general modes add the per-frame packet map and valid bitmap)
size_t decode_lds_bytes(const Geometry& g, int tile, bool general, bool beam_lds, uint32_t slots_per_frame = 0);
// img_words: the tile image [tw][column slot] + 4 slack words (the fix-up pass: at least resolve_frame's scratch)
size_t decode_wide_lds_bytes(int tw, uint32_t rows_per_tile, uint32_t img_words);
size_t slotmap_lds_bytes(uint32_t W, uint32_t cpp, uint32_t slots_per_frame);   // resolve_frame's LDS scratch, bytes

// ---- knobs ---------------------------------------------------------------------------------------------------------------
// experiment / test knobs of a context: defaults from OUSTER_HIP_* environment variables read ONCE in
// ouster_hip_ctx_create, changed afterwards with ouster_hip_ctx_set_knob (never getenv on the call path).
// What each one means stands in knob_table (decode_plan.cpp), next to its name and environment variable.
struct Knobs {
    int tile = 0, wide = -1, wide_kb = 64, wide_rows = 0, wide_min_blocks = 512, tune = 1, xcd = 1, fast = 1;
    int dewarp_single_pass = 0, beam_lds = 1, fixup = 1, small = 1, fixup_rows = 0, hdr_words = 1, fixup_wide = 1;
    int stream = -1, stream_rows = 0, stream_wait = 1, stream_min_tiles = 8, stream_order = 0, slotmap = 1;
    int dwf_stream = -1, stream_loader = 4, stream_slots = 0;
    int pose_direct = 0;
    int tonemap_bands = 0;
};
struct KnobDef {
    const char* name;    // ouster_hip_ctx_set_knob
    const char* env;     // environment variable read at ouster_hip_ctx_create, nullptr: none
    int Knobs::*member;
};
extern const KnobDef knob_table[];
extern const int knob_count;
const KnobDef* find_knob(const char* name);   // nullptr: no such knob

// ---- the plan ------------------------------------------------------------------------------------------------------------
struct PlanInput {
    Geometry g;
    Knobs kn;
    uint32_t n_frames, slots_per_frame;
    size_t packet_stride;
    uintptr_t packets, xyz_poses;        // addresses: only their alignment (and poses != 0) counts
    int spec, xyzm;                      // SpecId after the xyz-field check | 0 no xyz, 1 / 2 separable f32 / f64, 3 full LUT
    bool vec_ok;
    uint32_t n_fields;
    uint64_t plane_mask, destagger_mask; // bit i: planes[i] / destaggered[i] requested
    uint32_t xyz_mask;                   // bit k: xyz[k] requested
    bool gate_counts;
    bool host_ts;                        // host timestamps are handed in and packet_timestamp is requested (two more dwords per tile)
    uint32_t cus, resident_wgs;
    bool may_resolve;                    // the build has k_decode_wide_resolved (OUSTER_EXPERIMENTS)
};

struct TileShape {   // DecodeArgs fields of the same names
    uint32_t rows_per_tile, row_chunks, lds_col_slot, tiles_per_frame, fix_rows_small;
};
enum class WideKind {
    OPTIMISTIC,  // k_decode_wide behind "slot c holds column c" or behind k_slotmap's maps
    FIXUP,       // the fix-up pass (k_decode_wide_fixup): resolve_frame's scratch lies under the tile image, the grid is persistent
    SMALL,       // small batches: rows chosen so that few frames still make about two workgroups per CU
};
struct StreamPlan {
    StreamArgs sa;
    TileShape shape;
};

// k_decode's tile width (64 / 32 / 16; 0: not even 16 columns fit in LDS) and whether its per-beam xyz table goes to LDS
struct NarrowPlan { int tile; uint32_t beam_lds; };
NarrowPlan plan_narrow(const PlanInput& in);
std::optional<TileShape> plan_wide(const PlanInput& in, int width, WideKind kind);
std::optional<StreamPlan> plan_stream(const PlanInput& in, int width);

// What is settled before the tuner is asked, and what it may choose from.
struct Candidates {
    int small_width = 0;       // small batch on wide tiles of this width (nothing else to choose)
    TileShape small_shape{};
    bool resolved = false;     //   ... in the one-launch form
    int forced_stream = 0;     // knob `stream`: the persistent kernel with this tile width
    int stream_auto = 0;       // tile width of the persistent candidate (0: not eligible)
    int stream_alt = 0;        //   ... and of the other width, when that is eligible too
    int n = 0;                 // > 0: the tuner chooses among variant[0 .. n); 0: forced by a knob, or a shape with nothing to choose
    int variant[5] = {0, 0, 0, 0, 0};   // 256 / 128: k_decode_wide, 0: k_decode, 1000 + tile width: the persistent kernel
};
Candidates plan_candidates(const PlanInput& in);
uint64_t tuner_key(const PlanInput& in, const Candidates& c);   // batches of similar size and the same outputs share a verdict

enum class Kernel { DECODE, WIDE, WIDE_RESOLVED, STREAM, STREAM2 };
const char* kernel_name(Kernel k);
enum class Fixup { NONE, NARROW, WIDE };   // NARROW: k_decode_fixup's 64-column (or narrower) tiles

struct DecodePlan {
    bool ok = false;              // false: not even k_decode's narrowest tile fits in LDS (nothing else is set then)
    Kernel kernel = Kernel::DECODE;
    int cols = 0;                 // tile width of `kernel`
    int narrow_tile = 0;          // k_decode's tile width (also that of a NARROW fix-up pass)
    TileShape shape{};            // the optimistic (or only) pass
    StreamArgs sa{};              // STREAM / STREAM2
    uint32_t beam_lds = 0, mode = MODE_FAST, xcd_map = 0;
    bool slotmap = false;         // k_slotmap runs first (general mapping on wide tiles)
    Fixup fixup = Fixup::NONE;
    int fix_cols = 0;             // WIDE: tile width
    TileShape fix_shape{};        // WIDE: its tiles; NARROW: the persistent grid of k_decode
    uint32_t fast_tiles = 0;      // fix-up pass: column tiles of the optimistic pass before it
    size_t hdr_words_bytes = 0;   // scratch the call needs before its first launch
    size_t slotmap_bytes = 0;     //   (slot map: for k_slotmap, or for a WIDE fix-up pass)
};
// selected: one of c.variant (ignored when c.n == 0).  A variant that turns out not to be possible falls back to 256-column wide tiles.
DecodePlan plan_decode(const PlanInput& in, const Candidates& c, int selected);
inline DecodePlan plan_decode(const PlanInput& in, int selected) { return plan_decode(in, plan_candidates(in), selected); }
// no slot map could be allocated for a WIDE fix-up pass: it runs on k_decode's tiles instead
void demote_fixup(const PlanInput& in, DecodePlan& p);

}  // namespace ouster_hip_dev
