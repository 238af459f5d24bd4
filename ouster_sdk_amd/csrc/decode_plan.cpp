// decode_plan.cpp -- the launch plan of ouster_hip_decode (decode_plan.h).  Plain C++: no HIP, no allocation, no state.
#include "decode_plan.h"

#include <string.h>

#include <algorithm>
#include <utility>

namespace ouster_hip_dev {

// ---- knobs -------------------------------------------------------------------------------------------------------------
const KnobDef knob_table[] = {
    {"tile", "OUSTER_HIP_TILE", &Knobs::tile},   // force k_decode's tile width (64/32/16)
    {"wide", "OUSTER_HIP_WIDE", &Knobs::wide},   // -1 auto (tuner), 0 narrow, 64/128/256/512 force k_decode_wide
    {"wide_kb", "OUSTER_HIP_WIDE_KB", &Knobs::wide_kb},       // LDS budget of a wide tile image
    {"wide_rows", "OUSTER_HIP_WIDE_ROWS", &Knobs::wide_rows}, // force the rows of a wide tile (experiments)
    {"wide_min_blocks", "OUSTER_HIP_WIDE_MIN_BLOCKS", &Knobs::wide_min_blocks},   // smaller launches stay on k_decode
    {"tune", "OUSTER_HIP_TUNE", &Knobs::tune},   // 0 pins the default wide variant
    {"xcd", "OUSTER_HIP_XCD", &Knobs::xcd},      // 0 disables the XCD-aware block -> frame mapping
    {"fast", "OUSTER_HIP_FAST", &Knobs::fast},   // 0 sends every frame through the general mapping
    {"dewarp_single_pass", "OUSTER_HIP_DWF_SINGLE", &Knobs::dewarp_single_pass},   // 1 = k_dwf_single instead of count / scan / emit (slower)
    {"beam_lds", "OUSTER_HIP_BEAM_LDS", &Knobs::beam_lds},   // 0 keeps k_decode's per-beam table in global memory (A/B)
    {"fixup", nullptr, &Knobs::fixup},           // tests only: 0 skips the fix-up pass (flagged frames are then left undone)
    // small batches: 1 = wide tiles of few rows (optimistic pass + fix-up pass; any other buffer shape: the one-launch
    // k_decode_wide_resolved) | 2 = the one-launch form always | 0 = k_decode's narrow tiles as in r03
    {"small", "OUSTER_HIP_SMALL", &Knobs::small},
    {"fixup_rows", "OUSTER_HIP_FIXUP_ROWS", &Knobs::fixup_rows},   // rows of a fix-up tile (0: 8)
    {"hdr_words", "OUSTER_HIP_HDR_WORDS", &Knobs::hdr_words},      // 0 = the fix-up pass reads the column headers from the packets again (A/B)
    // 1 = the fix-up pass on wide tiles where the format allows | 0 = 64-column tiles | 64 / 128 / 256 force
    {"fixup_wide", "OUSTER_HIP_FIXUP_WIDE", &Knobs::fixup_wide},
    {"stream", "OUSTER_HIP_STREAM", &Knobs::stream},   // -1 auto | 0 never | 128 / 256 force k_decode_stream with that tile width when eligible
    {"stream_rows", "OUSTER_HIP_STREAM_ROWS", &Knobs::stream_rows},   // force the rows of a streamed tile (experiments)
    {"stream_wait", "OUSTER_HIP_STREAM_WAIT", &Knobs::stream_wait},   // 1 vmcnt(0) before a prefetched tile is used | 0 rely on the in-order counter
    {"stream_min_tiles", "OUSTER_HIP_STREAM_MIN_TILES", &Knobs::stream_min_tiles},   // tiles per workgroup below which a launch stays on k_decode_wide
    {"stream_order", "OUSTER_HIP_STREAM_ORDER", &Knobs::stream_order},   // item order of k_decode_stream's groups (experiments)
    // 0 = buffers without one slot per column go through k_decode's general tiles (every tile scans the frame's headers)
    // instead of k_slotmap + k_decode_wide
    {"slotmap", "OUSTER_HIP_SLOTMAP", &Knobs::slotmap},
    {"dwf_stream", "OUSTER_HIP_DWF_STREAM", &Knobs::dwf_stream},   // the frame dewarp's emit kernel: -1 auto | 0 k_dwf_emit | 1 the persistent k_dwf_emit_stream where eligible
    {"stream_loader", "OUSTER_HIP_STREAM_LOADER", &Knobs::stream_loader},   // loader waves of k_decode_stream2 (0 = k_decode_stream: every wave fetches)
    // tile contexts of k_decode_stream2's ring, 2 .. 6: the loaders fetch that many tiles less one ahead (A/B).  0 = the plan's choice;
    // a depth that does not fit in LDS, or in the loaders' vmcnt, at any tile height is refused (the launch takes another kernel)
    {"stream_slots", "OUSTER_HIP_STREAM_SLOTS", &Knobs::stream_slots},
    {"pose_direct", "OUSTER_HIP_POSE_DIRECT", &Knobs::pose_direct},   // 1 = k_pose_interp stores each lane's own row (128 B lane stride) instead of going through LDS (A/B)
    {"tonemap_bands", "OUSTER_HIP_TONEMAP_BANDS", &Knobs::tonemap_bands},   // k_tm_hist: workgroups (bands of rows) per tile, 1 .. 64; 0 = the launch's own choice (A/B)
};
const int knob_count = (int)(sizeof knob_table / sizeof knob_table[0]);

const KnobDef* find_knob(const char* name) {
    for (const KnobDef& k : knob_table)
        if (!strcmp(k.name, name)) return &k;
    return nullptr;
}

// ---- LDS sizes ---------------------------------------------------------------------------------------------------------
size_t decode_lds_bytes(const Geometry& g, int tile, bool general, bool beam_lds, uint32_t slots_per_frame) {
    size_t tile_bytes = ((size_t)tile * g.col_size + 16 + 15) & ~(size_t)15;
    size_t h4 = (g.pixels_per_column + 3) & ~3u;
    size_t n = tile_bytes + (size_t)tile * 8 + 32 + h4 * 4 + XYZ_SCRATCH_BYTES;
    if (beam_lds) n += ((size_t)g.pixels_per_column * 9 + (g.pixels_per_column & 1)) * 8;
    if (general) {  // resolve_frame's scratch lies over the tile image (it is done before the tile is staged)
        const uint32_t npo = g.columns_per_frame / g.columns_per_packet;
        n = std::max(n, slotmap_lds_bytes(g.columns_per_frame, g.columns_per_packet, slots_per_frame ? slots_per_frame : npo));
        n = (n + 15) & ~(size_t)15;
    }
    return n;
}

size_t decode_wide_lds_bytes(int tw, uint32_t rows_per_tile, uint32_t img_words) {
    return ((size_t)img_words + 3 * (size_t)tw + 4 + ((rows_per_tile + 3) & ~3u)) * 4 +
           ((size_t)rows_per_tile * 9 + (rows_per_tile & 1)) * 8 + XYZ_SCRATCH_BYTES;
}

size_t slotmap_lds_bytes(uint32_t W, uint32_t cpp, uint32_t slots_per_frame) {
    return resolve_lds_words(W, W / cpp, slots_per_frame, cpp) * 4;
}

// ---- the pieces ----------------------------------------------------------------------------------------------------------
namespace {

// Does plan_stream give the 12 B/px static profiles a ring deeper than two on its own?  No: measured (profiles/r07_ring,
// DESIGN.md 3.2e), the decoders' wait at the tile barrier is not a wait for the fetch -- at 128 x 16 it is the same 12 % of the
// tile period with 2, 3 and 5 slots -- and the only heights that leave room for a third slot (128 x 16, 256 x 8) cost 7 - 12 %
// against the tall tile.  The rule below stays for the day a taller tile fits more than twice; stream_slots forces a depth.
constexpr bool STREAM_RING_DEFAULT = false;

// optimistic pass + fix-up pass when the buffer has one slot per column of the frame; everything through the general
// mapping otherwise
bool fast_possible(const PlanInput& in) {
    return in.kn.fast && (uint64_t)in.slots_per_frame * in.g.columns_per_packet == in.g.columns_per_frame;
}
size_t pose_bytes_per_col(const PlanInput& in) {   // LDS bytes of a column's pose
    return in.xyz_poses ? (size_t)12 * (in.xyzm == 1 ? 4 : 8) : 0;
}
uint32_t narrow_tiles(const PlanInput& in, int tile) { return (in.g.columns_per_frame + tile - 1) / tile; }

// the dwords a 64-bit field window needs, added to dws[0 .. n_dw)
bool plan_field(const ouster_hip_bits& b, uint32_t* dws, uint32_t& n_dw, uint32_t max_dw, FieldPlan& fp) {
    fp.slot[0] = fp.slot[1] = fp.slot[2] = -1;
    fp.sh = (uint8_t)((b.offset & 3u) * 8u);
    if (b.mask == 0) return true;
    const uint32_t lo = (uint32_t)__builtin_ctzll(b.mask) >> 3, hi = (63u - (uint32_t)__builtin_clzll(b.mask)) >> 3;
    const uint32_t d0 = b.offset >> 2, first = (b.offset + lo) >> 2, last = (b.offset + hi) >> 2;
    for (uint32_t d = first; d <= last; ++d) {
        if (d - d0 > 2) return false;
        uint32_t k = 0;
        while (k < n_dw && dws[k] != d) ++k;
        if (k == n_dw) {
            if (n_dw == max_dw) return false;
            dws[n_dw++] = d;
        }
        fp.slot[d - d0] = (int8_t)k;
    }
    return true;
}

// column pieces of at least 256 B per tile row chunk: 256 columns for the 8 / 16 / 4 B/px profiles, 128 for 12 B/px.
// probe(width) -> that width's plan, if possible.  Returns the preferred width (0: neither) and its plan.
uint32_t rows_of(const TileShape& s) { return s.rows_per_tile; }
uint32_t rows_of(const StreamPlan& p) { return p.sa.tr; }
template <class Probe>
auto prefer_256_bytes(const PlanInput& in, Probe probe) -> std::pair<int, decltype(probe(0))> {
    auto p256 = probe(256);
    if (p256 && rows_of(*p256) * in.g.channel_data_size >= 256) return {256, p256};
    if (auto p128 = probe(128)) return {128, p128};
    return {p256 ? 256 : 0, p256};
}

}  // namespace

NarrowPlan plan_narrow(const PlanInput& in) {
    const Geometry& g = in.g;
    const size_t pose_per_col = pose_bytes_per_col(in);
    auto lds = [&](int t, bool beam) { return decode_lds_bytes(g, t, true, beam, in.slots_per_frame); };
    // widest tile that still lets two workgroups share a CU's 160 KiB LDS
    int tile = 0;
    for (int t : {64, 32, 16})
        if (lds(t, false) + 16 + t * pose_per_col <= 80 * 1024) { tile = t; break; }
    if (!tile)
        for (int t : {64, 32, 16})
            if (lds(t, false) + 2048 + t * pose_per_col <= 160 * 1024) { tile = t; break; }
    if (!tile) return {0, 0u};
    // small batches: prefer narrower tiles so that at least ~2 workgroups per CU exist
    // (one 128x2048 frame is only 32 tiles of 64 columns -- latency, not bandwidth, bound)
    while (tile > 16 && (size_t)in.n_frames * narrow_tiles(in, tile) < 512) tile /= 2;
    const int forced = in.kn.tile;
    if ((forced == 64 || forced == 32 || forced == 16) && lds(forced, false) + 2048 + forced * pose_per_col <= 160 * 1024) tile = forced;
    // the per-beam xyz table goes to LDS (no vector load left in the row loop: stores are never waited
    // for) whenever that does not cost k_decode a workgroup per CU
    uint32_t beam_lds = 0;
    if (in.xyzm == 1 || in.xyzm == 2) {
        const size_t extra = 2048 + tile * pose_per_col;   // fix-up frame list + pose table
        const size_t without = lds(tile, false) + extra, with = lds(tile, true) + extra;
        beam_lds = (in.kn.beam_lds && with <= 160 * 1024 && (160 * 1024) / with == (160 * 1024) / without) ? 1u : 0u;
    }
    return {tile, beam_lds};
}

// wide, short tiles (k_decode_wide): TW columns x TR rows with TW*TR*chan <= ~64 KB, TR chosen so that the row chunks are
// equal.  An optimistic pass needs a batch large enough to fill the chip.
std::optional<TileShape> plan_wide(const PlanInput& in, int want, WideKind kind) {
    const Geometry& g = in.g;
    const Knobs& kn = in.kn;
    const uint32_t W = g.columns_per_frame, H = g.pixels_per_column, chan = g.channel_data_size;
    const bool fast = fast_possible(in), for_fix = kind == WideKind::FIXUP, small = kind == WideKind::SMALL;
    // General mapping on wide tiles: the column -> slot map of every frame is resolved once (k_slotmap), not by every tile
    const size_t resolver_lds = slotmap_lds_bytes(W, g.columns_per_packet, in.slots_per_frame);
    const bool mapped_ok = !fast && kn.slotmap && kn.tile == 0 && resolver_lds <= 160 * 1024;
    const size_t pose_per_col = pose_bytes_per_col(in);
    if (!((fast || mapped_ok || small) && (want == 64 || want == 128 || want == 256 || want == 512) && chan && chan % 4 == 0 &&
          W >= (uint32_t)want))
        return std::nullopt;
    if ((for_fix || small) && (want == 512 || want == 64 || in.gate_counts || resolver_lds > 64 * 1024)) return std::nullopt;
    if (in.xyz_poses & 15u) return std::nullopt;   // the wide tiles fetch the poses in 16 B pieces
    const uint32_t rpp = 1024u / (uint32_t)want;  // rows per pass of the 256-thread workgroup
    uint32_t budget = (uint32_t)(kn.wide_kb > 0 ? kn.wide_kb : 64) * 1024u;
    // with a pose table next to it the tile shrinks so that two workgroups still share a CU's LDS (a 256 x 32 tile +
    // 12 KB of poses is 84 KB = one workgroup per CU: 1.36 ms instead of 0.7)
    if (pose_per_col) budget = std::min<uint32_t>(budget, 72u * 1024u - (uint32_t)want * (uint32_t)pose_per_col);
    uint32_t tr_max = budget / ((uint32_t)want * chan) / rpp * rpp;
    tr_max = std::min(tr_max, 84u / rpp * rpp);   // k_decode_wide keeps a row chunk's table rows in registers (84 rows at most)
    if (tr_max < rpp) return std::nullopt;
    auto up = [&](uint32_t v) { return (v + rpp - 1) / rpp * rpp; };
    uint32_t nch = (H + tr_max - 1) / tr_max, tr = std::min(up((H + nch - 1) / nch), tr_max);
    for (uint32_t n2 = nch; n2 <= nch + 8 && n2 <= H; ++n2) {  // prefer equal chunks
        const uint32_t t2 = up((H + n2 - 1) / n2);
        if (t2 <= tr_max && t2 * n2 == H && t2 * 4 >= tr * 3) { nch = n2; tr = t2; break; }   // not at the price of much smaller tiles
    }
    const uint32_t tiles = (W + want - 1) / want;
    const size_t min_blocks = (size_t)std::max(kn.wide_min_blocks, 0);
    TileShape s{};
    if (small) {
        if ((size_t)in.n_frames * tiles * nch >= min_blocks) return std::nullopt;   // not a small batch
        const uint32_t want_blocks = 2u * in.cus;
        const uint32_t need = (want_blocks + in.n_frames * tiles - 1) / (in.n_frames * tiles);   // row chunks for that many workgroups
        tr = std::max(rpp, std::min(tr, H / std::max(need, 1u) / rpp * rpp));
    }
    if (for_fix) {
        // short tiles: the (few) flagged frames of a batch spread over a whole XCD instead of keeping a handful of
        // workgroups busy for a full-height tile each (tools/ab/fixup_prof.sh: 57 us for ONE flagged frame with 32-row tiles)
        // about 16 KB of packet bytes per tile (8 rows of 256 dual-return columns, 16 rows of 128 single-return ones): smaller
        // tiles are all prologue (the 12 B/px profile's 128 x 8 tiles made its fix-up pass slower than r03's)
        const uint32_t rows = kn.fixup_rows > 0 ? (uint32_t)kn.fixup_rows : (16384u + (uint32_t)want * chan - 1u) / ((uint32_t)want * chan);
        s.fix_rows_small = std::max(rpp, std::min(tr, up(rows)));   // the launch keeps the tall tile; the kernel takes the short one for few flagged frames
        if (tiles > 32) return std::nullopt;   // the frame's ready word carries one bit per column tile
    }
    if (kn.wide_rows > 0) tr = std::min((uint32_t)kn.wide_rows, H);
    if (tr > 84) return std::nullopt;   // k_decode_wide keeps a row chunk's table rows in registers (3 doubles per thread) while its tile loads
    nch = (H + tr - 1) / tr;
    if (in.gate_counts && nch > OUSTER_HIP_GATE_CHUNKS) return std::nullopt;  // one count slot per row chunk
    if (!for_fix && !small && (size_t)in.n_frames * tiles * nch < min_blocks) return std::nullopt;
    s.rows_per_tile = tr;
    s.row_chunks = nch;
    s.lds_col_slot = (tr * chan / 4 + 1) * 4;  // +1 dword: bank spread
    s.tiles_per_frame = tiles;
    size_t img_words = (size_t)want * (s.lds_col_slot >> 2) + 4;
    if (for_fix || small) img_words = std::max(img_words, (resolver_lds / 4 + 3) & ~(size_t)3);
    if (decode_wide_lds_bytes(want, tr, (uint32_t)img_words) + 16 + (size_t)want * pose_per_col > ((for_fix || small) ? 80u : 160u) * 1024)
        return std::nullopt;
    return s;
}

// Persistent, double-buffered tiles filled by LDS-DMA (k_decode_stream): the optimistic pass of the
// static profiles on large batches whose buffers keep every 16 B cell's phase fixed.
std::optional<StreamPlan> plan_stream(const PlanInput& in, int tw) {
    const Geometry& g = in.g;
    const Knobs& kn = in.kn;
    const uint32_t W = g.columns_per_frame, H = g.pixels_per_column, chan = g.channel_data_size, cpp = g.columns_per_packet;
    if (!(fast_possible(in) && in.spec != SPEC_GENERIC && in.xyzm != 3 && !in.xyz_poses && in.vec_ok &&
          (tw == 128 || tw == 256 || tw == 512 || tw == 1024)))
        return std::nullopt;
    if (W % (uint32_t)tw || (uint32_t)tw % cpp || (uint32_t)tw / cpp > 64 || chan == 0 || chan % 4) return std::nullopt;
    const uint32_t ct = W / (uint32_t)tw, per_xcd = std::max(in.cus / 8u, 1u);
    if (ct > per_xcd) return std::nullopt;
    // every 16 B cell keeps its phase from tile to tile: frame bases and the frame stride are multiples of 16
    const uint64_t frame_bytes = (uint64_t)in.slots_per_frame * in.packet_stride;
    if ((in.packets & 15) || (frame_bytes & 15)) return std::nullopt;
    // the last column's last cell must stay inside its frame's buffer
    const uint64_t last_end = (uint64_t)(in.slots_per_frame - 1) * in.packet_stride + g.packet_header_size +
                              (uint64_t)(cpp - 1) * g.col_size + g.col_header_size + (uint64_t)H * chan;
    if (last_end + 16 > frame_bytes) return std::nullopt;
    const uint32_t rpp = 2048u / (uint32_t)tw;   // rows per pass of the 512-thread workgroup
    StreamPlan p{};
    StreamArgs& sa = p.sa;
    if (!plan_field(g.col_measurement_id, sa.hdr_dw, sa.n_hdr, 8, sa.mid) ||
        !plan_field(g.col_status, sa.hdr_dw, sa.n_hdr, 8, sa.st) ||
        !plan_field(g.col_timestamp, sa.hdr_dw, sa.n_hdr, 8, sa.ts) ||
        !plan_field(g.alert_flags, sa.pkt_dw, sa.n_pkt, 4, sa.alert))
        return std::nullopt;
    // the loader-wave form (k_decode_stream2), the only one with a ring deeper than two
    sa.loader = (kn.stream_loader > 0 && (tw == 128 || tw == 256) && !in.gate_counts && kn.stream_order == 0)
                    ? (uint32_t)std::min(kn.stream_loader, 4) : 0u;
    // LDS-DMA instructions loader wave l issues per tile, in the kernel's own order: pixel instruction k belongs to wave
    // k % loader, and so does the k-th instruction of the small tables
    auto count_dma = [&]() {
        const uint32_t small = sa.n_hdr * ((uint32_t)tw / 64u) + sa.n_pkt + (in.host_ts ? 2u : 0u) +
                               (in.destagger_mask ? (sa.tr + 63u) / 64u : 0u) +
                               ((in.xyzm == 1 || in.xyzm == 2) ? (sa.tr * 18u + 63u) / 64u : 0u);
        uint32_t most = 0;
        for (uint32_t l = 0; l < 4; ++l) {
            auto share = [&](uint32_t n) { return (l < sa.loader && n > l) ? (n - l + sa.loader - 1) / sa.loader : 0u; };
            sa.dma_per_tile[l] = share(sa.npix_instr) + share(small);
            most = std::max(most, sa.dma_per_tile[l]);
        }
        return most;
    };
    auto fits = [&](uint32_t tr, uint32_t nslot) -> bool {
        if (tr == 0 || tr % rpp || H % tr || (tr * chan) % 16) return false;
        if (nslot < 2 || nslot > (sa.loader ? STREAM_MAX_SLOTS : 2u)) return false;
        sa.tr = tr;
        sa.nch = H / tr;
        sa.ncell = tr * chan / 16 + 1;
        sa.npix_instr = ((uint32_t)tw * sa.ncell + 63) / 64;
        if (sa.npix_instr > 72) return false;
        uint32_t o = sa.npix_instr * 1024u;
        sa.hdr_off = o; o += sa.n_hdr * (uint32_t)tw * 4u;
        sa.pkt_off = o; o += 6u * 256u;
        sa.off_off = o; o += ((tr + 63) / 64) * 256u;
        sa.beam_off = o; o += ((tr * 18u + 63) / 64) * 256u;
        sa.ctx_bytes = (o + 1023u) & ~1023u;
        sa.nslot = nslot;
        sa.fixed_off = nslot * sa.ctx_bytes;
        sa.lds_bytes = sa.fixed_off + 3u * (uint32_t)tw * 4u + 32u;
        if (sa.lds_bytes > 160u * 1024u) return false;
        // a loader waits for tile i behind nslot - 2 newer tiles of its own: that many instructions must fit in vmcnt
        return (nslot - 2u) * count_dma() <= STREAM_MAX_VMCNT;
    };
    // How deep, how tall.  A forced depth (knob stream_slots: A/B, tests) is taken as it is or refused, never clamped.
    // Left to the plan, every profile keeps the tallest tile that fits twice.  With STREAM_RING_DEFAULT set the 12 B/px
    // profiles (the shortest-lived tiles) would take, among the heights that fit twice, the one whose ring keeps the most
    // packet bytes in flight, (nslot - 1) * ctx_bytes, the taller on a tie, and no tile of fewer than two passes of the
    // workgroup.
    const uint32_t forced_slots = kn.stream_slots > 0 ? (uint32_t)kn.stream_slots : 0u;
    const uint32_t max_slots = sa.loader ? STREAM_MAX_SLOTS : 2u;
    const bool ring = STREAM_RING_DEFAULT && sa.loader && (in.spec == SPEC_SINGLE || in.spec == SPEC_LEGACY);
    auto deepest = [&](uint32_t tr) -> uint32_t {   // of the ring at this height (0: none); leaves sa at that plan
        if (forced_slots) return fits(tr, forced_slots) ? forced_slots : 0u;
        if (!fits(tr, 2u)) return 0u;
        for (uint32_t n = ring ? max_slots : 2u; n > 2; --n)
            if (fits(tr, n)) return n;
        return fits(tr, 2u) ? 2u : 0u;
    };
    uint32_t best_tr = 0, best_n = 0;
    if (kn.stream_rows > 0) {
        best_tr = (uint32_t)kn.stream_rows;
        best_n = deepest(best_tr);
    } else {
        uint32_t best_fly = 0;
        for (uint32_t tr = H / rpp * rpp; tr >= rpp; tr -= rpp) {
            const uint32_t n = deepest(tr);
            if (!n) continue;
            const uint32_t fly = (n - 1u) * sa.ctx_bytes;
            if (!best_n || (ring && !forced_slots && tr >= 2u * rpp && fly > best_fly)) { best_tr = tr; best_n = n; best_fly = fly; }
            if (!ring || forced_slots) break;   // the tallest tile that fits
        }
    }
    if (!best_n || !fits(best_tr, best_n)) return std::nullopt;
    if (in.gate_counts && sa.nch > OUSTER_HIP_GATE_CHUNKS) return std::nullopt;
    sa.groups = per_xcd / ct;
    const uint64_t tiles = (uint64_t)in.n_frames * ct * sa.nch, wgs = 8ull * ct * sa.groups;
    if (kn.stream_min_tiles > 0 && tiles < wgs * (uint64_t)kn.stream_min_tiles) return std::nullopt;
    // stores a wave issues per tile (one per output stream and lane row): with at least 63 of them behind a
    // prefetch the 6-bit in-order vmcnt itself proves the prefetch has landed
    uint32_t streams = (uint32_t)__builtin_popcountll(in.plane_mask) + (uint32_t)__builtin_popcountll(in.destagger_mask);
    streams += (uint32_t)__builtin_popcount(in.xyz_mask & 3u) * (in.xyzm == 1 ? 3u : 6u);
    const uint32_t stores_per_wave = streams * (sa.tr / rpp);
    sa.wait0 = (kn.stream_wait == 0 && stores_per_wave >= 64) ? 0u : 1u;
    sa.order = (uint32_t)kn.stream_order;
    p.shape = TileShape{sa.tr, sa.nch, 0u, ct, 0u};
    return p;
}

// ---- which optimistic-pass kernel ---------------------------------------------------------------------------------------
// Forced by a knob, or -- large batches of a static profile -- timed: k_decode_wide 256 x R, 128 x R, k_decode's 64-column
// tiles and (where the buffers allow it) the persistent k_decode_stream.  Which one wins depends on how the buffers
// happen to lie in HBM: the persistent kernel is 1.5 - 3 % ahead where the memory system is fastest
// and up to 10 % behind where it is slowest.
Candidates plan_candidates(const PlanInput& in) {
    const Knobs& kn = in.kn;
    const bool fast = fast_possible(in);
    Candidates c;
    // Small batches (one tick of a few sensors, a single frame).  Measured (tools/ab/small_batch.py, 4 x 128 x 2048 dual
    // return): optimistic wide tiles of 8 rows + the fix-up launch 27 us per call, k_decode's 16-column tiles + fix-up 33 us,
    // the one-launch form, where every wide tile resolves its frame's column maps itself, 35 us (its workgroups resolve the
    // frame before they can start: 14 us against the 3 us a second launch costs).  So: a buffer with one slot per column
    // takes the optimistic wide tiles, any other shape the one-launch form where the build has it (kn.small = 2 forces it
    // for both); without it such a buffer takes the general mapping like a large one (k_slotmap + k_decode_wide).
    if (kn.small && kn.stream <= 0 && kn.wide < 0 && kn.tile == 0 && kn.fast && (fast || in.may_resolve)) {
        for (int tw : {256, 128})
            if (in.g.columns_per_frame >= (uint32_t)tw) {   // the first width the frame has, even if its plan fails
                if (auto s = plan_wide(in, tw, WideKind::SMALL)) {
                    c.small_width = tw;
                    c.small_shape = *s;
                    c.resolved = in.may_resolve && (!fast || kn.small == 2);
                    return c;
                }
                break;
            }
    }
    if (kn.stream > 0) {
        if (plan_stream(in, kn.stream)) {
            c.forced_stream = kn.stream;
            return c;
        }
    } else if (kn.stream < 0 && kn.wide < 0 && kn.tile == 0) {
        c.stream_auto = prefer_256_bytes(in, [&](int tw) { return plan_stream(in, tw); }).first;
        // the other width too (round 4: the 12 B/px profile's 256 x 16 tiles beat its 128 x 32 ones by 3 - 4 % on some
        // boxes, tools/ab/single_variants.py)
        if (c.stream_auto) {
            const int other = c.stream_auto == 256 ? 128 : 256;
            if (plan_stream(in, other)) c.stream_alt = other;
        }
    }
    if (kn.wide < 0 && fast && plan_wide(in, 256, WideKind::OPTIMISTIC)) {
        const int v[5] = {256, 128, 0, 1000 + c.stream_auto, 1000 + c.stream_alt};
        memcpy(c.variant, v, sizeof v);
        c.n = c.stream_auto ? (c.stream_alt ? 5 : 4) : 3;
    }
    return c;
}

uint64_t tuner_key(const PlanInput& in, const Candidates& c) {
    uint64_t key = 1469598103934665603ull;
    auto mix = [&](uint64_t v) { key = (key ^ v) * 1099511628211ull; };
    uint32_t lg = 0;  // batches of similar size share a verdict
    while ((2u << lg) <= in.n_frames) ++lg;
    mix((uint64_t)in.spec); mix(in.g.columns_per_frame); mix(in.g.pixels_per_column); mix(in.g.channel_data_size); mix(lg); mix((uint64_t)in.xyzm);
    mix(in.plane_mask); mix(in.destagger_mask);
    mix((in.xyz_mask & 3u) | (in.gate_counts ? 4u : 0u) | (in.xyz_poses ? 8u : 0u));
    mix((uint64_t)c.stream_auto); mix((uint64_t)c.stream_alt);
    // the ring depth of the persistent candidates: a verdict timed on another depth is not this kernel's
    for (int tw : {c.stream_auto, c.stream_alt})
        if (tw)
            if (const auto s = plan_stream(in, tw))
                if (s->sa.nslot != 2) mix(0x100u + s->sa.nslot);
    return key;
}

const char* kernel_name(Kernel k) {
    switch (k) {
        case Kernel::WIDE: return "k_decode_wide";
        case Kernel::WIDE_RESOLVED: return "k_decode_wide_resolved";
        case Kernel::STREAM: return "k_decode_stream";     // every wave fetches
        case Kernel::STREAM2: return "k_decode_stream2";   // dedicated loader waves
        default: return "k_decode";
    }
}

static TileShape narrow_fixup_shape(const PlanInput& in, int tile) {
    return TileShape{0u, in.resident_wgs, 0u, narrow_tiles(in, tile), 0u};   // row_chunks: the persistent grid, what the device keeps resident
}

DecodePlan plan_decode(const PlanInput& in, const Candidates& c, int selected) {
    const Knobs& kn = in.kn;
    const bool fast = fast_possible(in);
    DecodePlan p;
    const NarrowPlan narrow = plan_narrow(in);
    if (!narrow.tile) return p;
    p.ok = true;
    p.narrow_tile = narrow.tile;
    p.beam_lds = narrow.beam_lds;

    auto take_wide = [&](int tw, const std::optional<TileShape>& s) {
        if (s) { p.kernel = Kernel::WIDE; p.cols = tw; p.shape = *s; }
        return s.has_value();
    };
    auto take_stream = [&](int tw) {
        const auto s = plan_stream(in, tw);
        if (s) { p.kernel = s->sa.loader ? Kernel::STREAM2 : Kernel::STREAM; p.cols = tw; p.shape = s->shape; p.sa = s->sa; }
        return s.has_value();
    };
    auto optimistic = [&](int tw) { return plan_wide(in, tw, WideKind::OPTIMISTIC); };
    if (c.small_width) {
        take_wide(c.small_width, c.small_shape);
        if (c.resolved) p.kernel = Kernel::WIDE_RESOLVED;
    } else if (c.forced_stream) {
        take_stream(c.forced_stream);
    } else if (kn.wide >= 0) {   // forced (experiments, tests)
        if (kn.wide) take_wide(kn.wide, optimistic(kn.wide));
    } else if (!fast) {
        // general mapping on wide tiles (k_slotmap first): column pieces of at least 256 B, like the persistent kernel's choice
        const auto best = prefer_256_bytes(in, optimistic);
        take_wide(best.first, best.second);
    } else if (c.n) {
        const int sel = selected;
        if (!((sel >= 1000 && take_stream(sel - 1000)) || (sel > 0 && sel < 1000 && take_wide(sel, optimistic(sel)))) && sel != 0)
            take_wide(256, optimistic(256));
    }
    if (p.kernel == Kernel::DECODE) {
        p.cols = narrow.tile;
        p.shape = TileShape{0u, 0u, 0u, narrow_tiles(in, narrow.tile), 0u};
    }
    p.xcd_map = (kn.xcd && in.n_frames >= 8) ? 1u : 0u;
    p.mode = c.resolved ? MODE_RESOLVED : fast ? MODE_FAST : MODE_GENERAL;
    const size_t map_bytes = (size_t)in.n_frames * in.g.columns_per_frame * sizeof(int32_t) * 2;   // slot_map + hdr_map
    p.slotmap = p.kernel == Kernel::WIDE && !fast;
    if (p.slotmap) p.slotmap_bytes = map_bytes;

    // The fix-up pass behind an optimistic pass: the tiles of the frames the optimistic pass flagged are looked at again
    // with the frame's real column maps and redone where those differ from "slot c holds column c".  Wide tiles
    // (fixup_crew, wide_tile.h) where the format allows them, k_decode_fixup's 64-column tiles otherwise.
    if (fast && kn.fixup && !c.resolved) {
        p.fixup = Fixup::NARROW;
        p.fix_shape = narrow_fixup_shape(in, narrow.tile);
        if (kn.fixup_wide && kn.tile == 0) {
            auto fix = [&](int tw) { return plan_wide(in, tw, WideKind::FIXUP); };
            const auto best = kn.fixup_wide > 1 ? std::make_pair(kn.fixup_wide, fix(kn.fixup_wide)) : prefer_256_bytes(in, fix);
            if (best.second) {
                p.fixup = Fixup::WIDE;
                p.fix_cols = best.first;
                p.fix_shape = *best.second;
                p.slotmap_bytes = map_bytes;
            }
        }
        if (kn.hdr_words) p.hdr_words_bytes = (size_t)in.n_frames * in.g.columns_per_frame * sizeof(uint32_t);   // the optimistic pass leaves the packed column ids
        p.fast_tiles = p.shape.tiles_per_frame;   // column tiles of the optimistic pass (slots of tile_valid)
    }
    return p;
}

void demote_fixup(const PlanInput& in, DecodePlan& p) {
    if (p.fixup != Fixup::WIDE) return;
    p.fixup = Fixup::NARROW;
    p.fix_cols = 0;
    p.fix_shape = narrow_fixup_shape(in, p.narrow_tile);
    if (!p.slotmap) p.slotmap_bytes = 0;
}

}  // namespace ouster_hip_dev
