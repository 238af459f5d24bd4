// decode_launch.hip -- the fused decode's host-side launch switches (one launcher per packet-profile specialisation lives in
// k_decode.hip / k_decode_stream.hip) and k_slotmap, the general column mapping of a whole frame.  Which of them a call
// takes is decided by decode_plan.cpp.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "kernels_common.h"
#include "launch_util.h"

namespace ouster_hip_dev {

// the decode's profile table: what ouster_hip_format_create matches a format description against (the Spec* tables of kernels_common.h)
const FieldC* spec_fields(int spec_id, int* nf, uint32_t* chan, int* r1, int* r2) {
    switch (spec_id) {
        case SPEC_DUAL_LB: *nf = SpecDualLB::nf; *chan = SpecDualLB::chan; *r1 = 0; *r2 = 4; return SpecDualLB::f;
        case SPEC_LB: *nf = SpecLB::nf; *chan = SpecLB::chan; *r1 = 0; *r2 = -1; return SpecLB::f;
        case SPEC_SINGLE: *nf = SpecSingle::nf; *chan = SpecSingle::chan; *r1 = 0; *r2 = -1; return SpecSingle::f;
        case SPEC_DUAL: *nf = SpecDual::nf; *chan = SpecDual::chan; *r1 = 0; *r2 = 3; return SpecDual::f;
        case SPEC_LEGACY: *nf = SpecLegacy::nf; *chan = SpecLegacy::chan; *r1 = 0; *r2 = -1; return SpecLegacy::f;
        default: *nf = 0; *chan = 0; *r1 = *r2 = -1; return nullptr;
    }
}

#define OUSTER_DECL_SPEC(sfx)                                                                             \
    hipError_t launch_decode_##sfx(const DecodeArgs& a, int tile, int xyzm, int device, hipStream_t st); \
    hipError_t launch_decode_wide_##sfx(const DecodeArgs& a, int tw, int xyzm, int device, hipStream_t st, uint32_t resident);
OUSTER_DECL_SPEC(generic)
OUSTER_DECL_SPEC(dual_lb)
OUSTER_DECL_SPEC(lb)
OUSTER_DECL_SPEC(single)
OUSTER_DECL_SPEC(dual)
OUSTER_DECL_SPEC(legacy)
#undef OUSTER_DECL_SPEC

hipError_t launch_decode(const DecodeArgs& a, int spec_id, int tile, int xyzm, int device, hipStream_t st) {
    switch (spec_id) {
        case SPEC_DUAL_LB: return launch_decode_dual_lb(a, tile, xyzm, device, st);
        case SPEC_LB: return launch_decode_lb(a, tile, xyzm, device, st);
        case SPEC_SINGLE: return launch_decode_single(a, tile, xyzm, device, st);
        case SPEC_DUAL: return launch_decode_dual(a, tile, xyzm, device, st);
        case SPEC_LEGACY: return launch_decode_legacy(a, tile, xyzm, device, st);
        default: return launch_decode_generic(a, tile, xyzm, device, st);
    }
}

hipError_t launch_decode_wide(const DecodeArgs& a, int spec_id, int tw, int xyzm, int device, hipStream_t st, uint32_t resident) {
    switch (spec_id) {
        case SPEC_DUAL_LB: return launch_decode_wide_dual_lb(a, tw, xyzm, device, st, resident);
        case SPEC_LB: return launch_decode_wide_lb(a, tw, xyzm, device, st, resident);
        case SPEC_SINGLE: return launch_decode_wide_single(a, tw, xyzm, device, st, resident);
        case SPEC_DUAL: return launch_decode_wide_dual(a, tw, xyzm, device, st, resident);
        case SPEC_LEGACY: return launch_decode_wide_legacy(a, tw, xyzm, device, st, resident);
        default: return launch_decode_wide_generic(a, tw, xyzm, device, st, resident);
    }
}

#define OUSTER_DECL_STREAM(sfx) \
    hipError_t launch_decode_stream_##sfx(const DecodeArgs& a, const StreamArgs& sp, int tw, int xyzm, int device, hipStream_t st);
OUSTER_DECL_STREAM(dual_lb)
OUSTER_DECL_STREAM(lb)
OUSTER_DECL_STREAM(single)
OUSTER_DECL_STREAM(dual)
OUSTER_DECL_STREAM(legacy)
#undef OUSTER_DECL_STREAM

hipError_t launch_decode_stream(const DecodeArgs& a, const StreamArgs& sp, int spec_id, int tw, int xyzm, int device,
                                hipStream_t st) {
    switch (spec_id) {
        case SPEC_DUAL_LB: return launch_decode_stream_dual_lb(a, sp, tw, xyzm, device, st);
        case SPEC_LB: return launch_decode_stream_lb(a, sp, tw, xyzm, device, st);
        case SPEC_SINGLE: return launch_decode_stream_single(a, sp, tw, xyzm, device, st);
        case SPEC_DUAL: return launch_decode_stream_dual(a, sp, tw, xyzm, device, st);
        case SPEC_LEGACY: return launch_decode_stream_legacy(a, sp, tw, xyzm, device, st);
        default: return hipErrorInvalidValue;   // run-time descriptors stay on k_decode / k_decode_wide
    }
}

// ------------------------------------------------------------------------------------
// k_slotmap: the general column mapping of a whole frame, once (one workgroup per frame) -- for buffers that do not have
// one slot per column of the frame (compacted after drops, any order, duplicates), where round 2 let EVERY 64-column tile
// of k_decode scan the frame's column headers.  resolve_frame (kernels_common.h) restates what FrameBatcher leaves behind
// after batching the frame's packets in buffer order, block path and column path alike
// (ouster_core/src/lidar_frame.cpp:1422-1576): per destination column the slot that supplies its pixels (slot_map) and the
// slot that supplies its header (hdr_map; the two differ only for an all-valid packet whose ids are not consecutive).
// Also everything the general path's tile 0 used to resolve: packet-level outputs (batch_lidar_packet :1534-1539), the
// frame-level values (start_frame :1709-1741, from the first packet of the buffer) and the valid-column count.
// k_decode_wide then decodes from the maps.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_slotmap(DecodeArgs a) {
    constexpr int NT = 256;
    extern __shared__ __align__(16) uint32_t smem[];
    __shared__ uint32_t s_n;
    const uint32_t f = blockIdx.x, tid = threadIdx.x;
    const uint32_t W = a.g.columns_per_frame, npo = a.n_packets_out;
    const uint8_t* fbase = a.packets + (size_t)f * a.slots_per_frame * a.packet_stride;
    uint32_t count = a.slots_per_frame;
    if (a.packet_counts) count = min(a.packet_counts[f], a.slots_per_frame);
    const ResolveLds L(smem, W, npo, a.slots_per_frame);
    int32_t *s_pix = L.pix, *s_hdr = L.hdr, *s_pkm = L.pkm;
    if (tid == 0) s_n = 0;
    resolve_frame<NT>(a.g, fbase, a.packet_stride, count, npo, L, true);
    uint32_t n = 0;
    for (uint32_t i = tid; i < W; i += NT) {
        const int32_t h = s_hdr[i];
        a.slot_map[(size_t)f * W + i] = s_pix[i];
        a.hdr_map[(size_t)f * W + i] = h;
        n += h >= 0 ? 1u : 0u;
    }
    n = wave_sum(n);
    if (n && (tid & 63u) == 0) atomicAdd(&s_n, n);
    // packet_timestamp is zeroed at frame start (lidar_frame.cpp:1719), alert_flags is not
    for (uint32_t i = tid; i < npo; i += NT) {
        const int32_t p = s_pkm[i];
        if (a.packet_timestamp && a.host_timestamps)
            a.packet_timestamp[(size_t)f * npo + i] = p >= 0 ? a.host_timestamps[(size_t)f * a.slots_per_frame + p] : 0ull;
        if (a.alert_flags && p >= 0)
            a.alert_flags[(size_t)f * npo + i] = (uint8_t)apply_bits(
                window_global(fbase + (size_t)p * a.packet_stride + a.g.alert_flags.offset), a.g.alert_flags.mask, a.g.alert_flags.shift);
    }
    __syncthreads();
    if (tid == 0 && a.frame_meta) {
        ouster_hip_frame_meta m = frame_meta_general(a, fbase, count);
        m.n_valid_columns = s_n;
        a.frame_meta[f] = m;
    }
}

hipError_t launch_slotmap(const DecodeArgs& a, int device, hipStream_t st) {
    const size_t lds = slotmap_lds_bytes(a.g.columns_per_frame, a.g.columns_per_packet, a.slots_per_frame);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    static LdsGrant grant;
    return launch_with_lds(k_slotmap, dim3(a.n_frames), dim3(256), lds, device, st, grant, a);
}

}  // namespace ouster_hip_dev
