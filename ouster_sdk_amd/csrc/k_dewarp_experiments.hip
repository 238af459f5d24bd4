// k_dewarp_experiments.hip -- the measured-slower forms of the range-gated frame dewarp, kept for A/B work (gfx950):
//
//   k_dwf_emit_stream     k_dwf_emit as a persistent kernel with a loader wave (knob "dwf_stream")
//   k_dwf_single / _fused the whole frame dewarp in one pass over the range planes (knob "dewarp_single_pass")
// and the two launch hooks launch_dewarp_frames (k_dewarp.hip) calls.  Compiled and linked only with make EXPERIMENTS=1.
#ifndef OUSTER_EXPERIMENTS
#error "k_dewarp_experiments.hip belongs to an EXPERIMENTS=1 build (-DOUSTER_EXPERIMENTS) only"
#endif
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdint.h>

#include "dwf_dev.h"
#include "kernels_common.h"
#include "launch_util.h"

namespace ouster_hip_dev {

// ------------------------------------------------------------------------------------
// k_dwf_emit_stream: k_dwf_emit as a PERSISTENT kernel with a loader wave (round 6; k_decode_stream2's skeleton).
// k_dwf_emit's time is the sum of its read side and its write side (0.127 ms without the stores, 0.19 with them, 256 frames):
// a workgroup asks for its 32 KB range tile, waits, and only then computes and stores, and four such workgroups per CU do not
// hide one another's wait behind a saturated memory system.  Here two workgroups per CU live for the whole launch and walk
// the (frame, column tile) list; each has TWO tile contexts in LDS: while eight waves rank, project and store tile i, the
// ninth has tile i+1 arriving by LDS-DMA (global_load_lds_dwordx4: no VGPR round trip; nothing for the column loop to wait on) and
// writes its column metadata.  One workgroup barrier per tile.  Same outputs, order and arithmetic as k_dwf_emit.
// Needs whole tiles (W % 64 == 0), ROWS == H, 16 B aligned range planes and the separable tables; anything else: k_dwf_emit.
// MEASURED (round 6, 256 frames of 128 x 2048, same box, same process): bit-identical output, 0.2173 ms for the chain against
// 0.2143 ms with k_dwf_emit -- hiding the tile's read latency buys nothing, so the emit kernel's time is NOT the sum of an
// exposed read side and a write side (the reading of DESIGN r05 section 10.2); 94 VGPRs, 2 x 79 KB of LDS, 18 waves per CU.
// Kept for A/B work only (make EXPERIMENTS=1, knob "dwf_stream" = 1); a default build does not compile it.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void dwf_glds16(const void* g, uint32_t lds) {   // one LDS-DMA wave instruction (k_decode_stream.hip: glds16)
    uint32_t keep;
    lds = __builtin_amdgcn_readfirstlane(lds);
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(g), "s"(lds) : "memory");
}
struct __attribute__((aligned(16))) DwfTileHdr {
    uint64_t fbase;
    uint32_t f, c0, any, easy, pad0, pad1;
};
template <class T, int ROWS>
constexpr uint32_t dwf_stream_ctx_bytes() { return (uint32_t)(ROWS * 64 * 4 + 64 * sizeof(DwfColMeta<T>) + sizeof(DwfTileHdr)); }

template <class T, int ROWS>
__global__ __launch_bounds__(576, 2) void k_dwf_emit_stream(DewarpFramesArgs a, uint32_t n_items) {
    constexpr int TILE = 64, NCW = 8, NR = ROWS / 64;
    constexpr uint32_t RNG_BYTES = ROWS * TILE * 4, META_BYTES = TILE * sizeof(DwfColMeta<T>), CTX = dwf_stream_ctx_bytes<T, ROWS>();
    extern __shared__ __align__(16) uint32_t smem[];
    const uint32_t W = a.w, H = a.h, tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t tiles = W / TILE;
    const uint32_t G = gridDim.x;
    if (blockIdx.x >= n_items) return;
    const uint32_t n_mine = (n_items - blockIdx.x + G - 1) / G;
    auto item = [&](uint32_t i) { return blockIdx.x + G * i; };
    auto ctx_rng = [&](uint32_t b) { return (uint32_t*)((uint8_t*)smem + b * CTX); };
    auto ctx_meta = [&](uint32_t b) { return (DwfColMeta<T>*)((uint8_t*)smem + b * CTX + RNG_BYTES); };
    auto ctx_hdr = [&](uint32_t b) { return (DwfTileHdr*)((uint8_t*)smem + b * CTX + RNG_BYTES + META_BYTES); };

    if (wave >= (uint32_t)NCW) {
        // ================= the loader wave: lane = column of the tile for the metadata, 16 B cell for the ranges =================
        const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
        auto fetch = [&](uint32_t it, uint32_t b) {
            const uint32_t f = it / tiles, c0 = (it - f * tiles) * TILE;
            const uint32_t* off = a.col_off + (size_t)f * (W + 1);
            const uint32_t mx = c0 + lane;
            const uint32_t base = off[mx], next = off[mx + 1];
            const uint32_t first = __builtin_amdgcn_readfirstlane(base), last = (uint32_t)__builtin_amdgcn_readlane((int)next, 63);
            const bool any = last != first;
            const uint64_t fbase = a.frame_off[f];
            if (any) {
                // ranges: instruction k brings rows 4k..4k+3; lane l -> row 4k + l/16, LDS cell l%16, i.e. columns 4*(cell ^ (row & 15))..
                const uint8_t* rp = (const uint8_t*)(a.range + (size_t)f * W * H) + (size_t)c0 * 4;
                const uint32_t r_in = lane >> 4, cell = lane & 15u;
#pragma unroll 8
                for (uint32_t k = 0; k < (uint32_t)ROWS / 4u; ++k) {
                    const uint32_t r = 4u * k + r_in;
                    dwf_glds16(rp + (size_t)r * W * 4 + ((cell ^ (r & 15u)) << 4), lds0 + b * CTX + k * 1024u);
                }
            }
            DwfColMeta<T> m;
#pragma unroll
            for (int k = 0; k < 12; ++k) m.pose[k] = (T)0;
#pragma unroll
            for (int k = 0; k < 5; ++k) m.col[k] = 0.0;
            m.base = base;
            m.cnt = next - base;
            m.ts = 0;
            if (m.cnt) {
                load_pose_rows<T>(a, (size_t)f * W + mx, m.pose);
                const LutDev* lp = a.luts + f % a.n_luts;
                const double* ct = lp->col_tab;
#pragma unroll
                for (int k = 0; k < 5; ++k) m.col[k] = as_global(ct)[(size_t)mx * 5 + k];
                if (a.timestamps_ns) m.ts = a.timestamp[(size_t)f * W + mx];
            }
            ctx_meta(b)[lane] = m;
            if (lane == 0) {
                DwfTileHdr h;
                h.fbase = fbase; h.f = f; h.c0 = c0; h.any = any ? 1u : 0u;
                h.easy = (fbase + last <= a.capacity && a.min_r > 0) ? 1u : 0u;
                h.pad0 = h.pad1 = 0;
                *ctx_hdr(b) = h;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the tile has landed (this wave's queue holds nothing else)
        };
        fetch(item(0), 0);
        for (uint32_t i = 0; i < n_mine; ++i) {
            __syncthreads();   // tile i is in its context; the other one is free (the column loops are done with tile i-1)
            if (i + 1 < n_mine) fetch(item(i + 1), (i + 1) & 1u);
        }
        return;
    }

    // ================= the eight column-loop waves: wave = 8 columns of the tile, lane = row =================
    uint32_t row[NR];
    double bt[NR][9];
    uint32_t cur_lut = 0xffffffffu;
    LutDev lut{};
#pragma unroll
    for (int hh = 0; hh < NR; ++hh) row[hh] = lane + 64 * hh;
    for (uint32_t i = 0; i < n_mine; ++i) {
        const uint32_t b = i & 1u;
        __syncthreads();
        const DwfTileHdr h = *ctx_hdr(b);
        if (!h.any) continue;
        const uint32_t li = h.f % a.n_luts;
        if (li != cur_lut) {   // the lane's rows of the beam table: once per launch for a one-sensor batch
            cur_lut = li;
            lut = a.luts[li];
#pragma unroll
            for (int hh = 0; hh < NR; ++hh)
#pragma unroll
                for (int k = 0; k < 9; ++k) bt[hh][k] = as_global(lut.beam_tab)[(size_t)min(row[hh], H - 1u) * 9 + k];
        }
        uint32_t m_run = 0;
        if (h.easy) dwf_column_loop<T, true, TILE, ROWS, true, NCW, true>(a, lut, ctx_rng(b), ctx_meta(b), h.f, h.c0, TILE, h.fbase, row, bt, m_run);
        else dwf_column_loop<T, true, TILE, ROWS, false, NCW, true>(a, lut, ctx_rng(b), ctx_meta(b), h.f, h.c0, TILE, h.fbase, row, bt, m_run);
    }
}

// the two single-pass forms of the frame dewarp: measured slower than count / scan / emit (DESIGN_HISTORY.md H3);
// out of the default build since round 6 (make EXPERIMENTS=1)
// ------------------------------------------------------------------------------------
// k_dwf_single: the same range-gated, compacting frame dewarp in ONE pass over the range planes.
// A workgroup owns a 64-column tile of one frame for ALL rows (H x 65 dwords of LDS), counts the kept
// points of its columns from LDS, and learns where its output starts from a decoupled look-back over
// the tiles before it (Merrill & Garland: every tile publishes {aggregate | inclusive prefix} in one
// 64-bit word; a wave inspects 64 predecessors per step).  Tiles take their index from ticket
// counters -- eight of them, one per blockIdx & 7 class (tile = 8 * ticket + class): a single counter
// serialises 8192 returning atomics (~90 us measured), eight run side by side.  Within a class a tile's
// predecessors have always started; across classes that holds because workgroups are dispatched in
// index order (a class would have to fall > 1000 workgroups behind the others for a wait to stall).  Output order, counts and provenance are exactly k_dwf_count/scan/emit's (= the reference's,
// impl/dewarp_impl.h:23-115); the range plane is read once instead of twice and three launches
// disappear.
//   tile_state[16 * c]   ticket counter of class c, c < 8  (the buffer is zeroed before the launch)
//   tile_state[128 + t]  [63:62] 0 nothing / 1 aggregate / 2 inclusive prefix, [61:0] points
// ------------------------------------------------------------------------------------
#ifndef OUSTER_DWF_NT
#define OUSTER_DWF_NT 256
#endif
constexpr int DWF_NT = OUSTER_DWF_NT;  // threads per tile of k_dwf_single
constexpr uint32_t DWF_WORDS = 128;  // tile words start behind the eight padded ticket counters
constexpr uint64_t DWF_AGG = 1ull << 62, DWF_INC = 2ull << 62, DWF_VAL = (1ull << 62) - 1;

// NT threads share one tile.  Measured (256 frames 128x2048, gate 0.5-400 m, same box): NT 256 0.428 ms,
// 512 0.500 ms, 1024 0.698 ms against 0.344 ms for the count / scan / emit kernels -- the emit loop is
// instruction bound (rocprofv3 --pmc: ~2600 VALU + ~1600 SALU per wave, the v_readlane broadcasts of the
// column metadata), and the whole-column tile (33 KB of LDS) halves the waves per CU that hide it; the
// range plane read it saves (65-75 us of k_dwf_count) does not pay for that.  Kept behind the
// "dewarp_single_pass" knob for sensors of more than 128 beams (k_dwf_fused below serves the others); the three kernels
// stay the default.
template <class T, bool SEP, int NT>
__global__ __launch_bounds__(NT) void k_dwf_single(DewarpFramesArgs a) {
    constexpr int TILE = 64, PITCH = TILE + 1, LPR = 16, RPP = NT / LPR, CPW = TILE / (NT / 64);
    extern __shared__ __align__(16) uint32_t s_rng[];   // [H][PITCH]
    __shared__ uint32_t s_cnt[TILE], s_ticket;
    __shared__ int s_lo, s_hi;
    __shared__ uint64_t s_base;
    const uint32_t W = a.w, H = a.h, tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t tiles = (W + TILE - 1) / TILE;
    if (tid == 0) {
        const uint32_t cls = blockIdx.x & 7u;
        s_ticket = (uint32_t)atomicAdd((unsigned long long*)&a.tile_state[16 * cls], 1ull) * 8u + cls;
        s_lo = 0x7fffffff;
        s_hi = -1;
    }
    if (tid < TILE) s_cnt[tid] = 0;
    __syncthreads();
    const uint32_t t = s_ticket, f = t / tiles, tile = t - f * tiles;
    const uint32_t c0 = tile * TILE, ncol = min((uint32_t)TILE, W - c0);
    const uint32_t* rp = a.range + (size_t)f * W * H;
    const uint32_t* st = a.status + (size_t)f * W;
    const LutDev lut = a.luts[f % a.n_luts];
    const bool vec = (W % 4 == 0) && ((((uintptr_t)a.range) & 15) == 0);

    // ---- first / last valid column of the frame (status & 1, lidar_frame.cpp:907-925)
    {
        int lo = 0x7fffffff, hi = -1;
        for (uint32_t x = tid; x < W; x += NT)
            if (st[x] & 1u) { lo = min(lo, (int)x); hi = max(hi, (int)x); }
        if (hi >= 0) { atomicMin(&s_lo, lo); atomicMax(&s_hi, hi); }
    }
    // ---- stage the tile's range values, all rows, coalesced row segments
    {
        const uint32_t q = tid % LPR, ty = tid / LPR, col = c0 + 4 * q;
        for (uint32_t r = ty; r < H; r += RPP) {
            uint32_t v[4] = {0, 0, 0, 0};
            if (col < W) {
                if (vec) {
                    const uint4 x = *(const uint4*)(rp + (size_t)r * W + col);
                    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
                } else {
                    for (uint32_t c = 0; c < 4 && col + c < W; ++c) v[c] = rp[(size_t)r * W + col + c];
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) s_rng[r * PITCH + 4 * q + c] = v[c];
        }
    }
    __syncthreads();
    const int lo = s_lo, hi = s_hi;

    // ---- column metadata: lane l of the wave holds column wave*CPW + l % CPW
    const uint32_t ml = lane % CPW, mj = wave * CPW + ml, mx = c0 + mj;
    const bool col_on = mj < ncol && (int)mx >= lo && (int)mx <= hi && st[mx] != 0;
    // kept points per column: wave = 16 columns, lane = row
    for (uint32_t jj = 0; jj < (uint32_t)CPW; ++jj) {
        const uint32_t j = wave * CPW + jj;
        if (j >= ncol) break;
        uint32_t n = 0;
        for (uint32_t r0 = 0; r0 < H; r0 += 64) {
            const uint32_t row = r0 + lane;
            const uint32_t r = row < H ? s_rng[row * PITCH + j] : 0u;
            n += (uint32_t)__popcll(__ballot(row < H && r >= a.min_r && r <= a.max_r));
        }
        if (lane == jj) s_cnt[j] = n;   // lane jj is the metadata lane of column j (ml == jj)
    }
    __syncthreads();
    // exclusive scan of the 64 column counts (masked), by every wave for itself
    uint32_t m_cnt = 0, m_base = 0, tile_total = 0;
    {
        const uint32_t jx = lane;  // column of the tile
        const bool on = jx < ncol && (int)(c0 + jx) >= lo && (int)(c0 + jx) <= hi && st[min(c0 + jx, W - 1)] != 0;
        const uint32_t v = on ? s_cnt[jx] : 0u;
        uint32_t inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(inc, d, 64);
            if (lane >= (uint32_t)d) inc += up;
        }
        tile_total = __shfl(inc, 63, 64);
        const uint32_t ex = inc - v;
        // hand column mj's numbers to its metadata lane
        m_base = __shfl(ex, (int)mj, 64);
        m_cnt = __shfl(v, (int)mj, 64);
        if (!col_on) m_cnt = 0;
    }

    // ---- where does this tile's output start?  publish, then look back (wave 0)
    if (wave == 0) {
        uint64_t excl = 0;
        unsigned long long* my = (unsigned long long*)&a.tile_state[DWF_WORDS + t];
        if (t == 0) {
            if (lane == 0) __hip_atomic_store(my, DWF_INC | (uint64_t)tile_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            if (lane == 0) __hip_atomic_store(my, DWF_AGG | (uint64_t)tile_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int64_t back = (int64_t)t - 1;        // nearest predecessor not yet accounted for
            while (true) {
                const int64_t i = back - (int64_t)lane;
                uint64_t w = DWF_INC;             // lanes before the first tile: a zero inclusive prefix
                if (i >= 0) {
                    do {
                        w = __hip_atomic_load((unsigned long long*)&a.tile_state[DWF_WORDS + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    } while ((w >> 62) == 0);
                }
                const uint64_t inc_mask = __ballot((w >> 62) == 2);
                const uint32_t first_inc = inc_mask ? (uint32_t)__builtin_ctzll(inc_mask) : 64u;
                uint64_t part = lane <= first_inc ? (w & DWF_VAL) : 0ull;   // aggregates up to (incl.) the first inclusive word
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) part += __shfl_xor(part, d, 64);
                excl += part;
                if (first_inc < 64u) break;
                back -= 64;
            }
            if (lane == 0) __hip_atomic_store(my, DWF_INC | (excl + tile_total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane == 0) {
            s_base = excl;
            if (tile == 0) a.frame_off[f] = excl;
            if (t + 1 == a.n_frames * tiles) a.frame_off[a.n_frames] = excl + tile_total;
        }
    }
    __syncthreads();
    const uint64_t fbase = s_base;
    if (tile_total == 0) return;

    // ---- emit (as k_dwf_emit, from the resident tile)
    uint64_t m_ts = 0;
    T m_pose[12];
    double m_col[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 12; ++k) m_pose[k] = (T)0;
    if (m_cnt) {
        const double* pm = a.poses + ((size_t)f * W + mx) * 16;
#pragma unroll
        for (int k = 0; k < 12; ++k) m_pose[k] = (T)pm[k];
        if constexpr (SEP) {
#pragma unroll
            for (int k = 0; k < 5; ++k) m_col[k] = lut.col_tab[(size_t)mx * 5 + k];
        }
        if (a.timestamps_ns) m_ts = a.timestamp[(size_t)f * W + mx];
    }
    uint32_t m_run = 0;  // points of my column already written (previous row chunks)
    for (uint32_t r0 = 0; r0 < H; r0 += 64) {
        const uint32_t row = r0 + lane;
        double bt[9];
        if constexpr (SEP) {
#pragma unroll
            for (int k = 0; k < 9; ++k) bt[k] = row < H ? lut.beam_tab[(size_t)row * 9 + k] : 0.0;
        }
        for (uint32_t jj = 0; jj < (uint32_t)CPW; ++jj) {
            const uint32_t j = wave * CPW + jj, x = c0 + j;  // wave-uniform
            if (j >= ncol) break;
            if (bcast_u32(m_cnt, jj) == 0) continue;  // masked out or empty column
            const uint32_t r = row < H ? s_rng[row * PITCH + j] : 0u;
            const bool keep = row < H && r >= a.min_r && r <= a.max_r;
            const uint64_t mask = __ballot(keep);
            const uint32_t n_keep = (uint32_t)__popcll(mask);
            if (n_keep == 0) continue;
            const uint32_t rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            const uint64_t g0 = fbase + bcast_u32(m_base, jj) + bcast_u32(m_run, jj);  // first point of this run
            const uint64_t room = g0 < a.capacity ? a.capacity - g0 : 0;
            if (keep && rank < room) {
                double p[3];
                if constexpr (SEP) {
                    const double cx = bcast(m_col[0], jj), sx = bcast(m_col[1], jj);
                    const double rm = (double)r - lut.n;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const double d = fma(cx, bt[k], fma(sx, bt[3 + k], bt[6 + k]));
                        p[k] = r ? fma(rm, d, bcast(m_col[2 + k], jj)) : 0.0;
                    }
                } else {
                    const size_t pix = (size_t)row * W + x;
                    if (lut.full_dtype == OUSTER_HIP_F32)
                        project_full<float>((const float*)lut.full_dir, (const float*)lut.full_ofs, pix, r, p);
                    else
                        project_full<double>((const double*)lut.full_dir, (const double*)lut.full_ofs, pix, r, p);
                }
                const T px = (T)p[0], py = (T)p[1], pz = (T)p[2];
                Pt3<T> o;
                // the same three nested FMAs per component as k_dwf_emit (the two routes agree bit for bit)
                o.x = fma(bcast(m_pose[0], jj), px, fma(bcast(m_pose[1], jj), py, fma(bcast(m_pose[2], jj), pz, bcast(m_pose[3], jj))));
                o.y = fma(bcast(m_pose[4], jj), px, fma(bcast(m_pose[5], jj), py, fma(bcast(m_pose[6], jj), pz, bcast(m_pose[7], jj))));
                o.z = fma(bcast(m_pose[8], jj), px, fma(bcast(m_pose[9], jj), py, fma(bcast(m_pose[10], jj), pz, bcast(m_pose[11], jj))));
                ((Pt3<T>*)a.points)[g0 + rank] = o;
            }
            if (a.col_idxs || a.frame_idxs || a.timestamps_ns) {
                const uint64_t ts = (uint64_t)bcast_u32((uint32_t)m_ts, jj) |
                                    ((uint64_t)bcast_u32((uint32_t)(m_ts >> 32), jj) << 32);
                for (uint32_t i = lane; i < n_keep && i < room; i += 64) {
                    if (a.col_idxs) a.col_idxs[g0 + i] = x;
                    if (a.frame_idxs) a.frame_idxs[g0 + i] = f;
                    if (a.timestamps_ns) a.timestamps_ns[g0 + i] = ts;
                }
            }
            if (ml == jj) m_run += n_keep;
        }
    }
}

// ------------------------------------------------------------------------------------
// k_dwf_fused: the single-pass dewarp for sensors of up to 128 beams, rebuilt on k_dwf_emit's tile (64 columns x all
// rows in LDS, column metadata in LDS, dwf_column_loop) -- k_dwf_single above keeps every row count but walks memory the
// slow way (a guarded status scan per tile, guarded staging, metadata in lanes).  Per tile:
//   1. ticket -> (frame, tile); EVERY global read of the prologue is issued at once from clamped addresses: the frame's
//      status words (first / last valid column), the tile's range pieces, the 64 columns' poses / table rows / timestamps;
//   2. LDS: ranges, metadata; per-column kept counts from LDS (wave = 16 columns, lane = row);
//   3. wave 0: masked exclusive scan of the 64 counts -> column bases; publish the tile total; decoupled look-back;
//   4. dwf_column_loop with fbase = the tile's global start.
// Output, order and provenance are those of k_dwf_count / scan / emit.
// ------------------------------------------------------------------------------------
template <class T, bool SEP, int ROWS>
__global__ __launch_bounds__(256) void k_dwf_fused(DewarpFramesArgs a) {
    constexpr int TILE = 64, LPR = TILE / 4, PITCH = TILE + 1, CPW = TILE / 4, NR = ROWS / 64, RPP = 256 / LPR, NP = ROWS / RPP;
    constexpr uint32_t SEG = 8;
    __shared__ uint32_t s_rng[ROWS * PITCH];
    __shared__ DwfColMeta<T> s_meta[TILE];
    __shared__ uint32_t s_cnt[TILE], s_ticket, s_total;
    __shared__ int s_lo, s_hi;
    __shared__ uint64_t s_base;
    const uint32_t W = a.w, H = a.h, tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t q = tid % LPR, ty = tid / LPR;
    const uint32_t tiles = (W + TILE - 1) / TILE;
    if (tid == 0) {
        const uint32_t cls = blockIdx.x & 7u;
        s_ticket = (uint32_t)atomicAdd((unsigned long long*)&a.tile_state[16 * cls], 1ull) * 8u + cls;
        s_lo = 0x7fffffff;
        s_hi = -1;
    }
    __syncthreads();
    const uint32_t t = s_ticket, f = t / tiles, tile = t - f * tiles;
    const uint32_t c0 = tile * TILE, ncol = min((uint32_t)TILE, W - c0);
    const uint32_t* rp = a.range + (size_t)f * W * H;
    const uint32_t* st = a.status + (size_t)f * W;
    const LutDev lut = a.luts[f % a.n_luts];
    const bool vec = (W % 4 == 0) && ((((uintptr_t)a.range) & 15) == 0);

    // ---- 1. the prologue's reads
    uint4 tp[NP];
    if (vec) {
        const uint32_t cc = min(c0 + 4 * q, W - 4u);
#pragma unroll
        for (int i = 0; i < NP; ++i) tp[i] = *(const uint4*)(rp + (size_t)min(ty + (uint32_t)i * RPP, H - 1u) * W + cc);
    }
    DwfColMeta<T> m;
    uint32_t my_status = 0;
    if (tid < (uint32_t)TILE) {
        const uint32_t mx = min(c0 + tid, W - 1u);
        const double* pm = a.poses + ((size_t)f * W + mx) * 16;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            m.pose[2 * k] = (T)pm[k];
            m.pose[2 * k + 1] = (T)pm[4 + k];
            m.pose[8 + k] = (T)pm[8 + k];
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) m.col[k] = SEP ? as_global(lut.col_tab)[(size_t)mx * 5 + k] : 0.0;
        m.ts = a.timestamps_ns ? a.timestamp[(size_t)f * W + mx] : 0;
        m.base = m.cnt = 0;
        my_status = st[mx];
    }
    {
        int lo = 0x7fffffff, hi = -1;
        for (uint32_t base = 0; base < W; base += 256u * SEG) {
            uint32_t v[SEG];
#pragma unroll
            for (uint32_t k = 0; k < SEG; ++k) v[k] = st[min(base + tid + 256u * k, W - 1u)];
#pragma unroll
            for (uint32_t k = 0; k < SEG; ++k) {
                const uint32_t x = base + tid + 256u * k;
                if (x < W && (v[k] & 1u)) { lo = min(lo, (int)x); hi = max(hi, (int)x); }
            }
        }
        if (hi >= 0) { atomicMin(&s_lo, lo); atomicMax(&s_hi, hi); }
    }
    // ---- 2. LDS image of the tile and its metadata
    if (vec) {
        const uint32_t col = c0 + 4 * q;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const uint32_t rr = ty + (uint32_t)i * RPP;
            const bool in = rr < H && col < W;
            uint32_t* d = &s_rng[rr * PITCH + 4 * q];
            d[0] = in ? tp[i].x : 0u; d[1] = in ? tp[i].y : 0u; d[2] = in ? tp[i].z : 0u; d[3] = in ? tp[i].w : 0u;
        }
    } else {
        for (uint32_t rr = ty; rr < (uint32_t)ROWS; rr += RPP) {
            const uint32_t col = c0 + 4 * q;
            uint32_t v[4] = {0, 0, 0, 0};
            if (rr < H)
                for (uint32_t c = 0; c < 4 && col + c < W; ++c) v[c] = rp[(size_t)rr * W + col + c];
#pragma unroll
            for (int c = 0; c < 4; ++c) s_rng[rr * PITCH + 4 * q + c] = v[c];
        }
    }
    if (tid < (uint32_t)TILE) {
        m.cnt = (tid < ncol && my_status != 0) ? 1u : 0u;   // for now: "this column may emit"; the count follows
        s_meta[tid] = m;
    }
    // the lane's rows of the beam table (L2 hits), asked for before the counting pass needs nothing from memory
    uint32_t row[NR];
    double bt[NR][9];
#pragma unroll
    for (int hh = 0; hh < NR; ++hh) {
        row[hh] = lane + 64 * hh;
        if constexpr (SEP) {
            const uint32_t rc = min(row[hh], H - 1u);
#pragma unroll
            for (int k = 0; k < 9; ++k) bt[hh][k] = as_global(lut.beam_tab)[(size_t)rc * 9 + k];
        }
    }
    __syncthreads();
    const int lo = s_lo, hi = s_hi;
    // kept points per column: wave = 16 columns, lane = row; lane jj ends up with column jj's count
    {
        uint32_t mine = 0;
        for (uint32_t jj = 0; jj < (uint32_t)CPW; ++jj) {
            const uint32_t j = wave * CPW + jj;
            uint32_t n = 0;
#pragma unroll
            for (int hh = 0; hh < NR; ++hh) {
                const uint32_t r = s_rng[(lane + 64 * hh) * PITCH + min(j, (uint32_t)TILE - 1u)];
                n += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(row[hh] < H && r >= a.min_r && r <= a.max_r));
            }
            if (lane == jj) mine = n;
        }
        if (lane < (uint32_t)CPW) s_cnt[wave * CPW + lane] = mine;
    }
    __syncthreads();
    // ---- 3. column bases inside the tile, then where the tile starts (wave 0)
    if (wave == 0) {
        const uint32_t jx = lane;
        const bool on = jx < ncol && (int)(c0 + jx) >= lo && (int)(c0 + jx) <= hi && s_meta[jx].cnt != 0;
        const uint32_t v = on ? s_cnt[jx] : 0u;
        uint32_t inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(inc, d, 64);
            if (lane >= (uint32_t)d) inc += up;
        }
        const uint32_t tile_total = __shfl(inc, 63, 64);
        s_meta[jx].base = inc - v;
        s_meta[jx].cnt = v;
        uint64_t excl = 0;
        unsigned long long* my = (unsigned long long*)&a.tile_state[DWF_WORDS + t];
        if (t == 0) {
            if (lane == 0) __hip_atomic_store(my, DWF_INC | (uint64_t)tile_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            if (lane == 0) __hip_atomic_store(my, DWF_AGG | (uint64_t)tile_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int64_t back = (int64_t)t - 1;        // nearest predecessor not yet accounted for
            // (asking for four windows of predecessors per step instead of one was tried: slower, 0.245 -> 0.259 ms; the wait is
            // for the slowest prologue among the few hundred tiles that started just before this one, not for the steps)
            while (true) {
                const int64_t i = back - (int64_t)lane;
                uint64_t w = DWF_INC;             // lanes before the first tile: a zero inclusive prefix
                if (i >= 0) {
                    do {
                        w = __hip_atomic_load((unsigned long long*)&a.tile_state[DWF_WORDS + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    } while ((w >> 62) == 0);
                }
                const uint64_t inc_mask = __ballot((w >> 62) == 2);
                const uint32_t first_inc = inc_mask ? (uint32_t)__builtin_ctzll(inc_mask) : 64u;
                uint64_t part = lane <= first_inc ? (w & DWF_VAL) : 0ull;   // aggregates up to (incl.) the first inclusive word
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) part += __shfl_xor(part, d, 64);
                excl += part;
                if (first_inc < 64u) break;
                back -= 64;
            }
            if (lane == 0) __hip_atomic_store(my, DWF_INC | (excl + tile_total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane == 0) {
            s_base = excl;
            s_total = tile_total;
            if (tile == 0) a.frame_off[f] = excl;
            if (t + 1 == a.n_frames * tiles) a.frame_off[a.n_frames] = excl + tile_total;
        }
    }
    __syncthreads();
    const uint64_t fbase = s_base;
    const uint32_t tile_total = s_total;
    if (tile_total == 0) return;
    // ---- 4. emit
    uint32_t m_run = 0;
    if (fbase + tile_total <= a.capacity && a.min_r > 0)
        dwf_column_loop<T, SEP, TILE, ROWS, true>(a, lut, s_rng, s_meta, f, c0, ncol, fbase, row, bt, m_run);
    else
        dwf_column_loop<T, SEP, TILE, ROWS, false>(a, lut, s_rng, s_meta, f, c0, ncol, fbase, row, bt, m_run);
}

// ------------------------------------------------------------------------------------
// launch hooks (host): called by launch_dewarp_frames, declared in dwf_dev.h
// ------------------------------------------------------------------------------------
bool launch_dwf_single_pass(const DewarpFramesArgs& a, bool separable, hipStream_t st, hipError_t* err) {
    const uint32_t tiles = (a.w + 63) / 64;
    const size_t lds = (size_t)a.h * 65 * 4;
    if (!(a.tile_state && lds <= 96 * 1024)) return false;
    *err = [&]() -> hipError_t {
        // single pass with a decoupled look-back over the tiles (the state buffer must be zero)
        hipError_t e = hipMemsetAsync(a.tile_state, 0, ((size_t)a.n_frames * tiles + DWF_WORDS) * 8, st);
        if (e != hipSuccess) return e;
        const dim3 grid(a.n_frames * tiles);
        static LdsGrant grants[4];   // one per k_dwf_single instantiation below
        auto go = [&](auto kernel, LdsGrant& grant) -> hipError_t {
            int device = -1;   // not remembered if the runtime cannot say
            (void)hipGetDevice(&device);
            return launch_with_lds(kernel, grid, dim3(DWF_NT), lds, device, st, grant, a);
        };
        if (a.h <= 128) {   // the rebuilt single pass: static LDS, k_dwf_emit's tile
            auto fused = [&](auto rows) -> hipError_t {
                constexpr int R = decltype(rows)::value;
                if (a.dtype == OUSTER_HIP_F32) {
                    if (separable) hipLaunchKernelGGL((k_dwf_fused<float, true, R>), grid, dim3(256), 0, st, a);
                    else hipLaunchKernelGGL((k_dwf_fused<float, false, R>), grid, dim3(256), 0, st, a);
                } else {
                    if (separable) hipLaunchKernelGGL((k_dwf_fused<double, true, R>), grid, dim3(256), 0, st, a);
                    else hipLaunchKernelGGL((k_dwf_fused<double, false, R>), grid, dim3(256), 0, st, a);
                }
                return hipGetLastError();
            };
            return a.h > 64 ? fused(std::integral_constant<int, 128>{}) : fused(std::integral_constant<int, 64>{});
        }
        if (a.dtype == OUSTER_HIP_F32)
            return separable ? go(k_dwf_single<float, true, DWF_NT>, grants[0]) : go(k_dwf_single<float, false, DWF_NT>, grants[1]);
        return separable ? go(k_dwf_single<double, true, DWF_NT>, grants[2]) : go(k_dwf_single<double, false, DWF_NT>, grants[3]);
    }();
    return true;
}

bool launch_dwf_emit_stream(const DewarpFramesArgs& a, bool separable, hipStream_t st, int stream_mode, hipError_t* err) {
    // the persistent form (k_dwf_emit_stream) where it applies: whole 64-column tiles of exactly h rows, 16 B aligned planes,
    // the separable tables, and enough tiles to give every persistent workgroup a run of them
    static const uint32_t wgs = [] {
        int dev = 0, cus = 256;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        return (uint32_t)(2 * (cus > 0 ? cus : 256));
    }();
    const uint32_t tiles = (a.w + 63) / 64;
    const uint32_t n_items = a.n_frames * tiles;
    const bool ok = stream_mode != 0 && separable && a.dtype == OUSTER_HIP_F32 && a.w % 64 == 0 && (a.h == 64 || a.h == 128) &&
                    ((uintptr_t)a.range & 15) == 0 && n_items >= (stream_mode > 0 ? 1u : 4u * wgs);
    if (!ok) return false;
    const uint32_t g = std::min(n_items, wgs);
    static LdsGrant grants[2];   // one per k_dwf_emit_stream instantiation below
    auto go = [&](auto kernel, uint32_t ctx_bytes, LdsGrant& grant) -> hipError_t {
        int device = -1;   // not remembered if the runtime cannot say
        (void)hipGetDevice(&device);
        return launch_with_lds(kernel, dim3(g), dim3(576), 2 * (size_t)ctx_bytes, device, st, grant, a, n_items);
    };
    *err = a.h == 128 ? go(k_dwf_emit_stream<float, 128>, dwf_stream_ctx_bytes<float, 128>(), grants[0])
                      : go(k_dwf_emit_stream<float, 64>, dwf_stream_ctx_bytes<float, 64>(), grants[1]);
    return true;
}

}  // namespace ouster_hip_dev
