// dwf_dev.h -- device helpers of the frame dewarp's emit kernels: k_dwf_emit (k_dewarp.hip) and the experimental forms
// (k_dewarp_experiments.hip, make EXPERIMENTS=1) share the column loop and what it stands on.
#pragma once
#include "kernels_common.h"

namespace ouster_hip_dev {

// wave-uniform broadcast of a register of lane `src` (v_readlane_b32 with an SGPR lane select)
__device__ __forceinline__ uint32_t bcast_u32(uint32_t v, uint32_t src) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)src);
}
__device__ __forceinline__ float bcast(float v, uint32_t src) {
    return __uint_as_float(bcast_u32(__float_as_uint(v), src));
}
__device__ __forceinline__ double bcast(double v, uint32_t src) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint64_t r = (uint64_t)bcast_u32((uint32_t)u, src) | ((uint64_t)bcast_u32((uint32_t)(u >> 32), src) << 32);
    return __longlong_as_double((long long)r);
}
template <class T> struct __attribute__((packed, aligned(4))) Pt3 { T x, y, z; };
// A pointer that was itself loaded from memory is a generic one and is read with flat_load, which counts on lgkmcnt as well
// as vmcnt: the s_waitcnt lgkmcnt(0) in front of the next barrier then waits for it.  Device tables are global memory.
template <class T>
__device__ __forceinline__ const __attribute__((address_space(1))) T* as_global(const T* p) {
    return (const __attribute__((address_space(1))) T*)(uintptr_t)p;
}

// rows 0..2 of a column's pose in the emit kernels' register order (rows 0 and 1 interleaved, see DwfColMeta), cast to T:
// from the caller's float table (48 B per column, three 16 B loads) or from the 4 x 4 doubles (128 B)
template <class T>
__device__ __forceinline__ void load_pose_rows(const DewarpFramesArgs& a, size_t col, T (&pose)[12]) {
    if constexpr (sizeof(T) == 4) {
        if (a.pose_rows) {
            const float4* pr = (const float4*)(a.pose_rows + col * 12);
            const float4 r0 = pr[0], r1 = pr[1], r2 = pr[2];
            pose[0] = r0.x; pose[2] = r0.y; pose[4] = r0.z; pose[6] = r0.w;
            pose[1] = r1.x; pose[3] = r1.y; pose[5] = r1.z; pose[7] = r1.w;
            pose[8] = r2.x; pose[9] = r2.y; pose[10] = r2.z; pose[11] = r2.w;
            return;
        }
    }
    const double* pm = a.poses + col * 16;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        pose[2 * k] = (T)pm[k];
        pose[2 * k + 1] = (T)pm[4 + k];
        pose[8 + k] = (T)pm[8 + k];
    }
}

// column metadata of an emit tile, staged once in LDS and read back as wave-uniform broadcasts
template <class T>
struct __attribute__((aligned(16))) DwfColMeta {
    T pose[12];      // rows 0..2 of the column's 4x4 pose, cast to the output type; rows 0 and 1 interleaved
                     // (p0 p4 p1 p5 p2 p6 p3 p7 | p8..p11) so that x and y are formed by packed f32 FMAs on adjacent registers
    double col[5];   // separable LUT: cos, sin of the encoder angle and the column constant
    uint32_t base, cnt;
    uint64_t ts;
};

// The column loop of the emit kernels: wave = CPW columns of a tile that sits in LDS (ranges, pitch TILE + 1) with its
// column metadata (count, output base, pose, table row), lane = row (NR rows per lane).  EASY: everything the tile emits lies
// below `capacity` and no kept range can be zero (the gate's lower bound is at least 1) -- then the loop carries neither the
// per-point room check nor the zero-range select.
// SWZ: the tile image came by LDS-DMA (k_dwf_emit_stream): lane-linear, so it cannot be padded per row; instead the 16 B
// cell of columns 4k..4k+3 of row r sits at cell position k ^ (r & 15) of its row -- a wave reading one column over 64 rows
// then spreads over 16 four-bank groups (4-way conflicts on two reads per column, against 64-way for the plain layout).
template <class T, bool SEP, int TILE, int ROWS, bool EASY, int NWAVES = 4, bool SWZ = false>
__device__ __forceinline__ void dwf_column_loop(const DewarpFramesArgs& a, const LutDev& lut, const uint32_t* s_rng,
                                                const DwfColMeta<T>* s_meta, uint32_t f, uint32_t c0, uint32_t ncol,
                                                uint64_t fbase, const uint32_t (&row)[ROWS / 64],
                                                const double (&bt)[ROWS / 64][9], uint32_t& m_run) {
    constexpr int PITCH = SWZ ? TILE : TILE + 1, CPW = TILE / NWAVES, NR = ROWS / 64;
    constexpr bool roomy = EASY, no_zero = EASY;
    const uint32_t W = a.w, H = a.h;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the column loop is software-pipelined over LDS: a column's ranges and count are read one column ahead, so the
    // keep masks can be formed the moment the iteration starts and no LDS round trip stands between two columns
    uint32_t rn[NR], cntn;
    auto fetch_col = [&](uint32_t jj_next) {
        const uint32_t jn = min(wave * CPW + jj_next, (uint32_t)TILE - 1u);
        cntn = s_meta[jn].cnt;
#pragma unroll
        for (int hh = 0; hh < NR; ++hh) {
            const uint32_t rr = lane + 64 * hh;
            rn[hh] = SWZ ? s_rng[rr * PITCH + ((((jn >> 2) ^ (rr & 15u)) << 2) | (jn & 3u))] : s_rng[rr * PITCH + jn];
        }
    };
    fetch_col(0);
    for (uint32_t jj = 0; jj < (uint32_t)CPW; ++jj) {
        const uint32_t j = wave * CPW + jj, x = c0 + j;  // wave-uniform
        if (j >= ncol) break;
        const DwfColMeta<T>& m = s_meta[j];
        uint32_t r[NR];
#pragma unroll
        for (int hh = 0; hh < NR; ++hh) r[hh] = rn[hh];
        const uint32_t cnt = __builtin_amdgcn_readfirstlane(cntn);
        if (cnt == 0) {  // masked out or empty column
            fetch_col(jj + 1);
            continue;
        }
        // this column's constants first (they are needed soonest), then the next column's ranges
        const uint32_t m_base = m.base;
        T ps[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) ps[k] = m.pose[k];
        double cx = 0, sx = 0, kc[3] = {0, 0, 0};
        if constexpr (SEP) {
            cx = m.col[0]; sx = m.col[1];
            kc[0] = m.col[2]; kc[1] = m.col[3]; kc[2] = m.col[4];
        }
        fetch_col(jj + 1);
        uint32_t rank[NR];
        bool keep[NR];
        uint32_t n_keep = 0;
#pragma unroll
        for (int hh = 0; hh < NR; ++hh) {
            // rows past H were staged as range 0, which the easy path's gate (min_r > 0) rejects by itself: one
            // subtract-and-compare whose result IS the ballot
            if constexpr (no_zero) keep[hh] = r[hh] - a.min_r <= a.max_r - a.min_r;
            else keep[hh] = row[hh] < H && r[hh] >= a.min_r && r[hh] <= a.max_r;
            const uint64_t mask = __builtin_amdgcn_ballot_w64(keep[hh]);
            // kept rows below this lane (v_mbcnt_lo / _hi), on top of the rows kept by the earlier row groups
            rank[hh] = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, n_keep));
            n_keep += (uint32_t)__popcll(mask);
        }
        if (n_keep == 0) continue;
        const uint64_t g0 = fbase + __builtin_amdgcn_readfirstlane(m_base) + bcast_u32(m_run, jj);  // first point of this run
        const uint64_t room = roomy ? ~0ull : (g0 < a.capacity ? a.capacity - g0 : 0);
        T* const run = (T*)a.points + g0 * 3;   // wave-uniform: the stores take it as a scalar base + a 32-bit lane offset
#pragma unroll
        for (int hh = 0; hh < NR; ++hh) {
            if (!(keep[hh] && (roomy || rank[hh] < room))) continue;
            T pt[3];
#ifdef OUSTER_ABLATE_DWF_MATH    // experiment builds only: every load and store stays, the projection and the pose do not
            if constexpr (SEP) {
                Pt3<T> o0;
                o0.x = (T)r[hh]; o0.y = (T)rank[hh]; o0.z = (T)x;
                ((Pt3<T>*)run)[rank[hh]] = o0;
                continue;
            }
#endif
            if constexpr (SEP) {
                const double rm = (double)r[hh] - lut.n;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double d = fma(cx, bt[hh][k], fma(sx, bt[hh][3 + k], bt[hh][6 + k]));
                    const T t = (T)fma(rm, d, kc[k]);
                    pt[k] = (no_zero || r[hh]) ? t : (T)0;
                }
            } else {
                double p[3];
                const size_t pix = (size_t)row[hh] * W + x;
                if (lut.full_dtype == OUSTER_HIP_F32)
                    project_full<float>((const float*)lut.full_dir, (const float*)lut.full_ofs, pix, r[hh], p);
                else
                    project_full<double>((const double*)lut.full_dir, (const double*)lut.full_ofs, pix, r[hh], p);
                pt[0] = (T)p[0]; pt[1] = (T)p[1]; pt[2] = (T)p[2];
            }
            const T px = pt[0], py = pt[1], pz = pt[2];
            Pt3<T> o;
            // three fused multiply-adds per component, the translation as the innermost addend
            o.x = fma(ps[0], px, fma(ps[2], py, fma(ps[4], pz, ps[6])));
            o.y = fma(ps[1], px, fma(ps[3], py, fma(ps[5], pz, ps[7])));
            o.z = fma(ps[8], px, fma(ps[9], py, fma(ps[10], pz, ps[11])));
#ifdef OUSTER_ABLATE_DWF_STORE   // experiment builds only: the arithmetic stays, (almost) nothing is stored
            if (!(o.x == (T)-12345.678 && o.y == (T)8765.4321)) continue;
#endif
#if OUSTER_NT_STANDALONE
            {
                T* pd = run + rank[hh] * 3u;
                __builtin_nontemporal_store(o.x, pd);
                __builtin_nontemporal_store(o.y, pd + 1);
                __builtin_nontemporal_store(o.z, pd + 2);
            }
#else
            ((Pt3<T>*)run)[rank[hh]] = o;
#endif
        }
        // every point of the run carries the same provenance: dense lanes 0..n_keep-1
        if (a.col_idxs || a.frame_idxs || a.timestamps_ns) {
            const uint64_t ts = m.ts;
            for (uint32_t i = lane; i < n_keep && i < room; i += 64) {
                if (a.col_idxs) a.col_idxs[g0 + i] = x;
                if (a.frame_idxs) a.frame_idxs[g0 + i] = f;
                if (a.timestamps_ns) a.timestamps_ns[g0 + i] = ts;
            }
        }
        if (lane == jj) m_run += n_keep;
    }
}

#ifdef OUSTER_EXPERIMENTS
// The two places where launch_dewarp_frames hands over to k_dewarp_experiments.hip.  Each returns whether it took the call;
// *err is then what launch_dewarp_frames returns.
//   single pass   instead of the whole count / scan / emit chain (a.tile_state set: knob "dewarp_single_pass")
//   emit stream   the persistent k_dwf_emit_stream in place of k_dwf_emit, where it applies (stream_mode: knob "dwf_stream")
__attribute__((visibility("hidden"))) bool launch_dwf_single_pass(const DewarpFramesArgs& a, bool separable, hipStream_t st, hipError_t* err);
__attribute__((visibility("hidden"))) bool launch_dwf_emit_stream(const DewarpFramesArgs& a, bool separable, hipStream_t st, int stream_mode, hipError_t* err);
#endif

}  // namespace ouster_hip_dev
