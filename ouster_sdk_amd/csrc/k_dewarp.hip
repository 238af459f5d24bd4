// k_dewarp.hip -- the dense dewarp and the range-gated frame dewarp of the hot path (gfx950), and their launch dispatch.
//
//   k_dewarp(_tiled)      per-column pose applied to a dense point cloud
//   k_dwf_*               range-gated, compacting frame dewarp (count, scans, emit)
// Reference loops:
//   dewarp<T>                                ouster_core/include/ouster/core/pose_util.h:38-56, impl/dewarp_impl.h:23-115
// The experimental forms of the frame dewarp are in k_dewarp_experiments.hip (make EXPERIMENTS=1); what they share with
// k_dwf_emit is in dwf_dev.h.  Memory bound: no MFMA anywhere.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "dwf_dev.h"
#include "kernels_common.h"
#include "standalone_plan.h"

namespace ouster_hip_dev {

// ------------------------------------------------------------------------------------
// k_dewarp: p' = R_col * p + t_col for every point (pose_util.h:38-56).  One thread per point;
// a wave reads 64 consecutive points = 768 contiguous bytes (f32) of one row, the 64 column
// poses come from the L2-resident pose table.  HBM bound: 2 x 3 x sizeof(T) B/point.
// ------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void k_dewarp(DewarpArgs a) {
    const size_t npix = (size_t)a.w * a.h, total = npix * a.n_images;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (size_t)gridDim.x * blockDim.x) {
        const size_t img = i / npix, pix = i - img * npix;
        const uint32_t col = (uint32_t)(pix % a.w);
        const double* m = a.poses + (img * a.w + col) * 16;
        const T* p = (const T*)a.points + i * 3;
        const T x = p[0], y = p[1], z = p[2];
        T* o = (T*)a.out + i * 3;
        // rotation * s + translation in T, row by row, like the reference's Eigen expression
        o[0] = (T)m[0] * x + (T)m[1] * y + (T)m[2] * z + (T)m[3];
        o[1] = (T)m[4] * x + (T)m[5] * y + (T)m[6] * z + (T)m[7];
        o[2] = (T)m[8] * x + (T)m[9] * y + (T)m[10] * z + (T)m[11];
    }
}

// ------------------------------------------------------------------------------------
// k_dewarp_tiled: p' = R_col * p + t_col (pose_util.h:38-56) with the k_decode lane mapping:
// each lane keeps the 3x4 poses of its 4 columns in registers for the whole row loop.
// ------------------------------------------------------------------------------------
template <class T, int TILE>
__global__ __launch_bounds__(256) void k_dewarp_tiled(DewarpArgs a) {
    constexpr int LPR = TILE / 4, RPP = 256 / LPR;
    constexpr int NV = 3 * sizeof(T) / 4;  // 16 B chunks per lane quad: 3 (f32) or 6 (f64)
    __shared__ float4 s_xyz[RPP * NV * LPR];
    const uint32_t W = a.w, H = a.h;
    const uint32_t tiles = (W + TILE - 1) / TILE;
    const uint32_t tile = blockIdx.x % tiles, chunk = blockIdx.x / tiles;
    const uint32_t img = blockIdx.y, tid = threadIdx.x;
    const uint32_t q = tid % LPR, ty = tid / LPR;
    const uint32_t c0 = tile * TILE, col = c0 + 4 * q;
    const bool full_tile = c0 + TILE <= W;
    const bool live = col < W;
    const uint32_t r_begin = chunk * a.rows_per_block;
    const uint32_t r_end = min(H, r_begin + a.rows_per_block);
    const size_t npix = (size_t)W * H;
    float4* sc = s_xyz + ty * (NV * LPR);
    T m[4][12];
    if (live) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double* pm = a.poses + ((size_t)img * W + col + c) * 16;
#pragma unroll
            for (int k = 0; k < 12; ++k) m[c][k] = (T)pm[k];
        }
    }
    for (uint32_t r = r_begin + ty; r < r_end; r += RPP) {
        const size_t i = ((size_t)img * npix + (size_t)r * W + col) * 3;
        union { float4 f4[NV]; T t[12]; } v, o;
        if (full_tile) {
            // coalesced row-segment read (LPR x 16 B contiguous per instruction), transposed
            // to "lane owns 4 points" through the lane-row's private scratch
            load_quad_coalesced<NV, LPR>(sc, (const float4*)((const T*)a.points + i - (size_t)(4 * q) * 3), q, v.f4);
        } else if (live) {
            const float4* src = (const float4*)((const T*)a.points + i);
#pragma unroll
            for (int k = 0; k < NV; ++k) v.f4[k] = src[k];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const T x = v.t[3 * c], y = v.t[3 * c + 1], z = v.t[3 * c + 2];
            o.t[3 * c + 0] = m[c][0] * x + m[c][1] * y + m[c][2] * z + m[c][3];
            o.t[3 * c + 1] = m[c][4] * x + m[c][5] * y + m[c][6] * z + m[c][7];
            o.t[3 * c + 2] = m[c][8] * x + m[c][9] * y + m[c][10] * z + m[c][11];
        }
        if (full_tile) {
            store_quad_coalesced<NV, LPR>(sc, (float4*)((T*)a.out + i - (size_t)(4 * q) * 3), q, o.f4);
        } else if (live) {
            float4* dst = (float4*)((T*)a.out + i);
#pragma unroll
            for (int k = 0; k < NV; ++k) dst[k] = o.f4[k];
        }
    }
}

// ------------------------------------------------------------------------------------
// Range-gated, compacting frame dewarp: dewarp(LidarFrame|FrameSet, XYZLut, min_range, max_range)
// (impl/dewarp_impl.h:23-115).  Output order is the reference's: frame, then column
// first_valid..last_valid with status != 0, then row; a point is kept when min_r <= r <= max_r.
//   k_dwf_count       kept points per (frame, column) from the range plane (ignores status)
//   k_dwf_scan        per frame: first/last valid column (status & 1, lidar_frame.cpp:907-925),
//                     mask, exclusive scan over the columns; frame total
//   k_dwf_frame_scan  exclusive scan of the frame totals
//   k_dwf_emit        stage a 64-row x 64-column range tile in LDS, wave = column, lane = row:
//                     ballot-rank the kept rows, project (f64 tables or the full LUT), apply the
//                     column pose in T, and write the compacted run through a wave-private LDS
//                     buffer so the global stores are contiguous dwords.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dwf_count(DewarpFramesArgs a) {
    constexpr int TILE = 64, LPR = 16, RPP = 16;
    __shared__ uint32_t s_cnt[TILE];
    const uint32_t W = a.w, H = a.h, f = blockIdx.y, tid = threadIdx.x;
    const uint32_t q = tid % LPR, ty = tid / LPR;
    const uint32_t c0 = blockIdx.x * TILE, col = c0 + 4 * q;
    if (tid < TILE) s_cnt[tid] = 0;
    __syncthreads();
    const uint32_t* rp = a.range + (size_t)f * W * H;
    const bool vec = (W % 4 == 0) && ((((uintptr_t)a.range) & 15) == 0);
    uint32_t cnt[4] = {0, 0, 0, 0};
    if (col < W) {
        for (uint32_t r = ty; r < H; r += RPP) {
            uint32_t v[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
            if (vec) {
                const uint4 t = *(const uint4*)(rp + (size_t)r * W + col);
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            } else {
                for (uint32_t c = 0; c < 4 && col + c < W; ++c) v[c] = rp[(size_t)r * W + col + c];
            }
#pragma unroll
            for (int c = 0; c < 4; ++c)
                cnt[c] += (col + c < W && v[c] >= a.min_r && v[c] <= a.max_r) ? 1u : 0u;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (cnt[c]) atomicAdd(&s_cnt[4 * q + c], cnt[c]);
    }
    __syncthreads();
    if (tid < TILE && c0 + tid < W) a.col_off[(size_t)f * (W + 1) + c0 + tid] = s_cnt[tid];
}

// block-wide exclusive scan of one value per thread (256 threads); returns the exclusive prefix,
// *total = block sum
__device__ __forceinline__ uint32_t block_exscan_256(uint32_t v, uint32_t* s_wave, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d, 64);
        if (lane >= (uint32_t)d) inc += t;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t k = 0; k < wave; ++k) base += s_wave[k];
    *total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
    return base + inc - v;
}

__global__ __launch_bounds__(256) void k_dwf_scan(DewarpFramesArgs a) {
    // One workgroup per frame.  Every global access is coalesced (thread t takes columns t, t + 256, ...) and a block's
    // loads are issued together from clamped addresses; the exclusive scan wants eight CONSECUTIVE columns per thread, so the
    // counts cross an LDS image (2048 columns per block, +1 dword of padding every 32).  The first form of this kernel walked
    // eight consecutive columns per thread straight from memory, twice, behind per-column guards: ~16 dependent round
    // trips, 16 us for 256 frames; this one takes two round trips per block of 2048 columns.
    constexpr uint32_t SEG = 8, BLK = 256 * SEG;
    __shared__ int s_lo, s_hi;
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_c[BLK + BLK / 32];
    const uint32_t W = a.w, f = blockIdx.x, tid = threadIdx.x;
    const uint32_t* st = a.status + (size_t)f * W;
    uint32_t* off = a.col_off + (size_t)f * (W + 1);
    if (tid == 0) { s_lo = 0x7fffffff; s_hi = -1; }
    __syncthreads();
    // first / last valid column (status bit 0; lidar_frame.cpp:907-925)
    int lo = 0x7fffffff, hi = -1;
    for (uint32_t base = 0; base < W; base += BLK) {
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
    __syncthreads();
    lo = s_lo; hi = s_hi;
    // kept points per column: k_dwf_count's, or the decode kernel's range-gate by-product (partial counts per row chunk,
    // summed here)
    const uint16_t* ext = a.gate_counts ? a.gate_counts + (size_t)f * OUSTER_HIP_GATE_CHUNKS * W : nullptr;
    auto pad = [](uint32_t i) { return i + (i >> 5); };
    uint32_t carry = 0;
    for (uint32_t base = 0; base < W; base += BLK) {
        uint32_t v[SEG], n[SEG], xc[SEG];
#pragma unroll
        for (uint32_t k = 0; k < SEG; ++k) {
            xc[k] = min(base + tid + 256u * k, W - 1u);
            v[k] = st[xc[k]];
        }
        // the branch on `ext` stays outside the column loop: inside it every column's partial counts were loaded and waited
        // for on their own (eight round trips per block)
        if (ext) {
            uint16_t g[SEG][OUSTER_HIP_GATE_CHUNKS];
#pragma unroll
            for (uint32_t k = 0; k < SEG; ++k)
#pragma unroll
                for (uint32_t c = 0; c < OUSTER_HIP_GATE_CHUNKS; ++c) g[k][c] = ext[(size_t)c * W + xc[k]];
#pragma unroll
            for (uint32_t k = 0; k < SEG; ++k) {
                n[k] = 0;
#pragma unroll
                for (uint32_t c = 0; c < OUSTER_HIP_GATE_CHUNKS; ++c) n[k] += g[k][c];
            }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < SEG; ++k) n[k] = off[xc[k]];
        }
#pragma unroll
        for (uint32_t k = 0; k < SEG; ++k) {
            const uint32_t x = base + tid + 256u * k;
            const bool keep = x < W && (int)x >= lo && (int)x <= hi && v[k] != 0;
            s_c[pad(tid + 256u * k)] = keep ? n[k] : 0u;
        }
        __syncthreads();
        uint32_t c[SEG], sum = 0;
#pragma unroll
        for (uint32_t i = 0; i < SEG; ++i) {
            c[i] = s_c[pad(tid * SEG + i)];
            sum += c[i];
        }
        uint32_t total;
        uint32_t run = carry + block_exscan_256(sum, s_wave, &total);   // (two barriers inside: s_c is read by now)
#pragma unroll
        for (uint32_t i = 0; i < SEG; ++i) {
            s_c[pad(tid * SEG + i)] = run;
            run += c[i];
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < SEG; ++k) {
            const uint32_t x = base + tid + 256u * k;
            if (x < W) off[x] = s_c[pad(tid + 256u * k)];
        }
        carry += total;
        __syncthreads();
    }
    if (tid == 0) {
        off[W] = carry;
        a.frame_off[f + 1] = carry;
    }
}

__global__ __launch_bounds__(256) void k_dwf_frame_scan(DewarpFramesArgs a) {
    __shared__ uint32_t s_wave[4];
    const uint32_t tid = threadIdx.x;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < a.n_frames; base += 256) {
        const uint32_t f = base + tid;
        const uint32_t v = f < a.n_frames ? (uint32_t)a.frame_off[f + 1] : 0u;
        uint32_t total;
        const uint32_t ex = block_exscan_256(v, s_wave, &total);
        if (f < a.n_frames) a.frame_off[f + 1] = carry + ex + v;
        carry += total;
    }
    if (tid == 0) a.frame_off[0] = 0;
}

template <class T, bool SEP, int TILE, int ROWS>
__global__ __launch_bounds__(256) void k_dwf_emit(DewarpFramesArgs a) {
    // tile = TILE columns x ROWS rows (64 x 128: a 128-beam sensor's whole columns).  A wave owns CPW
    // columns and walks them one at a time, lane = row (NR rows per lane): the kept rows are ranked
    // with ballots and every lane stores its own 12 / 24 B point, so one store instruction writes one
    // dense run.  The column's metadata (output base, pose cast to T, table row, timestamp) sits in
    // LDS and comes back as broadcast reads -- no dependent global loads in the column loop.
    constexpr int LPR = TILE / 4, PITCH = TILE + 1, CPW = TILE / 4, NR = ROWS / 64;
    constexpr int RPP = 256 / LPR;  // rows staged per pass
    static_assert(ROWS % 64 == 0 && TILE % 4 == 0 && TILE <= 256, "emit tile");
    __shared__ uint32_t s_rng[ROWS * PITCH];
    __shared__ DwfColMeta<T> s_meta[TILE];
    const uint32_t W = a.w, H = a.h, f = blockIdx.y, tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t q = tid % LPR, ty = tid / LPR;
    const uint32_t c0 = blockIdx.x * TILE;
    const uint32_t ncol = min((uint32_t)TILE, W - c0);
    const uint32_t* rp = a.range + (size_t)f * W * H;
    const uint32_t* off = a.col_off + (size_t)f * (W + 1);
    // nothing kept in this tile: leave before touching the range plane (uniform over the workgroup)
    if (off[c0 + ncol] == off[c0]) return;
    const uint64_t fbase = a.frame_off[f];
    const LutDev lut = a.luts[f % a.n_luts];
    const bool vec = (W % 4 == 0) && ((((uintptr_t)a.range) & 15) == 0);
    if (tid < (uint32_t)TILE) {
        DwfColMeta<T> m;
#pragma unroll
        for (int k = 0; k < 12; ++k) m.pose[k] = (T)0;
#pragma unroll
        for (int k = 0; k < 5; ++k) m.col[k] = 0.0;
        m.base = m.cnt = 0;
        m.ts = 0;
        const uint32_t mx = c0 + tid;
        if (tid < ncol) {
            m.base = off[mx];
            m.cnt = off[mx + 1] - m.base;
            if (m.cnt) {
                load_pose_rows<T>(a, (size_t)f * W + mx, m.pose);
                if constexpr (SEP) {
#pragma unroll
                    for (int k = 0; k < 5; ++k) m.col[k] = as_global(lut.col_tab)[(size_t)mx * 5 + k];
                }
                if (a.timestamps_ns) m.ts = a.timestamp[(size_t)f * W + mx];
            }
        }
        s_meta[tid] = m;
    }
    // The common case, decided once per tile: everything this tile emits lies below `capacity`, and no kept range can be
    // zero (the gate's lower bound is at least 1): then the column loop carries neither the per-point room check nor the
    // zero-range select.
    const bool easy = fbase + off[c0 + ncol] <= a.capacity && a.min_r > 0;
    uint32_t m_run = 0;  // lane jj of the wave: points of its jj-th column already written (previous row chunks)
    for (uint32_t r0 = 0; r0 < H; r0 += ROWS) {
        // the lane's rows of the beam table (a few KB shared by every tile): asked for before the tile is staged, so that the
        // two latencies overlap
        uint32_t row[NR];
        double bt[NR][9];
#pragma unroll
        for (int hh = 0; hh < NR; ++hh) {
            row[hh] = r0 + lane + 64 * hh;
            if constexpr (SEP) {
                const uint32_t rc = min(row[hh], H - 1u);   // unconditional loads: a guarded one is waited for on its own
#pragma unroll
                for (int k = 0; k < 9; ++k) bt[hh][k] = as_global(lut.beam_tab)[(size_t)rc * 9 + k];
            }
        }
        __syncthreads();  // previous chunk consumed (and, first time, the metadata published)
        if (vec) {
            // all passes' 16 B loads are issued before the first LDS write (clamped addresses instead of guards: a guarded
            // load and its guarded write compile to load / s_waitcnt vmcnt(0) / write, one memory round trip per pass).
            // Issuing them above the metadata block as well was tried: 164 VGPRs, three waves per SIMD, no gain.
            constexpr int NP = ROWS / RPP;
            uint4 t[NP];
            const uint32_t col = c0 + 4 * q, cc = min(col, W - 4u);
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                const uint32_t rc = min(r0 + ty + (uint32_t)i * RPP, H - 1u);
                t[i] = *(const uint4*)(rp + (size_t)rc * W + cc);
            }
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                const uint32_t rr = ty + (uint32_t)i * RPP;
                const bool in = r0 + rr < H && col < W;
                uint32_t* d = &s_rng[rr * PITCH + 4 * q];
                d[0] = in ? t[i].x : 0u; d[1] = in ? t[i].y : 0u; d[2] = in ? t[i].z : 0u; d[3] = in ? t[i].w : 0u;
            }
        } else {
            for (uint32_t rr = ty; rr < (uint32_t)ROWS; rr += RPP) {
                const uint32_t r = r0 + rr, col = c0 + 4 * q;
                uint32_t v[4] = {0, 0, 0, 0};
                if (r < H)
                    for (uint32_t c = 0; c < 4 && col + c < W; ++c) v[c] = rp[(size_t)r * W + col + c];
#pragma unroll
                for (int c = 0; c < 4; ++c) s_rng[rr * PITCH + 4 * q + c] = v[c];
            }
        }
        __syncthreads();
        if (easy) dwf_column_loop<T, SEP, TILE, ROWS, true>(a, lut, s_rng, s_meta, f, c0, ncol, fbase, row, bt, m_run);
        else dwf_column_loop<T, SEP, TILE, ROWS, false>(a, lut, s_rng, s_meta, f, c0, ncol, fbase, row, bt, m_run);
    }
}

// ------------------------------------------------------------------------------------
// launchers (host)
// ------------------------------------------------------------------------------------
// which kernel and which launch shape: standalone_plan.cpp (plain C++, tested on the CPU); the launchers only launch
hipError_t launch_dewarp(const DewarpArgs& a_in, hipStream_t st) {
    DewarpArgs a = a_in;
    const bool aligned = (((uintptr_t)a.points | (uintptr_t)a.out) & 15) == 0;
    const TiledPlan p = plan_dewarp(a.w, a.h, a.n_images, aligned, standalone_tile_width());
    const dim3 grid(p.grid_x, p.grid_y);
    if (p.tiled) {
        a.rows_per_block = p.rows_per_block;
        if (p.tile_width == 256) {
            if (a.dtype == OUSTER_HIP_F32) hipLaunchKernelGGL((k_dewarp_tiled<float, 256>), grid, dim3(256), 0, st, a);
            else hipLaunchKernelGGL((k_dewarp_tiled<double, 256>), grid, dim3(256), 0, st, a);
        } else {
            if (a.dtype == OUSTER_HIP_F32) hipLaunchKernelGGL((k_dewarp_tiled<float, 64>), grid, dim3(256), 0, st, a);
            else hipLaunchKernelGGL((k_dewarp_tiled<double, 64>), grid, dim3(256), 0, st, a);
        }
        return hipGetLastError();
    }
    if (a.dtype == OUSTER_HIP_F32) hipLaunchKernelGGL(k_dewarp<float>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_dewarp<double>, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_dewarp_frames(const DewarpFramesArgs& a, bool separable, hipStream_t st, int stream_mode) {
    const uint32_t tiles = (a.w + 63) / 64;
#ifdef OUSTER_EXPERIMENTS
    hipError_t exp_err = hipSuccess;
    if (launch_dwf_single_pass(a, separable, st, &exp_err)) return exp_err;
#endif
    if (!a.gate_counts) hipLaunchKernelGGL(k_dwf_count, dim3(tiles, a.n_frames), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_dwf_scan, dim3(a.n_frames), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_dwf_frame_scan, dim3(1), dim3(256), 0, st, a);
    // 64-column emit tiles (32-column ones measured 15 % slower); 128 rows per pass when the sensor has
    // more than 64 beams: the per-column overhead is paid once per column instead of once per 64 rows
#ifdef OUSTER_EXPERIMENTS
    if (launch_dwf_emit_stream(a, separable, st, stream_mode, &exp_err)) return exp_err;
#else
    (void)stream_mode;
#endif
    const dim3 grid(tiles, a.n_frames);
    auto emit = [&](auto rows) {
        constexpr int R = decltype(rows)::value;
        if (a.dtype == OUSTER_HIP_F32) {
            if (separable) hipLaunchKernelGGL((k_dwf_emit<float, true, 64, R>), grid, dim3(256), 0, st, a);
            else hipLaunchKernelGGL((k_dwf_emit<float, false, 64, R>), grid, dim3(256), 0, st, a);
        } else {
            if (separable) hipLaunchKernelGGL((k_dwf_emit<double, true, 64, R>), grid, dim3(256), 0, st, a);
            else hipLaunchKernelGGL((k_dwf_emit<double, false, 64, R>), grid, dim3(256), 0, st, a);
        }
    };
    // (round 6 A/B: two 64-row passes for a 128-beam sensor -- 23 KB of LDS, 80 VGPRs, six workgroups per CU instead of four --
    // 0.254 - 0.269 ms against 0.219 - 0.220: the per-column overhead paid twice costs more than the occupancy gives)
    if (a.h > 64) emit(std::integral_constant<int, 128>{});
    else emit(std::integral_constant<int, 64>{});
    return hipGetLastError();
}

}  // namespace ouster_hip_dev
