// k_osf.hip -- the device half of the OSF field decode (gfx950): the PNG scanline filters reversed, pixel bytes unpacked
// into field planes, and their launchers.
//
//   k_osf_png_unfilter    what libpng's png_read_row does, one wave per image
//   k_osf_unpack          PNG / ZPNG pixel bytes -> staggered field plane
// Memory-bound byte/bit work: no MFMA anywhere.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "kernels_common.h"
#include "launch_util.h"

namespace ouster_hip_dev {

// ------------------------------------------------------------------------------------
// k_osf_unpack: the device half of the OSF field decode.  One workgroup per
// (row, plane job).
//   PNG   decode_{8,16,24,32,64}bit_image, ouster_osf/src/png_tools.cpp:182-660: pixel bytes -> value
//         (16-bit samples byte-swapped), then stagger(): dst[r][(c + off[r]) % w] = value(r, c) with
//         off[] = destagger's offsets for inverse = true (impl/lidar_frame_impl.h:733-760)
//   ZPNG  UnpackAndUnfilter<N>, thirdparty/zpng/zpng.cpp:101-352: every byte lane of a row is the
//         running sum (mod 256) of its deltas -- a 256-thread block scan per lane; 3 / 4-byte pixels
//         arrive as colour planes and go through the inverse GB-RG transform first
// HBM bound: src bytes + dst bytes per pixel, each read / written once.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t block_incl_scan_u8(uint32_t v, uint32_t* s_wave) {
    // inclusive scan of one value per thread over the 256-thread block (only the low 8 bits matter)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d, 64);
        if (lane >= (uint32_t)d) v += t;
    }
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t k = 0; k < wave; ++k) base += s_wave[k];
    __syncthreads();
    return v + base;
}

// ------------------------------------------------------------------------------------
// k_osf_png_unfilter (round 5; VERDICT r04 "missing" item 3): the PNG scanline filters of an OSF field reversed on the device
// -- what libpng's png_read_row does behind decode_{8,16,24,32,64}bit_image (ouster_osf/src/png_tools.cpp:182-660; the filters:
// PNG specification section 9, RFC 2083 6.2 - 6.6).  Sub is a prefix sum and Up is elementwise, but Average and Paeth are
// recurrences in x AND depend on the row above, so a row cannot be split over lanes and rows cannot be done independently.
// What is parallel is the ANTI-DIAGONAL: pixel (x, y) needs (x-1, y), (x, y-1), (x-1, y-1) only.  One wave per image, lane =
// row of a 64-row band; at step t lane r reconstructs pixel x = t - r of its row.  Its left neighbour is its own result of
// step t-1; the pixel above and the one above-left are lane r-1's results of steps t-1 and t-2: two wave shifts per step, no
// memory.  A band's last row goes to LDS as it is produced (lane 63 is 63 pixels behind lane 0, so one row buffer serves both
// the band that reads it and the band that writes it); W + 63 steps per band.  Every byte of a pixel is its own recurrence
// (bpp = 1, 2, 3, 4 or 8 of them in one 64-bit register).  Input rows start at odd addresses (the filter byte), hence byte
// loads; output pixels are stored whole.  2300 images of a 256-frame batch are 2300 independent waves: 9 per CU.
// ------------------------------------------------------------------------------------
// Memory never sits inside a step: every lane keeps a RING of three 64-pixel blocks of its own row in LDS.  Block m+1 is read
// from global memory into registers when window m (64 steps) starts and copied to the ring when it ends; a step reads its raw
// pixel from the ring and writes the reconstructed one over it; block m-2 -- finished by every row -- leaves for global memory
// when window m starts.  16 bytes per lane per access on both sides.  (The first form loaded and stored inside the step: 2.9 ms
// per image whatever the batch, ~1.3 us a step -- on gfx9 a load's wait also waits for the stores before it.  With the ring
// 1.95 ms, then the step itself made branch free -- uf_byte -- 0.64 ms per 128 x 1024 image: 0.29 us a step.)
constexpr uint32_t UF_BLK = 64, UF_RING = 3 * UF_BLK, UF_G = 8;   // UF_G steps share their LDS reads (2, 4, 16: within 2 %)
typedef uint32_t uf_v4 __attribute__((ext_vector_type(4)));   // a plain vector: HIP's uint4 is a class and cannot live in an address space
typedef uf_v4 __attribute__((aligned(1))) uf_chunk_u;   // rows start where they start: the hardware takes unaligned 16-byte accesses
// explicit address spaces: the job's pointers were loaded from memory and the ring is reached through a lambda -- as generic
// pointers both become flat_load / flat_store, which count on vmcnt AND lgkmcnt and tie the LDS steps to the global traffic again
typedef __attribute__((address_space(1))) uint8_t g_u8;
typedef __attribute__((address_space(3))) uint8_t l_u8;
typedef __attribute__((address_space(1))) uf_chunk_u g_chunk_u;
typedef __attribute__((address_space(3))) uf_v4 l_uint4;

__host__ __device__ constexpr uint32_t uf_pitch(uint32_t bpp) { return UF_RING * bpp + 16u; }
__host__ __device__ constexpr uint32_t uf_ring_bytes(uint32_t bpp) { return 64u * uf_pitch(bpp); }

template <uint32_t BPP>
__device__ __forceinline__ uint64_t uf_px_load(const l_u8* p) {
    if (BPP == 1) return *p;
    if (BPP == 2) return *reinterpret_cast<const __attribute__((address_space(3))) uint16_t*>(p);
    if (BPP == 4) return *reinterpret_cast<const __attribute__((address_space(3))) uint32_t*>(p);
    if (BPP == 8) return *reinterpret_cast<const __attribute__((address_space(3))) uint64_t*>(p);
    return (uint64_t)p[0] | ((uint64_t)p[1] << 8) | ((uint64_t)p[2] << 16);
}
template <uint32_t BPP>
__device__ __forceinline__ void uf_px_store(l_u8* p, uint64_t v) {
    if (BPP == 1) *p = (uint8_t)v;
    else if (BPP == 2) *reinterpret_cast<__attribute__((address_space(3))) uint16_t*>(p) = (uint16_t)v;
    else if (BPP == 4) *reinterpret_cast<__attribute__((address_space(3))) uint32_t*>(p) = (uint32_t)v;
    else if (BPP == 8) *reinterpret_cast<__attribute__((address_space(3))) uint64_t*>(p) = v;
    else { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); }
}
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "k_osf_png_unfilter relies on the gfx9 DPP row control wave_shr:1 and on more than 64 KB of LDS per workgroup: build for gfx950"
#endif
__device__ __forceinline__ uint32_t wave_shr1(uint32_t v) {   // lane r receives lane r-1's value (lane 0: zero)
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}

// One byte of one pixel, every filter computed and the row's one picked by masks (m1..m4: all ones for the lane's filter type,
// zero otherwise).  Written as branches (if ft == 1 ... else if ...) the step compiled to ~260 VALU + ~400 SALU instructions of
// exec-mask juggling, 0.9 us a step; this is ~25 VALU per byte and no branch.
__device__ __forceinline__ uint32_t uf_byte(uint32_t a, uint32_t b, uint32_t c, uint32_t raw, uint32_t m1, uint32_t m2,
                                            uint32_t m3, uint32_t m4) {
    const uint32_t avg = (a + b) >> 1;
    const uint32_t pa = __usad(b, c, 0u), pb = __usad(a, c, 0u), pc = __usad(a + b, 2u * c, 0u);   // |p - a|, |p - b|, |p - c|
    const uint32_t paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    const uint32_t pred = (a & m1) | (b & m2) | (avg & m3) | (paeth & m4);
    return (raw + pred) & 0xffu;
}
template <uint32_t K, class P>
__device__ __forceinline__ uint32_t uf_get(P v) { return (uint32_t)(v >> (8u * K)) & 0xffu; }

template <uint32_t BPP>
__device__ __forceinline__ void unfilter_band(const OsfUnfilterJob& job, uint32_t H, uint32_t W, uint32_t band, l_u8* smem) {
    constexpr uint32_t BLKB = UF_BLK * BPP, NCH = BLKB / 16u;
    const uint32_t lane = threadIdx.x;
    l_u8* ring = smem + lane * uf_pitch(BPP);
    l_u8* s_up = smem + uf_ring_bytes(BPP);   // [W * BPP]: the last row of the band above
    const size_t stride = (size_t)W * BPP;
    const uint32_t row = band + lane;
    const bool has_row = row < H;
    const g_u8* in = (const g_u8*)(uintptr_t)job.raw + (size_t)(has_row ? row : 0) * (stride + 1);
    g_u8* out = (g_u8*)(uintptr_t)job.out + (size_t)(has_row ? row : 0) * stride;
    const uint32_t ft = has_row ? in[0] : 0u;
    ++in;
    const bool first_row = row == 0;          // nothing above: b = c = 0
    const bool from_lds = lane == 0 && band != 0;
    const bool feeds_next = lane == 63u || row + 1u == H;   // the next band's row above (the last band writes it for nobody)
    const uint32_t nblk = (W + UF_BLK - 1) / UF_BLK, steps = W + 63u, nwin = (steps + UF_BLK - 1) / UF_BLK;

    // A full block travels as 16-byte pieces through registers (fetch at the start of a window, commit at its end); the last,
    // partial block of a row goes byte by byte straight between memory and the ring (nothing is read or written past a row).
    // Lanes without a row read row 0's bytes (harmless) and store nothing.
    uf_v4 stage[NCH];
    auto fetch = [&](uint32_t blk) -> bool {    // global -> registers; false: the block already lies in the ring
        const uint32_t nb = min(UF_BLK, W - blk * UF_BLK) * BPP;
        const g_u8* src = in + (size_t)blk * BLKB;
        if (nb == BLKB) {
#pragma unroll
            for (uint32_t c = 0; c < NCH; ++c) stage[c] = *reinterpret_cast<const g_chunk_u*>(src + c * 16u);
            return true;
        }
        l_u8* d = ring + (blk % 3u) * BLKB;
#pragma nounroll
        for (uint32_t i = 0; i < nb; ++i) d[i] = src[i];
        return false;
    };
    auto commit = [&](uint32_t blk) {   // registers -> my ring
        l_uint4* d = reinterpret_cast<l_uint4*>(ring + (blk % 3u) * BLKB);
#pragma unroll
        for (uint32_t c = 0; c < NCH; ++c) d[c] = stage[c];
    };
    auto flush = [&](uint32_t blk) {    // my ring -> global
        if (!has_row) return;
        const uint32_t nb = min(UF_BLK, W - blk * UF_BLK) * BPP;
        g_u8* dst = out + (size_t)blk * BLKB;
        if (nb == BLKB) {
            const l_uint4* sp = reinterpret_cast<const l_uint4*>(ring + (blk % 3u) * BLKB);
#pragma unroll
            for (uint32_t c = 0; c < NCH; ++c) *reinterpret_cast<g_chunk_u*>(dst + c * 16u) = sp[c];
            return;
        }
        const l_u8* sp = ring + (blk % 3u) * BLKB;
#pragma nounroll
        for (uint32_t i = 0; i < nb; ++i) dst[i] = sp[i];
    };

    if (fetch(0)) commit(0);
    using P = typename std::conditional<(BPP <= 4u), uint32_t, uint64_t>::type;   // a pixel's bytes in one register
    const uint32_t m1 = ft == 1u ? ~0u : 0u, m2 = ft == 2u ? ~0u : 0u, m3 = ft == 3u ? ~0u : 0u, m4 = ft == 4u ? ~0u : 0u;
    P res1 = 0, res2 = 0;                     // my results of the two steps before (pixels x-1 and x-2 of my row)
    P up_prev = 0;                            // lane 0: the pixel above-left (pixel x-1 of the band above's last row)
    uint32_t pos = (UF_RING - lane) % UF_RING;   // ring position of pixel x = t - lane (meaningful once x >= 0)
    for (uint32_t m = 0; m < nwin; ++m) {
        if (m >= 2 && m - 2 < nblk) flush(m - 2);                    // its ring slot is the one block m + 1 goes to
        const bool staged = m + 1 < nblk && fetch(m + 1);
        for (uint32_t g = 0; g < UF_BLK / UF_G; ++g) {
            const uint32_t t0 = m * UF_BLK + g * UF_G;
            P raw[UF_G], up[UF_G], rec_g[UF_G];
            uint32_t at[UF_G];
#pragma unroll
            for (uint32_t j = 0; j < UF_G; ++j) {
                const uint32_t x = t0 + j - lane;                       // "negative" before the lane's first pixel: huge
                uint32_t q = pos + j;
                if (q >= UF_RING) q -= UF_RING;
                at[j] = q * BPP;
                // unguarded LDS reads (a guard is a branch): what a lane without a pixel reads is never used
                raw[j] = (P)uf_px_load<BPP>(ring + at[j]);
                up[j] = (P)uf_px_load<BPP>(s_up + min(x, W - 1u) * BPP);   // lane 0's; rewritten 63 steps from now at the earliest
            }
#pragma unroll
            for (uint32_t j = 0; j < UF_G; ++j) {
                const uint32_t x = t0 + j - lane;
                const bool valid = has_row && x < W;   // steps past W + 62 are valid for nobody
                // the row above: lane r-1 finished pixel x at step t-1 and pixel x-1 at step t-2
                P b, c;
                if constexpr (BPP <= 4u) {
                    b = wave_shr1(res1);
                    c = wave_shr1(res2);
                } else {
                    b = (uint64_t)wave_shr1((uint32_t)res1) | ((uint64_t)wave_shr1((uint32_t)(res1 >> 32)) << 32);
                    c = (uint64_t)wave_shr1((uint32_t)res2) | ((uint64_t)wave_shr1((uint32_t)(res2 >> 32)) << 32);
                }
                if (lane == 0) {   // the band's first row takes the row above from LDS (or has none)
                    b = from_lds ? up[j] : (P)0;
                    c = up_prev;
                    up_prev = b;
                }
                if (first_row) b = c = 0;
                const P left = (x != 0u) ? res1 : (P)0;   // res1 is zero while the lane has not started
                if (x == 0u) c = 0;
                P rec = 0;
                [&]<uint32_t... K>(std::integer_sequence<uint32_t, K...>) {
                    ((rec |= (P)uf_byte(uf_get<K>(left), uf_get<K>(b), uf_get<K>(c), uf_get<K>(raw[j]), m1, m2, m3, m4) << (8u * K)), ...);
                }(std::make_integer_sequence<uint32_t, BPP>{});
                rec_g[j] = rec;
                res2 = res1;
                res1 = valid ? rec : (P)0;
            }
#pragma unroll
            for (uint32_t j = 0; j < UF_G; ++j) {
                // the ring takes every lane's result: what a lane without a pixel writes lands in a slot that is free (before its
                // first pixel: block 2's, committed at the end of window 1; behind its last: a flushed block's or past the row's end)
                uf_px_store<BPP>(ring + at[j], rec_g[j]);
            }
            if (feeds_next) {
#pragma unroll
                for (uint32_t j = 0; j < UF_G; ++j) {
                    const uint32_t x = t0 + j - lane;
                    if (has_row && x < W) uf_px_store<BPP>(s_up + (size_t)x * BPP, rec_g[j]);
                }
            }
            pos += UF_G;
            if (pos >= UF_RING) pos -= UF_RING;
        }
        if (staged) commit(m + 1);
    }
    for (uint32_t blk = nwin >= 2 ? nwin - 2 : 0; blk < nblk; ++blk) flush(blk);
}

__global__ __launch_bounds__(64) void k_osf_png_unfilter(OsfUnfilterArgs a) {
    extern __shared__ __align__(16) uint8_t s_unf[];   // 64 row rings, then the last row of the band above
    const OsfUnfilterJob job = a.jobs[blockIdx.x];
    for (uint32_t band = 0; band < a.h; band += 64) {
        switch (job.bpp) {   // uniform over the workgroup
            case 1: unfilter_band<1>(job, a.h, a.w, band, (l_u8*)s_unf); break;
            case 2: unfilter_band<2>(job, a.h, a.w, band, (l_u8*)s_unf); break;
            case 3: unfilter_band<3>(job, a.h, a.w, band, (l_u8*)s_unf); break;
            case 4: unfilter_band<4>(job, a.h, a.w, band, (l_u8*)s_unf); break;
            default: unfilter_band<8>(job, a.h, a.w, band, (l_u8*)s_unf); break;
        }
        __syncthreads();   // one wave: orders the band's LDS writes before the next band's reads
    }
}

__global__ __launch_bounds__(256) void k_osf_unpack(OsfUnpackArgs a) {
    __shared__ uint32_t s_wave[4];
    const ouster_hip_osf_plane job = a.planes[blockIdx.y];
    const uint32_t r = blockIdx.x, W = a.w, tid = threadIdx.x;
    const uint32_t pb = job.src_pixel_bytes, es = job.dst_elem_size;
    uint8_t* drow = (uint8_t*)job.dst + (size_t)r * W * es;
    const uint64_t keep = es >= 8 ? ~0ull : ((1ull << (8 * es)) - 1);
    if (job.encoding != OUSTER_HIP_OSF_ZPNG) {
        const uint8_t* srow = (const uint8_t*)job.src + (size_t)r * W * pb;
        const bool swap16 = job.encoding == OUSTER_HIP_OSF_PNG_GRAY16 || job.encoding == OUSTER_HIP_OSF_PNG_RGBA16;
        const uint32_t off = a.offsets ? (uint32_t)a.offsets[r] : 0u;
        for (uint32_t c = tid; c < W; c += 256) {
            uint64_t v = 0;
            for (uint32_t k = 0; k < pb; ++k) v |= (uint64_t)srow[(size_t)c * pb + (swap16 ? (k ^ 1u) : k)] << (8 * k);
            uint32_t dc = c + off;
            if (dc >= W) dc -= W;
            store1(drow + (size_t)dc * es, v & keep, es);
        }
        return;
    }
    // ZPNG: thread t owns the contiguous pixels [t*seg, (t+1)*seg) of the row
    const uint32_t seg = (W + 255) / 256, x0 = tid * seg, x1 = min(W, x0 + seg);
    const uint8_t* src = (const uint8_t*)job.src;
    const size_t plane = (size_t)W * a.h;   // bytes of one colour plane (3 / 4-byte pixels)
    const bool planar = pb == 3 || pb == 4;
    // residual of byte lane k of pixel x in this row (after the inverse colour transform)
    auto resid = [&](uint32_t x, uint32_t k) -> uint32_t {
        if (!planar) return src[((size_t)r * W + x) * pb + k];
        const size_t i = (size_t)r * W + x;
        const uint32_t y = src[i], u = src[plane + i], v = src[2 * plane + i];
        const uint32_t G = (u + y) & 0xffu;
        return k == 0 ? ((G - v) & 0xffu) : k == 1 ? G : k == 2 ? y : src[3 * plane + i];
    };
    uint64_t carry_in = 0;   // byte lane k of the running value just before my segment
    for (uint32_t k = 0; k < pb; ++k) {
        uint32_t sum = 0;
        for (uint32_t x = x0; x < x1; ++x) sum += resid(x, k);
        const uint32_t incl = block_incl_scan_u8(sum, s_wave);
        carry_in |= (uint64_t)((incl - sum) & 0xffu) << (8 * k);
    }
    for (uint32_t x = x0; x < x1; ++x) {
        uint64_t v = 0;
        for (uint32_t k = 0; k < pb; ++k) {
            const uint32_t b = (uint32_t)((carry_in >> (8 * k)) & 0xffu) + resid(x, k);
            v |= (uint64_t)(b & 0xffu) << (8 * k);
        }
        carry_in = v;
        store1(drow + (size_t)x * es, v & keep, es);
    }
}

// ------------------------------------------------------------------------------------
// launchers (host)
// ------------------------------------------------------------------------------------
size_t osf_png_unfilter_lds_bytes(uint32_t w, uint32_t max_row_bytes) {
    const uint32_t bpp = w ? (max_row_bytes + w - 1) / w : 1u;   // the widest pixel of the batch sizes everybody's LDS
    return uf_ring_bytes(bpp) + (((size_t)max_row_bytes + 15) & ~(size_t)15);
}

hipError_t launch_osf_png_unfilter(const OsfUnfilterArgs& a, uint32_t n_jobs, uint32_t max_row_bytes, hipStream_t st) {
    const size_t lds = osf_png_unfilter_lds_bytes(a.w, max_row_bytes);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    static LdsGrant grant;
    int device = -1;   // not remembered if the runtime cannot say
    if (lds > LdsGrant::FREE_BYTES) (void)hipGetDevice(&device);
    return launch_with_lds(k_osf_png_unfilter, dim3(n_jobs), dim3(64), lds, device, st, grant, a);
}

hipError_t launch_osf_unpack(const OsfUnpackArgs& a, uint32_t n_planes, hipStream_t st) {
    hipLaunchKernelGGL(k_osf_unpack, dim3(a.h, n_planes), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace ouster_hip_dev
