// k_image.h -- launch interface of the display-image kernels (k_image.hip), and the selection machinery k_tonemap.hip shares.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/ouster_hip.h"

namespace ouster_hip_dev {

constexpr uint32_t IMAGE_MAX_W_DARK = 4096;   // k_img_dark_rows keeps one row of keys in LDS: 4096 doubles = 32 KB

// n_images images of h x w elements of in_type, image i at in + i * in_stride elements; out_type is F32 or F64 (= T)
struct ImageArgs {
    const void* in;
    void* out;                           // k_img_apply only: image i at out + i * out_stride elements of T
    size_t in_stride, out_stride;
    uint32_t n_images, h, w;
    uint32_t vec;                        // 4-element vector loads (and stores) are aligned for every image
    uint64_t* col_mask;                  // [n_images][(w + 63) / 64]: bit c set when column c holds a non-zero pixel
    void* medians;                       // k_img_dark_rows: T [n_images][h - 1]
    uint32_t* n_cols;                    // k_img_dark_rows: [n_images] (nullable)
    const void* dark;                    // T [n_images][h] dark counts (nullable)
    double lo_percentile, hi_percentile;
    uint32_t* n_positive;                // k_img_percentiles: [n_images]
    void* lo_hi;                         // k_img_percentiles: T [n_images][2]
    const ouster_hip_image_map* maps;    // k_img_apply: [n_images] (nullable: dark counts only)
};

hipError_t launch_image_dark_rows(const ImageArgs& a, int in_type, int out_type, hipStream_t st);
hipError_t launch_image_percentiles(const ImageArgs& a, int in_type, int out_type, hipStream_t st);
// in_type F16 with out_type F32 as well: FLOAT16 patterns converted by tonemap_dev.h's formula on load
hipError_t launch_image_apply(const ImageArgs& a, int in_type, int out_type, hipStream_t st);

// four consecutive elements as one access (u8: 4 B, 16-bit: 8 B, 32-bit: 16 B, f64: 2 x 16 B)
template <class TIN> struct __attribute__((aligned(sizeof(TIN) * 4 > 16 ? 16 : sizeof(TIN) * 4))) Vec4 { TIN v[4]; };

#ifdef __HIPCC__
// ---- exact order statistics by radix select, shared by k_img_dark_rows, k_img_percentiles and k_tm_lum_percentiles ----------
template <class T> struct KeyOf;
template <> struct KeyOf<float> { typedef uint32_t type; };
template <> struct KeyOf<double> { typedef uint64_t type; };

__device__ __forceinline__ uint32_t f_bits(float v) { return __float_as_uint(v); }
__device__ __forceinline__ uint64_t f_bits(double v) { return (uint64_t)__double_as_longlong(v); }
__device__ __forceinline__ float bits_f(uint32_t b) { return __uint_as_float(b); }
__device__ __forceinline__ double bits_f(uint64_t b) { return __longlong_as_double((long long)b); }

// total order of the non-NaN values as unsigned integers: negatives are complemented, the others get the top bit
template <class K> __device__ __forceinline__ K ordered_key(K b) {
    constexpr K top = (K)1 << (sizeof(K) * 8 - 1);
    return (b & top) ? (K)~b : (K)(b | top);
}
template <class K> __device__ __forceinline__ K ordered_key_inv(K k) {
    constexpr K top = (K)1 << (sizeof(K) * 8 - 1);
    return (k & top) ? (K)(k ^ top) : (K)~k;
}

// histogram[d] += 1 for every lane with `valid`, called by whole waves.  Lanes of one wave that hit the same LDS word are served
// one after the other, and display data is full of ties (8-bit planes, a shared exponent in the top digit), so the two
// most frequent digits of a wave -- the first pending lane's, twice -- go as ONE add of their lane count; what is left adds
// for itself.
__device__ __forceinline__ void hist_add(uint32_t* hist, uint32_t d, bool valid) {
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t rem = __builtin_amdgcn_ballot_w64(valid);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        if (rem == 0) break;   // wave-uniform
        const uint32_t lead = (uint32_t)__builtin_ctzll(rem);
        const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)d, (int)lead);
        const bool mine = valid && d == d0;
        const uint64_t m = __builtin_amdgcn_ballot_w64(mine);
        if (lane == lead) atomicAdd(&hist[d0], (uint32_t)__popcll(m));
        if (mine) valid = false;
        rem &= ~m;
    }
    if (valid) atomicAdd(&hist[d], 1u);
}

// One wave finds the bin of rank k in a 256-bin histogram kept as NSUB partial histograms: lane l owns bins 4l .. 4l + 3.
// Writes sel[0] = bin, sel[1] = rank inside the bin, sel[2] = total count.
template <int NSUB>
__device__ __forceinline__ void select_bin(const uint32_t (*hist)[256], uint32_t k, uint32_t* sel) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t c[4], tot = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = 0;
#pragma unroll
        for (int s = 0; s < NSUB; ++s) c[j] += hist[s][4 * lane + j];
        tot += c[j];
    }
    uint32_t inc = tot;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d, 64);
        if (lane >= (uint32_t)d) inc += t;
    }
    uint32_t run = inc - tot;
    if (k >= run && k < inc) {   // exactly one lane while k < total
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (k >= run && k < run + c[j]) {
                sel[0] = 4 * lane + j;
                sel[1] = k - run;
            }
            run += c[j];
        }
    }
    if (lane == 63) sel[2] = inc;
}

// A workgroup of 1024 lanes counts the positive values of a sample of nsamp entries and selects two exact order statistics of
// them: the floor(n * lo_percentile)-th and the (n - floor(n * hi_percentile) - 1)-th smallest (the reference's indices,
// products in double).  load(j) returns entry j in T; entries <= 0 are dropped.  Positive values order like their bit patterns.
// Both statistics are selected in the same passes (two histograms once their prefixes differ); every digit pass calls load()
// for the whole sample again.  n is reported as it is (also below 100: the host decides); n == 0 gives lo = hi = 0.
template <class T, class LOAD>
__device__ __forceinline__ void select_percentiles(LOAD load, uint32_t nsamp, double lo_percentile, double hi_percentile,
                                                   uint32_t* n_out, T* lo_hi_out) {
    typedef typename KeyOf<T>::type K;
    constexpr int KB = sizeof(K) * 8, UNR = 4;
    __shared__ uint32_t s_hist[2][4][256];
    __shared__ uint32_t s_sel[2][3];
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    uint32_t k[2] = {0, 0}, n = 0;
    K prefix[2] = {0, 0};
    for (int shift = KB - 8; shift >= 0; shift -= 8) {
        const bool first = shift == KB - 8;
        const bool same = prefix[0] == prefix[1];   // uniform: one histogram serves both
        for (uint32_t i = tid; i < 2 * 4 * 256; i += 1024) (&s_hist[0][0][0])[i] = 0;
        __syncthreads();
        for (uint32_t base = 0; base < nsamp; base += 1024 * UNR) {
            T v[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const uint32_t j = base + u * 1024 + tid;
                v[u] = j < nsamp ? load(j) : (T)0;
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const T x = v[u];
                const bool pos = x > (T)0;   // lanes past the sample hold 0
                const K key = f_bits(x);
                const uint32_t d = (uint32_t)(key >> shift) & 255u;
                bool m0 = pos, m1 = pos;
                if (!first) {
                    const K hi = (K)(key >> (shift + 8));
                    m0 = pos && hi == prefix[0];
                    m1 = pos && hi == prefix[1];
                }
                hist_add(s_hist[0][wave & 3u], d, m0);
                if (!same) hist_add(s_hist[1][wave & 3u], d, m1);
            }
        }
        __syncthreads();
        if (first) {
            if (wave == 0) select_bin<4>(s_hist[0], 0u, s_sel[0]);   // sel[2] = n
            __syncthreads();
            n = s_sel[0][2];
            if (n == 0) break;
            const uint32_t tl = (uint32_t)((double)n * lo_percentile), th = (uint32_t)((double)n * hi_percentile);
            k[0] = tl < n ? tl : n - 1;
            k[1] = th + 1 <= n ? n - th - 1 : 0;
            __syncthreads();
        }
        if (wave == 0) select_bin<4>(s_hist[0], k[0], s_sel[0]);
        if (wave == 1) select_bin<4>(same ? s_hist[0] : s_hist[1], k[1], s_sel[1]);
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            prefix[s] = (K)(prefix[s] << 8) | (K)s_sel[s][0];
            k[s] = s_sel[s][1];
        }
    }
    if (tid == 0) {
        *n_out = n;
        lo_hi_out[0] = n ? bits_f(prefix[0]) : (T)0;
        lo_hi_out[1] = n ? bits_f(prefix[1]) : (T)0;
    }
}
#endif   // __HIPCC__

}  // namespace ouster_hip_dev
