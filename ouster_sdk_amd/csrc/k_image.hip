// k_image.hip -- display images on the device (gfx950): BeamUniformityCorrector and AutoExposure.
//
//   k_img_colmask       per image: which columns hold a non-zero pixel (w bits)
//   k_img_dark_rows     per (image, row pair): exact n_cols / 2-th smallest of the masked row differences
//   k_img_percentiles   per image: count of the positive samples (every 4th element) and two exact order statistics
//   k_img_apply         the streaming pass: convert, subtract the dark counts, map, clamp, store
// Reference loops (single-channel overloads only):
//   AutoExposure::apply                 ouster_core/src/image_processing.cpp:220-296
//   compute_dark_count / BUC::apply     ouster_core/src/image_processing.cpp:427-498
// The smoothing recurrences and the choice of the map stay on the host in double (csrc/host/image_processing.cpp): these
// kernels return a few numbers per image and k_img_apply gets one parameter record per image.
//
// Order statistics are found by radix select on order-preserving integer keys, 8-bit digits from the top: a histogram of the
// digit over the elements that still match the prefix, a scan of its 256 bins by one wave, the bin that holds rank k
// becomes the next digit.  nth_element's answer is the k-th smallest VALUE, which is unique whatever the ties, so the result
// is bit-exact.  Every arithmetic step is one IEEE operation in the image type: no contraction in this file.
#pragma clang fp contract(off)
#include "k_image.h"
#include "tonemap_dev.h"

#include <stdint.h>
#include <type_traits>

#ifndef OUSTER_NT_STANDALONE
#define OUSTER_NT_STANDALONE 1   // as in kernels_common.h: the non-temporal hint on the stores of the standalone kernels
#endif

namespace ouster_hip_dev {
namespace {

// ------------------------------------------------------------------------------------
// k_img_colmask: thread = column, walks the rows (a wave reads 64 consecutive elements per row); one ballot per wave is
// 64 bits of the mask.  `!= 0` like Eigen's cast<bool>.
// ------------------------------------------------------------------------------------
template <class TIN>
__global__ __launch_bounds__(256) void k_img_colmask(ImageArgs a) {
    const uint32_t img = blockIdx.y, col = blockIdx.x * 256 + threadIdx.x;
    const uint32_t words = (a.w + 63) / 64;
    const TIN* p = (const TIN*)a.in + (size_t)img * a.in_stride;
    bool any = false;
    if (col < a.w) {
#pragma unroll 8
        for (uint32_t r = 0; r < a.h; ++r) any |= p[(size_t)r * a.w + col] != (TIN)0;
    }
    const uint64_t b = __builtin_amdgcn_ballot_w64(any);
    if ((threadIdx.x & 63u) == 0 && (col >> 6) < words) a.col_mask[(size_t)img * words + (col >> 6)] = b;
}

// ------------------------------------------------------------------------------------
// k_img_dark_rows: workgroup = (row pair, image).  Rows i - 1 and i are read once, the differences image(i, c) -
// image(i - 1, c) (one rounding in T) become ordered keys in LDS, and the n_cols / 2-th smallest over the masked columns is
// selected in sizeof(T) passes over that LDS row.  n_cols == 0: the median is 0.
// ------------------------------------------------------------------------------------
template <class TIN, class T>
__global__ __launch_bounds__(256) void k_img_dark_rows(ImageArgs a) {
    typedef typename KeyOf<T>::type K;
    constexpr int KB = sizeof(K) * 8;
    extern __shared__ uint64_t s_dyn[];   // w keys
    K* s_key = (K*)s_dyn;
    __shared__ uint64_t s_mask[IMAGE_MAX_W_DARK / 64];
    __shared__ uint32_t s_hist[4][256];
    __shared__ uint32_t s_sel[3];
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const uint32_t row = blockIdx.x + 1, img = blockIdx.y, w = a.w;
    const uint32_t words = (w + 63) / 64;
    if (tid < words) s_mask[tid] = a.col_mask[(size_t)img * words + tid];
    __syncthreads();
    uint32_t n_cols = 0;
    for (uint32_t i = 0; i < words; ++i) n_cols += (uint32_t)__popcll(s_mask[i]);
    T* out = (T*)a.medians + (size_t)img * (a.h - 1) + (row - 1);
    if (row == 1 && tid == 0 && a.n_cols) a.n_cols[img] = n_cols;
    if (n_cols == 0) {
        if (tid == 0) *out = (T)0;
        return;
    }
    const TIN* r1 = (const TIN*)a.in + (size_t)img * a.in_stride + (size_t)row * w;
    const TIN* r0 = r1 - w;
    if (a.vec) {
        for (uint32_t q = tid; q < w / 4; q += 256) {
            const Vec4<TIN> x1 = ((const Vec4<TIN>*)r1)[q], x0 = ((const Vec4<TIN>*)r0)[q];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                T d = (T)x1.v[j] - (T)x0.v[j];
                if (d == (T)0) d = (T)0;   // one zero: nth_element cannot tell -0 from +0
                s_key[4 * q + j] = ordered_key<K>(f_bits(d));
            }
        }
    } else {
        for (uint32_t c = tid; c < w; c += 256) {
            T d = (T)r1[c] - (T)r0[c];
            if (d == (T)0) d = (T)0;
            s_key[c] = ordered_key<K>(f_bits(d));
        }
    }
    uint32_t k = n_cols / 2;
    K prefix = 0;
    for (int shift = KB - 8; shift >= 0; shift -= 8) {
        for (uint32_t i = tid; i < 4 * 256; i += 256) (&s_hist[0][0])[i] = 0;
        __syncthreads();   // (first pass: also the keys)
        for (uint32_t base = 0; base < w; base += 256) {
            const uint32_t c = base + tid;
            bool valid = false;
            uint32_t d = 0;
            if (c < w) {
                const K key = s_key[c];
                valid = (s_mask[c >> 6] >> (c & 63u)) & 1u;
                if (shift != KB - 8) valid = valid && (K)(key >> (shift + 8)) == prefix;
                d = (uint32_t)(key >> shift) & 255u;
            }
            hist_add(s_hist[wave], d, valid);
        }
        __syncthreads();
        if (wave == 0) select_bin<4>(s_hist, k, s_sel);
        __syncthreads();
        prefix = (K)(prefix << 8) | (K)s_sel[0];
        k = s_sel[1];
    }
    if (tid == 0) *out = bits_f(ordered_key_inv<K>(prefix));
}

// ------------------------------------------------------------------------------------
// k_img_percentiles: workgroup = image, 1024 lanes.  The sample is every 4th flat element, converted, optionally corrected by
// the row's dark count (max(x - dc[row], 0), as BeamUniformityCorrector leaves it), kept when > 0.  Positive values order like
// their bit patterns.  Both order statistics are selected in the same passes (two histograms once their prefixes differ).
// The sample of a 128 x 2048 image (65 536 values) does not fit LDS, so every digit pass reads it again: the plane was written
// by the previous kernel and the passes follow each other at once, so all but the first come from L2 / MALL.
// n is reported as it is (also below 100: the host decides); n == 0 gives lo = hi = 0.  The selection itself is k_image.h's
// select_percentiles, which k_tm_lum_percentiles runs over luminances.
// ------------------------------------------------------------------------------------
template <class TIN, class T>
__global__ __launch_bounds__(1024) void k_img_percentiles(ImageArgs a) {
    const uint32_t img = blockIdx.x, w = a.w, hw = a.h * a.w;
    const TIN* in = (const TIN*)a.in + (size_t)img * a.in_stride;
    const T* dark = a.dark ? (const T*)a.dark + (size_t)img * a.h : nullptr;
    select_percentiles<T>(
        [&](uint32_t j) {
            T x = (T)in[(size_t)j * 4];
            if (dark) {
                x = x - dark[(j * 4) / w];
                x = x < (T)0 ? (T)0 : x;
            }
            return x;
        },
        (hw + 3) / 4, a.lo_percentile, a.hi_percentile, &a.n_positive[img], (T*)a.lo_hi + (size_t)img * 2);
}

// ------------------------------------------------------------------------------------
// k_img_apply: lane = 4 consecutive elements of one image (blockIdx.y), grid-stride over the image.  16 B stores (2 x 16 B for
// double), one vector load of the input; in place for float inputs (a lane reads its four elements before it writes them).
//   dark counts:  x = max(x - T(dc[row]), 0)                                BeamUniformityCorrector::apply :493-497
//   map SCALE:    x = x * T(mul)                 AFFINE: x = x - T(sub); x = x * T(mul); x = x + T(add)    AutoExposure::apply :275-288
//   then clamp to [0, 1] (:291).  Map NONE on an image that is already where it belongs is the reference's early return.
// ------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ void store4(T* p, const T (&v)[4], bool vec, uint32_t n) {
    typedef uint32_t v4 __attribute__((ext_vector_type(4)));
    if (vec && n == 4) {
        union { T t[4]; v4 q[sizeof(T) / 4]; } o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o.t[j] = v[j];
#pragma unroll
        for (int i = 0; i < (int)(sizeof(T) / 4); ++i) {
#if OUSTER_NT_STANDALONE
            __builtin_nontemporal_store(o.q[i], (v4*)p + i);
#else
            ((v4*)p)[i] = o.q[i];
#endif
        }
    } else {
        for (uint32_t j = 0; j < n; ++j) p[j] = v[j];
    }
}

template <class TIN, class T>
__global__ __launch_bounds__(256) void k_img_apply(ImageArgs a) {
    const uint32_t img = blockIdx.y, w = a.w, hw = a.h * a.w, nchunk = (hw + 3) / 4;
    int mode = OUSTER_HIP_IMAGE_MAP_NONE;
    bool use_dark = a.dark != nullptr;
    T sub = 0, mul = 1, add = 0;
    if (a.maps) {
        const ouster_hip_image_map m = a.maps[img];
        mode = m.mode;
        use_dark = use_dark && m.use_dark != 0;
        sub = (T)m.sub;
        mul = (T)m.mul;
        add = (T)m.add;
    }
    const TIN* in = (const TIN*)a.in + (size_t)img * a.in_stride;
    T* out = (T*)a.out + (size_t)img * a.out_stride;
    if (mode == OUSTER_HIP_IMAGE_MAP_NONE && !use_dark && (const void*)in == (const void*)out) return;
    const T* dark = use_dark ? (const T*)a.dark + (size_t)img * a.h : nullptr;
    for (uint32_t q = blockIdx.x * 256 + threadIdx.x; q < nchunk; q += gridDim.x * 256) {
        const uint32_t i0 = q * 4, n = hw - i0 < 4 ? hw - i0 : 4;
        T v[4] = {0, 0, 0, 0};
        if (a.vec && n == 4) {
            const Vec4<TIN> t = *(const Vec4<TIN>*)(in + i0);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (T)t.v[j];
        } else {
            for (uint32_t j = 0; j < n; ++j) v[j] = (T)in[i0 + j];
        }
        if (dark) {
            uint32_t row = i0 / w, col = i0 - row * w;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                while (col >= w) {
                    col -= w;
                    ++row;
                }
                if ((uint32_t)j < n) {
                    T x = v[j] - dark[row];
                    v[j] = x < (T)0 ? (T)0 : x;
                }
                ++col;
            }
        }
        if (mode != OUSTER_HIP_IMAGE_MAP_NONE) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                T x = v[j];
                if (mode == OUSTER_HIP_IMAGE_MAP_AFFINE) {
                    x = x - sub;
                    x = x * mul;
                    x = x + add;
                } else {
                    x = x * mul;
                }
                x = x < (T)0 ? (T)0 : x;
                v[j] = x > (T)1 ? (T)1 : x;
            }
        }
        store4<T>(out + i0, v, a.vec != 0, n);
    }
}

template <class F>
hipError_t by_types(int in_type, int out_type, F&& f) {
    if (out_type == OUSTER_HIP_F32) {
        switch (in_type) {
            case OUSTER_HIP_U8: return f((uint8_t)0, 0.0f);
            case OUSTER_HIP_U16: return f((uint16_t)0, 0.0f);
            case OUSTER_HIP_U32: return f((uint32_t)0, 0.0f);
            case OUSTER_HIP_F32: return f(0.0f, 0.0f);
        }
    } else if (out_type == OUSTER_HIP_F64) {
        switch (in_type) {
            case OUSTER_HIP_U8: return f((uint8_t)0, 0.0);
            case OUSTER_HIP_U16: return f((uint16_t)0, 0.0);
            case OUSTER_HIP_U32: return f((uint32_t)0, 0.0);
            case OUSTER_HIP_F64: return f(0.0, 0.0);
        }
    }
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_image_dark_rows(const ImageArgs& a, int in_type, int out_type, hipStream_t st) {
    if (a.n_images == 0 || a.h < 2 || a.w == 0) return hipSuccess;
    if (a.w > IMAGE_MAX_W_DARK) return hipErrorInvalidValue;
    return by_types(in_type, out_type, [&](auto tin, auto t) {
        typedef decltype(tin) TIN;
        typedef decltype(t) T;
        k_img_colmask<TIN><<<dim3((a.w + 255) / 256, a.n_images), 256, 0, st>>>(a);
        const size_t lds = (size_t)a.w * sizeof(T);
        k_img_dark_rows<TIN, T><<<dim3(a.h - 1, a.n_images), 256, lds, st>>>(a);
        return hipGetLastError();
    });
}

hipError_t launch_image_percentiles(const ImageArgs& a, int in_type, int out_type, hipStream_t st) {
    if (a.n_images == 0) return hipSuccess;
    return by_types(in_type, out_type, [&](auto tin, auto t) {
        k_img_percentiles<decltype(tin), decltype(t)><<<dim3(a.n_images), 1024, 0, st>>>(a);
        return hipGetLastError();
    });
}

hipError_t launch_image_apply(const ImageArgs& a, int in_type, int out_type, hipStream_t st) {
    if (a.n_images == 0 || a.h == 0 || a.w == 0) return hipSuccess;
    const uint32_t nchunk = (a.h * a.w + 3) / 4, want = (nchunk + 255) / 256;
    uint32_t cap = 8192 / a.n_images;
    if (cap < 8) cap = 8;
    if (in_type == OUSTER_HIP_F16) {   // FLOAT16 patterns (the RGB planes): tonemap_dev.h's integer formula on load
        if (out_type != OUSTER_HIP_F32) return hipErrorInvalidValue;
        k_img_apply<F16Bits, float><<<dim3(want < cap ? want : cap, a.n_images), 256, 0, st>>>(a);
        return hipGetLastError();
    }
    return by_types(in_type, out_type, [&](auto tin, auto t) {
        k_img_apply<decltype(tin), decltype(t)><<<dim3(want < cap ? want : cap, a.n_images), 256, 0, st>>>(a);
        return hipGetLastError();
    });
}

}  // namespace ouster_hip_dev
