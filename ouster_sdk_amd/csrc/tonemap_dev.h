// tonemap_dev.h -- the per-pixel arithmetic of LocalToneMapper (k_tonemap.hip) and the float16 front end of the RGB overloads.
//
// Plain C++: no wave intrinsics, no contraction (every product, sum and quotient below is one IEEE operation in the image type T
// or in float, as tests/tonemap_model.py states them), so the kernels and the host-lanes program of the tests share these
// functions.  Reference loops: ouster_core/src/image_processing.cpp:59-76 (front end, fast_log10), :137-197 (look-up),
// :586-690 (LocalToneMapper::apply after its state machine).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/ouster_hip.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ouster_hip_dev {

constexpr int TM_TILES = 8, TM_BINS = 1024;
constexpr uint32_t TM_LUT_ELEMS = TM_TILES * TM_TILES * TM_BINS;   // per image: 64 tables of 1024 entries

// float16 bit pattern -> float by the reference's integer formula (:59-65): 0 and the quiet NaN 0x7e00 are 0, everything else
// is rebiased and shifted.  Not an IEEE conversion; the result is always finite.
__device__ __forceinline__ float tm_f16(uint16_t bits) {
    const uint32_t expanded = ((uint32_t)bits + 0x1C000u) << 13;
    const uint32_t r = (bits == 0 || bits == 0x7e00) ? 0u : expanded;
    float f;
    __builtin_memcpy(&f, &r, 4);
    return f;
}
// an element of a FLOAT16 plane: converts like the formula above wherever a kernel writes (T)element
struct F16Bits {
    uint16_t b;
    __device__ __forceinline__ operator float() const { return tm_f16(b); }
};

// fast_log10 (:68-76): exponent and mantissa read as one fixed-point number
__device__ __forceinline__ float tm_fast_log10(float x) {
    uint32_t bits;
    __builtin_memcpy(&bits, &x, 4);
    const float log2_approx = (float)((int32_t)bits - 0x3F800000) * 1.1920929e-7f;
    return log2_approx * 0.30103f;
}

template <class T> __device__ __forceinline__ T tm_lum(T r, T g, T b) { return (r * (T)0.299 + g * (T)0.587) + b * (T)0.114; }

// one image's parameter record in the image type
template <class T> struct TmConsts {
    int mode;
    bool compress, color;
    T sub, mul, add, cf;
};
template <class T> __device__ __forceinline__ TmConsts<T> tm_consts(const ouster_hip_tonemap_params& p) {
    TmConsts<T> c;
    c.mode = p.map.mode;
    c.compress = p.compress != 0;
    c.sub = (T)p.map.sub;
    c.mul = (T)p.map.mul;
    c.add = (T)p.map.add;
    c.cf = (T)0.75 * (T)p.color_ramp;                 // :647-652
    c.color = p.color_correct != 0 && c.cf != (T)0;   // :654
    return c;
}

// map (:592-600), dynamic-range compression (:610-625), Reinhard (:628-629) on one pixel; returns lum_ae (:631-633)
template <class T> __device__ __forceinline__ T tm_front(const TmConsts<T>& c, T (&v)[3]) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        T x = v[j];
        if (c.mode == OUSTER_HIP_IMAGE_MAP_AFFINE) {
            x = x - c.sub;
            x = x * c.mul;
            x = x + c.add;
        } else {
            x = x * c.mul;
        }
        v[j] = x;
    }
    if (c.compress) {
        const T lum = tm_lum(v[0], v[1], v[2]);
        if (lum > (T)0.8) {
            const float x = (float)((double)(lum - (T)0.8) + 1.0);
            const T new_lum = (T)0.8 + (T)tm_fast_log10(x);
            const T scale = new_lum / lum;
#pragma unroll
            for (int j = 0; j < 3; ++j) v[j] = v[j] * scale;
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        T x = v[j];
        x = x < (T)0 ? (T)0 : x;
        v[j] = x / ((T)1 + x);
    }
    return tm_lum(v[0], v[1], v[2]);
}

// histogram bin of a luminance (:104-105).  The lower clamp is for memory safety alone: a finite image gives lum >= 0.
template <class T> __device__ __forceinline__ int tm_bin(T lum) {
    int b = (int)((float)lum * 1024.0f);
    b = b > TM_BINS - 1 ? TM_BINS - 1 : b;
    return b < 0 ? 0 : b;
}

// tile bounds (:95-98)
__device__ __forceinline__ uint32_t tm_tile_begin(uint32_t t, uint32_t n) { return t * n / (uint32_t)TM_TILES; }

// the two tiles a coordinate blends and its weight (:153-157, :164-167); f < 0 in the first half tile: the blend extrapolates
struct TmCoord {
    int t0, t1;
    float f;
};
__device__ __forceinline__ TmCoord tm_coord(uint32_t x, uint32_t n) {
    const float t_f = ((float)x + 0.5f) * 8.0f / (float)n - 0.5f;
    int t0 = (int)floorf(t_f);
    t0 = t0 > TM_TILES - 1 ? TM_TILES - 1 : t0;
    t0 = t0 < 0 ? 0 : t0;
    TmCoord c;
    c.t0 = t0;
    c.t1 = t0 + 1 > TM_TILES - 1 ? TM_TILES - 1 : t0 + 1;
    c.f = t_f - (float)t0;
    return c;
}
// bilinear blend of the four tables at `bin` (:182-190); luts: this image's [64][1024]
__device__ __forceinline__ float tm_blend(const float* luts, const TmCoord& cx, const TmCoord& cy, int bin) {
    const float l00 = luts[(cy.t0 * TM_TILES + cx.t0) * TM_BINS + bin], l01 = luts[(cy.t0 * TM_TILES + cx.t1) * TM_BINS + bin];
    const float l10 = luts[(cy.t1 * TM_TILES + cx.t0) * TM_BINS + bin], l11 = luts[(cy.t1 * TM_TILES + cx.t1) * TM_BINS + bin];
    const float fx = cx.f, fy = cy.f;
    return (1.0f - fy) * ((1.0f - fx) * l00 + fx * l01) + fy * ((1.0f - fx) * l10 + fx * l11);
}

// the last pass (:654-689) on one pixel
template <class T> __device__ __forceinline__ void tm_last(const TmConsts<T>& c, T (&v)[3], T lum_ae, T lum_clahe) {
    const T scale = lum_ae > (T)1e-6 ? lum_clahe / lum_ae : (T)1;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        T x = v[j] * scale;
        if (c.color) x = (-lum_clahe * c.cf) + x * ((T)1 + c.cf);
        x = x > (T)1 ? (T)1 : x;            // std::min(x, 1)
        if (c.color) x = x > (T)0 ? x : (T)0;   // std::max(0, x): -0.0 becomes +0.0
        v[j] = x;
    }
}

}  // namespace ouster_hip_dev
