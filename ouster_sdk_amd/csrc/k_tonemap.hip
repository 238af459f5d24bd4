// k_tonemap.hip -- RGB display images on the device (gfx950): the luminance percentiles of the RGB AutoExposure overloads and
// LocalToneMapper.
//
//   k_tm_lum_percentiles   per image: count of the positive luminances of every 4th pixel and two exact order statistics
//   k_tm_hist              per (image, tile band): 1024-bin histogram of the tone-mapped luminance, integer counts
//   k_tm_luts              per (image, tile): clip, redistribute, CDF in bin order -> one look-up table
//   k_tm_finish            the streaming pass: recompute the pixel, blend four tables, saturation pass, store
// Reference loops: AutoExposure::apply(rgb) ouster_core/src/image_processing.cpp:307-384, compute_clahe_luts :86-133,
// apply_clahe_luts :137-197, LocalToneMapper::apply :532-690.  The state machine stays on the host in double
// (csrc/host/image_processing.cpp); every image gets one ouster_hip_tonemap_params record.
//
// Nothing between the input and the output image is stored per pixel: k_tm_hist and k_tm_finish both start from the ORIGINAL
// pixel and recompute convert -> map -> compression -> Reinhard -> lum_ae (tonemap_dev.h), so the float and double forms work in
// place and a FLOAT16 image moves 6 + 6 + 12 bytes per pixel.  Counts are integers (LDS and global atomics: exact, order-free);
// the float sums of k_tm_luts run in bin order on one lane, because their order decides the bits.  Every arithmetic step is
// one IEEE operation: no contraction in this file.
//
// The three tone-map kernels use no wave intrinsic and take their workgroup size as a template argument: tests/cpp/tonemap_lanes.cpp
// compiles this file for the host, one thread per lane, with 64 lanes.
#pragma clang fp contract(off)
#include "k_tonemap.h"

#include <stdint.h>
#include <type_traits>

#include "k_image.h"
#include "tonemap_dev.h"

namespace ouster_hip_dev {
namespace {

template <class F>
hipError_t tm_by_types(int in_type, int out_type, F&& f) {
    if (out_type == OUSTER_HIP_F32 && in_type == OUSTER_HIP_F16) return f(F16Bits{0}, 0.0f);
    if (out_type == OUSTER_HIP_F32 && in_type == OUSTER_HIP_F32) return f(0.0f, 0.0f);
    if (out_type == OUSTER_HIP_F64 && in_type == OUSTER_HIP_F64) return f(0.0, 0.0);
    return hipErrorInvalidValue;
}

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------
// k_tm_lum_percentiles: workgroup = image, 1024 lanes, k_image.h's selection over the luminance of pixels 0, 4, 8, ...: three
// elements per sample (6 / 12 / 24 bytes), converted, (r * T(0.299) + g * T(0.587)) + b * T(0.114), kept when > 0.
// ------------------------------------------------------------------------------------
template <class TIN, class T>
__global__ __launch_bounds__(1024) void k_tm_lum_percentiles(TonemapArgs a) {
    const uint32_t img = blockIdx.x, hw = a.h * a.w;
    const TIN* in = (const TIN*)a.in + (size_t)img * a.in_stride;
    select_percentiles<T>(
        [&](uint32_t j) {
            const TIN* p = in + (size_t)j * 12;
            return tm_lum((T)p[0], (T)p[1], (T)p[2]);
        },
        (hw + 3) / 4, a.lo_percentile, a.hi_percentile, &a.n_positive[img], (T*)a.lo_hi + (size_t)img * 2);
}
#endif

// ------------------------------------------------------------------------------------
// k_tm_hist: workgroup = (band of a tile's rows, image).  Lane i of the band takes pixels i, i + WG, ... of the band in row-major
// order (consecutive lanes read consecutive pixels of a tile row), recomputes lum_ae and counts its bin in LDS; the non-empty bins
// are added to the tile's global histogram.  An image whose record says NONE (the early return) is skipped.
// ------------------------------------------------------------------------------------
template <class TIN, class T, int WG>
__global__ __launch_bounds__(WG) void k_tm_hist(TonemapArgs a) {
    __shared__ uint32_t s_hist[TM_BINS];
    const uint32_t tid = threadIdx.x, img = blockIdx.y, tile = blockIdx.x / a.pieces, piece = blockIdx.x % a.pieces;
    const ouster_hip_tonemap_params p = a.params[img];
    if (p.map.mode == OUSTER_HIP_IMAGE_MAP_NONE) return;
    const TmConsts<T> c = tm_consts<T>(p);
    const uint32_t ty = tile / TM_TILES, tx = tile % TM_TILES;
    const uint32_t y0 = tm_tile_begin(ty, a.h), y1 = tm_tile_begin(ty + 1, a.h);
    const uint32_t x0 = tm_tile_begin(tx, a.w), tw = tm_tile_begin(tx + 1, a.w) - x0;
    const uint32_t r0 = y0 + piece * (y1 - y0) / a.pieces, r1 = y0 + (piece + 1) * (y1 - y0) / a.pieces;
    if (r0 == r1) return;   // more bands than rows
    for (uint32_t i = tid; i < (uint32_t)TM_BINS; i += WG) s_hist[i] = 0;
    __syncthreads();
    const TIN* in = (const TIN*)a.in + (size_t)img * a.in_stride;
    const uint32_t npx = (r1 - r0) * tw;
    for (uint32_t i = tid; i < npx; i += WG) {
        const uint32_t r = i / tw, col = i - r * tw;
        const TIN* px = in + ((size_t)(r0 + r) * a.w + x0 + col) * 3;
        T v[3] = {(T)px[0], (T)px[1], (T)px[2]};
        const T lum_ae = tm_front(c, v);
        atomicAdd(&s_hist[tm_bin(lum_ae)], 1u);
    }
    __syncthreads();
    uint32_t* g = a.hist + ((size_t)img * (TM_TILES * TM_TILES) + tile) * TM_BINS;
    for (uint32_t i = tid; i < (uint32_t)TM_BINS; i += WG) {
        const uint32_t n = s_hist[i];
        if (n) atomicAdd(&g[i], n);
    }
}

// ------------------------------------------------------------------------------------
// k_tm_luts: workgroup = (tile, image).  compute_clahe_luts :110-129 on the tile's counts: the excess over the clip threshold and
// the CDF are float sums in bin order, 2 x 1024 dependent additions that one lane walks over LDS (float addition is not
// associative; a tree would give other bits); the loads, the clipping and the final scaling are spread over the lanes.
// ------------------------------------------------------------------------------------
constexpr int TM_WALK = 32;   // bins the walking lane holds in registers at a time: their LDS latency is paid once per chunk
template <int WG>
__global__ __launch_bounds__(WG) void k_tm_luts(TonemapArgs a) {
    __shared__ __attribute__((aligned(16))) float s_h[TM_BINS];   // counts, then the clipped counts + redistribute
    __shared__ __attribute__((aligned(16))) float s_c[TM_BINS];   // the CDF: an array of its own, so the walk's stores alias no load
    __shared__ float s_red;
    const uint32_t tid = threadIdx.x, tile = blockIdx.x, img = blockIdx.y;
    if (a.params[img].map.mode == OUSTER_HIP_IMAGE_MAP_NONE) return;
    const uint32_t ty = tile / TM_TILES, tx = tile % TM_TILES;
    const uint32_t pixels = (tm_tile_begin(ty + 1, a.h) - tm_tile_begin(ty, a.h)) * (tm_tile_begin(tx + 1, a.w) - tm_tile_begin(tx, a.w));
    const size_t at = ((size_t)img * (TM_TILES * TM_TILES) + tile) * TM_BINS;
    const float clip = (float)pixels / 1024.0f;   // clip limit 1.0f
    for (uint32_t i = tid; i < (uint32_t)TM_BINS; i += WG) s_h[i] = (float)a.hist[at + i];
    __syncthreads();
    if (tid == 0) {
        float excess = 0.0f;
        for (int base = 0; base < TM_BINS; base += TM_WALK) {   // a chunk's loads first, then its dependent additions
            float v[TM_WALK];
#pragma unroll
            for (int j = 0; j < TM_WALK; ++j) v[j] = s_h[base + j];
#pragma unroll
            for (int j = 0; j < TM_WALK; ++j) excess += v[j] > clip ? v[j] - clip : 0.0f;   // + 0.0f leaves the sum as it is
        }
        s_red = excess / 1024.0f;
    }
    __syncthreads();
    const float redistribute = s_red;
    for (uint32_t i = tid; i < (uint32_t)TM_BINS; i += WG) {
        const float hv = s_h[i];
        s_h[i] = (hv > clip ? clip : hv) + redistribute;
    }
    __syncthreads();
    if (tid == 0) {
        float cdf = 0.0f;
        for (int base = 0; base < TM_BINS; base += TM_WALK) {
            float v[TM_WALK];
#pragma unroll
            for (int j = 0; j < TM_WALK; ++j) v[j] = s_h[base + j];
#pragma unroll
            for (int j = 0; j < TM_WALK; ++j) {
                cdf += v[j];
                v[j] = cdf;
            }
#pragma unroll
            for (int j = 0; j < TM_WALK; ++j) s_c[base + j] = v[j];
        }
    }
    __syncthreads();
    const float inv_pix = 1.0f / (float)pixels;
    for (uint32_t i = tid; i < (uint32_t)TM_BINS; i += WG) {
        const float v = s_c[i] * inv_pix;
        a.luts[at + i] = v > 1.0f ? 1.0f : v;
    }
}

// ------------------------------------------------------------------------------------
// k_tm_finish: lane = 4 consecutive pixels (12 elements) of one image (blockIdx.y), grid-stride over the image: three vector loads,
// three (double: six) 16-byte stores.  Per pixel: recompute up to lum_ae, take its bin, blend the four tables of the pixel's tile
// neighbourhood (read through L2: 256 KB per image, shared by the whole grid), apply the last pass.  In place for float and
// double (a lane reads its pixels before it writes them).  A NONE record: the converted image, or nothing when in == out.
// ------------------------------------------------------------------------------------
template <class TIN, class T, int WG>
__global__ __launch_bounds__(WG) void k_tm_finish(TonemapArgs a) {
    const uint32_t img = blockIdx.y, w = a.w, h = a.h, hw = a.h * a.w, nquad = (hw + 3) / 4;
    const ouster_hip_tonemap_params p = a.params[img];
    const TIN* in = (const TIN*)a.in + (size_t)img * a.in_stride;
    T* out = (T*)a.out + (size_t)img * a.out_stride;
    const bool none = p.map.mode == OUSTER_HIP_IMAGE_MAP_NONE;
    if (none && (const void*)in == (const void*)out) return;
    const TmConsts<T> c = tm_consts<T>(p);
    const float* luts = a.luts + (size_t)img * TM_LUT_ELEMS;
    for (uint32_t q = blockIdx.x * WG + threadIdx.x; q < nquad; q += a.grid_x * WG) {
        const uint32_t p0 = q * 4, n = hw - p0 < 4 ? hw - p0 : 4;
        const TIN* src = in + (size_t)p0 * 3;
        T* dst = out + (size_t)p0 * 3;
        T v[12];
        if (a.vec && n == 4) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const Vec4<TIN> t = ((const Vec4<TIN>*)src)[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[4 * i + j] = (T)t.v[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 12; ++j) v[j] = (uint32_t)j < 3 * n ? (T)src[j] : (T)0;
        }
        if (!none) {
            uint32_t y = p0 / w, x = p0 - y * w;
            TmCoord cy = tm_coord(y, h);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if ((uint32_t)j < n) {
                    if (x >= w) {   // w >= 8: at most one row change per lane
                        x -= w;
                        ++y;
                        cy = tm_coord(y, h);
                    }
                    T px[3] = {v[3 * j], v[3 * j + 1], v[3 * j + 2]};
                    const T lum_ae = tm_front(c, px);
                    const T lum_clahe = (T)tm_blend(luts, tm_coord(x, w), cy, tm_bin(lum_ae));
                    tm_last(c, px, lum_ae, lum_clahe);
                    v[3 * j] = px[0];
                    v[3 * j + 1] = px[1];
                    v[3 * j + 2] = px[2];
                    ++x;
                }
            }
        }
        if (a.vec && n == 4) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                Vec4<T> t;
#pragma unroll
                for (int j = 0; j < 4; ++j) t.v[j] = v[4 * i + j];
                ((Vec4<T>*)dst)[i] = t;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 12; ++j)
                if ((uint32_t)j < 3 * n) dst[j] = v[j];
        }
    }
}

// k_tm_luts is one serial walk per tile: one wave per workgroup, so that every tile of a large batch is resident at once
constexpr int TM_WG_LUTS = 64;

// the launches with the workgroup size open: WG = TM_WG on the device, 64 in the host-lanes program
template <int WG>
hipError_t tm_hist_launch(TonemapArgs a, int in_type, int out_type, hipStream_t st) {
    if (a.n_images == 0) return hipSuccess;
    // bands per tile: enough for about 4096 workgroups in all (one band from 64 images on), each of at least 512 pixels (two per
    // lane) and one row: 8 / 4 / 1 for 1 / 16 / 64 images of 128 x 2048, the fastest of 1, 2, 4, 8, 16 at each of the three in
    // tools/ab/tonemap_bench.py's sweep
    const uint32_t rows_min = a.h / TM_TILES, tile_px = ((a.h + 7) / 8) * ((a.w + 7) / 8);
    if (a.pieces == 0) {   // not forced by the caller (the host-lanes program does)
        uint32_t pieces = 4096u / (a.n_images * (TM_TILES * TM_TILES));
        pieces = pieces < tile_px / 512 ? pieces : tile_px / 512;
        pieces = pieces < rows_min ? pieces : rows_min;
        a.pieces = pieces < 1 ? 1 : pieces;
    }
    return tm_by_types(in_type, out_type, [&](auto tin, auto t) {
        hipLaunchKernelGGL((k_tm_hist<decltype(tin), decltype(t), WG>), dim3(TM_TILES * TM_TILES * a.pieces, a.n_images), dim3(WG), 0, st, a);
        return hipGetLastError();
    });
}
template <int WG>
hipError_t tm_luts_launch(const TonemapArgs& a, hipStream_t st) {
    if (a.n_images == 0) return hipSuccess;
    hipLaunchKernelGGL(k_tm_luts<WG>, dim3(TM_TILES * TM_TILES, a.n_images), dim3(WG), 0, st, a);
    return hipGetLastError();
}
template <int WG>
hipError_t tm_finish_launch(TonemapArgs a, int in_type, int out_type, hipStream_t st) {
    if (a.n_images == 0) return hipSuccess;
    const uint32_t nquad = (a.h * a.w + 3) / 4, want = (nquad + WG - 1) / WG;
    uint32_t cap = 8192 / a.n_images;
    if (cap < 8) cap = 8;
    a.grid_x = want < cap ? want : cap;
    return tm_by_types(in_type, out_type, [&](auto tin, auto t) {
        hipLaunchKernelGGL((k_tm_finish<decltype(tin), decltype(t), WG>), dim3(a.grid_x, a.n_images), dim3(WG), 0, st, a);
        return hipGetLastError();
    });
}

}  // namespace

#ifdef __HIPCC__
hipError_t launch_tm_lum_percentiles(const TonemapArgs& a, int in_type, int out_type, hipStream_t st) {
    if (a.n_images == 0) return hipSuccess;
    return tm_by_types(in_type, out_type, [&](auto tin, auto t) {
        k_tm_lum_percentiles<decltype(tin), decltype(t)><<<dim3(a.n_images), 1024, 0, st>>>(a);
        return hipGetLastError();
    });
}
#endif
hipError_t launch_tm_hist(TonemapArgs a, int in_type, int out_type, hipStream_t st) { return tm_hist_launch<TM_WG>(a, in_type, out_type, st); }
hipError_t launch_tm_luts(const TonemapArgs& a, hipStream_t st) { return tm_luts_launch<TM_WG_LUTS>(a, st); }
hipError_t launch_tm_finish(TonemapArgs a, int in_type, int out_type, hipStream_t st) { return tm_finish_launch<TM_WG>(a, in_type, out_type, st); }

}  // namespace ouster_hip_dev
