// k_cartesian.hip -- the standalone cartesian projection of the hot path (gfx950) and its launch dispatch.
//
//   k_cartesian(_tiled)   range image -> XYZ
// Reference loops:
//   impl::make_xyz_lut / cartesianT<T>       ouster_core/src/xyzlut.cpp:11-89, impl/cartesian.h:36-66
// Memory bound: no MFMA anywhere.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "kernels_common.h"
#include "standalone_plan.h"

namespace ouster_hip_dev {

// ------------------------------------------------------------------------------------
// k_cartesian: standalone range image -> xyz, 4 consecutive pixels per lane
//   (cartesianT<T>, impl/cartesian.h:36-66)
// ------------------------------------------------------------------------------------
template <int MODE /*1 sep->f32, 2 sep->f64, 3 full*/>
__global__ __launch_bounds__(256) void k_cartesian(CartesianArgs a) {
    const uint32_t W = a.w, H = a.h;
    const size_t npix = (size_t)W * H;
    const size_t quads = (npix + 3) / 4;
    const LutDev lut = a.lut;
    for (size_t qi = (size_t)blockIdx.x * blockDim.x + threadIdx.x; qi < quads * a.n_images;
         qi += (size_t)gridDim.x * blockDim.x) {
        const size_t img = qi / quads, q = qi - img * quads;
        const size_t pix = q * 4;
        const uint32_t n = (npix - pix) < 4 ? (uint32_t)(npix - pix) : 4;
        const uint32_t* rp = a.range + img * npix + pix;
        uint32_t r[4] = {0, 0, 0, 0};
        const bool vec = (n == 4) && a.vec_ok;
        if (vec) { uint4 t = *(const uint4*)rp; r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w; }
        else for (uint32_t c = 0; c < n; ++c) r[c] = rp[c];
        double p[4][3];
        if constexpr (MODE == 1 || MODE == 2) {
            for (uint32_t c = 0; c < n; ++c) {
                const size_t i = pix + c;
                const uint32_t row = (uint32_t)(i / W), cc = (uint32_t)(i - (size_t)row * W);
                const double* b = lut.beam_tab + (size_t)row * 9;
                const double* t = lut.col_tab + (size_t)cc * 5;
                const double cxx = t[0], sxx = t[1];
                const double rm = (double)r[c] - lut.n;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double d = fma(cxx, b[k], fma(sxx, b[3 + k], b[6 + k]));
                    p[c][k] = r[c] ? fma(rm, d, t[2 + k]) : 0.0;
                }
            }
        } else {
            for (uint32_t c = 0; c < n; ++c) {
                if (lut.full_dtype == OUSTER_HIP_F32)
                    project_full<float>((const float*)lut.full_dir, (const float*)lut.full_ofs,
                                        pix + c, r[c], p[c]);
                else
                    project_full<double>((const double*)lut.full_dir, (const double*)lut.full_ofs,
                                         pix + c, r[c], p[c]);
            }
        }
        if (a.xyz_dtype == OUSTER_HIP_F32) {
            float* dst = (float*)a.xyz + (img * npix + pix) * 3;
            if (vec) store_xyz4<float>(dst, p);
            else for (uint32_t c = 0; c < n; ++c) store_xyz1<float>(dst + c * 3, p[c]);
        } else {
            double* dst = (double*)a.xyz + (img * npix + pix) * 3;
            if (vec) store_xyz4<double>(dst, p);
            else for (uint32_t c = 0; c < n; ++c) store_xyz1<double>(dst + c * 3, p[c]);
        }
    }
}

// ------------------------------------------------------------------------------------
// k_cartesian_tiled: the fast standalone form for W % 4 == 0 and 16 B aligned buffers.
// Same lane mapping as k_decode's compute phase: a workgroup owns 64 columns x RC rows of one
// image, lane = (row within pass, quad of 4 consecutive columns).  Per-column constants live in
// registers for the whole row loop, the row's 9 beam constants come from the L1-resident table,
// the range quad is one 16 B load and f32 XYZ goes out through the wave-private LDS transpose
// (256 contiguous bytes per row per store instruction).
//   MODE 1: separable tables -> f32, 2: separable -> f64, 3: full LUT (runtime dtypes)
// ------------------------------------------------------------------------------------
// full-LUT projection of a lane's 4 pixels from registers; LT = LUT element type
template <class LT>
__device__ __forceinline__ void project_full4(const LT (&dir)[12], const LT (&ofs)[12],
                                              const uint32_t (&rng)[4], double (&p)[4][3]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const LT rr = (LT)rng[c];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            LT m = rr * dir[3 * c + k];
            asm volatile("" : "+v"(m));  // no fma contraction (cartesianT host build)
            p[c][k] = rng[c] ? (double)(LT)(m + ofs[3 * c + k]) : 0.0;
        }
    }
}

template <int MODE, int TILE>
__global__ __launch_bounds__(256) void k_cartesian_tiled(CartesianArgs a) {
    constexpr int LPR = TILE / 4, RPP = 256 / LPR;
    __shared__ float4 s_xyz[RPP * 6 * LPR];  // one 6-chunk scratch per lane-row
    const uint32_t W = a.w, H = a.h;
    const uint32_t tiles = (W + TILE - 1) / TILE;
    const uint32_t tile = blockIdx.x % tiles, chunk = blockIdx.x / tiles;
    const uint32_t tid = threadIdx.x;
    // full-LUT mode: a workgroup projects its tile for a GROUP of images, so the tile's LUT rows (24 B/px for f32,
    // 1.5 x everything else the kernel moves) are fetched once per group instead of once per image
    const uint32_t ipb = a.images_per_block ? a.images_per_block : 1u;
    const uint32_t img0 = blockIdx.y * ipb, img1 = min(a.n_images, img0 + ipb);
    const uint32_t q = tid % LPR, ty = tid / LPR;
    const uint32_t c0 = tile * TILE, col = c0 + 4 * q;
    const uint32_t r_begin = chunk * a.rows_per_block;
    const uint32_t r_end = min(H, r_begin + a.rows_per_block);
    const bool full_tile = c0 + TILE <= W;
    const bool live = col < W;  // W % 4 == 0: a quad is entirely inside or outside
    const LutDev lut = a.lut;
    const size_t npix = (size_t)W * H;
    float4* sc = s_xyz + ty * (6 * LPR);

    double cx[4] = {0, 0, 0, 0}, sx[4] = {0, 0, 0, 0}, kc[4][3] = {};
    if constexpr (MODE == 1 || MODE == 2) {
        if (live) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const double* t = lut.col_tab + (size_t)(col + c) * 5;
                cx[c] = t[0]; sx[c] = t[1]; kc[c][0] = t[2]; kc[c][1] = t[3]; kc[c][2] = t[4];
            }
        }
    }
    auto store = [&](uint32_t img, size_t rowpix, const double (&p)[4][3]) {
        if (a.xyz_dtype == OUSTER_HIP_F32) {
            float* dst = (float*)a.xyz + ((size_t)img * npix + rowpix) * 3;
            if (full_tile) {
                union { float4 f4[3]; float t[12]; } o;
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int k = 0; k < 3; ++k) o.t[3 * c + k] = (float)p[c][k];
                store_quad_coalesced<3, LPR>(sc, (float4*)(dst - (size_t)(4 * q) * 3), q, o.f4);
            } else if (live) store_xyz4<float>(dst, p);
        } else {
            double* dst = (double*)a.xyz + ((size_t)img * npix + rowpix) * 3;
            if (full_tile) {
                union { float4 f4[6]; double t[12]; } o;
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int k = 0; k < 3; ++k) o.t[3 * c + k] = p[c][k];
                store_quad_coalesced<6, LPR>(sc, (float4*)(dst - (size_t)(4 * q) * 3), q, o.f4);
            } else if (live) store_xyz4<double>(dst, p);
        }
    };
    auto load_range = [&](uint32_t img, size_t rowpix, uint32_t (&rng)[4]) {
        rng[0] = rng[1] = rng[2] = rng[3] = 0;
        if (live) {
            const uint4 t = *(const uint4*)(a.range + (size_t)img * npix + rowpix);
            rng[0] = t.x; rng[1] = t.y; rng[2] = t.z; rng[3] = t.w;
        }
    };
    for (uint32_t r = r_begin + ty; r < r_end; r += RPP) {
        const size_t rowpix = (size_t)r * W + col;
        const size_t rowpix0 = (size_t)r * W + c0;
        // the images of the group, four at a time: the next four range quads are in flight while these four are
        // projected and stored (one load per iteration left the full-LUT kernel latency bound: 53 % of the roofline)
        auto project_group = [&](auto&& project) {
            constexpr int B = 4;
            uint32_t cur[B][4], nxt[B][4];
#pragma unroll
            for (int k = 0; k < B; ++k)
                if (img0 + k < img1) load_range(img0 + k, rowpix, cur[k]);
            for (uint32_t img = img0; img < img1; img += B) {
#pragma unroll
                for (int k = 0; k < B; ++k)
                    if (img + B + k < img1) load_range(img + B + k, rowpix, nxt[k]);
#pragma unroll
                for (int k = 0; k < B; ++k) {
                    if (img + k >= img1) break;
                    double p[4][3];
                    project(cur[k], p);
                    store(img + k, rowpix, p);
                }
#pragma unroll
                for (int k = 0; k < B; ++k)
#pragma unroll
                    for (int c = 0; c < 4; ++c) cur[k][c] = nxt[k][c];
            }
        };
        if constexpr (MODE == 1 || MODE == 2) {
            const double* b = lut.beam_tab + (size_t)r * 9;
            const double u0 = b[0], u1 = b[1], u2 = b[2], v0 = b[3], v1 = b[4], v2 = b[5],
                         w0 = b[6], w1 = b[7], w2 = b[8];
            double dd[4][3];   // the row's directions for my four columns: the same for every image of the group
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                dd[c][0] = fma(cx[c], u0, fma(sx[c], v0, w0));
                dd[c][1] = fma(cx[c], u1, fma(sx[c], v1, w1));
                dd[c][2] = fma(cx[c], u2, fma(sx[c], v2, w2));
            }
            project_group([&](const uint32_t (&rng)[4], double (&p)[4][3]) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double rm = (double)rng[c] - lut.n;
#pragma unroll
                    for (int k = 0; k < 3; ++k) p[c][k] = rng[c] ? fma(rm, dd[c][k], kc[c][k]) : 0.0;
                }
            });
        } else {
            // the LUT rows are streamed like the output: coalesced row segments, transposed to "lane owns 4 pixels"
            // through the scratch -- once, then every image of the group is projected from registers
            if (lut.full_dtype == OUSTER_HIP_F32) {
                union { float4 f4[3]; float t[12]; } d, o;
                if (full_tile) {
                    load_quad_coalesced<3, LPR>(sc, (const float4*)((const float*)lut.full_dir + rowpix0 * 3), q, d.f4);
                    load_quad_coalesced<3, LPR>(sc, (const float4*)((const float*)lut.full_ofs + rowpix0 * 3), q, o.f4);
                } else if (live) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        d.f4[k] = ((const float4*)((const float*)lut.full_dir + rowpix * 3))[k];
                        o.f4[k] = ((const float4*)((const float*)lut.full_ofs + rowpix * 3))[k];
                    }
                }
                project_group([&](const uint32_t (&rng)[4], double (&p)[4][3]) { project_full4<float>(d.t, o.t, rng, p); });
            } else {
                union { float4 f4[6]; double t[12]; } d, o;
                if (full_tile) {
                    load_quad_coalesced<6, LPR>(sc, (const float4*)((const double*)lut.full_dir + rowpix0 * 3), q, d.f4);
                    load_quad_coalesced<6, LPR>(sc, (const float4*)((const double*)lut.full_ofs + rowpix0 * 3), q, o.f4);
                } else if (live) {
#pragma unroll
                    for (int k = 0; k < 6; ++k) {
                        d.f4[k] = ((const float4*)((const double*)lut.full_dir + rowpix * 3))[k];
                        o.f4[k] = ((const float4*)((const double*)lut.full_ofs + rowpix * 3))[k];
                    }
                }
                project_group([&](const uint32_t (&rng)[4], double (&p)[4][3]) { project_full4<double>(d.t, o.t, rng, p); });
            }
        }
    }
}

// which kernel and which launch shape: standalone_plan.cpp (plain C++, tested on the CPU); the launcher only launches
hipError_t launch_cartesian(const CartesianArgs& a_in, int mode, hipStream_t st) {
    CartesianArgs a = a_in;
    const TiledPlan p = plan_cartesian(a.w, a.h, a.n_images, a.vec_ok != 0, standalone_tile_width());
    const dim3 grid(p.grid_x, p.grid_y);
    if (p.tiled) {
        a.rows_per_block = p.rows_per_block;
        a.images_per_block = p.images_per_block;
        if (p.tile_width == 256) {
            switch (mode) {
                case 1: hipLaunchKernelGGL((k_cartesian_tiled<1, 256>), grid, dim3(256), 0, st, a); break;
                case 2: hipLaunchKernelGGL((k_cartesian_tiled<2, 256>), grid, dim3(256), 0, st, a); break;
                default: hipLaunchKernelGGL((k_cartesian_tiled<3, 256>), grid, dim3(256), 0, st, a); break;
            }
        } else {
            switch (mode) {
                case 1: hipLaunchKernelGGL((k_cartesian_tiled<1, 64>), grid, dim3(256), 0, st, a); break;
                case 2: hipLaunchKernelGGL((k_cartesian_tiled<2, 64>), grid, dim3(256), 0, st, a); break;
                default: hipLaunchKernelGGL((k_cartesian_tiled<3, 64>), grid, dim3(256), 0, st, a); break;
            }
        }
        return hipGetLastError();
    }
    switch (mode) {
        case 1: hipLaunchKernelGGL(k_cartesian<1>, grid, dim3(256), 0, st, a); break;
        case 2: hipLaunchKernelGGL(k_cartesian<2>, grid, dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL(k_cartesian<3>, grid, dim3(256), 0, st, a); break;
    }
    return hipGetLastError();
}

}  // namespace ouster_hip_dev
