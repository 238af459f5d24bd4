// k_destagger.hip -- the standalone destagger of the hot path (gfx950) and its launch dispatch.
//
//   k_destagger(_rows)    per-row circular shift
// Reference loop:
//   destagger_into<T>                        ouster_core/include/ouster/core/impl/lidar_frame_impl.h:733-760
// Memory-bound byte work: no MFMA anywhere.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>

#include "kernels_common.h"
#include "standalone_plan.h"

namespace ouster_hip_dev {

// ------------------------------------------------------------------------------------
// k_destagger: dst[img][u][(v + off[u]) % w] = src[img][u][v], element = elem bytes.
// One workgroup per (row, image).  The source row is fetched ONCE with aligned 16 B loads into LDS
// (every byte crosses the memory system -- or, for a host image worked on in place, the PCIe link --
// exactly once); lanes then walk the DESTINATION row in 16 B chunks so every store is an aligned,
// coalesced 16 B vector, and assemble each chunk from the LDS image of the row at an arbitrary byte
// offset (five dword reads and a funnel shift; the wrap point of the rotation is just an index modulo).
// Rows that do not fit the LDS budget (or are not 16 B granular) take the direct path below.
//   offset arithmetic: destagger_into, impl/lidar_frame_impl.h:753-759
// ------------------------------------------------------------------------------------
// k_destagger_rows: the same for short rows, several consecutive rows per workgroup, software pipelined: the aligned 16 B
// loads of row j + 1 are in flight while row j is assembled from its LDS image and stored.  (Built to overlap the two
// directions of the PCIe link for a host image worked on in place; it does not -- a kernel that reads and writes host memory
// gets 1 MB in + 1 MB out in 50 us whatever its shape, tools/copybench -- but it is the faster form for 8 / 16-bit planes in HBM.)
template <int CH>
__global__ __launch_bounds__(256) void k_destagger_rows(DestaggerArgs a, uint32_t rows_per_wg) {
    extern __shared__ uint4 s_row[];   // 2 x row
    const uint32_t img = blockIdx.y;
    const size_t row_bytes = (size_t)a.w * a.elem;
    const uint32_t nchunk = (uint32_t)(row_bytes >> 4), ndw = nchunk * 4;
    const uint32_t r0 = blockIdx.x * rows_per_wg, r1 = min(a.h, r0 + rows_per_wg);
    const uint8_t* sbase = (const uint8_t*)a.src + (size_t)img * a.h * row_bytes;
    uint8_t* dbase = (uint8_t*)a.dst + (size_t)img * a.h * row_bytes;
    uint4 regs[CH];
    auto fetch = [&](uint32_t u) {
        const uint4* srow = (const uint4*)(sbase + (size_t)u * row_bytes);
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const uint32_t i = threadIdx.x + k * 256;
            if (i < nchunk) regs[k] = srow[i];
        }
    };
    if (r0 < r1) fetch(r0);
    for (uint32_t u = r0; u < r1; ++u) {
        uint4* buf = s_row + ((u - r0) & 1) * nchunk;
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const uint32_t i = threadIdx.x + k * 256;
            if (i < nchunk) buf[i] = regs[k];
        }
        __syncthreads();
        if (u + 1 < r1) fetch(u + 1);
        const uint32_t* s_dw = (const uint32_t*)buf;
        const uint32_t sb0 = (uint32_t)(row_bytes - (size_t)a.offsets[u] * a.elem);
        const uint32_t sh = (sb0 & 3) * 8;
        uint8_t* drow = dbase + (size_t)u * row_bytes;
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const uint32_t i = threadIdx.x + k * 256;
            if (i >= nchunk) break;
            uint32_t dw = (sb0 >> 2) + i * 4;
            if (dw >= ndw) dw -= ndw;
            uint32_t d[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                uint32_t j = dw + q;
                if (j >= ndw) j -= ndw;
                d[q] = s_dw[j];
            }
            typedef uint32_t v4 __attribute__((ext_vector_type(4)));
            v4 o;
            if (sh == 0) {
                o = v4{d[0], d[1], d[2], d[3]};
            } else {
                o = v4{(d[0] >> sh) | (d[1] << (32 - sh)), (d[1] >> sh) | (d[2] << (32 - sh)),
                       (d[2] >> sh) | (d[3] << (32 - sh)), (d[3] >> sh) | (d[4] << (32 - sh))};
            }
#if OUSTER_NT_STANDALONE
            __builtin_nontemporal_store(o, (v4*)(drow + ((size_t)i << 4)));
#else
            *(v4*)(drow + ((size_t)i << 4)) = o;
#endif
        }
    }
}

__global__ __launch_bounds__(256) void k_destagger(DestaggerArgs a, uint32_t lds_row) {
    extern __shared__ uint4 s_row[];
    const uint32_t u = blockIdx.x, img = blockIdx.y;
    const size_t row_bytes = (size_t)a.w * a.elem;
    const uint8_t* srow = (const uint8_t*)a.src + ((size_t)img * a.h + u) * row_bytes;
    uint8_t* drow = (uint8_t*)a.dst + ((size_t)img * a.h + u) * row_bytes;
    const size_t shift_bytes = (size_t)a.offsets[u] * a.elem;  // dst byte b <- src byte (b - shift) mod row
    const bool fast = ((row_bytes & 15) == 0) && ((((uintptr_t)a.src | (uintptr_t)a.dst) & 15) == 0);
    if (fast && lds_row) {
        const uint32_t nchunk = (uint32_t)(row_bytes >> 4), ndw = nchunk * 4;
        for (uint32_t i = threadIdx.x; i < nchunk; i += blockDim.x) s_row[i] = ((const uint4*)srow)[i];
        __syncthreads();
        const uint32_t* s_dw = (const uint32_t*)s_row;
        const uint32_t sb0 = (uint32_t)(row_bytes - shift_bytes);   // source byte of destination byte 0 (== row_bytes: no shift)
        const uint32_t sh = (sb0 & 3) * 8;
        for (uint32_t i = threadIdx.x; i < nchunk; i += blockDim.x) {
            uint32_t dw = (sb0 >> 2) + i * 4;     // first source dword of this chunk, before the wrap
            if (dw >= ndw) dw -= ndw;
            uint32_t d[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                uint32_t j = dw + k;
                if (j >= ndw) j -= ndw;
                d[k] = s_dw[j];
            }
            uint4 o;
            if (sh == 0) {
                o = make_uint4(d[0], d[1], d[2], d[3]);
            } else {
                o.x = (d[0] >> sh) | (d[1] << (32 - sh));
                o.y = (d[1] >> sh) | (d[2] << (32 - sh));
                o.z = (d[2] >> sh) | (d[3] << (32 - sh));
                o.w = (d[3] >> sh) | (d[4] << (32 - sh));
            }
#if OUSTER_NT_STANDALONE
            {
                typedef uint32_t v4 __attribute__((ext_vector_type(4)));
                __builtin_nontemporal_store(v4{o.x, o.y, o.z, o.w}, (v4*)(drow + ((size_t)i << 4)));
            }
#else
            *(uint4*)(drow + ((size_t)i << 4)) = o;
#endif
        }
    } else if (fast) {
        const uint32_t nchunk = (uint32_t)(row_bytes >> 4);
        for (uint32_t i = threadIdx.x; i < nchunk; i += blockDim.x) {
            const size_t db = (size_t)i << 4;
            size_t sb = db + row_bytes - shift_bytes;
            if (sb >= row_bytes) sb -= row_bytes;
            uint32_t o[4];
            if (sb + 16 <= row_bytes) {
                const uint32_t sh = (uint32_t)(sb & 3) * 8;
                const uint32_t* q = (const uint32_t*)(srow + (sb & ~(size_t)3));
                if (sh == 0) {
                    o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3];
                } else {
                    const uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3], d4 = q[4];
                    o[0] = (d0 >> sh) | (d1 << (32 - sh));
                    o[1] = (d1 >> sh) | (d2 << (32 - sh));
                    o[2] = (d2 >> sh) | (d3 << (32 - sh));
                    o[3] = (d3 >> sh) | (d4 << (32 - sh));
                }
            } else {  // the chunk straddles the wrap point of the source row
                uint8_t b[16];
                for (int k = 0; k < 16; ++k) {
                    size_t s = sb + k;
                    if (s >= row_bytes) s -= row_bytes;
                    b[k] = srow[s];
                }
                for (int k = 0; k < 4; ++k)
                    o[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) |
                           ((uint32_t)b[4 * k + 3] << 24);
            }
            *(uint4*)(drow + db) = make_uint4(o[0], o[1], o[2], o[3]);
        }
    } else {
        for (size_t b = threadIdx.x; b < row_bytes; b += blockDim.x) {
            size_t s = b + row_bytes - shift_bytes;
            if (s >= row_bytes) s -= row_bytes;
            drow[b] = srow[s];
        }
    }
}

// which kernel and which launch shape: standalone_plan.cpp (plain C++, tested on the CPU); the launcher only launches
hipError_t launch_destagger(const DestaggerArgs& a, uint32_t n_images, hipStream_t st) {
    const size_t row_bytes = (size_t)a.w * a.elem;
    const bool pointers_aligned = (((uintptr_t)a.src | (uintptr_t)a.dst) & 15) == 0;
    static const int rows_env = [] { const char* e = getenv("OUSTER_HIP_DESTAGGER_ROWS"); return e ? atoi(e) : -1; }();   // A/B
    const DestaggerPlan p = plan_destagger(row_bytes, pointers_aligned, rows_env, a.h, n_images);
    const dim3 grid(p.grid_x, p.grid_y);
    switch (p.route) {
        case DestaggerRoute::ROWS1: hipLaunchKernelGGL(k_destagger_rows<1>, grid, dim3(256), p.lds_bytes, st, a, p.rows_per_wg); break;
        case DestaggerRoute::ROWS2: hipLaunchKernelGGL(k_destagger_rows<2>, grid, dim3(256), p.lds_bytes, st, a, p.rows_per_wg); break;
        case DestaggerRoute::ROWS4: hipLaunchKernelGGL(k_destagger_rows<4>, grid, dim3(256), p.lds_bytes, st, a, p.rows_per_wg); break;
        default: hipLaunchKernelGGL(k_destagger, grid, dim3(256), p.lds_bytes, st, a, p.lds_bytes); break;
    }
    return hipGetLastError();
}

}  // namespace ouster_hip_dev
