// k_frame_ops.hip -- ouster::sdk::core::frame_ops on the device (reference: ouster_core/src/frame_ops.cpp): per-pixel,
// memory-bound, integer-exact.  Three kernels, each batched over images and over a list of planes of mixed element types:
//   k_fops_clip         in place: keep v iff lower <= double(v) <= upper, else write the plane's invalid value (ClipOp)
//   k_fops_invalidate   one predicate per pixel (key range / row range / destaggered column range / u8 mask / one coordinate of
//                       a cloud), then every target plane gets its own invalid value at the pixels that fail it.  The targets are
//                       WRITE-ONLY here: nothing is loaded from them, a kept pixel costs them no traffic at all.
//   k_fops_select_rows  gather of whole rows (copy_selected_rows)
// Compiled with -ffp-contract=off like k_image.hip; the comparisons are on converted values only, no arithmetic feeds them.
#include "k_frame_ops.h"

namespace ouster_hip_dev {
namespace {

template <class T>
struct alignas(16) Chunk {
    T v[16 / sizeof(T)];
};
template <uint32_t E> struct UIntOf;
template <> struct UIntOf<1> { typedef uint8_t type; };
template <> struct UIntOf<2> { typedef uint16_t type; };
template <> struct UIntOf<4> { typedef uint32_t type; };
template <> struct UIntOf<8> { typedef uint64_t type; };

__device__ __forceinline__ bool inside(double v, double lo, double hi) { return v >= lo && v <= hi; }   // false for NaN

template <class F>
__host__ __device__ __forceinline__ bool by_type(int type, F&& f) {
    switch (type) {
        case OUSTER_HIP_U8: f((uint8_t)0); return true;
        case OUSTER_HIP_U16: f((uint16_t)0); return true;
        case OUSTER_HIP_U32: f((uint32_t)0); return true;
        case OUSTER_HIP_U64: f((uint64_t)0); return true;
        case OUSTER_HIP_I8: f((int8_t)0); return true;
        case OUSTER_HIP_I16: f((int16_t)0); return true;
        case OUSTER_HIP_I32: f((int32_t)0); return true;
        case OUSTER_HIP_I64: f((int64_t)0); return true;
        case OUSTER_HIP_F32: f(0.0f); return true;
        case OUSTER_HIP_F64: f(0.0); return true;
    }
    return false;
}

// ---- clip ------------------------------------------------------------------------------------------------------------
// One image of one plane per (blockIdx.y, blockIdx.z).  The 16-byte aligned middle of the image goes in 16-byte loads (and a
// 16-byte store only where a value changed); the elements in front of the first and behind the last aligned chunk -- an image
// of an odd number of bytes puts the next one off the grid -- are done one per lane by the first block.
template <class T>
__device__ void clip_image(T* p, uint32_t n, double lo, double hi, uint64_t invalid_bits) {
    typedef typename UIntOf<sizeof(T)>::type U;
    constexpr uint32_t PER = 16 / sizeof(T);
    const U ub = (U)invalid_bits;
    T inv;
    __builtin_memcpy(&inv, &ub, sizeof(T));
    uint32_t head = (uint32_t)(((16u - ((uintptr_t)p & 15u)) & 15u) / sizeof(T));
    if (head > n) head = n;
    const uint32_t nchunk = (n - head) / PER, tail0 = head + nchunk * PER;
    Chunk<T>* body = (Chunk<T>*)(p + head);
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < nchunk; q += gridDim.x * blockDim.x) {
        Chunk<T> c = body[q];
        bool changed = false;
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j) {
            if (!inside((double)c.v[j], lo, hi)) {
                c.v[j] = inv;
                changed = true;
            }
        }
        if (changed) body[q] = c;
    }
    if (blockIdx.x == 0) {
        for (uint32_t i = threadIdx.x; i < head; i += blockDim.x)
            if (!inside((double)p[i], lo, hi)) p[i] = inv;
        for (uint32_t i = tail0 + threadIdx.x; i < n; i += blockDim.x)
            if (!inside((double)p[i], lo, hi)) p[i] = inv;
    }
}

__global__ __launch_bounds__(256) void k_fops_clip(FopsClipArgs a) {
    const FopsPlane& pl = a.planes[blockIdx.y];
    const size_t off = (size_t)blockIdx.z * pl.stride;
    by_type(pl.type, [&](auto t) {
        typedef decltype(t) T;
        clip_image<T>((T*)pl.data + off, a.hw, a.lower, a.upper, pl.invalid_bits);
    });
}

// ---- invalidate --------------------------------------------------------------------------------------------------------
// A thread takes FOPS_GROUP = 16 consecutive pixels of the flat image, evaluates the predicate once for each (bit j of `bits`
// set: pixel i0 + j is invalidated) and then walks the target list.
//
// Stores.  A target is never read, so a 16-byte chunk of it can only be written whole when every pixel of the chunk is
// invalidated (then: one 16-byte store, where the address is aligned); a chunk with kept pixels in it gets one store of the
// element's own width per invalidated pixel, issued per lane.  Assembling such a chunk in registers would need the kept values,
// i.e. a read of the target -- twice the traffic of the common case (few pixels invalidated) to save store instructions in the
// rare one.  The twin (destaggered) plane is written per lane always: the pixels of a chunk land in different columns.
template <uint32_t E>
__device__ __forceinline__ void store_group(void* data, void* twin, size_t img_off, uint32_t i0, uint32_t n, uint32_t bits,
                                            uint64_t invalid_bits, uint32_t row0, uint32_t col0, uint32_t w,
                                            const uint32_t* shifts) {
    typedef typename UIntOf<E>::type U;
    constexpr uint32_t PER = 16 / E, FULL = (1u << PER) - 1u;
    const U inv = (U)invalid_bits;
    U* p = (U*)data + img_off + i0;
    Chunk<U> splat;
#pragma unroll
    for (uint32_t j = 0; j < PER; ++j) splat.v[j] = inv;
    const bool aligned = ((uintptr_t)p & 15u) == 0;
#pragma unroll
    for (uint32_t k = 0; k < E; ++k) {   // 16 pixels of E bytes: E chunks of 16 bytes
        const uint32_t sub = (bits >> (k * PER)) & FULL;
        if (sub == 0) continue;
        if (sub == FULL && aligned) {    // bits beyond n are never set: a full chunk lies inside the image
            ((Chunk<U>*)p)[k] = splat;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < PER; ++j)
                if (sub & (1u << j)) p[k * PER + j] = inv;
        }
    }
    if (twin) {
        U* t = (U*)twin + img_off;
        uint32_t row = row0, col = col0;
        for (uint32_t j = 0; j < n; ++j) {
            while (col >= w) {
                col -= w;
                ++row;
            }
            if (bits & (1u << j)) {
                uint32_t dc = col + shifts[row];   // both < w: one conditional subtraction is the mod
                if (dc >= w) dc -= w;
                t[(size_t)row * w + dc] = inv;
            }
            ++col;
        }
    }
}

// A cloud as a target: the point of an invalidated pixel becomes (0, 0, 0), what projection gives for range 0.  DW dwords per
// point (3 floats or 3 doubles), written per lane like every scattered store here.
template <uint32_t DW>
__device__ __forceinline__ void store_points(void* data, size_t img_off, uint32_t i0, uint32_t n, uint32_t bits) {
    uint32_t* p = (uint32_t*)data + (img_off + i0) * DW;
    for (uint32_t j = 0; j < n; ++j)
        if (bits & (1u << j)) {
#pragma unroll
            for (uint32_t k = 0; k < DW; ++k) p[j * DW + k] = 0u;
        }
}

template <class T>
__device__ __forceinline__ uint32_t key_bits(const T* key, uint32_t n, double lo, double hi) {
    constexpr uint32_t PER = 16 / sizeof(T);
    uint32_t bits = 0;
    if (n == FOPS_GROUP && ((uintptr_t)key & 15u) == 0) {
#pragma unroll
        for (uint32_t k = 0; k < sizeof(T); ++k) {
            const Chunk<T> c = ((const Chunk<T>*)key)[k];
#pragma unroll
            for (uint32_t j = 0; j < PER; ++j)
                if (inside((double)c.v[j], lo, hi)) bits |= 1u << (k * PER + j);
        }
    } else {
        for (uint32_t j = 0; j < n; ++j)
            if (inside((double)key[j], lo, hi)) bits |= 1u << j;
    }
    return bits;
}

__global__ __launch_bounds__(256) void k_fops_invalidate(FopsInvalidateArgs a) {
    const uint32_t img = blockIdx.y, w = a.w, hw = a.h * a.w, ngroup = (hw + FOPS_GROUP - 1) / FOPS_GROUP;
    const uint32_t* shifts = a.shifts ? a.shifts + (size_t)(img % a.n_tables) * a.h : nullptr;
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < ngroup; g += gridDim.x * blockDim.x) {
        const uint32_t i0 = g * FOPS_GROUP, n = hw - i0 < FOPS_GROUP ? hw - i0 : FOPS_GROUP;
        const uint32_t row0 = i0 / w, col0 = i0 - row0 * w;   // one division per 16 pixels; the pixels step from there
        uint32_t bits = 0;
        switch (a.kind) {
            case OUSTER_HIP_FOPS_PRED_KEY:
                by_type(a.src_type, [&](auto t) {
                    typedef decltype(t) T;
                    bits = key_bits<T>((const T*)a.src + (size_t)img * a.src_stride + i0, n, a.lower, a.upper);
                });
                break;
            case OUSTER_HIP_FOPS_PRED_MASK: {
                const uint8_t* m = (const uint8_t*)a.src + (size_t)(img % a.n_masks) * a.src_stride + i0;
                if (n == FOPS_GROUP && ((uintptr_t)m & 15u) == 0) {
                    const Chunk<uint8_t> c = *(const Chunk<uint8_t>*)m;
#pragma unroll
                    for (uint32_t j = 0; j < FOPS_GROUP; ++j)
                        if (c.v[j] == 0) bits |= 1u << j;
                } else {
                    for (uint32_t j = 0; j < n; ++j)
                        if (m[j] == 0) bits |= 1u << j;
                }
                break;
            }
            case OUSTER_HIP_FOPS_PRED_XYZ: {
                const size_t p0 = ((size_t)img * a.src_stride + i0) * 3 + a.axis;
                if (a.src_type == OUSTER_HIP_F32) {
                    const float* c = (const float*)a.src + p0;
                    for (uint32_t j = 0; j < n; ++j)
                        if (inside((double)c[3 * j], a.lower, a.upper)) bits |= 1u << j;
                } else {
                    const double* c = (const double*)a.src + p0;
                    for (uint32_t j = 0; j < n; ++j)
                        if (inside(c[3 * j], a.lower, a.upper)) bits |= 1u << j;
                }
                break;
            }
            case OUSTER_HIP_FOPS_PRED_ROWS:
            case OUSTER_HIP_FOPS_PRED_COLS: {
                uint32_t row = row0, col = col0;
                for (uint32_t j = 0; j < n; ++j) {
                    while (col >= w) {
                        col -= w;
                        ++row;
                    }
                    uint32_t x = row;
                    if (a.kind == OUSTER_HIP_FOPS_PRED_COLS) {
                        x = col + shifts[row];
                        if (x >= w) x -= w;
                    }
                    if (x >= a.lo && x < a.hi) bits |= 1u << j;
                    ++col;
                }
                break;
            }
        }
        if (bits == 0) continue;
        for (uint32_t p = 0; p < a.n_planes; ++p) {
            const FopsPlane& pl = a.planes[p];
            const size_t off = (size_t)img * pl.stride;
            switch (pl.elem) {
                case 1: store_group<1>(pl.data, pl.twin, off, i0, n, bits, pl.invalid_bits, row0, col0, w, shifts); break;
                case 2: store_group<2>(pl.data, pl.twin, off, i0, n, bits, pl.invalid_bits, row0, col0, w, shifts); break;
                case 4: store_group<4>(pl.data, pl.twin, off, i0, n, bits, pl.invalid_bits, row0, col0, w, shifts); break;
                case 8: store_group<8>(pl.data, pl.twin, off, i0, n, bits, pl.invalid_bits, row0, col0, w, shifts); break;
                case 12: store_points<3>(pl.data, off, i0, n, bits); break;
                case 24: store_points<6>(pl.data, off, i0, n, bits); break;
            }
        }
    }
}

// ---- select_rows -------------------------------------------------------------------------------------------------------
// blockIdx.y = selected row, blockIdx.z = image; the block copies that row of every plane: 16 bytes per lane where both row
// addresses are aligned (and the bytes behind the last chunk one at a time), one element per lane otherwise.
__global__ __launch_bounds__(256) void k_fops_select_rows(FopsSelectArgs a) {
    const uint32_t sel = blockIdx.y, img = blockIdx.z, srow = a.indices[sel];
    for (uint32_t p = 0; p < a.n_planes; ++p) {
        const size_t rb = (size_t)a.w * a.elem[p];
        const uint8_t* s = (const uint8_t*)a.src[p] + ((size_t)img * a.h + srow) * rb;
        uint8_t* d = (uint8_t*)a.dst[p] + ((size_t)img * a.n_sel + sel) * rb;
        const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
        if ((((uintptr_t)s | (uintptr_t)d) & 15u) == 0) {
            const size_t nchunk = rb / 16;
            for (size_t q = t; q < nchunk; q += nt) ((Chunk<uint8_t>*)d)[q] = ((const Chunk<uint8_t>*)s)[q];
            for (size_t i = nchunk * 16 + t; i < rb; i += nt) d[i] = s[i];
        } else {
            switch (a.elem[p]) {
                case 1: for (size_t i = t; i < a.w; i += nt) d[i] = s[i]; break;
                case 2: for (size_t i = t; i < a.w; i += nt) ((uint16_t*)d)[i] = ((const uint16_t*)s)[i]; break;
                case 4: for (size_t i = t; i < a.w; i += nt) ((uint32_t*)d)[i] = ((const uint32_t*)s)[i]; break;
                case 8: for (size_t i = t; i < a.w; i += nt) ((uint64_t*)d)[i] = ((const uint64_t*)s)[i]; break;
            }
        }
    }
}

uint32_t blocks_for(uint32_t items, uint32_t n_launch_units) {
    const uint32_t want = (items + 255) / 256;
    uint32_t cap = 8192 / (n_launch_units ? n_launch_units : 1);
    if (cap < 8) cap = 8;
    return want < cap ? (want ? want : 1) : cap;
}

}  // namespace

hipError_t launch_fops_clip(const FopsClipArgs& a, hipStream_t st) {
    if (a.n_planes == 0 || a.n_images == 0 || a.hw == 0) return hipSuccess;
    if (a.n_planes > FOPS_MAX_PLANES || a.n_images > 65535u) return hipErrorInvalidValue;
    k_fops_clip<<<dim3(blocks_for(a.hw / 4 + 1, a.n_planes * a.n_images), a.n_planes, a.n_images), 256, 0, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_fops_invalidate(const FopsInvalidateArgs& a, hipStream_t st) {
    if (a.n_planes == 0 || a.n_images == 0 || a.h == 0 || a.w == 0) return hipSuccess;
    if (a.n_planes > FOPS_MAX_PLANES || a.n_images > 65535u) return hipErrorInvalidValue;
    const uint32_t ngroup = (a.h * a.w + FOPS_GROUP - 1) / FOPS_GROUP;
    k_fops_invalidate<<<dim3(blocks_for(ngroup, a.n_images), a.n_images), 256, 0, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_fops_select_rows(const FopsSelectArgs& a, hipStream_t st) {
    if (a.n_planes == 0 || a.n_images == 0 || a.n_sel == 0 || a.w == 0) return hipSuccess;
    if (a.n_planes > FOPS_MAX_PLANES || a.n_images > 65535u || a.n_sel > 65535u) return hipErrorInvalidValue;
    const uint32_t per_row = (a.w + 255) / 256;   // one lane per element at the narrowest; wider elements take fewer steps
    k_fops_select_rows<<<dim3(per_row < 4 ? per_row : 4, a.n_sel, a.n_images), 256, 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace ouster_hip_dev
