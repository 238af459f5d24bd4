// k_normals.hip -- algorithm::normals (ouster_algorithm/src/normals.cpp) on the GPU, held bit for bit to tests/normals_model.py.
// Built with -ffp-contract=off: every multiply, add, divide and sqrt below is one IEEE double operation, in the model's order
// (dot = (a0 b0 + a1 b1) + a2 b2, cross and the component-wise divisions as written).  No transcendental function is evaluated
// here: acos / tan live in the per-call constants the host makes with libm (host/normals_util.cpp) between the two kernels.
//
// k_normals_subtent: one workgroup per (frame, return); a thread takes columns t, t + 256, ... , finds the highest and lowest
//   row with range in each (loops bounded by h) and keeps the column with the smallest visiting rank
//   2 |col - w / 2| + (col > w / 2); the 256 ranks are reduced in LDS and the winner writes dot and top - bottom.
// k_normals: one thread per destaggered pixel, tiles of 64 columns x 4 rows.  A wave reads 64 consecutive pixels of a row (of
//   the source row, rotated, when the inputs are staggered); the rows above and below are the other waves' rows or the next
//   tile's, so the neighbour loads are served by L1 / L2 and nothing is staged: any pixel_search_range takes the same path and
//   every loop is bounded by it.
#include <hip/hip_runtime.h>

#include "k_normals.h"

namespace ouster_hip_dev {
namespace {

constexpr double TWO_PI = 2.0 * 3.14159265358979323846;
constexpr double EPS = 2.220446049250313e-16;
constexpr int64_t FOREGROUND_SALIENCE_MM = 500;

struct V3 {
    double x, y, z;
};

__device__ __forceinline__ double dot3(const V3& a, const V3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

template <class T>
__device__ __forceinline__ V3 load3(const void* base, uint64_t i) {
    const T* p = static_cast<const T*>(base) + i * 3;
    return V3{(double)p[0], (double)p[1], (double)p[2]};
}

// column of destaggered pixel (u, v) in the input arrays
__device__ __forceinline__ uint32_t src_col(const NormalsArgs& a, uint32_t u, uint32_t v) {
    if (!a.shifts) return v;
    const uint32_t c = v + a.w - a.shifts[u];   // shifts are reduced to [0, w)
    return c >= a.w ? c - a.w : c;
}

__device__ __forceinline__ V3 origin_of(const NormalsArgs& a, uint32_t frame, uint32_t v) {
    if (a.origins) return V3{a.origins[3 * (size_t)v], a.origins[3 * (size_t)v + 1], a.origins[3 * (size_t)v + 2]};
    if (!a.s2b) return V3{0.0, 0.0, 0.0};
    const double* s = a.s2b + 4 * (size_t)(frame % a.n_s2b);
    if (!a.poses) return V3{s[0], s[1], s[2]};
    const double* p = a.poses + ((size_t)frame * a.w + v) * 16;
    return V3{((p[0] * s[0] + p[1] * s[1]) + p[2] * s[2]) + p[3] * s[3],
              ((p[4] * s[0] + p[5] * s[1]) + p[6] * s[2]) + p[7] * s[3],
              ((p[8] * s[0] + p[9] * s[1]) + p[10] * s[2]) + p[11] * s[3]};
}

__device__ __forceinline__ V3 beam_of(const V3& p, const V3& o) {
    const V3 d{p.x - o.x, p.y - o.y, p.z - o.z};
    const double m = sqrt(dot3(d, d));
    if (m > 0.0) return V3{d.x / m, d.y / m, d.z / m};
    return V3{0.0, 0.0, 0.0};
}

template <class T>
__global__ __launch_bounds__(256) void k_normals_subtent(NormalsArgs a) {
    __shared__ uint32_t s_rank[256];
    const uint32_t t = threadIdx.x;
    const uint32_t frame = blockIdx.x / a.n_ret, ret = blockIdx.x - frame * a.n_ret;
    const size_t plane = (size_t)a.h * a.w;
    const uint32_t* rng = a.range[ret] + (size_t)frame * plane;
    const uint32_t mid = a.w / 2;
    uint32_t best = 0xffffffffu, best_top = 0, best_bottom = 0;
    for (uint32_t col = t; col < a.w; col += 256) {
        uint32_t top = 0, bottom = 0;
        bool any = false;
        for (uint32_t k = 0; k < a.h; ++k) {   // from the last row up: the highest row with range
            const uint32_t u = a.h - 1 - k;
            if (rng[(size_t)u * a.w + src_col(a, u, col)] != 0) {
                top = u;
                any = true;
                break;
            }
        }
        if (!any) continue;
        for (uint32_t u = 0; u < a.h; ++u) {
            if (rng[(size_t)u * a.w + src_col(a, u, col)] != 0) {
                bottom = u;
                break;
            }
        }
        if (top == bottom) continue;
        const uint32_t rank = col > mid ? 2 * (col - mid) + 1 : 2 * (mid - col);
        if (rank < best) best = rank, best_top = top, best_bottom = bottom;
    }
    s_rank[t] = best;
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
        if (t < s) s_rank[t] = min(s_rank[t], s_rank[t + s]);
        __syncthreads();
    }
    const uint32_t winner = s_rank[0];
    NormalsPair* out = a.pairs + blockIdx.x;
    if (winner == 0xffffffffu) {
        if (t == 0) *out = NormalsPair{0.0, 0u, 0u};
        return;
    }
    if (best != winner) return;   // ranks are distinct per column: one thread is left
    const uint32_t col = (winner & 1u) ? mid + (winner >> 1) : mid - (winner >> 1);
    const V3 o = origin_of(a, frame, col);
    const V3 bt = beam_of(load3<T>(a.xyz[ret], frame * plane + (size_t)best_top * a.w + src_col(a, best_top, col)), o);
    const V3 bb = beam_of(load3<T>(a.xyz[ret], frame * plane + (size_t)best_bottom * a.w + src_col(a, best_bottom, col)), o);
    *out = NormalsPair{dot3(bt, bb), best_top - best_bottom, col};
}

// find_best_neighbor's state; consider() is the reference's consider_neighbor
struct Search {
    V3 best_diff;
    double min_distance_sq;
    uint32_t best_radius;
    bool best_flip, thin;
};

template <class T>
__device__ __forceinline__ void consider(Search& s, const void* xyz, const uint32_t* rng, uint64_t idx, const V3& center,
                                         uint32_t center_range, double target_sq, bool flip, uint32_t radius) {
    const uint32_t nr = rng[idx];
    if (nr == 0) return;
    const V3 p = load3<T>(xyz, idx);
    const V3 d{p.x - center.x, p.y - center.y, p.z - center.z};
    const double dsq = dot3(d, d);
    if ((int64_t)nr - (int64_t)center_range < FOREGROUND_SALIENCE_MM) s.thin = false;
    if (fabs(dsq - target_sq) < fabs(s.min_distance_sq - target_sq)) {
        s.best_diff = d;
        s.min_distance_sq = dsq;
        s.best_flip = flip;
        s.best_radius = radius;
    }
}

// Case B: the beam's component perpendicular to the one usable difference, negated; false: the pixel stays zero
__device__ __forceinline__ bool perpendicular(const V3& diff, const V3& beam, V3& n) {
    const double denom = dot3(diff, diff);
    if (fabs(denom) < EPS) return false;
    const double s = dot3(diff, beam) / denom;
    const V3 pr{beam.x - s * diff.x, beam.y - s * diff.y, beam.z - s * diff.z};
    const double n_sq = dot3(pr, pr);
    if (fabs(n_sq) < EPS) return false;
    const double m = sqrt(n_sq);
    n = V3{-(pr.x / m), -(pr.y / m), -(pr.z / m)};
    return true;
}

template <class T, bool DUAL>
__global__ __launch_bounds__(NORMALS_TILE_W* NORMALS_TILE_H) void k_normals(NormalsArgs a) {
    const uint32_t v = blockIdx.x * NORMALS_TILE_W + threadIdx.x, u = blockIdx.y * NORMALS_TILE_H + threadIdx.y;
    if (u >= a.h || v >= a.w) return;
    const uint32_t frame = blockIdx.z / a.n_ret, ret = blockIdx.z - frame * a.n_ret;
    const size_t plane = (size_t)a.h * a.w, fbase = (size_t)frame * plane;
    const void* xyz = a.xyz[ret];
    const uint32_t* rng = a.range[ret];
    const void* xyz_o = DUAL ? a.xyz[1 - ret] : nullptr;       // the other return's pixels are candidates as well
    const uint32_t* rng_o = DUAL ? a.range[1 - ret] : nullptr;
    const double* k = a.consts + (size_t)blockIdx.z * 4;
    const double px_res_h = k[0], px_res_v = k[1], tan_safe = k[2], target_sq = k[3];
    const uint32_t psr = a.pixel_search_range;

    const size_t row_base = fbase + (size_t)u * a.w;
    const size_t src = row_base + src_col(a, u, v);
    double* o = a.out[ret] + 3 * (a.staggered_out ? src : row_base + v);
    V3 normal{0.0, 0.0, 0.0};
    const uint32_t center_range = rng[src];
    if (center_range != 0) {
        const V3 center = load3<T>(xyz, src);
        const V3 beam = beam_of(center, origin_of(a, frame, v));
        if (!(dot3(beam, beam) <= EPS)) {
            const double perimeter_m = TWO_PI * ((double)center_range * 0.001);
            const double nd_h = (perimeter_m / px_res_h) / tan_safe, nd_h_sq = nd_h * nd_h;
            const double nd_v = (perimeter_m / px_res_v) / tan_safe, nd_v_sq = nd_v * nd_v;
            const uint32_t max_up = min(psr, u), max_down = min(psr, a.h - 1 - u);

            // vertical: up, down, up of the other return, down of the other return
            Search sv{V3{0.0, 0.0, 0.0}, __builtin_inf(), 1u, false, true};
            bool v_good = false;
            for (uint32_t radius = 1; radius <= psr; ++radius) {
                if (radius > max_up && radius > max_down) break;
                if (v_good && !sv.thin) break;
                const bool up = radius <= max_up, down = radius <= max_down;
                const size_t i_up = up ? fbase + (size_t)(u - radius) * a.w + src_col(a, u - radius, v) : 0;
                const size_t i_down = down ? fbase + (size_t)(u + radius) * a.w + src_col(a, u + radius, v) : 0;
                if (up) consider<T>(sv, xyz, rng, i_up, center, center_range, target_sq, true, radius);
                if (down) consider<T>(sv, xyz, rng, i_down, center, center_range, target_sq, false, radius);
                if (DUAL) {
                    if (up) consider<T>(sv, xyz_o, rng_o, i_up, center, center_range, target_sq, true, radius);
                    if (down) consider<T>(sv, xyz_o, rng_o, i_down, center, center_range, target_sq, false, radius);
                }
                const double limit = ((double)sv.best_radius * (double)sv.best_radius) * nd_v_sq;
                if (target_sq <= sv.min_distance_sq && sv.min_distance_sq < limit) v_good = true;
                else if (radius == psr && sv.min_distance_sq > 0 && sv.min_distance_sq < limit) v_good = true;
            }
            const bool v_found = v_good && sv.min_distance_sq < __builtin_inf();

            // horizontal, wrapping: left, left of the other return, right, right of the other return
            Search sh{V3{0.0, 0.0, 0.0}, __builtin_inf(), 1u, false, true};
            bool h_good = false;
            const uint32_t shift = a.shifts ? a.shifts[u] : 0u;
            for (uint32_t radius = 1; radius <= psr; ++radius) {
                if (h_good && !sh.thin) break;
                const uint32_t r = radius % a.w;
                uint32_t left = v + a.w - r, right = v + r;   // both in [0, 2 w)
                if (left >= a.w) left -= a.w;
                if (right >= a.w) right -= a.w;
                left += a.w - shift;                          // to source columns
                right += a.w - shift;
                if (left >= a.w) left -= a.w;
                if (right >= a.w) right -= a.w;
                consider<T>(sh, xyz, rng, row_base + left, center, center_range, target_sq, true, radius);
                if (DUAL) consider<T>(sh, xyz_o, rng_o, row_base + left, center, center_range, target_sq, true, radius);
                consider<T>(sh, xyz, rng, row_base + right, center, center_range, target_sq, false, radius);
                if (DUAL) consider<T>(sh, xyz_o, rng_o, row_base + right, center, center_range, target_sq, false, radius);
                const double limit = ((double)sh.best_radius * (double)sh.best_radius) * nd_h_sq;
                if (target_sq <= sh.min_distance_sq && sh.min_distance_sq < limit) h_good = true;
                else if (radius == psr && sh.min_distance_sq > 0 && sh.min_distance_sq < limit) h_good = true;
            }
            const bool h_found = h_good && sh.min_distance_sq < __builtin_inf();

            if ((!v_found && !h_found) || (sv.thin && sh.thin)) {
                normal = V3{-beam.x, -beam.y, -beam.z};                                   // case A
            } else if (v_found && (!h_found || sh.thin)) {
                V3 n;
                if (perpendicular(sv.best_diff, beam, n)) normal = n;                      // case B, vertical
            } else if (h_found && (!v_found || sv.thin)) {
                V3 n;
                if (perpendicular(sh.best_diff, beam, n)) normal = n;                      // case B, horizontal
            } else {                                                                       // case C
                V3 vd = sv.best_diff;
                const V3 hd = sh.best_diff;
                if (sh.best_flip != sv.best_flip) vd = V3{-vd.x, -vd.y, -vd.z};
                const V3 c{vd.y * hd.z - vd.z * hd.y, vd.z * hd.x - vd.x * hd.z, vd.x * hd.y - vd.y * hd.x};
                const double m = sqrt(dot3(c, c));
                if (m != 0.0) normal = V3{c.x / m, c.y / m, c.z / m};
            }
        }
    }
    o[0] = normal.x;
    o[1] = normal.y;
    o[2] = normal.z;
}

}  // namespace

hipError_t launch_normals_subtent(const NormalsArgs& a, hipStream_t st) {
    const uint64_t blocks = (uint64_t)a.n_frames * a.n_ret;
    if (blocks == 0 || a.h == 0 || a.w == 0) return hipSuccess;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    if (a.f32) hipLaunchKernelGGL(k_normals_subtent<float>, dim3((uint32_t)blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_normals_subtent<double>, dim3((uint32_t)blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_normals(const NormalsArgs& a, hipStream_t st) {
    const uint64_t z = (uint64_t)a.n_frames * a.n_ret;
    if (z == 0 || a.h == 0 || a.w == 0) return hipSuccess;
    const uint32_t gx = (a.w + NORMALS_TILE_W - 1) / NORMALS_TILE_W, gy = (a.h + NORMALS_TILE_H - 1) / NORMALS_TILE_H;
    if (z > 65535 || gy > 65535) return hipErrorInvalidValue;
    const dim3 grid(gx, gy, (uint32_t)z), wg(NORMALS_TILE_W, NORMALS_TILE_H);
    const bool dual = a.n_ret == 2;
    if (a.f32) {
        if (dual) hipLaunchKernelGGL((k_normals<float, true>), grid, wg, 0, st, a);
        else hipLaunchKernelGGL((k_normals<float, false>), grid, wg, 0, st, a);
    } else {
        if (dual) hipLaunchKernelGGL((k_normals<double, true>), grid, wg, 0, st, a);
        else hipLaunchKernelGGL((k_normals<double, false>), grid, wg, 0, st, a);
    }
    return hipGetLastError();
}

}  // namespace ouster_hip_dev
