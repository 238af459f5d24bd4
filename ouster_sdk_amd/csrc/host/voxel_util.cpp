// voxel_util.cpp -- the plain C++ half of voxel down-sampling inside libouster_hip.so: what is refused, with the reference's
// messages, and ouster_hip_voxel_downsample_ref, the restatement of core::voxel_downsample_3d / _xd and
// algorithm::voxel_downsample_with_normals on one core (ouster_core/src/voxel_hash_map.cpp:312-393,
// include/ouster/core/voxel_hash_map.h, ouster_algorithm/src/voxel_downsample.cpp).  Built with -ffp-contract=off, an object of
// its own (Makefile): its rows are compared bit for bit with tests/voxel_model.py.  Rows come in first-seen order.
#include <cmath>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "../voxel_host.h"

namespace ouster_hip_dev {

const char* voxel_validate(const ouster_hip_voxel_desc* d) {
    if (d->normals) {
        if (d->cols != 3) return "voxel_downsample_with_normals expects Nx3 inputs";
        if (!(d->voxel_size > 0.0) || !std::isfinite(d->voxel_size)) return "voxel_downsample_with_normals voxel_size must be > 0";
        return nullptr;
    }
    if (d->cols < 3) return "voxel_downsample_xd: frame must be Nx>=3 (x,y,z + optional attributes)";
    if (d->strategy != OUSTER_HIP_VOXEL_FIRST_N_POINT && d->strategy != OUSTER_HIP_VOXEL_AVERAGE_POINT &&
        d->strategy != OUSTER_HIP_VOXEL_RANDOM)
        return "voxel_downsample: unknown strategy";
    if (d->max_points_per_voxel == 0) return "max_points_per_voxel must be greater than 0";
    if (!(d->voxel_size > 0.0) || !std::isfinite(d->voxel_size)) return "voxel_size must be greater than 0";
    return nullptr;
}

VoxelForm voxel_form(const ouster_hip_voxel_desc* d) {
    if (d->normals) return VOXEL_FORM_NORMALS;
    if (d->strategy == OUSTER_HIP_VOXEL_AVERAGE_POINT) return VOXEL_FORM_AVERAGE;
    if (d->max_points_per_voxel != 1) return VOXEL_FORM_HOST;
    return d->strategy == OUSTER_HIP_VOXEL_FIRST_N_POINT ? VOXEL_FORM_FIRST : VOXEL_FORM_LAST;
}

namespace {

struct Key {
    int32_t v[3];
    bool operator==(const Key& o) const { return v[0] == o.v[0] && v[1] == o.v[1] && v[2] == o.v[2]; }
};
struct KeyHash {
    size_t operator()(const Key& k) const {
        return ((size_t)(uint32_t)k.v[0] * 73856093u) ^ ((size_t)(uint32_t)k.v[1] * 19349669u) ^ ((size_t)(uint32_t)k.v[2] * 83492791u);
    }
};

// VoxelHashMap::point_to_voxel; false where the reference's static_cast<int> is undefined
bool point_to_voxel(const double* p, double inv, Key& key) {
    for (int k = 0; k < 3; ++k) {
        const double f = std::floor(p[k] * inv);
        if (!(f >= -2147483648.0 && f <= 2147483647.0)) return false;
        key.v[k] = static_cast<int32_t>(f);
    }
    return true;
}

struct Bucket {
    uint64_t count = 0;          // AVERAGE_POINT, with normals: points folded in
    std::vector<double> sum;     // AVERAGE_POINT: cols sums; with normals: point sum, then the sum of the unit normals
    std::vector<double> points;  // FIRST_N_POINT, RANDOM: the kept rows, cols each, in admission order
};

struct Rows {
    const ouster_hip_voxel_desc* d;
    uint64_t stride;
    void load(uint64_t i, double* row) const {
        if (d->dtype == OUSTER_HIP_F32) {
            const float* p = static_cast<const float*>(d->points) + i * stride;
            for (uint32_t c = 0; c < d->cols; ++c) row[c] = static_cast<double>(p[c]);
        } else {
            std::memcpy(row, static_cast<const double*>(d->points) + i * stride, sizeof(double) * d->cols);
        }
    }
};

bool finite3(const double* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

}  // namespace
}  // namespace ouster_hip_dev

extern "C" int ouster_hip_voxel_downsample_ref(const ouster_hip_voxel_desc* d, uint64_t* n_out) {
    using namespace ouster_hip_dev;
    if (!d || !n_out) return fail_msg(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
    *n_out = 0;
    if (d->n == 0 && !d->normals) return OUSTER_HIP_OK;
    if (const char* msg = voxel_validate(d)) return fail_msg(OUSTER_HIP_ERR_INVALID_ARGUMENT, msg);
    if (d->dtype != OUSTER_HIP_F32 && d->dtype != OUSTER_HIP_F64) return fail_msg(OUSTER_HIP_ERR_INVALID_ARGUMENT, "dtype must be F32 or F64");
    if (d->row_stride && d->row_stride < d->cols) return fail_msg(OUSTER_HIP_ERR_INVALID_ARGUMENT, "row_stride is smaller than cols");
    if (d->n == 0) return OUSTER_HIP_OK;
    if (!d->points || (d->out_capacity && (!d->out || (d->normals && !d->out_normals))))
        return fail_msg(OUSTER_HIP_ERR_INVALID_ARGUMENT, "NULL pointer");
    const uint32_t cols = d->cols;
    const Rows rows{d, d->row_stride ? d->row_stride : cols};
    const VoxelForm form = voxel_form(d);
    const bool average = form == VOXEL_FORM_AVERAGE, with_normals = form == VOXEL_FORM_NORMALS;
    const bool first_n = !average && !with_normals && d->strategy == OUSTER_HIP_VOXEL_FIRST_N_POINT;
    const double inv = 1.0 / d->voxel_size;
    const uint64_t max_points = d->max_points_per_voxel;
    const double resolution_sq = d->voxel_size * d->voxel_size / static_cast<double>(max_points);
    uint32_t rng = 42u;

    std::unordered_map<Key, size_t, KeyHash> index;
    std::vector<Bucket> buckets;   // first seen first
    std::vector<double> row(with_normals ? 6 : cols);
    for (uint64_t i = 0; i < d->n; ++i) {
        rows.load(i, row.data());
        if (with_normals) {
            double* m = row.data() + 3;
            std::memcpy(m, d->normals + 3 * i, 3 * sizeof(double));
            if (!finite3(row.data()) || !finite3(m)) continue;
            const double len = std::sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
            if (len <= 1e-12) continue;
            for (int k = 0; k < 3; ++k) m[k] = m[k] / len;
        }
        Key key;
        if (!point_to_voxel(row.data(), inv, key)) return fail_msg(OUSTER_HIP_ERR_INVALID_ARGUMENT, VOXEL_MSG_GRID);
        auto it = index.find(key);
        if (it == index.end()) {
            it = index.emplace(key, buckets.size()).first;
            buckets.emplace_back();
            if (average || with_normals) buckets.back().sum.assign(row.size(), 0.0);
        }
        Bucket& b = buckets[it->second];
        if (average || with_normals) {
            for (size_t c = 0; c < row.size(); ++c) b.sum[c] = b.sum[c] + row[c];
            ++b.count;
        } else if (first_n) {
            const uint64_t held = b.points.size() / cols;
            if (held == max_points) continue;
            bool close = false;
            for (uint64_t q = 0; q < held && !close; ++q) {
                const double* v = b.points.data() + q * cols;
                const double dx = v[0] - row[0], dy = v[1] - row[1], dz = v[2] - row[2];
                close = (dx * dx + dy * dy) + dz * dz < resolution_sq;
            }
            if (!close) b.points.insert(b.points.end(), row.begin(), row.end());
        } else {
            const uint64_t held = b.points.size() / cols;
            if (held < max_points) {
                b.points.insert(b.points.end(), row.begin(), row.end());
            } else {
                rng ^= rng << 13;
                rng ^= rng >> 17;
                rng ^= rng << 5;
                // (uint64(rand) * max_points_per_voxel) >> 32 of the reference, in 128 bits so that no size_t value wraps
                const uint64_t j = static_cast<uint64_t>((static_cast<unsigned __int128>(rng) * max_points) >> 32);
                std::memcpy(b.points.data() + j * cols, row.data(), sizeof(double) * cols);
            }
        }
    }

    // count first: a result that does not fit writes nothing
    uint64_t total = 0;
    std::vector<double> norm_len(with_normals ? buckets.size() : 0);
    for (size_t v = 0; v < buckets.size(); ++v) {
        const Bucket& b = buckets[v];
        if (average) {
            total += b.count >= d->min_pts_threshold;
        } else if (with_normals) {
            const double* s = b.sum.data() + 3;
            norm_len[v] = std::sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
            total += !(norm_len[v] <= 1e-12);
        } else {
            total += b.points.size() / cols;
        }
    }
    *n_out = total;
    if (total > d->out_capacity) return fail_msg(OUSTER_HIP_ERR_INVALID_ARGUMENT, "voxel_downsample: out_capacity is too small");
    uint64_t r = 0;
    for (size_t v = 0; v < buckets.size(); ++v) {
        const Bucket& b = buckets[v];
        if (average) {
            if (b.count < d->min_pts_threshold) continue;
            for (uint32_t c = 0; c < cols; ++c) d->out[r * cols + c] = b.sum[c] / static_cast<double>(b.count);
            ++r;
        } else if (with_normals) {
            if (norm_len[v] <= 1e-12) continue;
            for (int c = 0; c < 3; ++c) {
                d->out[r * 3 + c] = b.sum[c] / static_cast<double>(b.count);
                d->out_normals[r * 3 + c] = b.sum[3 + c] / norm_len[v];
            }
            ++r;
        } else {
            std::memcpy(d->out + r * cols, b.points.data(), b.points.size() * sizeof(double));
            r += b.points.size() / cols;
        }
    }
    return OUSTER_HIP_OK;
}
