// image_processing.cpp -- host half of AutoExposure / BeamUniformityCorrector / LocalToneMapper
// (include/ouster/core/image_processing.h).
//
// The state machines of the reference (ouster_core/src/image_processing.cpp:201-384, :415-506 and :508-604), operation by
// operation in double; everything per pixel and every order statistic comes from the kernels behind ouster_hip_image_*
// (csrc/k_image.hip, csrc/k_tonemap.hip).
// every product and sum below is rounded on its own, as in the reference's build: no contraction into fused multiply-adds
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif
#include "ouster/core/image_processing.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <type_traits>

#include "host_internal.h"
#include "ouster_hip.h"

namespace ouster {
namespace sdk {
namespace core {
namespace image {

namespace {
const double AE_DEFAULT_DAMPING = 0.90;
const int AE_DEFAULT_UPDATE_EVERY = 3;
const uint32_t AE_MIN_NONZERO_POINTS = 100;
const double AE_DEFAULT_PERCENTILE = 0.1;
const double BUC_DAMPING = 0.92;

template <typename T> constexpr int tag() {
    return std::is_same<typename std::remove_const<T>::type, float16_t>::value ? OUSTER_HIP_F16
           : std::is_same<typename std::remove_const<T>::type, float>::value   ? OUSTER_HIP_F32
                                                                                : OUSTER_HIP_F64;
}
const uint32_t TONEMAP_MIN_DIM = 8;   // LocalToneMapper's 8 x 8 tiles must not be empty

void* scratch(ouster_hip_ctx* c, uint32_t slot, size_t bytes) {
    void* p = nullptr;
    hip::check(ouster_hip_ctx_scratch(c, slot, bytes, &p));
    return p;
}
uint32_t dim32(size_t v) {
    if (v > 0xffffffffull) throw std::invalid_argument("image dimension too large");
    return static_cast<uint32_t>(v);
}
}  // namespace

AutoExposure::AutoExposure()
    : lo_percentile_(AE_DEFAULT_PERCENTILE), hi_percentile_(AE_DEFAULT_PERCENTILE), ae_update_every_(AE_DEFAULT_UPDATE_EVERY),
      damping_(AE_DEFAULT_DAMPING) {}
AutoExposure::AutoExposure(int update_every)
    : lo_percentile_(AE_DEFAULT_PERCENTILE), hi_percentile_(AE_DEFAULT_PERCENTILE), ae_update_every_(update_every),
      damping_(AE_DEFAULT_DAMPING) {}
AutoExposure::AutoExposure(double lo_percentile, double hi_percentile, int update_every, double damping)
    : lo_percentile_(lo_percentile), hi_percentile_(hi_percentile), ae_update_every_(update_every), damping_(damping) {}

// AutoExposure::apply (image_processing.cpp:224-295) with the sample's statistics already known
void AutoExposure::step(uint32_t n, double lo, double hi, bool update_state, ::ouster_hip_image_map& map) {
    map.mode = OUSTER_HIP_IMAGE_MAP_NONE;
    map.sub = 0.0;
    map.mul = 1.0;
    map.add = 0.0;
    if (counter_ == 0 && update_state) {
        if (n < AE_MIN_NONZERO_POINTS) return;   // too few nonzero values: nothing happens, the counter included
        lo_ = lo;
        hi_ = hi;
        if (!initialized_) {
            initialized_ = true;
            lo_state_ = lo_;
            hi_state_ = hi_;
        }
    }
    if (!initialized_) return;
    if (update_state) {
        lo_state_ = damping_ * lo_state_ + (1.0 - damping_) * lo_;
        hi_state_ = damping_ * hi_state_ + (1.0 - damping_) * hi_;
    }
    const double lo_hi_scale = (1.0 - (lo_percentile_ + hi_percentile_)) / (hi_state_ - lo_state_);
    if (std::isinf(lo_hi_scale) || std::isnan(lo_hi_scale)) {
        map.mode = OUSTER_HIP_IMAGE_MAP_SCALE;
        map.mul = 0.5 / hi_state_;
    } else if (lo_hi_scale * (0.0 - lo_state_) + lo_percentile_ <= 0.00) {
        map.mode = OUSTER_HIP_IMAGE_MAP_AFFINE;
        map.sub = lo_state_;
        map.mul = lo_hi_scale;
        map.add = lo_percentile_;
    } else {
        map.mode = OUSTER_HIP_IMAGE_MAP_SCALE;
        map.mul = (1.0 - hi_percentile_) / hi_state_;
    }
    if (update_state) counter_ = (counter_ + 1) % ae_update_every_;
}

template <typename T>
void AutoExposure::apply(ImgRef<T> image, bool update_state) {
    ouster_hip_ctx* c = hip::default_ctx();   // throws without a GPU, before anything is touched
    const uint32_t h = dim32(image.rows()), w = dim32(image.cols());
    uint32_t n = 0;
    T lo_hi[2] = {0, 0};
    if (wants_percentiles(update_state) && image.size())
        hip::check(ouster_hip_image_percentiles_host(c, image.data(), tag<T>(), h, w, nullptr, lo_percentile_, hi_percentile_,
                                                     &n, lo_hi));
    ::ouster_hip_image_map map{};
    step(n, static_cast<double>(lo_hi[0]), static_cast<double>(lo_hi[1]), update_state, map);
    if (map.mode != OUSTER_HIP_IMAGE_MAP_NONE)
        hip::check(ouster_hip_image_apply_host(c, image.data(), tag<T>(), h, w, nullptr, &map));
}

void AutoExposure::update(ImgRef<float> image, bool update_state) { apply(image, update_state); }
void AutoExposure::update(ImgRef<double> image, bool update_state) { apply(image, update_state); }

template <typename T>
void AutoExposure::update_batch(hip::Context& ctx, const void* planes, ChanFieldType elem_type, uint32_t n_images, uint32_t h,
                                uint32_t w, T* out_images, bool update_state, size_t in_stride, size_t out_stride) {
    if (n_images == 0 || h == 0 || w == 0) return;
    ouster_hip_ctx* c = ctx.handle();
    const int in_type = static_cast<int>(elem_type);
    std::vector<uint32_t> n(n_images, 0);
    std::vector<T> lo_hi(2 * static_cast<size_t>(n_images), T(0));
    if (update_state) {
        // every image's statistics in one launch: which images need them depends on the early returns before them
        uint8_t* d = static_cast<uint8_t*>(scratch(c, 6, static_cast<size_t>(n_images) * (8 + 2 * sizeof(T))));
        uint32_t* d_n = reinterpret_cast<uint32_t*>(d + 2 * sizeof(T) * n_images);
        hip::check(ouster_hip_image_percentiles(c, planes, in_type, tag<T>(), n_images, h, w, in_stride, nullptr, lo_percentile_,
                                                hi_percentile_, d_n, d));
        hip::check(ouster_hip_copy_out(c, lo_hi.data(), d, lo_hi.size() * sizeof(T)));
        hip::check(ouster_hip_copy_out(c, n.data(), d_n, n.size() * 4));
        hip::check(ouster_hip_sync(c));
    }
    std::vector<::ouster_hip_image_map> maps(n_images);
    for (uint32_t i = 0; i < n_images; ++i) {
        step(n[i], static_cast<double>(lo_hi[2 * i]), static_cast<double>(lo_hi[2 * i + 1]), update_state, maps[i]);
        maps[i].use_dark = 0;
    }
    void* d_maps = scratch(c, 7, maps.size() * sizeof(maps[0]));
    hip::check(ouster_hip_copy_in(c, d_maps, maps.data(), maps.size() * sizeof(maps[0])));
    hip::check(ouster_hip_image_apply(c, planes, in_type, out_images, tag<T>(), n_images, h, w, in_stride, out_stride, nullptr,
                                      static_cast<const ::ouster_hip_image_map*>(d_maps)));
    hip::check(ouster_hip_sync(c));
}
template void AutoExposure::update_batch<float>(hip::Context&, const void*, ChanFieldType, uint32_t, uint32_t, uint32_t, float*,
                                                bool, size_t, size_t);
template void AutoExposure::update_batch<double>(hip::Context&, const void*, ChanFieldType, uint32_t, uint32_t, uint32_t, double*,
                                                 bool, size_t, size_t);

// AutoExposure::apply on RGB images (:307-384): the same state machine on the luminance sample, the map on every element
template <typename TIN, typename T>
void AutoExposure::apply_rgb(RgbImgRef<TIN> in, RgbImgRef<T> out, bool update_state) {
    if (in.rows() != out.rows() || in.cols() != out.cols()) throw std::invalid_argument("AutoExposure: input and output shapes differ");
    ouster_hip_ctx* c = hip::default_ctx();   // throws without a GPU, before anything is touched
    const uint32_t h = dim32(in.rows()), w = dim32(in.cols());
    uint32_t n = 0;
    T lo_hi[2] = {0, 0};
    if (wants_percentiles(update_state) && in.size())
        hip::check(ouster_hip_image_lum_percentiles_host(c, in.data(), tag<TIN>(), tag<T>(), h, w, lo_percentile_, hi_percentile_, &n, lo_hi));
    ::ouster_hip_image_map map{};
    step(n, static_cast<double>(lo_hi[0]), static_cast<double>(lo_hi[1]), update_state, map);
    hip::check(ouster_hip_image_apply_rgb_host(c, in.data(), tag<TIN>(), out.data(), tag<T>(), h, w, &map));
}

void AutoExposure::update(RgbImgRef<float> image, bool update_state) { apply_rgb(image, image, update_state); }
void AutoExposure::update(RgbImgRef<double> image, bool update_state) { apply_rgb(image, image, update_state); }
void AutoExposure::update(RgbImgRef<const float16_t> input, RgbImgRef<float> out, bool update_state) { apply_rgb(input, out, update_state); }

namespace {
// every image's luminance statistics in one launch (which images need them depends on the early returns before them)
template <typename T>
void batch_lum_stats(ouster_hip_ctx* c, const void* images, int in_type, uint32_t n_images, uint32_t h, uint32_t w, size_t in_stride,
                     double lo_percentile, double hi_percentile, std::vector<uint32_t>& n, std::vector<T>& lo_hi) {
    uint8_t* d = static_cast<uint8_t*>(scratch(c, 6, static_cast<size_t>(n_images) * (8 + 2 * sizeof(T))));
    uint32_t* d_n = reinterpret_cast<uint32_t*>(d + 2 * sizeof(T) * n_images);
    hip::check(ouster_hip_image_lum_percentiles(c, images, in_type, tag<T>(), n_images, h, w, in_stride, lo_percentile, hi_percentile, d_n, d));
    hip::check(ouster_hip_copy_out(c, lo_hi.data(), d, lo_hi.size() * sizeof(T)));
    hip::check(ouster_hip_copy_out(c, n.data(), d_n, n.size() * 4));
    hip::check(ouster_hip_sync(c));
}
}  // namespace

template <typename T>
void AutoExposure::update_batch_rgb(hip::Context& ctx, const void* images, ChanFieldType elem_type, uint32_t n_images, uint32_t h,
                                    uint32_t w, T* out_images, bool update_state, size_t in_stride, size_t out_stride) {
    if (3ull * w > 0xffffffffull) throw std::invalid_argument("image dimension too large");   // before any state changes
    if (n_images == 0 || h == 0 || w == 0) return;   // an empty image: nothing to do, as in the single-channel update_batch
    ouster_hip_ctx* c = ctx.handle();
    const int in_type = static_cast<int>(elem_type);
    std::vector<uint32_t> n(n_images, 0);
    std::vector<T> lo_hi(2 * static_cast<size_t>(n_images), T(0));
    if (update_state) batch_lum_stats<T>(c, images, in_type, n_images, h, w, in_stride, lo_percentile_, hi_percentile_, n, lo_hi);
    std::vector<::ouster_hip_image_map> maps(n_images);
    for (uint32_t i = 0; i < n_images; ++i) {
        step(n[i], static_cast<double>(lo_hi[2 * i]), static_cast<double>(lo_hi[2 * i + 1]), update_state, maps[i]);
        maps[i].use_dark = 0;
    }
    void* d_maps = scratch(c, 7, maps.size() * sizeof(maps[0]));
    hip::check(ouster_hip_copy_in(c, d_maps, maps.data(), maps.size() * sizeof(maps[0])));
    hip::check(ouster_hip_image_apply(c, images, in_type, out_images, tag<T>(), n_images, h, 3 * w, in_stride, out_stride, nullptr,
                                      static_cast<const ::ouster_hip_image_map*>(d_maps)));
    hip::check(ouster_hip_sync(c));
}
template void AutoExposure::update_batch_rgb<float>(hip::Context&, const void*, ChanFieldType, uint32_t, uint32_t, uint32_t, float*,
                                                    bool, size_t, size_t);
template void AutoExposure::update_batch_rgb<double>(hip::Context&, const void*, ChanFieldType, uint32_t, uint32_t, uint32_t, double*,
                                                     bool, size_t, size_t);

// ---- LocalToneMapper (:508-604: constructors and the state machine; the rest of apply is ouster_hip_image_tonemap) ---------
LocalToneMapper::LocalToneMapper() : lo_percentile_(0.0), hi_percentile_(0.2), update_every_(1), damping_(0.3) {}
LocalToneMapper::LocalToneMapper(int update_every) : lo_percentile_(0.0), hi_percentile_(0.2), update_every_(update_every), damping_(0.3) {}
LocalToneMapper::LocalToneMapper(double lo_percentile, double hi_percentile, int update_every, double damping, double compress_dr_max_lum,
                                 bool color_correct)
    : lo_percentile_(lo_percentile), hi_percentile_(hi_percentile), update_every_(update_every), damping_(damping),
      compress_dr_max_lum_(compress_dr_max_lum), color_correct_(color_correct) {}
LocalToneMapper::LocalToneMapper(double lo_percentile, double hi_percentile, int update_every, double damping, bool compress_dr,
                                 bool color_correct)
    : lo_percentile_(lo_percentile), hi_percentile_(hi_percentile), update_every_(update_every), damping_(damping),
      compress_dr_max_lum_(compress_dr ? 0.2 : 0.0), color_correct_(color_correct) {}

// LocalToneMapper::apply (:538-604, :610, :647-652) with the sample's statistics already known
void LocalToneMapper::step(uint32_t n, double lo, double hi, bool update_state, ::ouster_hip_tonemap_params& params) {
    params = ::ouster_hip_tonemap_params{};
    params.map.mode = OUSTER_HIP_IMAGE_MAP_NONE;
    params.map.mul = 1.0;
    params.color_ramp = 1.0;
    params.color_correct = color_correct_ ? 1 : 0;
    if (counter_ == 0 && update_state) {
        if (n < AE_MIN_NONZERO_POINTS) return;   // too few positive luminances: nothing happens, the counter included
        lo_ = lo;
        hi_ = hi;
        if (!initialized_) {
            initialized_ = true;
            lo_state_ = lo_;
            hi_state_ = hi_;
        }
    }
    if (!initialized_) return;
    if (update_state) {
        lo_state_ = damping_ * lo_state_ + (1.0 - damping_) * lo_;
        hi_state_ = damping_ * hi_state_ + (1.0 - damping_) * hi_;
    }
    const double lo_hi_scale = (1.0 - (lo_percentile_ + hi_percentile_)) / (hi_state_ - lo_state_);
    if (std::isinf(lo_hi_scale) || std::isnan(lo_hi_scale)) {
        params.map.mode = OUSTER_HIP_IMAGE_MAP_SCALE;
        params.map.mul = 0.5 / hi_state_;
    } else if (lo_hi_scale * (0.0 - lo_state_) + lo_percentile_ <= 0.0) {
        params.map.mode = OUSTER_HIP_IMAGE_MAP_AFFINE;
        params.map.sub = lo_state_;
        params.map.mul = lo_hi_scale;
        params.map.add = lo_percentile_;
    } else {
        params.map.mode = OUSTER_HIP_IMAGE_MAP_SCALE;
        params.map.mul = (1.0 - hi_percentile_) / hi_state_;
    }
    if (update_state) counter_ = (counter_ + 1) % update_every_;
    params.compress = hi_state_ < compress_dr_max_lum_ ? 1 : 0;
    // the saturation fades out in dark scenes: the kernel multiplies T(0.75) by this ratio rounded to T (ramp from 0.5 to 1.0)
    if (hi_state_ < 1.0) params.color_ramp = std::max(0.0, (hi_state_ - 0.5) / 0.5);
}

template <typename TIN, typename T>
void LocalToneMapper::apply(RgbImgRef<TIN> in, RgbImgRef<T> out, bool update_state) {
    if (in.rows() != out.rows() || in.cols() != out.cols()) throw std::invalid_argument("LocalToneMapper: input and output shapes differ");
    if (in.rows() < TONEMAP_MIN_DIM || in.cols() < TONEMAP_MIN_DIM)
        throw std::invalid_argument("LocalToneMapper: the image must have at least 8 rows and 8 columns");
    ouster_hip_ctx* c = hip::default_ctx();   // throws without a GPU, before anything is touched
    const uint32_t h = dim32(in.rows()), w = dim32(in.cols());
    uint32_t n = 0;
    T lo_hi[2] = {0, 0};
    if (wants_percentiles(update_state))
        hip::check(ouster_hip_image_lum_percentiles_host(c, in.data(), tag<TIN>(), tag<T>(), h, w, lo_percentile_, hi_percentile_, &n, lo_hi));
    ::ouster_hip_tonemap_params params;
    step(n, static_cast<double>(lo_hi[0]), static_cast<double>(lo_hi[1]), update_state, params);
    hip::check(ouster_hip_image_tonemap_host(c, in.data(), tag<TIN>(), out.data(), tag<T>(), h, w, &params));
}

void LocalToneMapper::update(RgbImgRef<float> image, bool update_state) { apply(image, image, update_state); }
void LocalToneMapper::update(RgbImgRef<double> image, bool update_state) { apply(image, image, update_state); }
void LocalToneMapper::update(RgbImgRef<const float16_t> input, RgbImgRef<float> output, bool update_state) { apply(input, output, update_state); }

template <typename T>
void LocalToneMapper::update_batch(hip::Context& ctx, const void* images, ChanFieldType elem_type, uint32_t n_images, uint32_t h,
                                   uint32_t w, T* out_images, bool update_state, size_t in_stride, size_t out_stride) {
    if (n_images == 0) return;
    if (h < TONEMAP_MIN_DIM || w < TONEMAP_MIN_DIM) throw std::invalid_argument("LocalToneMapper: the image must have at least 8 rows and 8 columns");
    ouster_hip_ctx* c = ctx.handle();
    const int in_type = static_cast<int>(elem_type);
    std::vector<uint32_t> n(n_images, 0);
    std::vector<T> lo_hi(2 * static_cast<size_t>(n_images), T(0));
    if (update_state) batch_lum_stats<T>(c, images, in_type, n_images, h, w, in_stride, lo_percentile_, hi_percentile_, n, lo_hi);
    std::vector<::ouster_hip_tonemap_params> params(n_images);
    for (uint32_t i = 0; i < n_images; ++i)
        step(n[i], static_cast<double>(lo_hi[2 * i]), static_cast<double>(lo_hi[2 * i + 1]), update_state, params[i]);
    void* d_params = scratch(c, 7, params.size() * sizeof(params[0]));
    hip::check(ouster_hip_copy_in(c, d_params, params.data(), params.size() * sizeof(params[0])));
    hip::check(ouster_hip_image_tonemap(c, images, in_type, out_images, tag<T>(), n_images, h, w, in_stride, out_stride,
                                        static_cast<const ::ouster_hip_tonemap_params*>(d_params)));
    hip::check(ouster_hip_sync(c));   // `params` is the pageable source of an asynchronous copy
}
template void LocalToneMapper::update_batch<float>(hip::Context&, const void*, ChanFieldType, uint32_t, uint32_t, uint32_t, float*, bool,
                                                   size_t, size_t);
template void LocalToneMapper::update_batch<double>(hip::Context&, const void*, ChanFieldType, uint32_t, uint32_t, uint32_t, double*, bool,
                                                    size_t, size_t);

// BeamUniformityCorrector::apply (:478-491) around compute_dark_count (:427-474) with the row medians already known.
// The "linear fit" of :462-469 is fullPivLu().solve() on the h x 2 system [1 i]: full pivoting takes the element h - 1 in row
// h - 1 first, then the 1 in row 0, so the solve returns the line through the first and the last entry -- intercept d[0] = 0,
// slope d[h - 1] / T(h - 1) -- and row i loses T(i) * slope.
template <typename T>
void BeamUniformityCorrector::step(const T* medians, uint32_t n_cols, size_t h, bool update_state) {
    const bool first = dark_count_.size() != h;
    if (first || (update_state && counter_ == 0)) {
        std::vector<T> d(h, T(0));
        if (n_cols != 0 && h >= 2) {
            for (size_t i = 1; i < h; ++i) d[i] = d[i - 1] + medians[i - 1];
            const T slope = d[h - 1] / static_cast<T>(h - 1);
            for (size_t i = 0; i < h; ++i) {
                const T fit = static_cast<T>(i) * slope;
                d[i] = d[i] - fit;
            }
            const T mn = *std::min_element(d.begin(), d.end());
            for (size_t i = 0; i < h; ++i) d[i] = d[i] - mn;
        }
        if (first) {
            dark_count_.assign(d.begin(), d.end());
        } else {
            for (size_t i = 0; i < h; ++i) {
                dark_count_[i] = dark_count_[i] * BUC_DAMPING;
                const double add = static_cast<double>(d[i]) * (1.0 - BUC_DAMPING);
                dark_count_[i] = dark_count_[i] + add;
            }
        }
    }
    step_keep();
}
template void BeamUniformityCorrector::step<float>(const float*, uint32_t, size_t, bool);
template void BeamUniformityCorrector::step<double>(const double*, uint32_t, size_t, bool);

template <typename T>
void BeamUniformityCorrector::apply(ImgRef<T> image, bool update_state) {
    ouster_hip_ctx* c = hip::default_ctx();
    const uint32_t h = dim32(image.rows()), w = dim32(image.cols());
    if (image.size() == 0) return;
    if (wants_dark_rows(h, update_state)) {
        std::vector<T> med(h > 1 ? h - 1 : 0);
        uint32_t n_cols = 0;
        if (h >= 2) hip::check(ouster_hip_image_dark_rows_host(c, image.data(), tag<T>(), h, w, med.data(), &n_cols));
        step<T>(med.data(), n_cols, h, update_state);
    } else {
        step_keep();
    }
    std::vector<T> dc(h);
    for (size_t i = 0; i < h; ++i) dc[i] = static_cast<T>(dark_count_[i]);
    hip::check(ouster_hip_image_apply_host(c, image.data(), tag<T>(), h, w, dc.data(), nullptr));
}

void BeamUniformityCorrector::update(ImgRef<float> image, bool update_state) { apply(image, update_state); }
void BeamUniformityCorrector::update(ImgRef<double> image, bool update_state) { apply(image, update_state); }

template <typename T>
void BeamUniformityCorrector::update_batch(hip::Context& ctx, const void* planes, ChanFieldType elem_type, uint32_t n_images,
                                           uint32_t h, uint32_t w, T* out_images, bool update_state, AutoExposure* then,
                                           size_t in_stride, size_t out_stride) {
    if (n_images == 0 || h == 0 || w == 0) return;
    ouster_hip_ctx* c = ctx.handle();
    const int in_type = static_cast<int>(elem_type);
    const size_t hm = h - 1;
    bool any = false;
    {
        int cnt = counter_;
        for (uint32_t i = 0; i < n_images && !any; ++i, cnt = (cnt + 1) % 8)
            any = (i == 0 && dark_count_.size() != h) || (update_state && cnt == 0);
    }
    std::vector<T> med(hm * n_images, T(0));
    std::vector<uint32_t> n_cols(n_images, 0);
    if (any && h >= 2) {
        uint8_t* d = static_cast<uint8_t*>(scratch(c, 4, static_cast<size_t>(n_images) * (hm * sizeof(T) + 8)));
        uint32_t* d_nc = reinterpret_cast<uint32_t*>(d + hm * sizeof(T) * n_images);
        hip::check(ouster_hip_image_dark_rows(c, planes, in_type, tag<T>(), n_images, h, w, in_stride, d, d_nc));
        hip::check(ouster_hip_copy_out(c, med.data(), d, med.size() * sizeof(T)));
        hip::check(ouster_hip_copy_out(c, n_cols.data(), d_nc, n_cols.size() * 4));
        hip::check(ouster_hip_sync(c));
    }
    std::vector<T> dark(static_cast<size_t>(h) * n_images);
    for (uint32_t i = 0; i < n_images; ++i) {
        if (wants_dark_rows(h, update_state)) step<T>(med.data() + hm * i, n_cols[i], h, update_state);
        else step_keep();
        for (size_t r = 0; r < h; ++r) dark[static_cast<size_t>(h) * i + r] = static_cast<T>(dark_count_[r]);
    }
    void* d_dark = scratch(c, 5, dark.size() * sizeof(T));
    hip::check(ouster_hip_copy_in(c, d_dark, dark.data(), dark.size() * sizeof(T)));
    const ::ouster_hip_image_map* d_maps = nullptr;
    std::vector<::ouster_hip_image_map> maps;
    if (then) {
        std::vector<uint32_t> n(n_images, 0);
        std::vector<T> lo_hi(2 * static_cast<size_t>(n_images), T(0));
        if (update_state) {
            uint8_t* d = static_cast<uint8_t*>(scratch(c, 6, static_cast<size_t>(n_images) * (8 + 2 * sizeof(T))));
            uint32_t* d_n = reinterpret_cast<uint32_t*>(d + 2 * sizeof(T) * n_images);
            hip::check(ouster_hip_image_percentiles(c, planes, in_type, tag<T>(), n_images, h, w, in_stride, d_dark,
                                                    then->lo_percentile(), then->hi_percentile(), d_n, d));
            hip::check(ouster_hip_copy_out(c, lo_hi.data(), d, lo_hi.size() * sizeof(T)));
            hip::check(ouster_hip_copy_out(c, n.data(), d_n, n.size() * 4));
            hip::check(ouster_hip_sync(c));
        }
        maps.resize(n_images);
        for (uint32_t i = 0; i < n_images; ++i) {
            then->step(n[i], static_cast<double>(lo_hi[2 * i]), static_cast<double>(lo_hi[2 * i + 1]), update_state, maps[i]);
            maps[i].use_dark = 1;
        }
        void* dm = scratch(c, 7, maps.size() * sizeof(maps[0]));
        hip::check(ouster_hip_copy_in(c, dm, maps.data(), maps.size() * sizeof(maps[0])));
        d_maps = static_cast<const ::ouster_hip_image_map*>(dm);
    }
    hip::check(ouster_hip_image_apply(c, planes, in_type, out_images, tag<T>(), n_images, h, w, in_stride, out_stride, d_dark,
                                      d_maps));
    hip::check(ouster_hip_sync(c));   // `dark` and `maps` are pageable sources of asynchronous copies
}
template void BeamUniformityCorrector::update_batch<float>(hip::Context&, const void*, ChanFieldType, uint32_t, uint32_t, uint32_t,
                                                           float*, bool, AutoExposure*, size_t, size_t);
template void BeamUniformityCorrector::update_batch<double>(hip::Context&, const void*, ChanFieldType, uint32_t, uint32_t, uint32_t,
                                                            double*, bool, AutoExposure*, size_t, size_t);

}  // namespace image
}  // namespace core
}  // namespace sdk
}  // namespace ouster
