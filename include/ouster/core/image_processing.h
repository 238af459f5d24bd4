// image_processing.h -- ouster::sdk::core::image::AutoExposure, BeamUniformityCorrector and LocalToneMapper on the GPU.
//
// Mirrors the reference (ouster_core/include/ouster/core/image_processing.h:25-261): the step a caller runs right after
// destagger() to turn a SIGNAL / NEAR_IR / REFLECTIVITY / RANGE plane into a float image in [0, 1], and an RGB plane (FLOAT16 x 3
// in the colour profiles) into a displayable one -- LocalToneMapper().update(destagger(info, field)), as the reference's viewer does.
// RgbImgRef<T> (typedefs.h) stands where the reference takes Eigen::TensorMap<rgb_img_t<T>>.
//
// The per-pixel work and the order statistics run in HIP kernels (ouster_hip_image_*, include/ouster_hip.h); the state that
// is carried from frame to frame stays here, on the host, in double, and follows the reference's arithmetic operation by
// operation, so results are bit-identical to the reference's for float and for double images.
// Preconditions (the reference is undefined outside them): lo_percentile + hi_percentile < 1, no NaN in the image (RGB float /
// double images: every element finite; any FLOAT16 pattern is fine).  One deviation: LocalToneMapper refuses images with fewer than
// 8 rows or columns (std::invalid_argument), where the reference has empty tiles and blends NaN tables into the image.
// There is no CPU fallback: without a GPU update() throws std::runtime_error and leaves the image as it was.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "ouster/core/chanfield.h"
#include "ouster/core/typedefs.h"
#include "ouster/hip/context.h"

struct ouster_hip_image_map;
struct ouster_hip_tonemap_params;

namespace ouster {
namespace sdk {
namespace core {
namespace image {

/** Adjusts brightness to keep the image in a reasonable dynamic range (image_processing.h:25-124 of the reference). */
class AutoExposure {
   public:
    AutoExposure();
    explicit AutoExposure(int update_every);
    AutoExposure(double lo_percentile, double hi_percentile, int update_every, double damping = 0.9);

    /** Scales the image so that contrast is stretched between 0 and 1, in place.
     *  @param update_state false: apply the current state without advancing it */
    void update(ImgRef<float> image, bool update_state = true);
    void update(ImgRef<double> image, bool update_state = true);

    /** The RGB overloads (image_processing.h:102-124 of the reference): the percentiles are those of the luminance of every 4th
     *  pixel, the map is applied to all three channels.  In place for float / double; the FLOAT16 form converts `input` by the
     *  reference's integer formula into `out` first (an early return leaves the plain converted image there).
     *  @throw std::invalid_argument when `out` has another shape than `input` */
    void update(RgbImgRef<float> image, bool update_state = true);
    void update(RgbImgRef<double> image, bool update_state = true);
    void update(RgbImgRef<const float16_t> input, RgbImgRef<float> out, bool update_state = true);

    /** The RGB form of update_batch below: n_images images of h x w x 3 elements of `elem_type` (FLOAT16 with T = float, or T's
     *  own type) on DEVICE memory, strides in elements; out_images may be `images` itself when the types match. */
    template <typename T>
    void update_batch_rgb(hip::Context& ctx, const void* images, ChanFieldType elem_type, uint32_t n_images, uint32_t h,
                          uint32_t w, T* out_images, bool update_state = true, size_t in_stride = 0, size_t out_stride = 0);

    /** The same state machine over images 0 .. n_images - 1, in order, on DEVICE memory: `planes` holds n_images images of
     *  h x w elements of `elem_type` (UINT8 / UINT16 / UINT32, converted like astype(T), or T's own type), image i at
     *  planes + i * in_stride elements; the result goes to out_images + i * out_stride (strides 0: dense).  One launch per
     *  kernel whatever n_images is, one small round trip for the order statistics.  Synchronous. */
    template <typename T>
    void update_batch(hip::Context& ctx, const void* planes, ChanFieldType elem_type, uint32_t n_images, uint32_t h,
                      uint32_t w, T* out_images, bool update_state = true, size_t in_stride = 0, size_t out_stride = 0);

    // ---- extensions (not in the reference): read-only view of the state, for tests ---------------------------------
    double lo_state() const { return lo_state_; }
    double hi_state() const { return hi_state_; }
    bool initialized() const { return initialized_; }

    /** Extension: the host half of one update -- takes the order statistics the device returned for one image (n positive
     *  samples, the two percentile values; ignored unless wants_percentiles()) and returns the map to apply to it. */
    bool wants_percentiles(bool update_state) const { return counter_ == 0 && update_state; }
    void step(uint32_t n, double lo, double hi, bool update_state, ::ouster_hip_image_map& map);
    double lo_percentile() const { return lo_percentile_; }
    double hi_percentile() const { return hi_percentile_; }

   private:
    template <typename T> void apply(ImgRef<T> image, bool update_state);
    template <typename TIN, typename T> void apply_rgb(RgbImgRef<TIN> in, RgbImgRef<T> out, bool update_state);
    double lo_percentile_, hi_percentile_;
    int ae_update_every_;
    double damping_;
    double lo_state_ = -1.0, hi_state_ = -1.0, lo_ = -1.0, hi_ = -1.0;
    bool initialized_ = false;
    int counter_ = 0;
};

/** Corrects beam uniformity by subtracting a per-row "dark count" (image_processing.h:132-165 of the reference). */
class BeamUniformityCorrector {
   public:
    void update(ImgRef<float> image, bool update_state = true);
    void update(ImgRef<double> image, bool update_state = true);

    /** Batched, device-side form (see AutoExposure::update_batch).  With `then`, every corrected image goes straight
     *  through that AutoExposure as well -- buc.update(img); ae.update(img) of the reference for every image in order -- and
     *  the pair costs ONE pass over the pixels: the percentile kernel corrects its sample on the fly. */
    template <typename T>
    void update_batch(hip::Context& ctx, const void* planes, ChanFieldType elem_type, uint32_t n_images, uint32_t h,
                      uint32_t w, T* out_images, bool update_state = true, AutoExposure* then = nullptr,
                      size_t in_stride = 0, size_t out_stride = 0);

    /** Extension (not in the reference): the smoothed dark counts, one per row. */
    const std::vector<double>& dark_count() const { return dark_count_; }

    /** Extension: the host half -- whether the next call computes new dark counts for a h-row image, and the update itself from
     *  the device's row medians ((h - 1) values of T) and the number of non-empty columns. */
    bool wants_dark_rows(size_t h, bool update_state) const { return dark_count_.size() != h || (update_state && counter_ == 0); }
    template <typename T> void step(const T* medians, uint32_t n_cols, size_t h, bool update_state);
    void step_keep() { counter_ = (counter_ + 1) % 8; }

   private:
    template <typename T> void apply(ImgRef<T> image, bool update_state);
    int counter_ = 0;
    std::vector<double> dark_count_;
};

/** Tone-maps an HDR RGB image for display (image_processing.h:170-260 of the reference): auto exposure on the luminance, dynamic-
 *  range compression in dark scenes, Reinhard, CLAHE on 8 x 8 tiles and a saturation pass.  Results are bit-identical to the
 *  reference's for float and double images of at least 8 x 8 pixels. */
class LocalToneMapper {
   public:
    LocalToneMapper();
    explicit LocalToneMapper(int update_every);
    LocalToneMapper(double lo_percentile, double hi_percentile, int update_every, double damping, bool compress_dr,
                    bool color_correct);
    LocalToneMapper(double lo_percentile, double hi_percentile, int update_every, double damping, double compress_dr_max_lum,
                    bool color_correct);

    /** In place on a float / double image; the FLOAT16 form writes a float image of the same shape (an early return -- fewer
     *  than 100 positive samples, or no state yet -- leaves the image as it was, the FLOAT16 form the plain converted image).
     *  @throw std::invalid_argument for fewer than 8 rows or columns, or when `output` has another shape than `input` */
    void update(RgbImgRef<float> image, bool update_state = true);
    void update(RgbImgRef<double> image, bool update_state = true);
    void update(RgbImgRef<const float16_t> input, RgbImgRef<float> output, bool update_state = true);

    /** Extension: the same state machine over images 0 .. n_images - 1, in order, on DEVICE memory, like
     *  AutoExposure::update_batch: one percentile launch for all images, the state machine on the host, then one histogram /
     *  table / finish launch chain.  elem_type is FLOAT16 (T = float) or T's own type; strides in elements (0: dense,
     *  3 * h * w); out_images may be `images` itself when the types match.  Synchronous. */
    template <typename T>
    void update_batch(hip::Context& ctx, const void* images, ChanFieldType elem_type, uint32_t n_images, uint32_t h, uint32_t w,
                      T* out_images, bool update_state = true, size_t in_stride = 0, size_t out_stride = 0);

    // ---- extensions (not in the reference): read-only view of the state, and the host half of one update -------------
    double lo_state() const { return lo_state_; }
    double hi_state() const { return hi_state_; }
    bool initialized() const { return initialized_; }
    double lo_percentile() const { return lo_percentile_; }
    double hi_percentile() const { return hi_percentile_; }
    bool wants_percentiles(bool update_state) const { return counter_ == 0 && update_state; }
    /** Takes the luminance statistics the device returned for one image (ignored unless wants_percentiles()) and returns
     *  the record ouster_hip_image_tonemap applies to it (map.mode NONE: the early return). */
    void step(uint32_t n, double lo, double hi, bool update_state, ::ouster_hip_tonemap_params& params);

   private:
    template <typename TIN, typename T> void apply(RgbImgRef<TIN> in, RgbImgRef<T> out, bool update_state);
    double lo_percentile_, hi_percentile_;
    int update_every_;
    double damping_;
    double lo_state_ = -1.0, hi_state_ = -1.0, lo_ = -1.0, hi_ = -1.0;
    bool initialized_ = false;
    int counter_ = 0;
    double compress_dr_max_lum_ = 0.2;
    bool color_correct_ = true;
};

}  // namespace image
}  // namespace core
}  // namespace sdk
}  // namespace ouster
