/**
 * frame_ops.h -- ouster::sdk::core::frame_ops (reference: ouster_core/include/ouster/core/frame_ops.h, src/frame_ops.cpp):
 * clip / filter / mask a LidarFrame's pixel fields in place, and select beam rows.
 *
 * The pixel work runs on the GPU, in place on the frame's pooled (page-locked) storage: one launch per call for all target
 * fields, whatever their element types (csrc/k_frame_ops.hip).  The pure functions -- reduce_factor_to_indices, the
 * *_metadata forms and every validation -- need no GPU; pixel work without one throws std::runtime_error.
 *
 * Semantics are the reference's code, not its comments: filter_field invalidates the pixels whose key lies INSIDE
 * [lower, upper].  One deviation: `invalid` is truncated toward zero, and a value that then does not fit EVERY target field's
 * element type (or NaN for an integer type) throws std::invalid_argument before anything is touched -- the reference's
 * static_cast is undefined there.
 */
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "ouster/core/lidar_frame.h"
#include "ouster/core/types.h"

namespace ouster {
namespace sdk {
namespace core {
namespace frame_ops {

/** Values outside [lower, upper] (compared in double; NaN is outside) become `invalid`.  Empty `fields`: all pixel fields.
 *  @throw std::invalid_argument for a listed field that is present but not a PIXEL_FIELD */
void clip(LidarFrame& frame, const std::vector<std::string>& fields, double lower, double upper, double invalid = 0);

/** Pixels whose value of `field` lies inside [lower, upper] become `invalid` in every target field (nullptr: all pixel fields;
 *  `field` itself may be one of them).  A NaN key keeps its pixel.
 *  @throw std::invalid_argument if `field` does not have shape (h, w); std::out_of_range if it does not exist */
void filter_field(LidarFrame& frame, const std::string& field, double lower, double upper, double invalid = 0,
                  const std::vector<std::string>* filtered_fields = nullptr);

/** "u": rows [lower, upper) become `invalid`.  "v": columns [lower, upper) of the DESTAGGERED image do (needs
 *  frame.sensor_info); the frame stays staggered, the predicate is evaluated in staggered coordinates.
 *  @throw std::invalid_argument for another coord_2d, bounds beyond the extent, lower > upper */
void filter_uv(LidarFrame& frame, const std::string& coord_2d, size_t lower, size_t upper, double invalid = 0,
               const std::vector<std::string>* filtered_fields = nullptr);

/** Pixels where mask == 0 become 0.  Empty `fields`: all pixel fields.
 *  @throw std::invalid_argument("Used mask size doesn't match frame size") */
void mask(LidarFrame& frame, const std::vector<std::string>& fields, ImgRef<const uint8_t> mask);

/** Every factor-th row; {height / 2} when factor == height.
 *  @throw std::invalid_argument for factor 0 or a factor that does not divide height */
std::vector<size_t> reduce_factor_to_indices(size_t factor, size_t height);

/** Metadata of the selected beams: pixels_per_column, pixel_shift_by_row, beam angles and prod_line are rewritten.
 *  @throw std::invalid_argument for empty, duplicate or out-of-range indices */
SensorInfo select_by_index_metadata(const SensorInfo& metadata, const std::vector<size_t>& indices);

/** A new frame with the selected rows of every pixel field; header and non-pixel fields are copied.  sensor_info is set
 *  only with update_metadata.
 *  @throw std::invalid_argument as above, or when frame.sensor_info is empty */
LidarFrame select_by_index(const LidarFrame& frame, const std::vector<size_t>& indices, bool update_metadata = false);

SensorInfo reduce_by_factor_metadata(const SensorInfo& metadata, size_t factor);
LidarFrame reduce_by_factor(const LidarFrame& frame, size_t factor, bool update_metadata = false);

namespace impl {
/** Not part of the reference's surface: mask() writing `invalid` instead of 0.  The Python filter_xyz applies the masks it
 *  builds from its callable's points through this (the reference assigns through a numpy mask there). */
void mask_value(LidarFrame& frame, const std::vector<std::string>& fields, ImgRef<const uint8_t> mask, double invalid);
}  // namespace impl

}  // namespace frame_ops
}  // namespace core
}  // namespace sdk
}  // namespace ouster
