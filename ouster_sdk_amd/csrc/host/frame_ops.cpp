// frame_ops.cpp -- ouster::sdk::core::frame_ops over the C ABI (ouster_hip_frame_ops_*): field resolution, validation with the
// reference's messages (ouster_core/src/frame_ops.cpp) and the metadata functions on the host, the pixel work on the GPU in
// place on the frame's pooled storage.
#include "ouster/core/frame_ops.h"

#include <algorithm>
#include <cctype>
#include <memory>
#include <set>
#include <stdexcept>

#include "host_internal.h"

namespace ouster {
namespace sdk {
namespace core {
namespace frame_ops {
namespace {

// Which fields an op works on (frame_ops.cpp:19-62): pixel fields only; with a list, a missing field is skipped and a present
// non-pixel field is an error; without one, every pixel field present.
std::vector<std::string> resolve_pixel_fields(const LidarFrame& frame, const std::vector<std::string>* filtered_fields) {
    std::set<std::string> pixel;
    for (const auto& ft : frame.field_types())
        if (ft.field_class == FieldClass::PIXEL_FIELD) pixel.insert(ft.name);
    std::vector<std::string> requested;
    if (filtered_fields) {
        requested = *filtered_fields;
    } else {
        for (const auto& kv : frame.fields()) requested.push_back(kv.first);
    }
    std::vector<std::string> present, non_pixel;
    for (const auto& name : requested) {
        if (!frame.has_field(name)) continue;
        (pixel.count(name) ? present : non_pixel).push_back(name);
    }
    if (filtered_fields && !non_pixel.empty()) {
        std::string msg = "Only PIXEL_FIELD frame fields are supported here; requested non-pixel fields: [";
        for (size_t i = 0; i < non_pixel.size(); ++i) msg += (i ? ", " : "") + non_pixel[i];
        throw std::invalid_argument(msg + "]");
    }
    return present;
}

// impl::visit_field_2d's element types (impl/lidar_frame_impl.h:58-105): the others are skipped silently
bool visited_type(ChanFieldType t) {
    switch (t) {
        case ChanFieldType::UINT8: case ChanFieldType::UINT16: case ChanFieldType::UINT32: case ChanFieldType::UINT64:
        case ChanFieldType::INT8: case ChanFieldType::INT16: case ChanFieldType::INT32: case ChanFieldType::INT64:
        case ChanFieldType::FLOAT32: case ChanFieldType::FLOAT64:
            return true;
        default:
            return false;
    }
}

// The target planes of one call.  Everything that can be refused is refused here, before the GPU is asked for and before a
// writable pointer leaves a Field: element type, rank, and `invalid` against EVERY target's type.
struct Targets {
    std::vector<Field*> fields;
    std::vector<ouster_hip_fops_plane> planes;

    Targets(LidarFrame& frame, const std::vector<std::string>& names, double invalid) {
        for (const auto& name : names) {
            Field& f = frame.field(name);
            if (!visited_type(f.tag())) continue;
            if (f.shape().size() != 2)
                throw std::invalid_argument("Field: Eigen array conversion failed due to dimension mismatch. Underlying data has " +
                                            std::to_string(f.shape().size()) + " dimensions but must have 2 dimensions.");
            if (f.shape()[0] != frame.h || f.shape()[1] != frame.w)
                throw std::invalid_argument("frame_ops: field " + name + " does not have the frame's shape (h, w)");
            uint64_t bits;
            hip::check(ouster_hip_frame_ops_invalid_bits(static_cast<int>(f.tag()), invalid, &bits));
            fields.push_back(&f);
        }
        planes.resize(fields.size());
        for (size_t i = 0; i < fields.size(); ++i) {
            planes[i] = ouster_hip_fops_plane{};
            planes[i].type = static_cast<int>(fields[i]->tag());
            planes[i].invalid = invalid;
        }
    }
    // The same path as any other write into a Field (Field::get(), non-const): HBM mirror entries of the plane die with it.
    void open() {
        for (size_t i = 0; i < fields.size(); ++i) planes[i].data = fields[i]->get();
    }
};

void invalidate(LidarFrame& frame, Targets& t, ouster_hip_fops_pred& pred) {
    ouster_hip_ctx* ctx = hip::default_ctx();   // throws without a GPU, before anything is touched
    if (t.planes.empty()) return;
    t.open();
    hip::check(ouster_hip_frame_ops_invalidate_host(ctx, &pred, t.planes.data(), static_cast<uint32_t>(t.planes.size()),
                                                    static_cast<uint32_t>(frame.h), static_cast<uint32_t>(frame.w)));
}

void validate_beam_indices(const std::vector<size_t>& indices, size_t height) {
    if (indices.empty()) throw std::invalid_argument("beam indices can't be empty");
    std::set<size_t> seen;
    std::vector<size_t> bad;
    for (size_t i : indices) {
        if (!seen.insert(i).second) throw std::invalid_argument("beam indices can't contain duplicates");
        if (i >= height) bad.push_back(i);
    }
    if (!bad.empty()) {
        std::string msg = "beam indices [";
        for (size_t i = 0; i < bad.size(); ++i) msg += (i ? ", " : "") + std::to_string(bad[i]);
        throw std::invalid_argument(msg + "] must be in the range [0, " + std::to_string(height) + ")");
    }
}

template <typename T>
std::vector<T> select_vector(const std::vector<T>& values, const std::vector<size_t>& indices) {
    std::vector<T> out;
    out.reserve(indices.size());
    for (size_t i : indices) out.push_back(values.at(i));
    return out;
}

bool all_digits(const std::string& s) {
    return !s.empty() && std::all_of(s.begin(), s.end(), [](unsigned char c) { return std::isdigit(c) != 0; });
}

// "OS-1-128" -> "OS-1-<rows>", "OS-0-MAX-128" -> "OS0MAX-<rows>", "OS-DOME-64" -> "OSDOME-<rows>", "-RGB" kept: the form
// factor of the product line (sensor_info.cpp, ProductInfo) with the new beam count behind it (frame_ops.cpp:110-124)
std::string rewritten_prod_line(const std::string& prod_line, size_t rows) {
    std::string form_factor;
    bool rgb = false;
    if (!prod_line.empty()) {
        std::vector<std::string> tok(1);
        for (char c : prod_line) {
            if (c == '-') tok.emplace_back();
            else tok.back().push_back(c);
        }
        const bool word = !tok[0].empty() && std::all_of(tok[0].begin(), tok[0].end(), [](unsigned char c) { return std::isalnum(c) || c == '_'; });
        if (tok.size() < 2 || !word)
            throw std::runtime_error("Product Info \"" + prod_line + "\" is not a recognized product info");
        form_factor = tok[0];
        size_t i = 1;
        if (i < tok.size() && (all_digits(tok[i]) || tok[i] == "DOME")) form_factor += tok[i++];
        if (i < tok.size() && tok[i] == "MAX") form_factor += tok[i++];
        if (i < tok.size() && all_digits(tok[i])) ++i;   // the beam count
        if (i < tok.size() && tok[i] == "RGB") rgb = true;
    }
    if (form_factor.find("MAX") != std::string::npos) {
        form_factor = "OS" + form_factor.substr(2, 1) + "MAX";
    } else if (!form_factor.empty() && std::isdigit(static_cast<unsigned char>(form_factor.back()))) {
        form_factor = form_factor.substr(0, form_factor.size() - 1) + "-" + form_factor.back();
    }
    form_factor += "-" + std::to_string(rows);
    if (rgb) form_factor += "-RGB";
    return form_factor;
}

}  // namespace

void clip(LidarFrame& frame, const std::vector<std::string>& fields, double lower, double upper, double invalid) {
    Targets t(frame, resolve_pixel_fields(frame, fields.empty() ? nullptr : &fields), invalid);
    ouster_hip_ctx* ctx = hip::default_ctx();
    if (t.planes.empty()) return;
    t.open();
    hip::check(ouster_hip_frame_ops_clip_host(ctx, t.planes.data(), static_cast<uint32_t>(t.planes.size()),
                                              static_cast<uint32_t>(frame.h), static_cast<uint32_t>(frame.w), lower, upper));
}

void filter_field(LidarFrame& frame, const std::string& field, double lower, double upper, double invalid,
                  const std::vector<std::string>* filtered_fields) {
    const Field& key = static_cast<const LidarFrame&>(frame).field(field);
    if (key.shape().size() != 2 || key.shape()[0] != frame.h || key.shape()[1] != frame.w)
        throw std::invalid_argument("filter_field requires a pixel field with shape (h, w) to build a mask");
    Targets t(frame, resolve_pixel_fields(frame, filtered_fields), invalid);
    if (!visited_type(key.tag())) return;   // visit_field_2d builds no mask for such a key: nothing is applied
    ouster_hip_fops_pred pred{};
    pred.kind = OUSTER_HIP_FOPS_PRED_KEY;
    pred.src_type = static_cast<int>(key.tag());
    pred.src = key.get();
    pred.lower = lower;
    pred.upper = upper;
    invalidate(frame, t, pred);
}

void filter_uv(LidarFrame& frame, const std::string& coord_2d, size_t lower, size_t upper, double invalid,
               const std::vector<std::string>* filtered_fields) {
    if (coord_2d != "u" && coord_2d != "v")
        throw std::invalid_argument("coord_2d == " + coord_2d + " must be either 'u' or 'v'");
    const size_t coord_size = coord_2d == "u" ? frame.h : frame.w;
    if (lower > coord_size || upper > coord_size)
        throw std::invalid_argument("lower == " + std::to_string(lower) + " and upper == " + std::to_string(upper) +
                                    " must be in the range [0, " + std::to_string(coord_size) + "]");
    if (lower > upper)
        throw std::invalid_argument("lower == " + std::to_string(lower) + " must be less than upper == " + std::to_string(upper));
    Targets t(frame, resolve_pixel_fields(frame, filtered_fields), invalid);
    ouster_hip_fops_pred pred{};
    pred.lo = static_cast<uint32_t>(lower);
    pred.hi = static_cast<uint32_t>(upper);
    std::vector<int32_t> shifts;
    if (coord_2d == "u") {
        pred.kind = OUSTER_HIP_FOPS_PRED_ROWS;
    } else {
        if (!frame.sensor_info) throw std::invalid_argument("filter_uv requires frame.sensor_info");
        const auto& s = frame.sensor_info->format.pixel_shift_by_row;
        if (s.size() != frame.h) throw std::invalid_argument("image height does not match shifts size");
        shifts.assign(s.begin(), s.end());
        pred.kind = OUSTER_HIP_FOPS_PRED_COLS;
        pred.shifts = shifts.data();
        pred.n_shift_tables = 1;
    }
    invalidate(frame, t, pred);
}

void mask(LidarFrame& frame, const std::vector<std::string>& fields, ImgRef<const uint8_t> mask) {
    impl::mask_value(frame, fields, mask, 0);
}

namespace impl {
void mask_value(LidarFrame& frame, const std::vector<std::string>& fields, ImgRef<const uint8_t> mask, double invalid) {
    if (mask.rows() != frame.h || mask.cols() != frame.w)
        throw std::invalid_argument("Used mask size doesn't match frame size");
    Targets t(frame, resolve_pixel_fields(frame, fields.empty() ? nullptr : &fields), invalid);
    ouster_hip_fops_pred pred{};
    pred.kind = OUSTER_HIP_FOPS_PRED_MASK;
    pred.src = mask.data();
    pred.n_masks = 1;
    invalidate(frame, t, pred);
}
}  // namespace impl

std::vector<size_t> reduce_factor_to_indices(size_t factor, size_t height) {
    if (factor == 0) throw std::invalid_argument("factor == 0 can't be negative");
    if (height % factor != 0)
        throw std::invalid_argument("factor == " + std::to_string(factor) + " must be a divisor of " + std::to_string(height));
    if (factor == height) return {height / 2};
    std::vector<size_t> indices;
    for (size_t i = 0; i < height; i += factor) indices.push_back(i);
    return indices;
}

SensorInfo select_by_index_metadata(const SensorInfo& metadata, const std::vector<size_t>& indices) {
    validate_beam_indices(indices, metadata.h());
    SensorInfo out;   // member by member: a lookup table cached for the full sensor must not travel
    out.sn = metadata.sn;
    out.fw_rev = metadata.fw_rev;
    out.image_rev = metadata.image_rev;
    out.format = metadata.format;
    out.config = metadata.config;
    out.lidar_origin_to_beam_origin_mm = metadata.lidar_origin_to_beam_origin_mm;
    out.beam_to_lidar_transform = metadata.beam_to_lidar_transform;
    out.imu_to_sensor_transform = metadata.imu_to_sensor_transform;
    out.lidar_to_sensor_transform = metadata.lidar_to_sensor_transform;
    out.sensor_to_body = metadata.sensor_to_body;
    out.init_id = metadata.init_id;
    out.prod_line = rewritten_prod_line(metadata.prod_line, indices.size());
    out.format.pixels_per_column = static_cast<uint32_t>(indices.size());
    out.format.pixel_shift_by_row = select_vector(metadata.format.pixel_shift_by_row, indices);
    out.beam_azimuth_angles = select_vector(metadata.beam_azimuth_angles, indices);
    out.beam_altitude_angles = select_vector(metadata.beam_altitude_angles, indices);
    return out;
}

LidarFrame select_by_index(const LidarFrame& frame, const std::vector<size_t>& indices, bool update_metadata) {
    validate_beam_indices(indices, frame.h);
    if (!frame.sensor_info) throw std::invalid_argument("select_by_index requires frame.sensor_info");
    std::shared_ptr<SensorInfo> new_info;
    if (update_metadata) new_info = std::make_shared<SensorInfo>(select_by_index_metadata(*frame.sensor_info, indices));

    const auto types = frame.field_types();
    LidarFrame result(indices.size(), frame.w, types, frame.sensor_info->format.columns_per_packet);
    result.frame_id = frame.frame_id;
    result.frame_status = frame.frame_status;
    result.shutdown_countdown = frame.shutdown_countdown;
    result.shot_limiting_countdown = frame.shot_limiting_countdown;
    std::copy(frame.timestamp().data(), frame.timestamp().data() + frame.w, result.timestamp().data());
    std::copy(frame.measurement_id().data(), frame.measurement_id().data() + frame.w, result.measurement_id().data());
    std::copy(frame.status().data(), frame.status().data() + frame.w, result.status().data());
    const size_t np = std::min(frame.packet_count(), result.packet_count());
    std::copy(frame.packet_timestamp().data(), frame.packet_timestamp().data() + np, result.packet_timestamp().data());
    result.body_to_world() = frame.body_to_world();

    std::vector<const void*> src;
    std::vector<void*> dst;
    std::vector<uint32_t> elem;
    size_t row_elems = 0;
    std::vector<std::pair<size_t, std::string>> by_row;   // planes of one row length go in one launch
    for (const auto& ft : types) {
        const Field& f = frame.field(ft.name);
        if (ft.field_class != FieldClass::PIXEL_FIELD) {
            result.field(ft.name) = f;
            continue;
        }
        if (f.shape().empty()) throw std::invalid_argument("cannot select rows from non-array fields");
        size_t row = 1;
        for (size_t d = 1; d < f.shape().size(); ++d) row *= f.shape()[d];
        by_row.emplace_back(row, ft.name);
    }
    std::sort(by_row.begin(), by_row.end());
    ouster_hip_ctx* ctx = by_row.empty() ? nullptr : hip::default_ctx();
    std::vector<uint32_t> idx(indices.begin(), indices.end());
    for (size_t i = 0; i < by_row.size();) {
        size_t j = i;
        src.clear();
        dst.clear();
        elem.clear();
        row_elems = by_row[i].first;
        for (; j < by_row.size() && by_row[j].first == row_elems; ++j) {
            const Field& f = frame.field(by_row[j].second);
            src.push_back(f.get());
            dst.push_back(result.field(by_row[j].second).get());
            elem.push_back(static_cast<uint32_t>(f.element_size()));
        }
        hip::check(ouster_hip_frame_ops_select_rows_host(ctx, src.data(), dst.data(), elem.data(), static_cast<uint32_t>(src.size()),
                                                         static_cast<uint32_t>(frame.h), static_cast<uint32_t>(row_elems),
                                                         idx.data(), static_cast<uint32_t>(idx.size())));
        i = j;
    }
    if (update_metadata) result.sensor_info = new_info;
    return result;
}

SensorInfo reduce_by_factor_metadata(const SensorInfo& metadata, size_t factor) {
    return select_by_index_metadata(metadata, reduce_factor_to_indices(factor, metadata.h()));
}

LidarFrame reduce_by_factor(const LidarFrame& frame, size_t factor, bool update_metadata) {
    return select_by_index(frame, reduce_factor_to_indices(factor, frame.h), update_metadata);
}

}  // namespace frame_ops
}  // namespace core
}  // namespace sdk
}  // namespace ouster
