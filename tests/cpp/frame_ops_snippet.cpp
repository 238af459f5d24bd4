// A reference caller of ouster::sdk::core::frame_ops against the mirror (tests/test_frame_ops_api_cpu.py compiles, links and
// runs it).  First every validation error with the reference's message -- none of them needs a GPU -- then the metadata
// functions on the metadata file given as argv[1], then the pixel work: "no-gpu" when it refuses for lack of a GPU and
// leaves the frame untouched, "ok" when it ran and the results are what the semantics say.
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "ouster/core/frame_ops.h"

using namespace ouster::sdk::core;

static int failures = 0;

static void expect_invalid(const char* what, const std::string& message, const std::function<void()>& f) {
    try {
        f();
    } catch (const std::invalid_argument& e) {
        if (message != e.what()) {
            std::printf("%s: message \"%s\", expected \"%s\"\n", what, e.what(), message.c_str());
            ++failures;
        }
        return;
    } catch (const std::exception& e) {
        std::printf("%s: wrong exception type: %s\n", what, e.what());
        ++failures;
        return;
    }
    std::printf("%s: no exception\n", what);
    ++failures;
}

int main(int argc, char** argv) {
    const size_t h = 8, w = 32;
    auto info = std::make_shared<SensorInfo>();
    info->format.pixels_per_column = h;
    info->format.columns_per_frame = w;
    info->format.columns_per_packet = 16;
    info->format.pixel_shift_by_row = {0, 3, -2, 31, 33, -40, 1, 0};
    info->beam_azimuth_angles.assign(h, 0.0);
    info->beam_altitude_angles = {0, 1, 2, 3, 4, 5, 6, 7};
    info->prod_line = "OS-1-8";
    LidarFrameFieldTypes types = {{"RANGE", ChanFieldType::UINT32}, {"REFLECTIVITY", ChanFieldType::UINT8},
                                  {"F", ChanFieldType::FLOAT32}, {"PER_COL", ChanFieldType::UINT32, {}, FieldClass::COLUMN_FIELD}};
    LidarFrame frame(info, types);
    for (size_t i = 0; i < h * w; ++i) {
        frame.field("RANGE").get<uint32_t>()[i] = static_cast<uint32_t>(i % 100);
        frame.field("REFLECTIVITY").get<uint8_t>()[i] = static_cast<uint8_t>(i % 50);
        frame.field("F").get<float>()[i] = static_cast<float>(i % 10) - 5.f;
    }
    const LidarFrame before = frame;
    const std::vector<std::string> only_range = {"RANGE"}, per_col = {"RANGE", "PER_COL"}, range_refl = {"RANGE", "REFLECTIVITY"};

    // ---- validation: no GPU needed -------------------------------------------------------------------------------------
    expect_invalid("factor 0", "factor == 0 can't be negative", [] { frame_ops::reduce_factor_to_indices(0, 128); });
    expect_invalid("non-divisor", "factor == 3 must be a divisor of 128", [] { frame_ops::reduce_factor_to_indices(3, 128); });
    expect_invalid("empty indices", "beam indices can't be empty", [&] { frame_ops::select_by_index_metadata(*info, {}); });
    expect_invalid("duplicates", "beam indices can't contain duplicates", [&] { frame_ops::select_by_index(frame, {1, 1}); });
    expect_invalid("out of range", "beam indices [8, 9] must be in the range [0, 8)",
                   [&] { frame_ops::select_by_index(frame, {0, 8, 9}); });
    expect_invalid("coord_2d", "coord_2d == x must be either 'u' or 'v'", [&] { frame_ops::filter_uv(frame, "x", 0, 1); });
    expect_invalid("uv bounds", "lower == 0 and upper == 9 must be in the range [0, 8]", [&] { frame_ops::filter_uv(frame, "u", 0, 9); });
    expect_invalid("uv bounds v", "lower == 33 and upper == 2 must be in the range [0, 32]", [&] { frame_ops::filter_uv(frame, "v", 33, 2); });
    expect_invalid("lower > upper", "lower == 5 must be less than upper == 2", [&] { frame_ops::filter_uv(frame, "u", 5, 2); });
    {
        std::vector<uint8_t> m(h * (w + 1), 1);
        expect_invalid("mask shape", "Used mask size doesn't match frame size",
                       [&] { frame_ops::mask(frame, {}, ImgRef<const uint8_t>(m.data(), h, w + 1)); });
    }
    expect_invalid("non-pixel field", "Only PIXEL_FIELD frame fields are supported here; requested non-pixel fields: [PER_COL]",
                   [&] { frame_ops::clip(frame, per_col, 0, 1); });
    expect_invalid("non-pixel field (filter)", "Only PIXEL_FIELD frame fields are supported here; requested non-pixel fields: [PER_COL]",
                   [&] { frame_ops::filter_field(frame, "RANGE", 0, 1, 0, &per_col); });
    expect_invalid("key shape", "filter_field requires a pixel field with shape (h, w) to build a mask",
                   [&] { frame_ops::filter_field(frame, "PER_COL", 0, 1); });
    expect_invalid("invalid does not fit", "invalid == 256 does not fit a field of type UINT8",
                   [&] { frame_ops::clip(frame, range_refl, 0, 1, 256); });
    expect_invalid("invalid NaN", "invalid == nan does not fit a field of type UINT32",
                   [&] { frame_ops::filter_uv(frame, "u", 0, 1, std::numeric_limits<double>::quiet_NaN(), &only_range); });
    if (!(frame == before)) {
        std::printf("a refused call changed the frame\n");
        ++failures;
    }

    // ---- pure functions --------------------------------------------------------------------------------------------------
    if (frame_ops::reduce_factor_to_indices(128, 128) != std::vector<size_t>{64}) ++failures, std::printf("factor == height\n");
    if (frame_ops::reduce_factor_to_indices(4, 16) != std::vector<size_t>{0, 4, 8, 12}) ++failures, std::printf("factor 4\n");
    {
        const SensorInfo s = frame_ops::select_by_index_metadata(*info, {7, 1, 4});
        if (s.h() != 3 || s.format.pixel_shift_by_row != std::vector<int>{0, 3, 33} ||
            s.beam_altitude_angles != std::vector<double>{7, 1, 4} || s.prod_line != "OS-1-3" || s.w() != w)
            ++failures, std::printf("select_by_index_metadata\n");
    }
    if (argc > 1) {
        const SensorInfo meta = metadata_from_json(argv[1]);
        const SensorInfo r = frame_ops::reduce_by_factor_metadata(meta, 4);
        std::printf("meta %u %s -> %u %s\n", meta.h(), meta.prod_line.c_str(), r.h(), r.prod_line.c_str());
        bool ok = r.h() == meta.h() / 4 && r.beam_altitude_angles.size() == r.h() && r.format.pixel_shift_by_row.size() == r.h();
        for (size_t i = 0; ok && i < r.h(); ++i)
            ok = r.beam_altitude_angles[i] == meta.beam_altitude_angles[4 * i] && r.beam_azimuth_angles[i] == meta.beam_azimuth_angles[4 * i] &&
                 r.format.pixel_shift_by_row[i] == meta.format.pixel_shift_by_row[4 * i];
        if (!ok) ++failures, std::printf("reduce_by_factor_metadata\n");
    }
    if (failures) return 1;

    // ---- pixel work -----------------------------------------------------------------------------------------------------------
    try {
        frame_ops::clip(frame, only_range, 10, 59, 7);
    } catch (const std::invalid_argument&) {
        throw;
    } catch (const std::runtime_error& e) {
        if (!(frame == before)) {
            std::printf("frame changed by a failed call\n");
            return 2;
        }
        std::printf("no-gpu: %s\n", e.what());
        return 0;
    }
    frame_ops::filter_field(frame, "REFLECTIVITY", 0, 9);              // inside the range goes, in every pixel field
    frame_ops::filter_uv(frame, "v", 30, 32, 1, &only_range);
    std::vector<uint8_t> m(h * w, 1);
    for (size_t c = 0; c < w; ++c) m[2 * w + c] = 0;
    frame_ops::mask(frame, {"F"}, ImgRef<const uint8_t>(m.data(), h, w));
    const auto& shifts = info->format.pixel_shift_by_row;
    for (size_t r = 0; r < h; ++r)
        for (size_t c = 0; c < w; ++c) {
            const size_t i = r * w + c;
            uint32_t range = static_cast<uint32_t>(i % 100);
            if (range < 10 || range > 59) range = 7;
            const bool refl_in = i % 50 <= 9;
            if (refl_in) range = 0;
            const long dc = ((static_cast<long>(c) + shifts[r]) % static_cast<long>(w) + static_cast<long>(w)) % static_cast<long>(w);
            if (dc >= 30) range = 1;
            float f = static_cast<float>(i % 10) - 5.f;
            if (refl_in || r == 2) f = 0.f;
            const uint8_t refl = refl_in ? 0 : static_cast<uint8_t>(i % 50);
            if (frame.field("RANGE").get<uint32_t>()[i] != range || frame.field("F").get<float>()[i] != f ||
                frame.field("REFLECTIVITY").get<uint8_t>()[i] != refl) {
                std::printf("pixel (%zu, %zu) differs\n", r, c);
                return 3;
            }
        }
    const LidarFrame sel = frame_ops::select_by_index(frame, {5, 0}, true);
    if (sel.h != 2 || sel.w != w || !sel.sensor_info || sel.sensor_info->h() != 2 ||
        std::memcmp(sel.field("RANGE").get<uint32_t>(), frame.field("RANGE").get<uint32_t>() + 5 * w, w * 4) != 0 ||
        std::memcmp(sel.field("RANGE").get<uint32_t>() + w, frame.field("RANGE").get<uint32_t>(), w * 4) != 0 ||
        sel.field("PER_COL") != frame.field("PER_COL")) {
        std::printf("select_by_index differs\n");
        return 4;
    }
    std::printf("ok\n");
    return 0;
}
