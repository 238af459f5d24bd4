// batch_fixture.h -- what the *_batch_tool.cpp programs of this directory share (header-only, for the tests alone): the small
// synthetic sensors, the readers of the files tests/batch_cases.py writes, a decoded hip::DeviceFrameBatch made from them, and
// the few helpers every tool had a copy of.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "ouster/core/lidar_scan.h"
#include "ouster/hip/device_batch.h"

namespace fixture {
using namespace ouster::sdk::core;
namespace oh = ouster::sdk::hip;

// An h x w RNG15_RFL8_NIR8_DUAL sensor, 16 columns per packet; `variant` tilts the beams (another LUT per sensor).
//   wrap_shifts  rows 1 and 2 get their pixel shift wrapped by +w and -2w (the same pixels, other integers)
//   mounted      a sensor_to_body of its own per variant: a turn about z and an offset (identity otherwise)
inline SensorInfo make_info(uint32_t h, uint32_t w, int variant, bool wrap_shifts = false, bool mounted = false) {
    SensorInfo info;
    info.format.pixels_per_column = h;
    info.format.columns_per_frame = w;
    info.format.columns_per_packet = 16;
    info.format.column_window = {0, static_cast<int>(w) - 1};
    info.format.udp_profile_lidar = UDPProfileLidar::RNG15_RFL8_NIR8_DUAL;
    for (uint32_t i = 0; i < h; ++i) {
        const double az = (double[]){4.2, 1.4, -1.4, -4.2}[i % 4];
        info.format.pixel_shift_by_row.push_back(static_cast<int>(std::nearbyint(az / 360.0 * w)) +
                                                 (wrap_shifts && i == 1 ? static_cast<int>(w) : 0) -
                                                 (wrap_shifts && i == 2 ? 2 * static_cast<int>(w) : 0));
        info.beam_azimuth_angles.push_back(az);
        info.beam_altitude_angles.push_back((h > 1 ? 21.0 - 42.0 * i / (h - 1.0) : 0.0) + 0.7 * variant);
    }
    info.prod_line = "OS-2-128";
    info.beam_to_lidar_transform = default_beam_to_lidar_transform(info.prod_line);
    info.lidar_to_sensor_transform = DEFAULT_LIDAR_TO_SENSOR;
    info.sensor_to_body = mat4d::Identity();
    if (mounted) {
        const double a = 0.3 + 0.4 * variant;
        info.sensor_to_body.m[0] = std::cos(a), info.sensor_to_body.m[1] = -std::sin(a);
        info.sensor_to_body.m[4] = std::sin(a), info.sensor_to_body.m[5] = std::cos(a);
        info.sensor_to_body.m[3] = 0.35 - 0.6 * variant, info.sensor_to_body.m[7] = -0.2 + 0.15 * variant, info.sensor_to_body.m[11] = 1.1 + 0.25 * variant;
    }
    info.fw_rev = "v3.2.0";
    return info;
}

// known.bin: k doubles (seconds), then k x 16 doubles
inline void read_known(const char* path, uint32_t k, std::vector<double>& x_known, std::vector<mat4d>& poses_known) {
    x_known.resize(k);
    poses_known.resize(k);
    std::ifstream f(path, std::ios::binary);
    f.read(reinterpret_cast<char*>(x_known.data()), static_cast<std::streamsize>(k * 8));
    f.read(reinterpret_cast<char*>(poses_known.data()), static_cast<std::streamsize>(k * 128));
    if (!f) throw std::runtime_error("known poses file too short");
}

constexpr uint32_t SKIP_NOTHING = UINT32_MAX;

// A batch of n frames filled from packets.bin ([n][w / 16][lidar_packet_size] bytes) and decoded; packet <skip_packet> of frame
// <skip_frame> is left out.
inline std::unique_ptr<oh::DeviceFrameBatch> load_batch(const std::vector<SensorInfo>& sensors, uint32_t n, const oh::BatchOptions& opt,
                                                        const char* packets_path, uint32_t skip_frame = SKIP_NOTHING,
                                                        uint32_t skip_packet = SKIP_NOTHING) {
    auto b = std::make_unique<oh::DeviceFrameBatch>(sensors, n, opt);
    std::ifstream f(packets_path, std::ios::binary);
    const size_t ps = b->lidar_packet_size(), ppf = sensors.at(0).format.columns_per_frame / 16;
    std::vector<uint8_t> pk(ps * ppf);
    for (uint32_t fr = 0; fr < n; ++fr) {
        f.read(reinterpret_cast<char*>(pk.data()), static_cast<std::streamsize>(pk.size()));
        if (!f) throw std::runtime_error("packets file too short");
        std::vector<const uint8_t*> ptrs;
        for (size_t p = 0; p < ppf; ++p)
            if (fr != skip_frame || p != skip_packet) ptrs.push_back(pk.data() + p * ps);
        b->upload_frame_packets(fr, ptrs);
    }
    b->decode();
    return b;
}

inline void write_file(const std::string& path, const void* p, size_t bytes) {
    std::ofstream f(path, std::ios::binary);
    f.write(static_cast<const char*>(p), static_cast<std::streamsize>(bytes));
}

// one file of n frames: get(frame, buffer of `bytes` bytes) for each frame in turn
template <class Get>
void write_frames(const std::string& path, uint32_t n, size_t bytes, Get get) {
    std::vector<double> buf((bytes + 7) / 8);
    std::ofstream f(path, std::ios::binary);
    for (uint32_t fr = 0; fr < n; ++fr) {
        get(fr, buf.data());
        f.write(reinterpret_cast<const char*>(buf.data()), static_cast<std::streamsize>(bytes));
    }
}

// true when f() throws an E; another exception is named and counts as a failure
template <class E, class F>
bool throws(F f) {
    try {
        f();
    } catch (const E&) {
        return true;
    } catch (const std::exception& e) {
        std::printf("wrong exception: %s\n", e.what());
    }
    return false;
}
}   // namespace fixture
