// normals_batch_tool.cpp -- drives normals / normals_device / download_normals of hip::DeviceFrameBatch for
// tests/test_gpu_normals_batch.py (built by it with the flags of this directory's Makefile).
//   normals_batch_tool <packets.bin> <h> <w> <n_frames> <skip_frame> <skip_packet> <known.bin> <k> <out_prefix> <lo> <hi>
//       packets.bin, known.bin: as for pose_batch_tool.cpp.  The two sensors of that tool, each with a sensor_to_body of its own
//       (<prefix>.s2b, f64 [2][16]; <prefix>.shifts, i32 [h], the first sensor's).  Three dual-return batches, <B> =
//         body64   xyz_f64, body frame
//         body32   float, body frame
//         world64  xyz_f64, xyz_world_frame: decode(), interp_poses(known), decode() again
//       each leaves, [n] frames each, staggered as the batch holds them,
//         <prefix>.<B>.xyz0 / .xyz1   the clouds        <prefix>.<B>.r0 / .r1   RANGE / RANGE2        <prefix>.<B>.poses (world64)
//         <prefix>.<B>.d0 / .d1       normals({dual, pixel_search_range 1}), destaggered layout
//         <prefix>.<B>.s0 / .s1       normals({dual, pixel_search_range 2, staggered_output})
//         <prefix>.<B>.single         normals({pixel_search_range 3}), first return alone
//       body64 then gets filter_field(RANGE, lo, hi) and leaves .fxyz0 .fxyz1 .fr0 .fr1 and .fd0 / .fd1 as above.
//       Prints "no_xyz_throws 1" when normals() of a batch without BatchOptions::xyz throws std::invalid_argument,
//       "no_range2_throws 1" for the dual form on a batch whose planes lack RANGE2, "device_ptr 1" when normals_device() is null
//       before the first call and download_normals equals a copy from it afterwards.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "ouster/core/lidar_scan.h"
#include "ouster/hip/device_batch.h"

using namespace ouster::sdk::core;
namespace oh = ouster::sdk::hip;

static SensorInfo make_info(uint32_t h, uint32_t w, int variant) {
    SensorInfo info;
    info.format.pixels_per_column = h;
    info.format.columns_per_frame = w;
    info.format.columns_per_packet = 16;
    info.format.column_window = {0, static_cast<int>(w) - 1};
    info.format.udp_profile_lidar = UDPProfileLidar::RNG15_RFL8_NIR8_DUAL;
    for (uint32_t i = 0; i < h; ++i) {
        const double az = (double[]){4.2, 1.4, -1.4, -4.2}[i % 4];
        info.format.pixel_shift_by_row.push_back(static_cast<int>(std::nearbyint(az / 360.0 * w)));
        info.beam_azimuth_angles.push_back(az);
        info.beam_altitude_angles.push_back((h > 1 ? 21.0 - 42.0 * i / (h - 1.0) : 0.0) + 0.7 * variant);
    }
    info.prod_line = "OS-2-128";
    info.beam_to_lidar_transform = default_beam_to_lidar_transform(info.prod_line);
    info.lidar_to_sensor_transform = DEFAULT_LIDAR_TO_SENSOR;
    // a mount of its own per sensor: a turn about z and an offset
    const double a = 0.3 + 0.4 * variant;
    info.sensor_to_body = mat4d::Identity();
    info.sensor_to_body.m[0] = std::cos(a), info.sensor_to_body.m[1] = -std::sin(a);
    info.sensor_to_body.m[4] = std::sin(a), info.sensor_to_body.m[5] = std::cos(a);
    info.sensor_to_body.m[3] = 0.35 - 0.6 * variant, info.sensor_to_body.m[7] = -0.2 + 0.15 * variant, info.sensor_to_body.m[11] = 1.1 + 0.25 * variant;
    info.fw_rev = "v3.2.0";
    return info;
}

int main(int argc, char** argv) {
    if (argc != 12) {
        std::printf("usage: normals_batch_tool packets h w n skip_frame skip_packet known k prefix lo hi\n");
        return 64;
    }
    try {
        const uint32_t h = std::atoi(argv[2]), w = std::atoi(argv[3]), n = std::atoi(argv[4]);
        const uint32_t skip_frame = std::atoi(argv[5]), skip_packet = std::atoi(argv[6]), k = std::atoi(argv[8]);
        const std::string prefix = argv[9];
        const double lo = std::atof(argv[10]), hi = std::atof(argv[11]);
        std::vector<double> x_known(k);
        std::vector<mat4d> poses_known(k);
        {
            std::ifstream f(argv[7], std::ios::binary);
            f.read(reinterpret_cast<char*>(x_known.data()), static_cast<std::streamsize>(k * 8));
            f.read(reinterpret_cast<char*>(poses_known.data()), static_cast<std::streamsize>(k * 128));
            if (!f) throw std::runtime_error("known poses file too short");
        }
        const std::vector<SensorInfo> sensors = {make_info(h, w, 0), make_info(h, w, 1)};
        {
            std::ofstream f(prefix + ".s2b", std::ios::binary);
            for (const auto& s : sensors) f.write(reinterpret_cast<const char*>(s.sensor_to_body.m), 128);
            std::ofstream g(prefix + ".shifts", std::ios::binary);
            const std::vector<int32_t> sh(sensors[0].format.pixel_shift_by_row.begin(), sensors[0].format.pixel_shift_by_row.end());
            g.write(reinterpret_cast<const char*>(sh.data()), static_cast<std::streamsize>(sh.size() * 4));
        }
        const size_t npx = static_cast<size_t>(h) * w;
        auto make = [&](const oh::BatchOptions& opt) {
            auto b = std::make_unique<oh::DeviceFrameBatch>(sensors, n, opt);
            std::ifstream f(argv[1], std::ios::binary);
            const size_t ps = b->lidar_packet_size(), ppf = w / 16;
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
        };
        bool all = true;
        struct Kind {
            const char* tag;
            bool f64, world;
        };
        for (const Kind kind : {Kind{"body64", true, false}, Kind{"body32", false, false}, Kind{"world64", true, true}}) {
            oh::BatchOptions opt;
            opt.xyz = true;
            opt.xyz_f64 = kind.f64;
            opt.xyz_world_frame = kind.world;
            opt.auto_placement = false;
            auto b = make(opt);
            const std::string base = prefix + "." + kind.tag + ".";
            if (kind.world) {
                b->interp_poses(x_known, poses_known);
                b->decode();   // a world-frame batch applies its poses inside decode()
                std::vector<double> p(static_cast<size_t>(w) * 16);
                std::ofstream f(base + "poses", std::ios::binary);
                for (uint32_t fr = 0; fr < n; ++fr) {
                    b->download_poses(fr, p.data());
                    f.write(reinterpret_cast<const char*>(p.data()), static_cast<std::streamsize>(p.size() * 8));
                }
            }
            auto dump_inputs = [&](const std::string& pre) {
                std::vector<uint8_t> buf(std::max(b->xyz_bytes_per_frame(), npx * 4));
                for (int r = 0; r < 2; ++r) {
                    std::ofstream fx(base + pre + "xyz" + std::to_string(r), std::ios::binary);
                    std::ofstream fr_(base + pre + "r" + std::to_string(r), std::ios::binary);
                    for (uint32_t fr = 0; fr < n; ++fr) {
                        b->download_xyz(r, fr, buf.data());
                        fx.write(reinterpret_cast<const char*>(buf.data()), static_cast<std::streamsize>(b->xyz_bytes_per_frame()));
                        b->download_plane(r ? ChanField::RANGE2 : ChanField::RANGE, fr, buf.data());
                        fr_.write(reinterpret_cast<const char*>(buf.data()), static_cast<std::streamsize>(npx * 4));
                    }
                }
            };
            auto dump_normals = [&](int r, const std::string& name) {
                std::vector<double> nb(npx * 3);
                std::ofstream f(base + name, std::ios::binary);
                for (uint32_t fr = 0; fr < n; ++fr) {
                    b->download_normals(r, fr, nb.data());
                    f.write(reinterpret_cast<const char*>(nb.data()), static_cast<std::streamsize>(nb.size() * 8));
                }
            };
            dump_inputs("");
            bool ptr_ok = b->normals_device(0) == nullptr && b->normals_device(1) == nullptr;
            oh::NormalsOptions o;
            o.pixel_search_range = 3;
            b->normals(o);
            ptr_ok = ptr_ok && b->normals_device(0) != nullptr && b->normals_device(1) == nullptr;
            dump_normals(0, "single");
            o.dual_return = true;
            o.pixel_search_range = 1;
            b->normals(o);
            dump_normals(0, "d0");
            dump_normals(1, "d1");
            o.pixel_search_range = 2;
            o.staggered_output = true;
            b->normals(o);
            dump_normals(0, "s0");
            dump_normals(1, "s1");
            {   // download_normals is a copy from normals_device()
                std::vector<double> a(npx * 3), c(npx * 3);
                b->download_normals(1, n - 1, a.data());
                if (hipMemcpy(c.data(), b->normals_device(1) + static_cast<size_t>(n - 1) * npx * 3, npx * 24, hipMemcpyDeviceToHost) != hipSuccess)
                    throw std::runtime_error("hipMemcpy(normals) failed");
                ptr_ok = ptr_ok && a == c;
            }
            std::printf("device_ptr %s %d\n", kind.tag, ptr_ok ? 1 : 0);
            all = all && ptr_ok;
            if (std::string(kind.tag) == "body64") {
                b->filter_field(ChanField::RANGE, lo, hi);
                dump_inputs("f");
                o = oh::NormalsOptions();
                o.dual_return = true;
                b->normals(o);
                dump_normals(0, "fd0");
                dump_normals(1, "fd1");
            }
        }
        auto throws = [&](const oh::BatchOptions& opt, bool dual) {
            auto b = make(opt);
            oh::NormalsOptions o;
            o.dual_return = dual;
            try {
                b->normals(o);
            } catch (const std::invalid_argument&) {
                return true;
            }
            return false;
        };
        oh::BatchOptions plain;
        plain.auto_placement = false;
        const bool no_xyz = throws(plain, false);
        oh::BatchOptions first_only;
        first_only.auto_placement = false;
        first_only.xyz = true;
        first_only.planes = {ChanField::RANGE};
        const bool no_range2 = throws(first_only, true) && !throws(first_only, false);
        std::printf("no_xyz_throws %d\nno_range2_throws %d\n", no_xyz ? 1 : 0, no_range2 ? 1 : 0);
        return all && no_xyz && no_range2 ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 2;
    }
}
