// normals_batch_tool.cpp -- drives normals / normals_device / download_normals of hip::DeviceFrameBatch for
// tests/test_gpu_normals_batch.py (built by this directory's Makefile).
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

#include "batch_fixture.h"

using namespace fixture;

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
        std::vector<double> x_known;
        std::vector<mat4d> poses_known;
        read_known(argv[7], k, x_known, poses_known);
        // a mount of its own per sensor
        const std::vector<SensorInfo> sensors = {make_info(h, w, 0, false, true), make_info(h, w, 1, false, true)};
        {
            std::ofstream f(prefix + ".s2b", std::ios::binary);
            for (const auto& s : sensors) f.write(reinterpret_cast<const char*>(s.sensor_to_body.m), 128);
            const std::vector<int32_t> sh(sensors[0].format.pixel_shift_by_row.begin(), sensors[0].format.pixel_shift_by_row.end());
            write_file(prefix + ".shifts", sh.data(), sh.size() * 4);
        }
        const size_t npx = static_cast<size_t>(h) * w;
        auto make = [&](const oh::BatchOptions& opt) { return load_batch(sensors, n, opt, argv[1], skip_frame, skip_packet); };
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
                write_frames(base + "poses", n, static_cast<size_t>(w) * 128, [&](uint32_t fr, double* p) { b->download_poses(fr, p); });
            }
            auto dump_inputs = [&](const std::string& pre) {
                for (int r = 0; r < 2; ++r) {
                    write_frames(base + pre + "xyz" + std::to_string(r), n, b->xyz_bytes_per_frame(),
                                 [&](uint32_t fr, void* d) { b->download_xyz(r, fr, d); });
                    write_frames(base + pre + "r" + std::to_string(r), n, npx * 4,
                                 [&](uint32_t fr, void* d) { b->download_plane(r ? ChanField::RANGE2 : ChanField::RANGE, fr, d); });
                }
            };
            auto dump_normals = [&](int r, const std::string& name) {
                write_frames(base + name, n, npx * 24, [&](uint32_t fr, double* d) { b->download_normals(r, fr, d); });
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
        auto refuses = [&](const oh::BatchOptions& opt, bool dual) {
            auto b = make(opt);
            oh::NormalsOptions o;
            o.dual_return = dual;
            return throws<std::invalid_argument>([&] { b->normals(o); });
        };
        oh::BatchOptions plain;
        plain.auto_placement = false;
        const bool no_xyz = refuses(plain, false);
        oh::BatchOptions first_only;
        first_only.auto_placement = false;
        first_only.xyz = true;
        first_only.planes = {ChanField::RANGE};
        const bool no_range2 = refuses(first_only, true) && !refuses(first_only, false);
        std::printf("no_xyz_throws %d\nno_range2_throws %d\n", no_xyz ? 1 : 0, no_range2 ? 1 : 0);
        return all && no_xyz && no_range2 ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 2;
    }
}
