// voxel_batch_tool.cpp -- drives voxel_downsample / voxel_downsample_with_normals / voxels_device / download_voxels of
// hip::DeviceFrameBatch for tests/test_gpu_voxel_batch.py (built by this directory's Makefile).
//   voxel_batch_tool <packets.bin> <h> <w> <n_frames> <skip_frame> <skip_packet> <known.bin> <k> <out_prefix> <lo> <hi> <vs_a> <vs_b>
//       packets.bin, known.bin: as for normals_batch_tool.cpp, with its two sensors.  Two dual-return body-frame batches,
//       <B> = b64 (xyz_f64) and b32 (float); each gets interp_poses(known) and leaves
//         <prefix>.<B>.dw        download_dewarped points of dewarp(0.5, 100)      (f64 / f32, [total][3])
//         <prefix>.<B>.va / .vb  download_voxels after voxel_downsample(vs_a) / (vs_b, {AVERAGE_POINT, min_pts_threshold 2})
//         <prefix>.<B>.vlast     ... after voxel_downsample(vs_b, {RANDOM})
//         <prefix>.<B>.xyz0 / .nrm0   the first return's cloud and its normals({staggered_output}), [n] frames each
//         <prefix>.<B>.wnp / .wnn     download_voxels(points, normals) after voxel_downsample_with_normals(vs_b)
//       then filter_field(RANGE, lo, hi), a fresh dewarp() and normals(), and the same files with an "f" before the name
//       (.fdw .fva .fxyz0 .fnrm0 .fwnp .fwnn).
//       Prints "pre_dewarp_throws 1", "pre_normals_throws 1", "destaggered_throws 1" for the three precondition errors
//       (std::invalid_argument), "host_only_throws 1" for FIRST_N_POINT keeping 3 points (std::runtime_error), "grid_throws 1" for a
//       voxel size of 1e-12 (std::invalid_argument), "no_result_after_throw 1" when both leave voxels_device() null, and
//       "device_ptr <B> 1" when voxels_device() / voxel_normals_device() are null where they must be, voxel_count() is the
//       returned count and download_voxels equals a copy from the device pointers.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "batch_fixture.h"

using namespace fixture;

int main(int argc, char** argv) {
    if (argc != 14) {
        std::printf("usage: voxel_batch_tool packets h w n skip_frame skip_packet known k prefix lo hi vs_a vs_b\n");
        return 64;
    }
    try {
        const uint32_t h = std::atoi(argv[2]), w = std::atoi(argv[3]), n = std::atoi(argv[4]);
        const uint32_t skip_frame = std::atoi(argv[5]), skip_packet = std::atoi(argv[6]), k = std::atoi(argv[8]);
        const std::string prefix = argv[9];
        const double lo = std::atof(argv[10]), hi = std::atof(argv[11]), vs_a = std::atof(argv[12]), vs_b = std::atof(argv[13]);
        std::vector<double> x_known;
        std::vector<mat4d> poses_known;
        read_known(argv[7], k, x_known, poses_known);
        const std::vector<SensorInfo> sensors = {make_info(h, w, 0, false, true), make_info(h, w, 1, false, true)};
        const size_t npx = static_cast<size_t>(h) * w;
        bool all = true;
        for (const bool f64 : {true, false}) {
            oh::BatchOptions opt;
            opt.xyz = true;
            opt.xyz_f64 = f64;
            opt.auto_placement = false;
            auto b = load_batch(sensors, n, opt, argv[1], skip_frame, skip_packet);
            const std::string tag = f64 ? "b64" : "b32", base = prefix + "." + tag + ".";
            const size_t es = f64 ? 8 : 4;
            b->interp_poses(x_known, poses_known);

            // the three preconditions, and what a fresh batch reports
            bool ptr_ok = b->voxels_device() == nullptr && b->voxel_normals_device() == nullptr && b->voxel_count() == 0;
            const bool pre_dewarp = throws<std::invalid_argument>([&] { b->voxel_downsample(vs_a); });
            const bool pre_normals = throws<std::invalid_argument>([&] { b->voxel_downsample_with_normals(vs_b); });
            b->normals(oh::NormalsOptions());   // destaggered layout: normal i is not point i's
            const bool destaggered = throws<std::invalid_argument>([&] { b->voxel_downsample_with_normals(vs_b); });
            ptr_ok = ptr_ok && throws<std::invalid_argument>([&] { b->download_voxels(nullptr, nullptr); });
            std::printf("pre_dewarp_throws %d\npre_normals_throws %d\ndestaggered_throws %d\n", pre_dewarp, pre_normals, destaggered);
            all = all && pre_dewarp && pre_normals && destaggered;

            auto voxels = [&](const std::string& name, uint64_t count, bool with_normals, const std::string& normals_name) {
                if (b->voxel_count() != count) throw std::runtime_error("voxel_count() differs from the returned count");
                std::vector<double> p(count * 3), q(with_normals ? count * 3 : 0);
                b->download_voxels(p.data(), with_normals ? q.data() : nullptr);
                write_file(base + name, p.data(), p.size() * 8);
                if (with_normals) write_file(base + normals_name, q.data(), q.size() * 8);
                std::vector<double> c(count * 3);
                if (count && hipMemcpy(c.data(), b->voxels_device(), count * 24, hipMemcpyDeviceToHost) != hipSuccess)
                    throw std::runtime_error("hipMemcpy(voxels) failed");
                ptr_ok = ptr_ok && c == p && (b->voxel_normals_device() != nullptr) == with_normals;
                if (with_normals && count) {
                    if (hipMemcpy(c.data(), b->voxel_normals_device(), count * 24, hipMemcpyDeviceToHost) != hipSuccess)
                        throw std::runtime_error("hipMemcpy(voxel normals) failed");
                    ptr_ok = ptr_ok && c == q;
                } else if (!with_normals) {
                    ptr_ok = ptr_ok && throws<std::invalid_argument>([&] { b->download_voxels(nullptr, c.data()); });
                }
            };
            auto round = [&](const std::string& pre, bool every_form) {
                const uint64_t total = b->dewarp(0.5, 100.0);
                std::vector<uint8_t> pts(total * 3 * es);
                b->download_dewarped(pts.data(), nullptr, nullptr, nullptr);
                write_file(base + pre + "dw", pts.data(), pts.size());
                voxels(pre + "va", b->voxel_downsample(vs_a), false, "");
                if (every_form) {
                    oh::VoxelOptions o;
                    o.min_pts_threshold = 2;
                    voxels(pre + "vb", b->voxel_downsample(vs_b, o), false, "");
                    o = oh::VoxelOptions();
                    o.strategy = VoxelDownsampleStrategy::RANDOM;
                    voxels(pre + "vlast", b->voxel_downsample(vs_b, o), false, "");
                }
                oh::NormalsOptions no;
                no.staggered_output = true;
                b->normals(no);
                write_frames(base + pre + "xyz0", n, b->xyz_bytes_per_frame(), [&](uint32_t fr, void* d) { b->download_xyz(0, fr, d); });
                write_frames(base + pre + "nrm0", n, npx * 24, [&](uint32_t fr, double* d) { b->download_normals(0, fr, d); });
                voxels(pre + "wnp", b->voxel_downsample_with_normals(vs_b), true, pre + "wnn");
            };
            round("", true);
            oh::VoxelOptions several;
            several.strategy = VoxelDownsampleStrategy::FIRST_N_POINT;
            several.max_points_per_voxel = 3;
            const bool host_only = throws<std::runtime_error>([&] { b->voxel_downsample(vs_a, several); });
            // a call that throws leaves no result behind, whatever the call before it made
            bool no_result = b->voxels_device() == nullptr && b->voxel_count() == 0 &&
                             throws<std::invalid_argument>([&] { b->download_voxels(nullptr, nullptr); });
            b->voxel_downsample(vs_a);
            const bool grid = throws<std::invalid_argument>([&] { b->voxel_downsample(1e-12); });   // no int32 holds p / 1e-12
            no_result = no_result && grid && b->voxels_device() == nullptr && b->voxel_normals_device() == nullptr && b->voxel_count() == 0;
            std::printf("host_only_throws %d\ngrid_throws %d\nno_result_after_throw %d\n", host_only, grid, no_result);
            all = all && no_result;
            b->filter_field(ChanField::RANGE, lo, hi);
            round("f", false);
            std::printf("device_ptr %s %d\n", tag.c_str(), ptr_ok ? 1 : 0);
            all = all && ptr_ok && host_only;
        }
        return all ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 2;
    }
}
