// registration_batch_tool.cpp -- drives hip::DeviceFrameBatch::align_voxels_to_map and mapping::ICPRegistration's device overload for
// tests/test_gpu_registration_batch.py.
//   registration_batch_tool <packets.bin> <h> <w> <n_frames> <known.bin> <k> <out_prefix> <voxel_size> <map_voxel> <max_distance>
//                           <max_points> <reg_max_distance> <kernel_scale> <max_iterations>
//       packets.bin, known.bin: as for voxel_batch_tool.cpp, with its two sensors.  Two successive f64 body-frame batches of the same
//       packets: batch 0 is dewarped, voxel_downsample(voxel_size)d and goes into a VoxelHashMap3d(map_voxel, max_distance,
//       max_points) with add_voxels_to; batch 1 has its known poses moved by (0.05, -0.03, 0.02) m and packet 1 of frame 1 left out,
//       is aligned with align_voxels_to_map, its rows corrected by the pose on the host go into the map, and it is aligned again
//       against the grown map.  Leaves
//         <prefix>.r<r>.vox      download_voxels of batch r
//         <prefix>.pose1 / .pose2   the two poses, 16 doubles row-major
//         <prefix>.corrected     the rows that went into the map between the two calls
//       Prints "pre_voxel_throws 1" (before voxel_downsample: std::runtime_error), "host_map_throws 1" (a host map lives on no
//       device: std::invalid_argument), "bad_parameter_throws 1" (a negative max_distance: std::invalid_argument), "device_overload
//       1" (ICPRegistration::align_device_points_to_map on voxels_device() gives the same bits).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "batch_fixture.h"
#include "ouster/mapping/icp_registration.h"

using namespace fixture;
namespace om = ouster::sdk::mapping;

int main(int argc, char** argv) {
    if (argc != 15) {
        std::printf("usage: registration_batch_tool packets h w n known k prefix voxel_size map_voxel max_distance max_points reg_max_distance kernel_scale max_iterations\n");
        return 64;
    }
    try {
        const uint32_t h = std::atoi(argv[2]), w = std::atoi(argv[3]), n = std::atoi(argv[4]), k = std::atoi(argv[6]);
        const std::string prefix = argv[7];
        const double vs = std::atof(argv[8]), map_voxel = std::atof(argv[9]), max_distance = std::atof(argv[10]);
        const size_t max_points = std::atoi(argv[11]);
        const double reg_distance = std::atof(argv[12]), kernel = std::atof(argv[13]);
        const om::ICPRegistration reg(std::atoi(argv[14]));
        std::vector<double> x_known;
        std::vector<mat4d> poses_known;
        read_known(argv[5], k, x_known, poses_known);
        const std::vector<SensorInfo> sensors = {make_info(h, w, 0, false, true), make_info(h, w, 1, false, true)};
        const double step[3] = {0.05, -0.03, 0.02};
        VoxelHashMap3d map(map_voxel, max_distance, max_points);
        VoxelHashMap3d host = VoxelHashMap3d::on_host(map_voxel, max_distance, max_points);
        bool all = true;
        for (uint32_t r = 0; r < 2; ++r) {
            oh::BatchOptions opt;
            opt.xyz = true;
            opt.xyz_f64 = true;
            opt.auto_placement = false;
            auto b = load_batch(sensors, n, opt, argv[1], r, r);
            std::vector<mat4d> poses = poses_known;
            for (mat4d& p : poses) p.m[3] += r * step[0], p.m[7] += r * step[1], p.m[11] += r * step[2];
            b->interp_poses(x_known, poses);
            b->dewarp(0.5, 100.0);
            if (r == 0) {
                const bool pre = throws<std::runtime_error>([&] { b->align_voxels_to_map(map, reg, reg_distance, kernel); });
                std::printf("pre_voxel_throws %d\n", pre);
                all = all && pre;
            }
            const uint64_t count = b->voxel_downsample(vs);
            if (count == 0) throw std::runtime_error("a batch without voxel rows");
            std::vector<double> rows(count * 3);
            b->download_voxels(rows.data(), nullptr);
            write_file(prefix + ".r" + std::to_string(r) + ".vox", rows.data(), rows.size() * 8);
            if (r == 0) {
                b->add_voxels_to(map);
                continue;
            }
            const bool host_map = throws<std::invalid_argument>([&] { b->align_voxels_to_map(host, reg, reg_distance, kernel); });
            std::printf("host_map_throws %d\n", host_map);
            const bool bad = throws<std::invalid_argument>([&] { b->align_voxels_to_map(map, reg, -1.0, kernel); });
            std::printf("bad_parameter_throws %d\n", bad);
            const mat4d T = b->align_voxels_to_map(map, reg, reg_distance, kernel);
            write_file(prefix + ".pose1", T.data(), 128);
            const mat4d same = reg.align_device_points_to_map(b->voxels_device(), count, 3, map, reg_distance, kernel);
            const bool overload = std::memcmp(same.data(), T.data(), 128) == 0;
            std::printf("device_overload %d\n", overload);
            ArrayX3dR corrected(count);
            for (uint64_t i = 0; i < count; ++i)
                for (int c = 0; c < 3; ++c)
                    corrected.data()[3 * i + c] = T(c, 0) * rows[3 * i] + T(c, 1) * rows[3 * i + 1] + T(c, 2) * rows[3 * i + 2] + T(c, 3);
            write_file(prefix + ".corrected", corrected.data(), count * 24);
            map.add_points(corrected);
            const mat4d T2 = b->align_voxels_to_map(map, reg, reg_distance, kernel);
            write_file(prefix + ".pose2", T2.data(), 128);
            all = all && host_map && bad && overload;
        }
        return all ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 2;
    }
}
