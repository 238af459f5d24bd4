// voxel_map_batch_tool.cpp -- drives add_voxels_to / update_voxel_map / closest_in / map_neighbors_device / download_map_neighbors of
// hip::DeviceFrameBatch for tests/test_gpu_voxel_map_batch.py.
//   voxel_map_batch_tool <packets.bin> <h> <w> <n_frames> <known.bin> <k> <out_prefix> <voxel_size> <map_voxel> <max_distance> <max_points> <bound_sq>
//       packets.bin, known.bin: as for voxel_batch_tool.cpp, with its two sensors.  Three successive f64 body-frame batches r = 0, 1,
//       2 of the same packets, batch r with its known poses moved by r * (1.5, -0.75, 0.25) m and packet r of frame r left out; each
//       is dewarped, voxel_downsample(voxel_size)d and goes into ONE VoxelHashMap3d(map_voxel, max_distance, max_points) with
//       update_voxel_map(map, position r), position r = batch r's first voxel row.  Leaves
//         <prefix>.r<r>.pos     position r, 3 doubles
//         <prefix>.r<r>.vox     download_voxels of batch r
//         <prefix>.r<r>.cloud   map.pointcloud() after update r
//         <prefix>.nn / .d2     download_map_neighbors after closest_in(map, bound_sq) on batch 2
//         <prefix>.add.cloud    a second map after add_voxels_to on batches 0 and 2
//       Prints "pre_voxel_throws 1" (the four calls before voxel_downsample: std::runtime_error), "host_map_throws 1" (a host map:
//       std::invalid_argument), "pre_closest 1" (null pointers and a throwing download before closest_in, and again after a new
//       voxel_downsample), "device_ptr 1" (download_map_neighbors equals a copy from the device pointers), "grid_throws 1" (a position
//       outside the grid: std::invalid_argument, the map unchanged).
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "batch_fixture.h"

using namespace fixture;

int main(int argc, char** argv) {
    if (argc != 13) {
        std::printf("usage: voxel_map_batch_tool packets h w n known k prefix voxel_size map_voxel max_distance max_points bound_sq\n");
        return 64;
    }
    try {
        const uint32_t h = std::atoi(argv[2]), w = std::atoi(argv[3]), n = std::atoi(argv[4]), k = std::atoi(argv[6]);
        const std::string prefix = argv[7];
        const double vs = std::atof(argv[8]), map_voxel = std::atof(argv[9]), max_distance = std::atof(argv[10]), bound_sq = std::atof(argv[12]);
        const size_t max_points = std::atoi(argv[11]);
        std::vector<double> x_known;
        std::vector<mat4d> poses_known;
        read_known(argv[5], k, x_known, poses_known);
        const std::vector<SensorInfo> sensors = {make_info(h, w, 0, false, true), make_info(h, w, 1, false, true)};
        const double step[3] = {1.5, -0.75, 0.25};
        VoxelHashMap3d map(map_voxel, max_distance, max_points), added(map_voxel, max_distance, max_points);
        VoxelHashMap3d host = VoxelHashMap3d::on_host(map_voxel, max_distance, max_points);
        bool all = true;
        for (uint32_t r = 0; r < 3; ++r) {
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
                const double origin[3] = {0, 0, 0};
                const bool pre = throws<std::runtime_error>([&] { b->add_voxels_to(map); }) &&
                                 throws<std::runtime_error>([&] { b->update_voxel_map(map, origin); }) &&
                                 throws<std::runtime_error>([&] { b->closest_in(map); }) && map.empty() &&
                                 throws<std::invalid_argument>([&] { b->download_map_neighbors(nullptr, nullptr); });
                std::printf("pre_voxel_throws %d\n", pre);
                all = all && pre;
            }
            const uint64_t count = b->voxel_downsample(vs);
            std::vector<double> rows(count * 3);
            b->download_voxels(rows.data(), nullptr);
            const std::string base = prefix + ".r" + std::to_string(r) + ".";
            write_file(base + "vox", rows.data(), rows.size() * 8);
            if (count == 0) throw std::runtime_error("a batch without voxel rows");
            const double position[3] = {rows[0], rows[1], rows[2]};   // on the cloud, wherever the poses put it
            write_file(base + "pos", position, sizeof position);
            if (r == 0) {
                const bool host_map = throws<std::invalid_argument>([&] { b->add_voxels_to(host); }) &&
                                      throws<std::invalid_argument>([&] { b->update_voxel_map(host, position); }) &&
                                      throws<std::invalid_argument>([&] { b->closest_in(host); }) && host.empty();
                std::printf("host_map_throws %d\n", host_map);
                all = all && host_map;
            }
            b->update_voxel_map(map, position);
            if (r != 1) b->add_voxels_to(added);
            const ArrayX3dR cloud = map.pointcloud();
            write_file(base + "cloud", cloud.data(), cloud.rows() * 24);
            if (r == 2) {
                bool pre = b->map_neighbors_device() == nullptr && b->map_neighbor_dist_device() == nullptr &&
                           throws<std::invalid_argument>([&] { b->download_map_neighbors(nullptr, nullptr); });
                const double nan = std::numeric_limits<double>::quiet_NaN();
                const double outside[3] = {nan, 0, 0};
                const size_t before = map.num_points();
                const bool grid = throws<std::invalid_argument>([&] { b->update_voxel_map(map, outside); }) && map.num_points() == before;
                std::printf("grid_throws %d\n", grid);
                b->closest_in(map, bound_sq);
                std::vector<double> nn(count * 3), d2(count), c3(count * 3), c1(count);
                b->download_map_neighbors(nn.data(), d2.data());
                write_file(prefix + ".nn", nn.data(), nn.size() * 8);
                write_file(prefix + ".d2", d2.data(), d2.size() * 8);
                const bool ptr = count && hipMemcpy(c3.data(), b->map_neighbors_device(), count * 24, hipMemcpyDeviceToHost) == hipSuccess &&
                                 hipMemcpy(c1.data(), b->map_neighbor_dist_device(), count * 8, hipMemcpyDeviceToHost) == hipSuccess && c3 == nn && c1 == d2;
                std::printf("device_ptr %d\n", ptr);
                b->voxel_downsample(2.0 * vs);      // new rows: the neighbours of the old ones are gone
                pre = pre && b->map_neighbors_device() == nullptr && throws<std::invalid_argument>([&] { b->download_map_neighbors(nullptr, nullptr); });
                std::printf("pre_closest %d\n", pre);
                all = all && grid && ptr && pre;
            }
        }
        const ArrayX3dR cloud = added.pointcloud();
        write_file(prefix + ".add.cloud", cloud.data(), cloud.rows() * 24);
        return all ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 2;
    }
}
