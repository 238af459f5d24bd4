// icp_batch_tool.cpp -- drives hip::DeviceFrameBatch::align_voxels for tests/test_gpu_icp_batch.py (built by this directory's
// Makefile).
//   icp_batch_tool <capture.pcap> <metadata.json> <n_frames> <voxel_size> <max_corr_dist> <out_prefix>
// Two sensors with the capture's metadata (the second mounted elsewhere on the body), a batch of n_frames double-precision frames
// filled with the capture's frames in turn.  Prints "pre_voxel_throws 1" when align_voxels before any voxel call is
// std::runtime_error.  Then dewarp(), normals({staggered_output}) and, per route R:
//   plane: voxel_downsample_with_normals(voxel_size);  point: voxel_downsample(voxel_size)
//   <prefix>.<R>.src / .srcn     download_voxels (f64 [m][3]; .srcn on the plane route)
//   <prefix>.<R>.tgt / .tgtn     the same rows moved by a fixed small rigid transform: the target, uploaded to the device
//   <prefix>.<R>.pose            align_voxels: 16 doubles, then iterations, correspondences, solved, point_to_plane as doubles
// and "routes 1" when the plane route reported point_to_plane and the point route did not (target normals given to both: the point
// route has no voxel normals).
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "batch_fixture.h"
#include "ouster/pcap/pcap.h"

using namespace fixture;

struct DeviceCopy {
    double* p = nullptr;
    explicit DeviceCopy(const std::vector<double>& host) {
        if (hipMalloc(reinterpret_cast<void**>(&p), host.size() * 8 + 8) != hipSuccess) throw std::runtime_error("hipMalloc failed");
        if (!host.empty() && hipMemcpy(p, host.data(), host.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
            throw std::runtime_error("hipMemcpy failed");
    }
    ~DeviceCopy() { (void)hipFree(p); }
    DeviceCopy(const DeviceCopy&) = delete;
    DeviceCopy& operator=(const DeviceCopy&) = delete;
};

int main(int argc, char** argv) {
    if (argc != 7) {
        std::printf("usage: icp_batch_tool capture.pcap metadata.json n_frames voxel_size max_corr_dist prefix\n");
        return 64;
    }
    try {
        const uint32_t n = std::atoi(argv[3]);
        const double voxel_size = std::atof(argv[4]), max_corr_dist = std::atof(argv[5]);
        const std::string prefix = argv[6];
        SensorInfo first = metadata_from_json(argv[2]);
        SensorInfo second = first;
        second.sensor_to_body = mat4d::Identity();
        second.sensor_to_body.m[0] = std::cos(0.5), second.sensor_to_body.m[1] = -std::sin(0.5);
        second.sensor_to_body.m[4] = std::sin(0.5), second.sensor_to_body.m[5] = std::cos(0.5);
        second.sensor_to_body.m[3] = 0.4, second.sensor_to_body.m[7] = -0.3, second.sensor_to_body.m[11] = 0.2;
        const PacketFormat& pf = get_format(first);

        // the capture's lidar packets by frame, frames in order of appearance
        std::vector<uint32_t> order;
        std::map<uint32_t, std::vector<std::vector<uint8_t>>> frames;
        ouster::sdk::pcap::PcapReader pcap(argv[1]);
        while (pcap.next_packet()) {
            if (pcap.current_length() != pf.lidar_packet_size) continue;
            const uint32_t id = pf.frame_id(pcap.current_data());
            if (!frames.count(id)) order.push_back(id);
            frames[id].emplace_back(pcap.current_data(), pcap.current_data() + pcap.current_length());
        }
        if (order.empty()) throw std::runtime_error("no lidar packets in the capture");

        oh::BatchOptions opt;
        opt.xyz = true;
        opt.xyz_f64 = true;
        opt.auto_placement = false;
        oh::DeviceFrameBatch b(std::vector<SensorInfo>{first, second}, n, opt);
        for (uint32_t fr = 0; fr < n; ++fr) {
            std::vector<const uint8_t*> ptrs;
            for (const auto& pk : frames[order[fr % order.size()]]) ptrs.push_back(pk.data());
            b.upload_frame_packets(fr, ptrs);
        }
        b.decode();

        DeviceCopy nothing(std::vector<double>(60 * 3, 0.0));
        const bool pre = throws<std::runtime_error>([&] { b.align_voxels(nothing.p, nullptr, 60, nullptr); });
        std::printf("pre_voxel_throws %d\n", pre ? 1 : 0);

        // the move: a rotation of 0.01 rad about (1, 2, 3) / sqrt(14) by Rodrigues' formula, and a few centimetres
        const double ang = 0.01, ax[3] = {1 / std::sqrt(14.0), 2 / std::sqrt(14.0), 3 / std::sqrt(14.0)}, t[3] = {0.04, -0.03, 0.02};
        double R[3][3];
        const double c = std::cos(ang), s = std::sin(ang);
        const double K[3][3] = {{0, -ax[2], ax[1]}, {ax[2], 0, -ax[0]}, {-ax[1], ax[0], 0}};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R[i][j] = (i == j ? c : 0.0) + s * K[i][j] + (1 - c) * ax[i] * ax[j];

        b.dewarp(0.5, 100.0);
        oh::NormalsOptions no;
        no.staggered_output = true;
        b.normals(no);
        oh::AlignOptions ao;
        ao.max_corr_dist = max_corr_dist;
        bool routes = true;
        for (const bool plane : {true, false}) {
            const std::string base = prefix + (plane ? ".plane." : ".point.");
            const uint64_t m = plane ? b.voxel_downsample_with_normals(voxel_size) : b.voxel_downsample(voxel_size);
            std::vector<double> p(m * 3), q(plane ? m * 3 : 0), tp(m * 3), tq(m * 3);
            b.download_voxels(p.data(), plane ? q.data() : nullptr);
            for (uint64_t i = 0; i < m; ++i)
                for (int r = 0; r < 3; ++r) {
                    tp[3 * i + r] = R[r][0] * p[3 * i] + R[r][1] * p[3 * i + 1] + R[r][2] * p[3 * i + 2] + t[r];
                    // the point route has no normals of its own: any unit normals do for a target that offers some
                    tq[3 * i + r] = plane ? R[r][0] * q[3 * i] + R[r][1] * q[3 * i + 1] + R[r][2] * q[3 * i + 2] : (r == 2 ? 1.0 : 0.0);
                }
            write_file(base + "src", p.data(), p.size() * 8);
            if (plane) write_file(base + "srcn", q.data(), q.size() * 8);
            write_file(base + "tgt", tp.data(), tp.size() * 8);
            write_file(base + "tgtn", tq.data(), tq.size() * 8);
            DeviceCopy dp(tp), dq(tq);
            const oh::AlignResult res = b.align_voxels(dp.p, dq.p, m, nullptr, ao);
            routes = routes && res.point_to_plane == plane;
            std::vector<double> out(res.pose.data(), res.pose.data() + 16);
            out.push_back(res.iterations), out.push_back(static_cast<double>(res.correspondences)), out.push_back(res.solved);
            out.push_back(res.point_to_plane);
            write_file(base + "pose", out.data(), out.size() * 8);
        }
        std::printf("routes %d\n", routes ? 1 : 0);
        return pre && routes ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 2;
    }
}
