// icp_target_batch_tool.cpp -- drives hip::DeviceFrameBatch::make_icp_target and align_voxels(IcpTarget) for
// tests/test_gpu_icp_target_batch.py.
//   icp_target_batch_tool <capture.pcap> <metadata.json> <n_frames> <voxel_size> <max_corr_dist> <out_prefix>
// The fixture of icp_batch_tool: two sensors, n_frames double-precision frames from the capture, dewarp(), normals().  Prints
// "pre_voxel_throws 1" when make_icp_target and align_voxels(target) before any voxel call are std::runtime_error.  Then per route R
// (plane: voxel_downsample_with_normals; point: voxel_downsample) the batch's own voxel rows become the target -- the keyframe --
// and the batch is aligned against it from a small move as the guess, twice:
//   <prefix>.<R>.target    align_voxels(make_icp_target(), guess): 16 doubles, then iterations, correspondences, solved, point_to_plane
//   <prefix>.<R>.pointer   align_voxels(voxels_device(), voxel_normals_device(), voxel_count(), guess): the same
//   <prefix>.<R>.info      rows, has_normals, device_bytes of the target as doubles
// and "wrong_method_throws 1" when the point route's batch, which has no voxel normals, is refused by the plane route's target.
// Last the batch is destroyed and the plane route's target, which outlives it, aligns the downloaded rows once more from host
// memory: "outlives_batch 1" when that equals <prefix>.plane.target bit for bit.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "batch_fixture.h"
#include "ouster/pcap/pcap.h"

using namespace fixture;

static std::vector<double> flat(const oh::AlignResult& res) {
    std::vector<double> out(res.pose.data(), res.pose.data() + 16);
    out.push_back(res.iterations), out.push_back(static_cast<double>(res.correspondences)), out.push_back(res.solved);
    out.push_back(res.point_to_plane);
    return out;
}

int main(int argc, char** argv) {
    if (argc != 7) {
        std::printf("usage: icp_target_batch_tool capture.pcap metadata.json n_frames voxel_size max_corr_dist prefix\n");
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
        std::unique_ptr<oh::DeviceFrameBatch> batch(new oh::DeviceFrameBatch(std::vector<SensorInfo>{first, second}, n, opt));
        oh::DeviceFrameBatch& b = *batch;
        for (uint32_t fr = 0; fr < n; ++fr) {
            std::vector<const uint8_t*> ptrs;
            for (const auto& pk : frames[order[fr % order.size()]]) ptrs.push_back(pk.data());
            b.upload_frame_packets(fr, ptrs);
        }
        b.decode();

        oh::AlignOptions ao;
        ao.max_corr_dist = max_corr_dist;
        const bool pre = throws<std::runtime_error>([&] { b.make_icp_target(ao); });
        std::printf("pre_voxel_throws %d\n", pre ? 1 : 0);

        // the guess: a rotation of 0.01 rad about z and a few centimetres
        double guess[16] = {std::cos(0.01), -std::sin(0.01), 0, 0.04, std::sin(0.01), std::cos(0.01), 0, -0.03, 0, 0, 1, 0.02, 0, 0, 0, 1};

        b.dewarp(0.5, 100.0);
        oh::NormalsOptions no;
        no.staggered_output = true;
        b.normals(no);
        bool same = true, wrong = false;
        std::unique_ptr<ouster::sdk::algorithm::IcpTarget> plane_target;
        std::vector<double> kept_pts, kept_nrm, kept;   // the plane route's rows on the host, and its result
        for (const bool plane : {true, false}) {
            const std::string base = prefix + (plane ? ".plane." : ".point.");
            const uint64_t m = plane ? b.voxel_downsample_with_normals(voxel_size) : b.voxel_downsample(voxel_size);
            ouster::sdk::algorithm::IcpTarget target = b.make_icp_target(ao);
            const std::vector<double> a = flat(b.align_voxels(target, guess, ao));
            // the single-call route in between: the target does not live in the context's workspace
            const std::vector<double> p = flat(b.align_voxels(b.voxels_device(), b.voxel_normals_device(), m, guess, ao));
            const std::vector<double> again = flat(b.align_voxels(target, guess, ao));
            same = same && a == again && target.size() == m && target.has_normals() == plane;
            write_file(base + "target", a.data(), a.size() * 8);
            write_file(base + "pointer", p.data(), p.size() * 8);
            const double info[3] = {static_cast<double>(target.size()), target.has_normals() ? 1.0 : 0.0, static_cast<double>(target.device_bytes())};
            write_file(base + "info", info, sizeof info);
            if (plane) {
                kept_pts.resize(m * 3), kept_nrm.resize(m * 3), kept = a;
                b.download_voxels(kept_pts.data(), kept_nrm.data());
            }
            if (plane) plane_target.reset(new ouster::sdk::algorithm::IcpTarget(std::move(target)));
            else wrong = throws<std::invalid_argument>([&] { b.align_voxels(*plane_target, guess, ao); });
        }
        std::printf("repeatable %d\nwrong_method_throws %d\n", same ? 1 : 0, wrong ? 1 : 0);
        // the keyframe outlives the batch that made it: the batch's context goes on living with the target
        batch.reset();
        const size_t m = kept_pts.size() / 3;
        ouster::sdk::core::ArrayX3dR pts(m), nrm(m);
        for (size_t i = 0; i < m; ++i)
            for (int c = 0; c < 3; ++c) pts(i, c) = kept_pts[3 * i + c], nrm(i, c) = kept_nrm[3 * i + c];
        const mat4d late = plane_target->align(pts, nrm, mat4d::FromRowMajor(guess), ao.max_normal_angle_deg);
        const bool outlives = std::vector<double>(late.data(), late.data() + 16) == std::vector<double>(kept.begin(), kept.begin() + 16);
        std::printf("outlives_batch %d\n", outlives ? 1 : 0);
        return pre && same && wrong && outlives ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 2;
    }
}
