// pose_batch_tool.cpp -- drives interp_poses / download_poses / poses_device of hip::DeviceFrameBatch for
// tests/test_gpu_pose_batch.py (built by this directory's Makefile).
//   pose_batch_tool <packets.bin> <h> <w> <n_frames> <skip_frame> <skip_packet> <known.bin> <k> <out_prefix> <min_range> <max_range>
//       packets.bin: [n_frames][w / 16][lidar_packet_size] bytes of RNG15_RFL8_NIR8_DUAL packets; packet <skip_packet> of frame
//       <skip_frame> is left out.  known.bin: k doubles (seconds), then k x 16 doubles.  The two sensors of
//       frame_ops_batch_tool.cpp.  Once for a float batch ("f32") and once for an xyz_f64 batch ("f64"):
//         <prefix>.<T>.hdr   timestamps u64 [n][w], then status u32 [n][w]
//         <prefix>.<T>.p0    the poses of the fresh batch                                   f64 [n][w][16]
//         <prefix>.<T>.p1    after interp_poses(x_known, poses_known)
//         <prefix>.<T>.p2    a SECOND batch that got p1 through download_poses -> upload_poses -- with the rows of the INVALID
//                            columns (status bit 0 clear) replaced by a marker pose first: poses[k - 1] with element 3 raised
//                            by 0.5 * (column + 1) and element 7 lowered by the frame index -- after the two-pose overload
//                            interp_poses(x_known[0], poses[0], x_known[k - 1], poses[k - 1])
//         <prefix>.f32.rows2 the float rows of that second batch at the same moment (pose_rows_device()), f32 [n][w][12]
//       and dewarp(min, max, provenance) of the first batch after interp_poses is compared, bit for bit and with provenance,
//       with dewarp() of the second batch before its two-pose call ("dewarp_equal <T> 1"), and with the first batch's dewarp
//       on identity poses ("poses_matter <T> 1").
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "batch_fixture.h"

using namespace fixture;

struct Dewarped {
    std::vector<uint8_t> pts;
    std::vector<uint32_t> fi, ci;
    std::vector<uint64_t> ts, off;
    bool operator==(const Dewarped& o) const { return pts == o.pts && fi == o.fi && ci == o.ci && ts == o.ts && off == o.off; }
};

static Dewarped run_dewarp(oh::DeviceFrameBatch& b, double lo, double hi, size_t point_bytes) {
    Dewarped d;
    const uint64_t total = b.dewarp(lo, hi, true);
    d.pts.resize(total * point_bytes);
    d.fi.resize(total);
    d.ci.resize(total);
    d.ts.resize(total);
    b.download_dewarped(d.pts.data(), d.fi.data(), d.ci.data(), d.ts.data());
    d.off = b.dewarped_frame_offsets();
    return d;
}

int main(int argc, char** argv) {
    if (argc != 12) {
        std::printf("usage: pose_batch_tool packets h w n skip_frame skip_packet known k prefix min_range max_range\n");
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
        const std::vector<SensorInfo> sensors = {make_info(h, w, 0), make_info(h, w, 1)};
        bool all = true;
        for (const bool f64 : {false, true}) {
            const std::string tag = f64 ? "f64" : "f32";
            oh::BatchOptions opt;
            opt.xyz = true;
            opt.xyz_f64 = f64;
            opt.auto_placement = false;
            auto make = [&]() { return load_batch(sensors, n, opt, argv[1], skip_frame, skip_packet); };
            auto dump_poses = [&](oh::DeviceFrameBatch& b, const std::string& name) {
                write_frames(prefix + "." + tag + "." + name, n, static_cast<size_t>(w) * 128, [&](uint32_t fr, double* p) { b.download_poses(fr, p); });
            };
            auto b1 = make();
            {
                std::vector<uint64_t> ts(w);
                std::vector<uint32_t> st(w);
                std::ofstream f(prefix + "." + tag + ".hdr", std::ios::binary);
                std::vector<uint32_t> all_st;
                for (uint32_t fr = 0; fr < n; ++fr) {
                    b1->download_headers(fr, ts.data(), nullptr, st.data());
                    f.write(reinterpret_cast<const char*>(ts.data()), static_cast<std::streamsize>(w * 8));
                    all_st.insert(all_st.end(), st.begin(), st.end());
                }
                f.write(reinterpret_cast<const char*>(all_st.data()), static_cast<std::streamsize>(all_st.size() * 4));
            }
            const size_t pb = f64 ? 24 : 12;
            dump_poses(*b1, "p0");
            const Dewarped on_identity = run_dewarp(*b1, lo, hi, pb);
            b1->interp_poses(x_known, poses_known);
            dump_poses(*b1, "p1");
            const Dewarped interpolated = run_dewarp(*b1, lo, hi, pb);

            auto b2 = make();
            std::vector<double> p(static_cast<size_t>(w) * 16);
            std::vector<uint32_t> st(w);
            for (uint32_t fr = 0; fr < n; ++fr) {
                b1->download_poses(fr, p.data());
                b1->download_headers(fr, nullptr, nullptr, st.data());
                for (uint32_t c = 0; c < w; ++c) {
                    if (st[c] & 1u) continue;
                    std::memcpy(&p[static_cast<size_t>(c) * 16], poses_known.back().m, 128);   // a marker no interpolation produces
                    p[static_cast<size_t>(c) * 16 + 3] += 0.5 * (c + 1);
                    p[static_cast<size_t>(c) * 16 + 7] -= fr;
                }
                b2->upload_poses(fr, p.data());
            }
            const Dewarped uploaded = run_dewarp(*b2, lo, hi, pb);
            const bool equal = !interpolated.pts.empty() && interpolated == uploaded;
            const bool matter = on_identity.off == interpolated.off && on_identity.pts != interpolated.pts;
            std::printf("dewarp_equal %s %d\nposes_matter %s %d\npoints %s %zu\n", tag.c_str(), equal ? 1 : 0, tag.c_str(), matter ? 1 : 0,
                        tag.c_str(), interpolated.fi.size());
            all = all && equal && matter;
            b2->interp_poses(x_known.front(), poses_known.front(), x_known.back(), poses_known.back());
            dump_poses(*b2, "p2");
            if (b2->poses_device() == nullptr || (b2->pose_rows_device() == nullptr) != f64) all = false;
            if (!f64) {
                std::vector<float> rows(static_cast<size_t>(n) * w * 12);
                b2->sync();
                if (hipMemcpy(rows.data(), b2->pose_rows_device(), rows.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
                    throw std::runtime_error("hipMemcpy(pose rows) failed");
                write_file(prefix + ".f32.rows2", rows.data(), rows.size() * 4);
            }
        }
        return all ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 2;
    }
}
