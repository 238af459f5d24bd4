// frame_ops_batch_tool.cpp -- drives the frame_ops members of hip::DeviceFrameBatch for tests/test_gpu_frame_ops_batch.py (built
// by this directory's Makefile).
//   frame_ops_batch_tool <packets.bin> <h> <w> <n_frames> <masks.bin> <out_prefix> <clip_lo> <clip_hi> <key_lo> <key_hi>
//                        <gate_min_m> <gate_max_m> <z_lo> <z_hi>
//       packets.bin: [n_frames][w / 16][lidar_packet_size] bytes of RNG15_RFL8_NIR8_DUAL packets; masks.bin: u8 [2][h][w].
//       Two sensors (frame f -> sensor f % 2) that differ in their beam altitude angles, i.e. in their LUTs, and in their masks;
//       RANGE and REFLECTIVITY also destaggered, XYZ in double, the decode counting the dewarp gate.  After decode() and after
//       each of   clip({RANGE}) | filter_field(REFLECTIVITY -> all) | filter_uv v (all) + filter_uv u ({NEAR_IR}, invalid 5)
//                 | mask({RANGE2, REFLECTIVITY}) | filter_xyz(z, all)
//       everything the batch holds is written to <out_prefix>.s<k>: every staggered plane in the order printed ("plane NAME
//       ELEM"), the destaggered RANGE and REFLECTIVITY, the two clouds.  Then XYZLut(sensor)(filtered range) -- the C ABI's
//       ouster_hip_cartesian with the LUT the batch made -- is compared with the batch's clouds ("cartesian_equal 1"),
//       dewarp(gate) is run and its points / offsets written (<out_prefix>.dw, .dwoff), and the calls that must refuse are
//       tried ("refusals ok").
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <string>
#include <vector>

#include "batch_fixture.h"

using namespace fixture;

static bool refuses(const std::function<void()>& f) { return throws<std::invalid_argument>(f); }

int main(int argc, char** argv) {
    if (argc != 15) {
        std::printf("usage: frame_ops_batch_tool packets h w n masks prefix clip_lo clip_hi key_lo key_hi gate_min gate_max z_lo z_hi\n");
        return 64;
    }
    try {
        const uint32_t h = std::atoi(argv[2]), w = std::atoi(argv[3]), n = std::atoi(argv[4]);
        const std::string out = argv[6];
        const double clip_lo = std::atof(argv[7]), clip_hi = std::atof(argv[8]), key_lo = std::atof(argv[9]), key_hi = std::atof(argv[10]);
        const double gate_min = std::atof(argv[11]), gate_max = std::atof(argv[12]), z_lo = std::atof(argv[13]), z_hi = std::atof(argv[14]);
        // rows 1 and 2 carry their shifts wrapped by +w and -2w
        const std::vector<SensorInfo> sensors = {make_info(h, w, 0, true), make_info(h, w, 1, true)};
        oh::BatchOptions opt;
        opt.destagger = {"RANGE", "REFLECTIVITY"};
        opt.xyz = true;
        opt.xyz_f64 = true;
        opt.gate_min_range = gate_min;
        opt.gate_max_range = gate_max;
        opt.auto_placement = false;
        const auto batch = load_batch(sensors, n, opt, argv[1]);   // every packet, decoded
        oh::DeviceFrameBatch& b = *batch;
        const size_t npx = static_cast<size_t>(h) * w;
        std::vector<uint8_t> masks(2 * npx);
        {
            std::ifstream f(argv[5], std::ios::binary);
            f.read(reinterpret_cast<char*>(masks.data()), static_cast<std::streamsize>(masks.size()));
            if (!f) throw std::runtime_error("masks file too short");
        }
        std::vector<std::pair<std::string, size_t>> planes;
        for (const auto& ft : get_field_types(sensors[0])) {
            try {
                b.plane_device(ft.name);
            } catch (const std::out_of_range&) {
                continue;
            }
            planes.emplace_back(ft.name, b.plane_bytes_per_frame(ft.name));
            std::printf("plane %s %zu\n", ft.name.c_str(), planes.back().second / npx);
        }
        int stage = 0;
        auto dump = [&]() {
            b.sync();
            std::ofstream f(out + ".s" + std::to_string(stage++), std::ios::binary);
            std::vector<uint8_t> buf;
            auto put = [&](size_t bytes, const std::function<void(uint32_t, void*)>& get) {
                buf.resize(bytes);
                for (uint32_t fr = 0; fr < n; ++fr) {
                    get(fr, buf.data());
                    f.write(reinterpret_cast<const char*>(buf.data()), static_cast<std::streamsize>(bytes));
                }
            };
            for (const auto& p : planes) put(p.second, [&](uint32_t fr, void* d) { b.download_plane(p.first, fr, d); });
            for (const char* name : {"RANGE", "REFLECTIVITY"})
                put(b.plane_bytes_per_frame(name), [&](uint32_t fr, void* d) { b.download_plane(name, fr, d, true); });
            for (int k = 0; k < 2; ++k) put(b.xyz_bytes_per_frame(), [&](uint32_t fr, void* d) { b.download_xyz(k, fr, d); });
        };
        dump();
        b.clip({"RANGE"}, clip_lo, clip_hi);
        dump();
        b.filter_field("REFLECTIVITY", key_lo, key_hi);
        dump();
        b.filter_uv("v", w - w / 8, w);
        const std::vector<std::string> nir = {"NEAR_IR", "NOT_A_PLANE"};
        b.filter_uv("u", 1, 3, 5, &nir);
        dump();
        const std::vector<ImgRef<const uint8_t>> mrefs = {ImgRef<const uint8_t>(masks.data(), h, w),
                                                          ImgRef<const uint8_t>(masks.data() + npx, h, w)};
        b.mask({"RANGE2", "REFLECTIVITY"}, mrefs);
        dump();
        b.filter_xyz(2, z_lo, z_hi);
        dump();

        // the clouds are ouster_hip_cartesian of the filtered range planes with the sensors' LUTs
        bool equal = true;
        std::vector<XYZLut> luts = {XYZLut(sensors[0], opt.use_extrinsics), XYZLut(sensors[1], opt.use_extrinsics)};
        img_t<uint32_t> range(h, w);
        std::vector<double> cloud(npx * 3);
        for (int k = 0; k < 2; ++k)
            for (uint32_t fr = 0; fr < n; ++fr) {
                b.download_plane(k ? "RANGE2" : "RANGE", fr, range.data());
                b.download_xyz(k, fr, cloud.data());
                const auto want = luts[fr % 2](range);
                equal = equal && std::memcmp(want.data(), cloud.data(), npx * 24) == 0;
            }
        std::printf("cartesian_equal %d\n", equal ? 1 : 0);

        const uint64_t total = b.dewarp(gate_min, gate_max);
        std::vector<double> pts(total * 3);
        b.download_dewarped(pts.data(), nullptr, nullptr, nullptr);
        write_file(out + ".dw", pts.data(), pts.size() * 8);
        write_file(out + ".dwoff", b.dewarped_frame_offsets().data(), b.dewarped_frame_offsets().size() * 8);
        std::printf("dewarped %llu\n", static_cast<unsigned long long>(total));

        const std::vector<std::string> rng = {"RANGE"}, refl = {"REFLECTIVITY"};
        bool ok = refuses([&] { b.clip(rng, 0, 1, 7); });                       // invalid != 0 on a range plane with XYZ
        ok = refuses([&] { b.filter_uv("u", 0, 1, 3, nullptr); }) && ok;        // ... also when RANGE is one of "all"
        ok = refuses([&] { b.filter_xyz(0, 0, 1, 0, &refl, true); }) && ok;     // world_frame != BatchOptions::xyz_world_frame
        ok = refuses([&] { b.filter_xyz(3, 0, 1); }) && ok;
        ok = refuses([&] { b.mask(refl, {mrefs[0]}); }) && ok;                  // one mask for two sensors
        ok = refuses([&] { b.mask(refl, {mrefs[0], ImgRef<const uint8_t>(masks.data(), h, w - 1)}); }) && ok;
        ok = refuses([&] { b.filter_uv("x", 0, 1); }) && ok;
        ok = refuses([&] { b.filter_uv("u", 2, 1); }) && ok;
        ok = refuses([&] { b.filter_uv("v", 0, w + 1); }) && ok;
        ok = refuses([&] { b.clip(refl, 0, 1, 256); }) && ok;                   // does not fit u8
        std::printf(ok ? "refusals ok\n" : "refusals FAILED\n");
        dump();   // nothing a refused call touched
        return ok && equal ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 2;
    }
}
