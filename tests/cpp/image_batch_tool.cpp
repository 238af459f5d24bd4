// image_batch_tool.cpp -- drives hip::DeviceFrameBatch::render_images for tests/test_gpu_image_processing.py and
// tools/ab/image_bench.py (built by this directory's Makefile).
//   image_batch_tool render <packets.bin> <h> <w> <n_frames> <n_sensors> <out_prefix>
//       packets.bin: [n_frames][w / 16][lidar_packet_size] bytes of RNG15_RFL8_NIR8_DUAL packets.  Decodes with NEAR_IR
//       destaggered, render_images("NEAR_IR") TWICE (update_state true, then false) and writes
//       <out_prefix>.planes (the destaggered planes as decoded), .images0 / .images1 (float), .state (per sensor: lo_state,
//       hi_state, then h dark counts, doubles) and prints the plane's element size.
//   image_batch_tool refuse <h> <w>     render_images on a plane that was not requested: prints "invalid_argument: ..."
//   image_batch_tool time <n_frames> <reps>   wall time of render_images("NEAR_IR") over 128 x 2048 frames, median of reps
//   image_batch_tool cpp_update         AutoExposure / BeamUniformityCorrector::update on a std::vector-backed image
//       against the same calls on an img_t (pool memory): prints "same" when every bit and the states agree
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <string>
#include <vector>

#include "batch_fixture.h"

using namespace fixture;

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    try {
        if (mode == "render" && argc == 8) {
            const uint32_t h = std::atoi(argv[3]), w = std::atoi(argv[4]), n = std::atoi(argv[5]), ns = std::atoi(argv[6]);
            const std::string out = argv[7];
            oh::BatchOptions opt;
            opt.destagger = {"NEAR_IR"};
            opt.auto_placement = false;
            const auto batch = load_batch(std::vector<SensorInfo>(ns, make_info(h, w, 0)), n, opt, argv[2]);
            oh::DeviceFrameBatch& b = *batch;
            b.sync();
            const size_t pb = b.plane_bytes_per_frame("NEAR_IR"), npx = static_cast<size_t>(h) * w;
            std::vector<uint8_t> planes(pb * n);
            for (uint32_t fr = 0; fr < n; ++fr) b.download_plane("NEAR_IR", fr, planes.data() + pb * fr, true);
            write_file(out + ".planes", planes.data(), planes.size());
            oh::ImagePipeline pipe(ns);
            std::vector<float> img(npx * n);
            for (int pass = 0; pass < 2; ++pass) {
                b.render_images("NEAR_IR", pipe, pass == 0);
                for (uint32_t fr = 0; fr < n; ++fr) b.download_image("NEAR_IR", fr, img.data() + npx * fr);
                write_file(out + (pass ? ".images1" : ".images0"), img.data(), img.size() * 4);
            }
            std::vector<double> st;
            for (uint32_t s = 0; s < ns; ++s) {
                st.push_back(pipe.auto_exposure[s].lo_state());
                st.push_back(pipe.auto_exposure[s].hi_state());
                const auto& d = pipe.beam_uniformity[s].dark_count();
                st.insert(st.end(), d.begin(), d.end());
            }
            write_file(out + ".state", st.data(), st.size() * 8);
            std::printf("elem %zu\n", pb / npx);
            return 0;
        }
        if (mode == "refuse" && argc == 4) {
            const SensorInfo info = make_info(std::atoi(argv[2]), std::atoi(argv[3]), 0);
            oh::BatchOptions opt;
            opt.destagger = {"RANGE"};
            opt.auto_placement = false;
            oh::DeviceFrameBatch b(info, 2, opt);
            oh::ImagePipeline pipe(1);
            try {
                b.render_images("NEAR_IR", pipe);
            } catch (const std::invalid_argument& e) {
                std::printf("invalid_argument: %s\n", e.what());
                return 0;
            }
            std::printf("no exception\n");
            return 1;
        }
        if (mode == "time" && argc == 4) {
            const uint32_t n = std::atoi(argv[2]);
            const int reps = std::atoi(argv[3]);
            const SensorInfo info = make_info(128, 2048, 0);
            auto pf = std::make_shared<PacketFormat>(info);
            oh::BatchOptions opt;
            opt.destagger = {"NEAR_IR"};
            opt.planes = {"NEAR_IR"};
            opt.auto_placement = false;
            oh::DeviceFrameBatch b(info, n, opt);
            std::mt19937 g(3);
            std::vector<std::vector<LidarPacket>> pool;
            for (int fi = 0; fi < 4; ++fi) {
                LidarFrame fr(info);
                Field& fld = fr.field("NEAR_IR");
                uint8_t* p = static_cast<uint8_t*>(fld.get());
                for (size_t i = 0; i < fld.size(); ++i) {
                    const uint64_t v = 20 + g() % 200;
                    std::memcpy(p + i * fld.element_size(), &v, fld.element_size());
                }
                for (size_t i = 0; i < fr.w; ++i) { fr.timestamp()[i] = 1000 + i; fr.measurement_id()[i] = i; fr.status()[i] = 1; }
                fr.frame_id = 700 + fi;
                pool.push_back(impl::frame_to_packets(fr, pf, 0, 0));
            }
            for (uint32_t fr = 0; fr < n; ++fr) {
                std::vector<const uint8_t*> ptrs;
                for (auto& p : pool[fr % pool.size()]) ptrs.push_back(p.buf.data());
                b.upload_frame_packets(fr, ptrs);
            }
            b.decode();
            b.sync();
            oh::ImagePipeline pipe(1);
            for (int i = 0; i < 3; ++i) b.render_images("NEAR_IR", pipe);
            std::vector<double> ms;
            for (int i = 0; i < reps; ++i) {
                const auto t0 = std::chrono::steady_clock::now();
                b.render_images("NEAR_IR", pipe);
                ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            }
            std::sort(ms.begin(), ms.end());
            std::printf("{\"render_images_ms_median\": %.4f, \"min\": %.4f, \"max\": %.4f, \"frames\": %u, \"reps\": %d}\n",
                        ms[ms.size() / 2], ms.front(), ms.back(), n, reps);
            return 0;
        }
        if (mode == "cpp_update") {
            const size_t h = 48, w = 320;
            std::mt19937 g(5);
            int bad = 0;
            image::BeamUniformityCorrector buc_a, buc_b;
            image::AutoExposure ae_a, ae_b;
            for (int call = 0; call < 10; ++call) {
                img_t<float> pool_img(h, w);
                std::vector<float> vec(h * w);
                for (size_t i = 0; i < h * w; ++i) vec[i] = pool_img.data()[i] = 50.0f + (g() % 1000) * 0.1f + (i / w) * 0.25f;
                const bool flag = call % 3 != 1;
                buc_a.update(pool_img, flag);
                ae_a.update(pool_img, flag);
                ImgRef<float> ref(vec.data(), h, w);
                buc_b.update(ref, flag);
                ae_b.update(ref, flag);
                bad += std::memcmp(vec.data(), pool_img.data(), h * w * 4) != 0;
                bad += ae_a.lo_state() != ae_b.lo_state() || ae_a.hi_state() != ae_b.hi_state() || buc_a.dark_count() != buc_b.dark_count();
                for (float v : vec) bad += !(v >= 0.f && v <= 1.f);
            }
            std::printf(bad ? "different\n" : "same\n");
            return bad ? 1 : 0;
        }
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 2;
    }
    std::printf("usage: image_batch_tool render|refuse|time|cpp_update ...\n");
    return 64;
}
