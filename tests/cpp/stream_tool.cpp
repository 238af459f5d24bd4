// stream_tool.cpp -- drives hip::FrameStream for tests/test_gpu_frame_stream.py (built by this directory's Makefile).
//   stream_tool <packets.bin> <scenario> <out_prefix>
//       packets.bin: [2 sensors][12 frames][8 packets][lidar_packet_size] bytes, written by tests/stream_cases.py; the sensors are
//       make_info(16, 128, variant, false, true) of batch_fixture.h.  The scenarios mirror stream_cases.SCENARIOS by name (and
//       "laps_<frames per batch>x<batches in flight>"); another name is refused.  Frame i of a scenario is frame i / sensors of
//       sensor i % sensors; frame 5 of either sensor is pushed without its packet 2.
//       For one scenario the FrameStream is built and fed; the callback appends what the BatchResult offers -- n_frames frames,
//       n_points points, never a buffer's capacity -- to
//         <prefix>.stream.plane.<NAME> / .dst.<NAME> / .xyz0 / .xyz1 / .timestamp / .measurement_id / .status
//         <prefix>.stream.offsets (frames_per_batch + 1 u64 per batch) / .points / .frame_idxs / .col_idxs / .timestamps_ns
//       and prints "batch <first_frame> <n_frames> <n_points> null=<the null pointers> maps=<keys of planes>|<keys of destaggered>"
//       per batch (every name followed by a comma), then "frames <pushed> <delivered>" and "one_shot <frames> <points>".
//       The same frames then go through ONE DeviceFrameBatch of all of them with the same BatchOptions (upload_frame_packets,
//       decode(), dewarp(min, max, provenance)), written as <prefix>.batch.* (offsets: frames + 1 u64).  For `packets` those
//       frames are the ones the host FrameBatcher released.
//   stream_tool <packets.bin> refusals <out_prefix>
//       builds the configurations the constructor must refuse and prints "refusal <name> 1|0" for each; pushes nothing.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "batch_fixture.h"
#include "ouster/hip/frame_stream.h"

using namespace fixture;
using Names = std::vector<std::string>;

constexpr uint32_t H = 16, W = 128, PPF = 8, N_FRAMES = 12;
constexpr uint32_t MISSING_FRAME = 5, MISSING_PACKET = 2, LOST_FRAME = 2, LOST_PACKET = 5;

struct Scenario {
    std::string name;
    uint32_t fpb, in_flight, n_frames;
    uint32_t sensors = 1;
    bool f64 = false, gated = true;
    double lo = 1.5, hi = 6.0;
    bool provenance = true, xyz = false;
    Names planes, destaggered, keep_planes;
    uint32_t finish_after = 0;
    bool by_packet = false;
};

static bool find_scenario(const std::string& name, Scenario& s) {
    auto base = [&](uint32_t fpb, uint32_t in_flight, uint32_t n) {
        s = Scenario();
        s.name = name, s.fpb = fpb, s.in_flight = in_flight, s.n_frames = n;
    };
    unsigned a = 0, b = 0;
    int used = 0;
    if (name == "laps") {
        base(2, 2, 11), s.xyz = true, s.planes = {"RANGE", "REFLECTIVITY2"}, s.destaggered = {"RANGE"};
    } else if (name == "one_in_flight") {
        base(3, 1, 7);
    } else if (name == "f64_three") {
        base(1, 3, 7), s.f64 = true, s.provenance = false, s.xyz = true;
    } else if (name == "two_sensors") {
        base(4, 2, 10), s.sensors = 2, s.planes = {"RANGE"};
    } else if (name == "at_capacity") {
        base(2, 2, 8), s.lo = 0.0, s.hi = 1e9;
    } else if (name == "nothing_kept") {
        base(3, 2, 8), s.lo = 50.0, s.hi = 60.0;
    } else if (name == "empty_gate") {
        base(2, 2, 5), s.lo = 0.0011, s.hi = 0.0019;
    } else if (name == "finish_midway") {
        base(4, 2, 9), s.finish_after = 3;
    } else if (name == "packets") {
        base(2, 2, 6), s.by_packet = true, s.planes = {"RANGE"};
    } else if (name == "dense_only") {
        base(4, 2, 6), s.gated = false, s.provenance = false, s.xyz = true, s.planes = {"RANGE", "REFLECTIVITY"},
            s.keep_planes = {"RANGE", "REFLECTIVITY"};
    } else if (name == "range_added") {
        base(2, 2, 11), s.planes = {"REFLECTIVITY"}, s.keep_planes = {"REFLECTIVITY"};
    } else if (std::sscanf(name.c_str(), "laps_%ux%u%n", &a, &b, &used) == 2 && static_cast<size_t>(used) == name.size() && a && b) {
        base(a, b, 11), s.planes = {"RANGE"};
    } else {
        return false;
    }
    return true;
}

// append-only files under one prefix, made when first named (a batch without points still leaves an empty file)
struct Sink {
    std::string prefix;
    std::map<std::string, std::ofstream> files;
    void put(const std::string& name, const void* p, size_t bytes) {
        auto it = files.find(name);
        if (it == files.end()) it = files.emplace(name, std::ofstream(prefix + "." + name, std::ios::binary | std::ios::trunc)).first;
        if (bytes) it->second.write(static_cast<const char*>(p), static_cast<std::streamsize>(bytes));
    }
};

static oh::StreamOptions stream_options(const Scenario& s) {
    oh::StreamOptions o;
    o.frames_per_batch = s.fpb;
    o.batches_in_flight = s.in_flight;
    o.outputs.planes = s.keep_planes;
    o.outputs.destagger = s.destaggered;
    o.outputs.xyz_f64 = s.f64;
    o.download_xyz = s.xyz;
    o.download_planes = s.planes;
    o.download_destaggered = s.destaggered;
    if (s.gated) {
        o.dewarp_min_range = s.lo;
        o.dewarp_max_range = s.hi;
        o.dewarp_provenance = s.provenance;
    }
    return o;
}

template <class F>
static bool refuses(const char* needle, F f) {
    try {
        f();
    } catch (const std::invalid_argument& e) {
        if (std::strstr(e.what(), needle)) return true;
        std::printf("refused without naming '%s': %s\n", needle, e.what());
    } catch (const std::exception& e) {
        std::printf("wrong exception: %s\n", e.what());
    }
    return false;
}

static int refusals(const std::vector<SensorInfo>& two) {
    const std::vector<SensorInfo> one = {two[0]};
    bool all = true;
    auto say = [&](const char* name, bool ok) {
        std::printf("refusal %s %d\n", name, ok ? 1 : 0);
        all = all && ok;
    };
    say("download_of_a_plane_not_kept", refuses("RANGE", [&] {   // no gate: nothing adds RANGE to the kept planes
        oh::StreamOptions o;
        o.frames_per_batch = 2, o.batches_in_flight = 2;
        o.outputs.planes = {"REFLECTIVITY"};
        o.download_planes = {"RANGE"};
        oh::FrameStream s(one, o, nullptr);
    }));
    say("download_of_a_destaggered_only_plane", refuses("REFLECTIVITY", [&] {
        oh::StreamOptions o;
        o.frames_per_batch = 2, o.batches_in_flight = 2;
        o.outputs.planes = {"RANGE"};
        o.outputs.destagger = {"REFLECTIVITY"};
        o.download_planes = {"REFLECTIVITY"};
        oh::FrameStream s(one, o, nullptr);
    }));
    say("no_sensors", refuses("no sensors", [&] {
        oh::StreamOptions o;
        oh::FrameStream s(std::vector<SensorInfo>{}, o, nullptr);
    }));
    say("frames_per_batch_not_a_multiple", refuses("multiple of the sensor count", [&] {
        oh::StreamOptions o;
        o.frames_per_batch = 3;
        oh::FrameStream s(two, o, nullptr);
    }));
    say("no_batches_in_flight", refuses("batches_in_flight", [&] {
        oh::StreamOptions o;
        o.frames_per_batch = 2, o.batches_in_flight = 0;
        oh::FrameStream s(one, o, nullptr);
    }));
    return all ? 0 : 1;
}

int main(int argc, char** argv) {
    if (argc != 4) {
        std::printf("usage: stream_tool packets.bin scenario out_prefix\n");
        return 64;
    }
    try {
        std::vector<SensorInfo> two = {make_info(H, W, 0, false, true), make_info(H, W, 1, false, true)};
        for (auto& info : two) info.init_id = 0x123456;   // the packets' (push_packet's FrameBatcher looks)
        const std::string scenario = argv[2], prefix = argv[3];
        if (scenario == "refusals") return refusals(two);
        Scenario sc;
        if (!find_scenario(scenario, sc)) {
            std::printf("error: unknown scenario '%s'\n", scenario.c_str());
            return 64;
        }
        const std::vector<SensorInfo> sensors(two.begin(), two.begin() + sc.sensors);
        const PacketFormat pf(two[0]);
        const size_t ps = pf.lidar_packet_size;
        std::vector<uint8_t> file(static_cast<size_t>(2) * N_FRAMES * PPF * ps);
        {
            std::ifstream f(argv[1], std::ios::binary);
            f.read(reinterpret_cast<char*>(file.data()), static_cast<std::streamsize>(file.size()));
            if (!f) throw std::runtime_error("packets file too short");
        }
        // the packets of every pushed frame, in push order
        std::vector<std::vector<const uint8_t*>> pushed;
        for (uint32_t i = 0; i < sc.n_frames; ++i) {
            const uint32_t s = i % sc.sensors, f = i / sc.sensors;
            std::vector<const uint8_t*> ptrs;
            for (uint32_t p = 0; p < PPF; ++p) {
                if (f == MISSING_FRAME && p == MISSING_PACKET) continue;
                if (sc.by_packet && f == LOST_FRAME && p == LOST_PACKET) continue;
                ptrs.push_back(file.data() + ((static_cast<size_t>(s) * N_FRAMES + f) * PPF + p) * ps);
            }
            pushed.push_back(std::move(ptrs));
        }
        std::vector<LidarPacket> sequence;   // push_packet: end to end, the last packet of frame 0 after the first of frame 1
        if (sc.by_packet) {
            for (const auto& fr : pushed)
                for (const uint8_t* p : fr) {
                    sequence.emplace_back(static_cast<int>(ps));
                    std::memcpy(sequence.back().buf.data(), p, ps);
                    sequence.back().host_timestamp = 77;
                }
            std::swap(sequence[PPF - 1], sequence[PPF]);
        }

        const oh::StreamOptions opt = stream_options(sc);
        const size_t npx = static_cast<size_t>(H) * W, pb = sc.f64 ? 24 : 12;
        Sink out{prefix + ".stream", {}};
        bool shape_ok = true;
        {
            oh::FrameStream stream(sensors, opt, [&](const oh::BatchResult& r) {
                shape_ok = shape_ok && r.h == H && r.w == W && r.n_frames >= 1 && r.n_frames <= sc.fpb;
                std::string nulls;
                auto seen = [&](const char* name, const void* p) {
                    if (!p) nulls += std::string(name) + ",";
                    return p != nullptr;
                };
                const size_t n = r.n_frames;
                for (int k = 0; k < 2; ++k)
                    if (seen(k ? "xyz1" : "xyz0", r.xyz[k])) out.put(k ? "xyz1" : "xyz0", r.xyz[k], n * npx * (pb));
                for (const auto& kv : r.planes) {
                    const size_t es = kv.first == "RANGE" || kv.first == "RANGE2" ? 4 : 1;   // the dual profile: 32-bit ranges, 8-bit rest
                    if (seen(("plane." + kv.first).c_str(), kv.second)) out.put("plane." + kv.first, kv.second, n * npx * es);
                }
                for (const auto& kv : r.destaggered) {
                    const size_t es = kv.first == "RANGE" || kv.first == "RANGE2" ? 4 : 1;
                    if (seen(("dst." + kv.first).c_str(), kv.second)) out.put("dst." + kv.first, kv.second, n * npx * es);
                }
                if (seen("timestamp", r.timestamp)) out.put("timestamp", r.timestamp, n * W * 8);
                if (seen("measurement_id", r.measurement_id)) out.put("measurement_id", r.measurement_id, n * W * 2);
                if (seen("status", r.status)) out.put("status", r.status, n * W * 4);
                if (seen("frame_offsets", r.frame_offsets)) out.put("offsets", r.frame_offsets, (static_cast<size_t>(sc.fpb) + 1) * 8);
                if (seen("points", r.points)) out.put("points", r.points, r.n_points * pb);
                if (seen("point_frame_idxs", r.point_frame_idxs)) out.put("frame_idxs", r.point_frame_idxs, r.n_points * 4);
                if (seen("point_col_idxs", r.point_col_idxs)) out.put("col_idxs", r.point_col_idxs, r.n_points * 4);
                if (seen("point_timestamps_ns", r.point_timestamps_ns)) out.put("timestamps_ns", r.point_timestamps_ns, r.n_points * 8);
                std::string listed;
                for (const auto& kv : r.planes) listed += kv.first + ",";
                listed += "|";
                for (const auto& kv : r.destaggered) listed += kv.first + ",";
                std::printf("batch %llu %u %llu null=%s maps=%s\n", static_cast<unsigned long long>(r.first_frame), r.n_frames,
                            static_cast<unsigned long long>(r.n_points), nulls.c_str(), listed.c_str());
            });
            if (sc.by_packet) {
                for (const auto& p : sequence) stream.push_packet(p);
            } else {
                for (uint32_t i = 0; i < sc.n_frames; ++i) {
                    stream.push_frame(pushed[i]);
                    if (sc.finish_after && i + 1 == sc.finish_after) stream.finish();
                }
            }
            stream.finish();
            std::printf("frames %llu %llu\n", static_cast<unsigned long long>(stream.frames_pushed()),
                        static_cast<unsigned long long>(stream.frames_delivered()));
        }
        out.files.clear();

        // the same frames through one batch of all of them
        std::vector<std::vector<std::vector<uint8_t>>> released;   // `packets`: what the host FrameBatcher hands over, copied
        if (sc.by_packet) {
            FrameBatcher fb(sensors[0]);
            LidarFrame lf(sensors[0]);
            fb.set_packet_sink([&](const std::vector<const uint8_t*>& packets) {
                released.emplace_back();
                for (const uint8_t* p : packets) released.back().emplace_back(p, p + ps);
            });
            for (const auto& p : sequence) (void)fb.batch(p, lf);
            pushed.clear();
            for (const auto& fr : released) {
                pushed.emplace_back();
                for (const auto& p : fr) pushed.back().push_back(p.data());
            }
        }
        const uint32_t n = static_cast<uint32_t>(pushed.size());
        oh::BatchOptions bo = opt.outputs;
        bo.xyz = sc.xyz || sc.gated;
        if (sc.gated) {
            bo.gate_min_range = sc.lo;
            bo.gate_max_range = sc.hi;
            if (!bo.planes.empty() && std::find(bo.planes.begin(), bo.planes.end(), "RANGE") == bo.planes.end()) bo.planes.push_back("RANGE");
        }
        oh::DeviceFrameBatch batch(sensors, n, bo);
        for (uint32_t f = 0; f < n; ++f) batch.upload_frame_packets(f, pushed[f]);
        batch.decode();
        const std::string bp = prefix + ".batch.";
        for (const auto& name : sc.planes)
            write_frames(bp + "plane." + name, n, batch.plane_bytes_per_frame(name), [&](uint32_t f, double* p) { batch.download_plane(name, f, p); });
        for (const auto& name : sc.destaggered)
            write_frames(bp + "dst." + name, n, batch.plane_bytes_per_frame(name), [&](uint32_t f, double* p) { batch.download_plane(name, f, p, true); });
        if (sc.xyz)
            for (int k = 0; k < 2; ++k)
                write_frames(bp + (k ? "xyz1" : "xyz0"), n, npx * pb, [&](uint32_t f, double* p) { batch.download_xyz(k, f, p); });
        write_frames(bp + "timestamp", n, W * 8, [&](uint32_t f, double* p) { batch.download_headers(f, reinterpret_cast<uint64_t*>(p), nullptr, nullptr); });
        write_frames(bp + "measurement_id", n, W * 2, [&](uint32_t f, double* p) { batch.download_headers(f, nullptr, reinterpret_cast<uint16_t*>(p), nullptr); });
        write_frames(bp + "status", n, W * 4, [&](uint32_t f, double* p) { batch.download_headers(f, nullptr, nullptr, reinterpret_cast<uint32_t*>(p)); });
        if (sc.gated) {
            const uint64_t total = batch.dewarp(sc.lo, sc.hi, sc.provenance);
            std::vector<uint8_t> pts(total * pb);
            std::vector<uint32_t> fi(sc.provenance ? total : 0), ci(fi.size());
            std::vector<uint64_t> ts(fi.size());
            batch.download_dewarped(pts.data(), sc.provenance ? fi.data() : nullptr, sc.provenance ? ci.data() : nullptr,
                                    sc.provenance ? ts.data() : nullptr);
            const auto& off = batch.dewarped_frame_offsets();
            write_file(bp + "offsets", off.data(), off.size() * 8);
            write_file(bp + "points", pts.data(), pts.size());
            if (sc.provenance) {
                write_file(bp + "frame_idxs", fi.data(), fi.size() * 4);
                write_file(bp + "col_idxs", ci.data(), ci.size() * 4);
                write_file(bp + "timestamps_ns", ts.data(), ts.size() * 8);
            }
            std::printf("one_shot %u %llu\n", n, static_cast<unsigned long long>(total));
        } else {
            std::printf("one_shot %u 0\n", n);
        }
        return shape_ok ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 2;
    }
}
