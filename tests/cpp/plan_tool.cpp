// plan_tool -- evaluates the decode launch plan (ouster_sdk_amd/csrc/decode_plan.cpp) on the CPU: no HIP library is linked.
// stdin: one PlanInput per line as `name=value` tokens (g.<field>=v, g.<bits>=mask,offset,shift, k.<knob>=v, the other
// PlanInput members by name, sel=<variant the tuner selected>).  stdout: the plan of each line as one JSON object.
// Driven by tests/test_decode_plan.py over tests/golden/decode_plans.json.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../../ouster_sdk_amd/csrc/decode_plan.h"

using namespace ouster_hip_dev;

namespace {
struct GU { const char* name; uint32_t Geometry::*m; };
struct GB { const char* name; ouster_hip_bits Geometry::*m; };
const GU g_uints[] = {{"pixels_per_column", &Geometry::pixels_per_column}, {"columns_per_packet", &Geometry::columns_per_packet},
                      {"columns_per_frame", &Geometry::columns_per_frame}, {"packet_header_size", &Geometry::packet_header_size},
                      {"col_header_size", &Geometry::col_header_size}, {"channel_data_size", &Geometry::channel_data_size},
                      {"col_footer_size", &Geometry::col_footer_size}, {"packet_footer_size", &Geometry::packet_footer_size},
                      {"col_size", &Geometry::col_size}, {"lidar_packet_size", &Geometry::lidar_packet_size}};
const GB g_bits[] = {{"col_timestamp", &Geometry::col_timestamp}, {"col_measurement_id", &Geometry::col_measurement_id},
                     {"col_status", &Geometry::col_status}, {"frame_id", &Geometry::frame_id}, {"alert_flags", &Geometry::alert_flags},
                     {"thermal_shutdown", &Geometry::thermal_shutdown}, {"shot_limiting", &Geometry::shot_limiting},
                     {"countdown_thermal_shutdown", &Geometry::countdown_thermal_shutdown},
                     {"countdown_shot_limiting", &Geometry::countdown_shot_limiting}};

bool set(PlanInput& in, int& sel, const std::string& name, const char* v) {
    const unsigned long long u = strtoull(v, nullptr, 0);
    if (name.rfind("g.", 0) == 0) {
        for (const GU& f : g_uints)
            if (name.substr(2) == f.name) { in.g.*f.m = (uint32_t)u; return true; }
        for (const GB& f : g_bits)
            if (name.substr(2) == f.name) {
                ouster_hip_bits b{};
                unsigned long long mask; unsigned offset; int shift;
                if (sscanf(v, "%llu,%u,%d", &mask, &offset, &shift) != 3) return false;
                b.mask = mask; b.offset = offset; b.shift = shift;
                in.g.*f.m = b;
                return true;
            }
        return false;
    }
    if (name.rfind("k.", 0) == 0) {
        const KnobDef* k = find_knob(name.c_str() + 2);
        if (k) in.kn.*k->member = atoi(v);
        return k != nullptr;
    }
    if (name == "n_frames") in.n_frames = (uint32_t)u;
    else if (name == "slots_per_frame") in.slots_per_frame = (uint32_t)u;
    else if (name == "packet_stride") in.packet_stride = (size_t)u;
    else if (name == "packets") in.packets = (uintptr_t)u;
    else if (name == "poses") in.xyz_poses = (uintptr_t)u;
    else if (name == "spec") in.spec = atoi(v);
    else if (name == "xyzm") in.xyzm = atoi(v);
    else if (name == "vec_ok") in.vec_ok = u != 0;
    else if (name == "n_fields") in.n_fields = (uint32_t)u;
    else if (name == "plane_mask") in.plane_mask = u;
    else if (name == "destagger_mask") in.destagger_mask = u;
    else if (name == "xyz_mask") in.xyz_mask = (uint32_t)u;
    else if (name == "gate") in.gate_counts = u != 0;
    else if (name == "cus") in.cus = (uint32_t)u;
    else if (name == "resident_wgs") in.resident_wgs = (uint32_t)u;
    else if (name == "may_resolve") in.may_resolve = u != 0;
    else if (name == "sel") sel = atoi(v);
    else return false;
    return true;
}

void shape(const char* name, const TileShape& s, bool with_small) {
    printf("\"%s\":[%u,%u,%u,%u", name, s.rows_per_tile, s.row_chunks, s.lds_col_slot, s.tiles_per_frame);
    if (with_small) printf(",%u", s.fix_rows_small);
    printf("],");
}
void field(const char* name, const FieldPlan& f) { printf("\"%s\":[%d,%d,%d,%u],", name, f.slot[0], f.slot[1], f.slot[2], (unsigned)f.sh); }
}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        PlanInput in{};
        int sel = -1;
        std::istringstream ss(line);
        std::string tok;
        while (ss >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos || !set(in, sel, tok.substr(0, eq), tok.c_str() + eq + 1)) {
                fprintf(stderr, "plan_tool: bad token '%s'\n", tok.c_str());
                return 2;
            }
        }
        const Candidates c = plan_candidates(in);
        // the tuner's part: a row recorded without a tunable choice carries sel = -1
        DecodePlan p = plan_decode(in, c, sel);
        const DecodePlan again = plan_decode(in, sel);   // the convenience form must agree
        if (memcmp(&p.shape, &again.shape, sizeof p.shape) || p.kernel != again.kernel || p.cols != again.cols) {
            fprintf(stderr, "plan_tool: plan_decode(in, sel) differs from plan_decode(in, candidates, sel)\n");
            return 3;
        }
        if (!p.ok) { printf("{\"ok\":0}\n"); continue; }
        const bool stream = p.kernel == Kernel::STREAM || p.kernel == Kernel::STREAM2;
        const int rows = stream ? (int)p.sa.tr : p.kernel == Kernel::DECODE ? (int)in.g.pixels_per_column : (int)p.shape.rows_per_tile;
        printf("{\"kernel\":\"%s\",\"cols\":%d,\"rows\":%d,\"narrow_tile\":%d,", kernel_name(p.kernel), p.cols, rows, p.narrow_tile);
        shape("shape", p.shape, false);
        printf("\"beam_lds\":%u,\"mode\":%u,\"xcd_map\":%u,\"slotmap\":%d,\"tunable\":%d,\"stream_auto\":%d,\"stream_alt\":%d,", p.beam_lds, p.mode,
               p.xcd_map, (int)p.slotmap, c.n > 0, c.stream_auto, c.stream_alt);
        printf("\"key\":\"%016" PRIx64 "\",\"candidates\":[", c.n ? tuner_key(in, c) : (uint64_t)0);
        for (int i = 0; i < c.n; ++i) printf(i ? ",%d" : "%d", c.variant[i]);
        // the recorded fix-up shape is that of a wide fix-up pass (zeros otherwise)
        const TileShape fix = p.fixup == Fixup::WIDE ? p.fix_shape : TileShape{};
        printf("],\"fixup\":%d,\"fix_wide\":%d,", p.fixup != Fixup::NONE, p.fix_cols);
        shape("fix_shape", fix, true);
        shape("fix_launch_shape", p.fix_shape, true);
        printf("\"fast_tiles\":%u,\"hdr_words_bytes\":%zu,\"slotmap_bytes\":%zu", p.fast_tiles, p.hdr_words_bytes, p.slotmap_bytes);
        if (stream) {
            const StreamArgs& a = p.sa;
            printf(",\"stream\":{\"tr\":%u,\"nch\":%u,\"ncell\":%u,\"npix_instr\":%u,\"hdr_off\":%u,\"pkt_off\":%u,\"off_off\":%u,\"beam_off\":%u,"
                   "\"ctx_bytes\":%u,\"fixed_off\":%u,\"n_hdr\":%u,\"n_pkt\":%u,", a.tr, a.nch, a.ncell, a.npix_instr, a.hdr_off, a.pkt_off,
                   a.off_off, a.beam_off, a.ctx_bytes, a.fixed_off, a.n_hdr, a.n_pkt);
            printf("\"hdr_dw\":[%u,%u,%u,%u,%u,%u,%u,%u],\"pkt_dw\":[%u,%u,%u,%u],", a.hdr_dw[0], a.hdr_dw[1], a.hdr_dw[2], a.hdr_dw[3], a.hdr_dw[4],
                   a.hdr_dw[5], a.hdr_dw[6], a.hdr_dw[7], a.pkt_dw[0], a.pkt_dw[1], a.pkt_dw[2], a.pkt_dw[3]);
            field("mid", a.mid); field("st", a.st); field("ts", a.ts); field("alert", a.alert);
            printf("\"groups\":%u,\"wait0\":%u,\"lds_bytes\":%u,\"order\":%u,\"loader\":%u}", a.groups, a.wait0, a.lds_bytes, a.order, a.loader);
        }
        printf("}\n");
    }
    return 0;
}
