// ring_tool -- plan_stream (ouster_sdk_amd/csrc/decode_plan.cpp) on the CPU: the persistent kernel's tile ring as the plan lays it
// out.  stdin: plan_tool's `name=value` lines (its parser is used as it is) plus tw=<tile width> and host_ts=<0|1>; stdout: one JSON
// object per line, the StreamArgs of plan_stream(in, tw) or {"ok":0} where it refuses.  Driven by tests/test_decode_plan_ring_cpu.py.
#define main plan_tool_main
#include "plan_tool.cpp"
#undef main

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        PlanInput in{};
        int sel = -1, tw = 0;
        std::istringstream ss(line);
        std::string tok;
        while (ss >> tok) {
            const size_t eq = tok.find('=');
            const std::string name = eq == std::string::npos ? tok : tok.substr(0, eq);
            const char* v = eq == std::string::npos ? "" : tok.c_str() + eq + 1;
            if (name == "tw") tw = atoi(v);
            else if (name == "host_ts") in.host_ts = atoi(v) != 0;
            else if (eq == std::string::npos || !set(in, sel, name, v)) {
                fprintf(stderr, "ring_tool: bad token '%s'\n", tok.c_str());
                return 2;
            }
        }
        const auto p = plan_stream(in, tw);
        if (!p) { printf("{\"ok\":0}\n"); continue; }
        const StreamArgs& a = p->sa;
        printf("{\"ok\":1,\"tr\":%u,\"nch\":%u,\"ncell\":%u,\"npix_instr\":%u,\"hdr_off\":%u,\"pkt_off\":%u,\"off_off\":%u,\"beam_off\":%u,"
               "\"ctx_bytes\":%u,\"fixed_off\":%u,\"n_hdr\":%u,\"n_pkt\":%u,", a.tr, a.nch, a.ncell, a.npix_instr, a.hdr_off, a.pkt_off,
               a.off_off, a.beam_off, a.ctx_bytes, a.fixed_off, a.n_hdr, a.n_pkt);
        printf("\"hdr_dw\":[%u,%u,%u,%u,%u,%u,%u,%u],\"pkt_dw\":[%u,%u,%u,%u],", a.hdr_dw[0], a.hdr_dw[1], a.hdr_dw[2], a.hdr_dw[3], a.hdr_dw[4],
               a.hdr_dw[5], a.hdr_dw[6], a.hdr_dw[7], a.pkt_dw[0], a.pkt_dw[1], a.pkt_dw[2], a.pkt_dw[3]);
        field("mid", a.mid); field("st", a.st); field("ts", a.ts); field("alert", a.alert);
        printf("\"groups\":%u,\"wait0\":%u,\"lds_bytes\":%u,\"order\":%u,\"loader\":%u,\"nslot\":%u,\"dma_per_tile\":[%u,%u,%u,%u],", a.groups, a.wait0,
               a.lds_bytes, a.order, a.loader, a.nslot, a.dma_per_tile[0], a.dma_per_tile[1], a.dma_per_tile[2], a.dma_per_tile[3]);
        printf("\"key\":\"%016" PRIx64 "\"}\n", tuner_key(in, plan_candidates(in)));
    }
    return 0;
}
