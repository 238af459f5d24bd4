// icp_target_lanes.cpp -- k_icp_correspond_many of csrc/k_icp.hip compiled for the CPU (tests/cpp/host_lanes/hip/hip_runtime.h: one
// thread per lane), over a grid built by the library's own icp_grid_run the way icp_lanes.cpp builds it, a source table and the
// chunk table of csrc/host/icp_util.cpp: several sources against one target in ONE launch, a workgroup per chunk.  Built and run by
// tests/test_icp_target_lanes_cpu.py, which compares every source's rows with tests/icp_model.py bit for bit.
//   icp_target_lanes <case file> <result file>
// case file: u32 n_sources n_tgt tgt_stride tgt_n_stride tgt_f32 src_f32 plane table_log2, f64 max_corr_dist cos_gate, the target
// rows [, normals]; then per source u32 n stride n_stride active, f64 pose[16], its rows [, normals].
// result file: u32 status, u32 chunks, then nn i32 [rows + 16] and r f64 [rows + 16] of the concatenated sources, both filled with
// guard values (-77, -7.25) before the launch: an inactive source's rows must still hold them afterwards.
#include "../../ouster_sdk_amd/csrc/k_voxel.hip"
#include "../../ouster_sdk_amd/csrc/k_icp.hip"

#include "host_lanes/lanes_util.h"

namespace ouster_hip_dev {
int fail_msg(int code, const char*) { return code; }
}  // namespace ouster_hip_dev
using namespace ouster_hip_dev;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    uint32_t hd[8];
    double par[2];
    if (!f || !rd(hd, sizeof hd, f) || !rd(par, sizeof par, f)) return 2;
    const uint32_t n_sources = hd[0], n_tgt = hd[1], plane = hd[6], table_log2 = hd[7];
    if (n_sources == 0 || n_tgt == 0 || (1ull << table_log2) <= n_tgt) return 2;
    const size_t tes = hd[4] ? 4 : 8, ses = hd[5] ? 4 : 8;
    std::vector<uint8_t> tgt((size_t)n_tgt * hd[2] * tes), tgt_n(plane ? (size_t)n_tgt * hd[3] * tes : 0);
    if (!rd(tgt.data(), tgt.size(), f) || !rd(tgt_n.data(), tgt_n.size(), f)) return 2;
    std::vector<std::vector<uint8_t>> src(n_sources), src_n(n_sources);
    std::vector<IcpSource> sources(n_sources);
    std::vector<uint64_t> rows(n_sources), first_row(n_sources), first_chunk(n_sources);
    for (uint32_t k = 0; k < n_sources; ++k) {
        uint32_t sh[4];
        IcpSource& s = sources[k];
        if (!rd(sh, sizeof sh, f) || !rd(s.pose, sizeof s.pose, f)) return 2;
        src[k].resize((size_t)sh[0] * sh[1] * ses), src_n[k].resize(plane ? (size_t)sh[0] * sh[2] * ses : 0);
        if (!rd(src[k].data(), src[k].size(), f) || !rd(src_n[k].data(), src_n[k].size(), f)) return 2;
        s.src = src[k].data(), s.src_n = plane ? src_n[k].data() : nullptr, s.src_stride = sh[1], s.src_n_stride = sh[2];
        s.n = sh[0], s.active = (int32_t)sh[3];
        rows[k] = sh[0];
    }
    std::fclose(f);

    // the grid, as icp_lanes.cpp builds it: the library's icp_grid_run over a workspace full of stale content
    IcpReadback rb;
    std::memset(&rb, 0x5a, sizeof rb);
    const size_t slots = (size_t)1 << table_log2;
    std::vector<VoxelKey> keys(n_tgt, VoxelKey{9, 9, 9, 9});
    std::vector<int32_t> table(slots, 0);   // every slot held by row 0
    std::vector<uint32_t> slot(n_tgt, 0xdeadbeefu), first(n_tgt, 7), first_id(n_tgt, 7), vid(n_tgt, 7), idx(n_tgt, 7), svid(n_tgt, 7), sidx(n_tgt, 7),
        seg_begin(n_tgt, 0xdeadbeefu), seg_end(n_tgt, 0xdeadbeefu), slot_end(slots, 0xdeadbeefu);
    std::vector<IcpSlot> islots(slots, IcpSlot{9, 9, 9, 9});
    std::vector<double> trows((size_t)n_tgt * (plane ? 6 : 3), 1e300);
    IcpArgs a{};
    a.tgt = tgt.data(), a.tgt_n = plane ? tgt_n.data() : nullptr, a.tgt_stride = hd[2], a.tgt_n_stride = hd[3];
    a.n_tgt = n_tgt, a.f32 = (int32_t)hd[4], a.plane = (int32_t)plane;
    a.max_corr_dist = par[0], a.inv = 1.0 / par[0], a.max_d2 = par[0] * par[0], a.cos_gate = par[1];
    a.rb = &rb, a.keys = keys.data(), a.table = table.data(), a.table_mask = (uint32_t)slots - 1;
    a.first_id = first_id.data(), a.svid = svid.data(), a.sidx = sidx.data(), a.seg_begin = seg_begin.data(), a.seg_end = seg_end.data();
    a.slots = islots.data(), a.slot_end = slot_end.data(), a.rows = trows.data();
    VoxelArgs v{};
    v.n = n_tgt, v.hdr = &rb.grid, v.keys = a.keys, v.table = a.table, v.table_mask = a.table_mask;
    v.slot = slot.data(), v.first = first.data(), v.first_id = a.first_id, v.vid = vid.data(), v.idx = idx.data();
    v.svid = a.svid, v.sidx = a.sidx, v.seg_begin = a.seg_begin, v.seg_end = a.seg_end;
    size_t temp_bytes = 0;
    if (voxel_temp_bytes(n_tgt, &temp_bytes) != hipSuccess || temp_bytes == 0) return 3;
    std::vector<uint8_t> temp(temp_bytes);
    if (icp_grid_run(a, v, temp.data(), temp_bytes, nullptr) != hipSuccess) return 3;

    // the two tables of the many-source route, by the library's builder
    const uint64_t n_chunks = icp_chunk_table(rows.data(), n_sources, nullptr, 0, first_row.data(), first_chunk.data());
    std::vector<IcpChunk> chunks(n_chunks);
    icp_chunk_table(rows.data(), n_sources, chunks.data(), n_chunks, nullptr, nullptr);
    const size_t n_rows = (size_t)(first_row[n_sources - 1] + rows[n_sources - 1]);
    for (uint32_t k = 0; k < n_sources; ++k) {
        sources[k].first = (uint32_t)first_row[k], sources[k].first_chunk = (uint32_t)first_chunk[k];
        sources[k].chunks = icp_chunks(sources[k].n);
    }
    std::vector<int32_t> nn(n_rows + 16, -77);
    std::vector<double> r(n_rows + 16, -7.25), xq(n_rows * 6, 1e300);
    std::vector<uint64_t> key(n_rows, 5);
    std::vector<uint32_t> flag(n_rows, 7);
    IcpManyArgs m{};
    m.q = icp_query(a);
    m.q.nn = nn.data(), m.q.r = r.data(), m.q.key = key.data(), m.q.flag = flag.data(), m.q.xq = xq.data();
    m.sources = sources.data(), m.chunks = chunks.data();
    m.n_sources = n_sources, m.n_chunks = (uint32_t)n_chunks, m.n_rows = (uint32_t)n_rows;
    m.f32 = (int32_t)hd[5], m.max_corr_dist = par[0];
    if (!rb.pass.status && !rb.grid.status) {
        if (launch_icp_correspond_many(m, nullptr) != hipSuccess) return 3;
        for (uint32_t k = 0; k < n_sources; ++k)
            for (uint32_t i = sources[k].first; i < sources[k].first + sources[k].n; ++i)
                if (sources[k].active ? (flag[i] != (nn[i] >= 0) || (key[i] == ICP_NO_KEY) != (nn[i] < 0)) : (flag[i] != 7 || key[i] != 5)) return 4;
    }

    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    const uint32_t head[2] = {rb.pass.status | (rb.grid.status << 8), (uint32_t)n_chunks};
    std::fwrite(head, sizeof head, 1, f);
    std::fwrite(nn.data(), 4, nn.size(), f);
    std::fwrite(r.data(), 8, r.size(), f);
    std::fclose(f);
    return 0;
}
