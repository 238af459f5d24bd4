// icp_lanes.cpp -- the grid of csrc/k_icp.hip, through the library's own icp_grid_run (and with it voxel_group_run of
// csrc/k_voxel.hip), and k_icp_correspond, compiled for the CPU (tests/cpp/host_lanes: one thread per lane, rocPRIM's scan and radix
// sort replaced by stand-ins of the same calling convention) and driven the way ouster_hip_icp_step drives them.  The sum kernels
// use cross-lane operations and are covered on the GPU only (tests/test_gpu_icp.py).  Built and run by tests/test_icp_lanes_cpu.py,
// which compares the result with tests/icp_model.py bit for bit.
//   icp_lanes <case file> <result file>
// case file: u32 n_src n_tgt src_stride tgt_stride src_n_stride tgt_n_stride f32 plane table_log2 pad, f64 max_corr_dist cos_gate
// pose[16], then source, target [, source normals, target normals] rows of f32 / f64.  result file: u32 status, u32 cells, then
// nn i32 [n_src + 16] and r f64 [n_src + 16], both filled with guard values (-77, -7.25) before the run.
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
    uint32_t hd[10];
    double par[18];
    if (!f || !rd(hd, sizeof hd, f) || !rd(par, sizeof par, f)) return 2;
    const uint32_t n_src = hd[0], n_tgt = hd[1], f32 = hd[6], plane = hd[7], table_log2 = hd[8];
    if (n_src == 0 || n_tgt == 0 || (1ull << table_log2) <= n_tgt) return 2;
    const size_t es = f32 ? 4 : 8;
    std::vector<uint8_t> src((size_t)n_src * hd[2] * es), tgt((size_t)n_tgt * hd[3] * es), src_n(plane ? (size_t)n_src * hd[4] * es : 0),
        tgt_n(plane ? (size_t)n_tgt * hd[5] * es : 0);
    const bool ok = rd(src.data(), src.size(), f) && rd(tgt.data(), tgt.size(), f) && rd(src_n.data(), src_n.size(), f) &&
                    rd(tgt_n.data(), tgt_n.size(), f);
    std::fclose(f);
    if (!ok) return 2;

    // stale content everywhere the run is meant to write before it reads, the read-back and the table included: refusals, and
    // every slot held by row 0 (a row index in range, so that a run without the reset is refused, not sent on a wild read)
    IcpReadback rb;
    std::memset(&rb, 0x5a, sizeof rb);
    const size_t slots = (size_t)1 << table_log2;
    std::vector<VoxelKey> keys(n_tgt, VoxelKey{9, 9, 9, 9});
    std::vector<int32_t> table(slots, 0);
    std::vector<uint32_t> slot(n_tgt, 0xdeadbeefu), first(n_tgt, 7), first_id(n_tgt, 7), vid(n_tgt, 7), idx(n_tgt, 7), svid(n_tgt, 7), sidx(n_tgt, 7),
        seg_begin(n_tgt, 0xdeadbeefu), seg_end(n_tgt, 0xdeadbeefu), slot_end(slots, 0xdeadbeefu), flag(n_src, 7);
    std::vector<IcpSlot> islots(slots, IcpSlot{9, 9, 9, 9});
    std::vector<double> rows((size_t)n_tgt * (plane ? 6 : 3), 1e300), xq((size_t)n_src * 6, 1e300), r(n_src + 16, -7.25);
    std::vector<int32_t> nn(n_src + 16, -77);
    std::vector<uint64_t> key(n_src, 5);

    IcpArgs a{};
    a.src = src.data(), a.tgt = tgt.data(), a.src_n = plane ? src_n.data() : nullptr, a.tgt_n = plane ? tgt_n.data() : nullptr;
    a.src_stride = hd[2], a.tgt_stride = hd[3], a.src_n_stride = hd[4], a.tgt_n_stride = hd[5];
    a.n_src = n_src, a.n_tgt = n_tgt, a.f32 = (int32_t)f32, a.plane = (int32_t)plane;
    a.max_corr_dist = par[0], a.inv = 1.0 / par[0], a.max_d2 = par[0] * par[0], a.cos_gate = par[1];
    std::memcpy(a.pose, par + 2, sizeof a.pose);
    a.rb = &rb, a.keys = keys.data(), a.table = table.data(), a.table_mask = (uint32_t)slots - 1;
    a.first_id = first_id.data(), a.svid = svid.data(), a.sidx = sidx.data(), a.seg_begin = seg_begin.data(), a.seg_end = seg_end.data();
    a.slots = islots.data(), a.slot_end = slot_end.data(), a.rows = rows.data();
    a.nn = nn.data(), a.r = r.data(), a.key = key.data(), a.flag = flag.data(), a.xq = xq.data();
    VoxelArgs v{};
    v.n = n_tgt, v.hdr = &rb.grid, v.keys = a.keys, v.table = a.table, v.table_mask = a.table_mask;
    v.slot = slot.data(), v.first = first.data(), v.first_id = a.first_id, v.vid = vid.data(), v.idx = idx.data();
    v.svid = a.svid, v.sidx = a.sidx, v.seg_begin = a.seg_begin, v.seg_end = a.seg_end;

    size_t temp_bytes = 0;
    if (voxel_temp_bytes(n_tgt, &temp_bytes) != hipSuccess || temp_bytes == 0) return 3;
    std::vector<uint8_t> temp(temp_bytes);
    if (icp_grid_run(a, v, temp.data(), temp_bytes, nullptr) != hipSuccess) return 3;
    // like the library, only a clean grid is queried (a refused row would merely be absent from it)
    if (!rb.pass.status && !rb.grid.status) {
        // the device code writes nn / r to the workspace and copies n_src elements out; here they are the outputs themselves
        if (launch_icp_correspond(a, nullptr) != hipSuccess) return 3;
        for (uint32_t i = 0; i < n_src; ++i)
            if (flag[i] != (nn[i] >= 0) || (key[i] == ICP_NO_KEY) != (nn[i] < 0)) return 4;
    }

    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    const uint32_t head[2] = {rb.pass.status | (rb.grid.status << 8), rb.grid.n_vox};
    wr(head, sizeof head, f);
    wr(nn.data(), 4 * nn.size(), f);
    wr(r.data(), 8 * r.size(), f);
    std::fclose(f);
    return 0;
}
