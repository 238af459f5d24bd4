// voxel_lanes.cpp -- csrc/k_voxel.hip compiled for the CPU (tests/cpp/host_lanes: one thread per lane, rocPRIM's scan and radix sort
// replaced by stand-ins of the same calling convention) and run through the library's own voxel_run, the function
// ouster_hip_voxel_downsample calls: the reset, the order of the steps and the width of the sort are the library's.  Built and run
// by tests/test_voxel_lanes_cpu.py, which compares the result with tests/voxel_model.py bit for bit.
//   voxel_lanes <case file> <result file>
// case file: u32 n cols stride f32 form table_log2, f64 voxel_size, u64 min_pts capacity, points [n][stride] of f32 / f64
// [, normals f64 [n][3] when form == 3].  result file: u32 status n_vox, u64 n_out, out f64 [capacity][cols], out_normals f64
// [capacity][3], both filled with -7.25 before the run.
#include "../../ouster_sdk_amd/csrc/k_voxel.hip"

#include "host_lanes/lanes_util.h"

namespace ouster_hip_dev {
int fail_msg(int code, const char*) { return code; }
}  // namespace ouster_hip_dev
using namespace ouster_hip_dev;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    uint32_t hd[6];
    double voxel_size;
    uint64_t tail[2];
    if (!f || !rd(hd, sizeof hd, f) || !rd(&voxel_size, 8, f) || !rd(tail, 16, f)) return 2;
    const uint32_t n = hd[0], cols = hd[1], stride = hd[2], f32 = hd[3], form = hd[4], table_log2 = hd[5];
    const uint64_t min_pts = tail[0], cap = tail[1];
    if (n == 0 || stride < cols || cols < 3 || (1ull << table_log2) <= n) return 2;
    std::vector<uint8_t> pts((size_t)n * stride * (f32 ? 4 : 8));
    std::vector<double> nrm(form == VOXEL_FORM_NORMALS ? (size_t)n * 3 : 0);
    const bool ok = rd(pts.data(), pts.size(), f) && rd(nrm.data(), nrm.size() * 8, f);
    std::fclose(f);
    if (!ok) return 2;

    const bool folds = form == VOXEL_FORM_AVERAGE || form == VOXEL_FORM_NORMALS;
    // stale content everywhere the run is meant to write before it reads, the header and the table included: a refusal, and
    // every slot held by row 0 (a row index in range, so that a run without the reset is refused, not sent on a wild read)
    VoxelHeader hdr{VOXEL_STATUS_TABLE, 0xdeadbeefu, 0xdeadbeefdeadbeefull};
    std::vector<VoxelKey> keys(n, VoxelKey{9, 9, 9, 9});
    std::vector<int32_t> table((size_t)1 << table_log2, 0);
    std::vector<uint32_t> slot(n, 0xdeadbeefu), first(n, 7), first_id(n, 7), vid(n, 7), idx(n, 7), svid(n, 7), sidx(n, 7), seg_begin(n, 0xdeadbeefu),
        seg_end(n, 0xdeadbeefu), keep(n, 7), pos(n, 7);
    std::vector<double> rows(folds ? (size_t)n * (form == VOXEL_FORM_NORMALS ? 6 : cols) : 0, 1e300);
    std::vector<double> out((size_t)cap * cols, -7.25), out_n((size_t)cap * 3, -7.25);
    VoxelArgs a{};
    a.points = pts.data(), a.normals = nrm.empty() ? nullptr : nrm.data();
    a.stride = stride, a.n = n, a.cols = cols, a.f32 = (int32_t)f32, a.form = (int32_t)form;
    a.inv = 1.0 / voxel_size, a.min_pts = min_pts;
    a.hdr = &hdr, a.keys = keys.data(), a.table = table.data(), a.table_mask = (uint32_t)table.size() - 1;
    a.slot = slot.data(), a.first = first.data(), a.first_id = first_id.data();
    a.vid = vid.data(), a.idx = idx.data(), a.svid = svid.data(), a.sidx = sidx.data();
    a.seg_begin = seg_begin.data(), a.seg_end = seg_end.data(), a.rows = rows.data(), a.keep = keep.data(), a.pos = pos.data();
    a.out = out.data(), a.out_normals = out_n.data(), a.out_capacity = cap;

    size_t temp_bytes = 0;
    if (voxel_temp_bytes(n, &temp_bytes) != hipSuccess || temp_bytes == 0) return 3;
    std::vector<uint8_t> temp(temp_bytes);
    if (voxel_run(a, temp.data(), temp_bytes, nullptr) != hipSuccess) return 3;

    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    wr(&hdr, sizeof hdr, f);
    wr(out.data(), 8 * out.size(), f);
    wr(out_n.data(), 8 * out_n.size(), f);
    std::fclose(f);
    return 0;
}
