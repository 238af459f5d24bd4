// voxel_map_lanes.cpp -- csrc/k_voxel_map.hip compiled for the CPU (tests/cpp/host_lanes: one thread per lane, rocPRIM's scan and
// radix sort replaced by stand-ins of the same calling convention) and run through the library's own vmap_add_prepare,
// vmap_add_commit, vmap_far_prepare, vmap_far_commit, vmap_rebuild, vmap_cloud and vmap_closest in the order capi_voxel_map.hip
// calls them, over the call-local grid of k_voxel.hip's voxel_group_run.  Built and run by tests/test_voxel_map_lanes_cpu.py, which
// compares every output with tests/voxel_map_model.py bit for bit.
//   voxel_map_lanes <case file> <result file>
// case file: u32 n_calls P n_queries cap, f64 voxel_size max_distance bound_sq origin[3]; per call u32 n, pad, f64 rows [n][3]; f64
// queries [n_queries][3].  The map has room for `cap` voxels and 2 * cap slots (a power of two) from the start: it never grows.
// result file: u32 status voxels points kept, f64 cloud [points][3] after the last add, then (after removal at `origin`) u32
// evicted_rows pad, f64 extracted [evicted_rows][3], f64 cloud [points - evicted_rows][3], f64 nn [n_queries][3], f64 d2 [n_queries].
#include "../../ouster_sdk_amd/csrc/k_voxel.hip"
#include "../../ouster_sdk_amd/csrc/k_voxel_map.hip"

#include "host_lanes/lanes_util.h"

#include <cstdlib>

using namespace ouster_hip_dev;

// what an earlier call left in a header: every field set
static VMapHeader stale_header() {
    VMapHeader h;
    std::memset(&h, 0x5a, sizeof h);
    return h;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    uint32_t hd[4];
    double par[6];
    if (!f || !rd(hd, sizeof hd, f) || !rd(par, sizeof par, f)) return 2;
    const uint32_t n_calls = hd[0], P = hd[1], nq = hd[2], cap = hd[3];
    uint32_t slots = 2;
    while (slots < 2 * cap) slots <<= 1;
    // the map's arrays, both sets
    std::vector<VoxelKey> cell[2] = {std::vector<VoxelKey>(cap), std::vector<VoxelKey>(cap)};
    std::vector<uint32_t> count[2] = {std::vector<uint32_t>(cap), std::vector<uint32_t>(cap)};
    std::vector<double> pts[2] = {std::vector<double>((size_t)cap * P * 3), std::vector<double>((size_t)cap * P * 3)};
    std::vector<int32_t> table(slots, 0);   // stale: every slot claims voxel 0 until the library resets the table
    VMapDev m;
    m.s = VMapSet{cell[0].data(), count[0].data(), pts[0].data()};
    m.table = table.data(), m.table_mask = slots - 1, m.cap = cap, m.P = P;
    m.voxel_size = par[0], m.inv = 1.0 / par[0], m.resolution_sq = par[0] * par[0] / (double)P;
    VMapHeader mh{};
    if (vmap_rebuild(m, &mh, nullptr) != hipSuccess) return 3;   // an empty map: the table reset alone, as at creation
    uint64_t points = 0;
    for (uint32_t c = 0; c < n_calls; ++c) {
        uint32_t nh[2];
        if (!rd(nh, sizeof nh, f)) return 2;
        const uint32_t n = nh[0];
        std::vector<double> rows((size_t)n * 3);
        if (!rd(rows.data(), rows.size() * 8, f)) return 2;
        if (n == 0) continue;
        // the call-local grid, as capi_voxel_map.hip lays it out
        VoxelArgs a{};
        a.points = rows.data(), a.stride = 3, a.n = n, a.cols = 3, a.form = VOXEL_FORM_FIRST, a.inv = m.inv;
        uint32_t log2 = 1;
        while ((1ull << log2) < 2ull * n) ++log2;
        a.table_mask = (uint32_t)((1ull << log2) - 1);
        // stale content in both headers and the call-local table (every slot held by row 0, a row index in range: without the
        // reset a refusal, not a wild read) and everywhere else the run writes before it reads
        VoxelHeader vh{VOXEL_STATUS_TABLE, 0xdeadbeefu, 0xdeadbeefdeadbeefull};
        mh = stale_header();
        std::vector<VoxelKey> keys(n, VoxelKey{9, 9, 9, 9});
        std::vector<int32_t> local((size_t)a.table_mask + 1, 0);
        std::vector<uint32_t> slot(n, 7), first(n, 7), first_id(n, 7), vid(n, 7), idx(n, 7), svid(n, 7), sidx(n, 7), seg_begin(n, 7), seg_end(n, 7),
            found(n, 7), is_new(n, 7), new_pos(n, 7);
        a.hdr = &vh, a.keys = keys.data(), a.table = local.data(), a.slot = slot.data(), a.first = first.data(), a.first_id = first_id.data();
        a.vid = vid.data(), a.idx = idx.data(), a.svid = svid.data(), a.sidx = sidx.data(), a.seg_begin = seg_begin.data(), a.seg_end = seg_end.data();
        VMapAddArgs x{&mh, found.data(), is_new.data(), new_pos.data()};
        size_t temp_bytes = 0;
        if (voxel_temp_bytes(n, &temp_bytes) != hipSuccess || temp_bytes == 0) return 3;
        std::vector<uint8_t> temp(temp_bytes);
        if (vmap_add_prepare(a, m, x, temp.data(), temp_bytes, nullptr) != hipSuccess) return 3;
        if (vh.status || m.n_vox + mh.n_new > cap) return 4;
        if (vmap_add_commit(a, m, x, nullptr) != hipSuccess) return 3;
        m.n_vox += mh.n_new, points += mh.n_admitted;
        if (mh.status) return 5;
    }
    std::vector<double> queries((size_t)nq * 3);
    if (!rd(queries.data(), queries.size() * 8, f)) return 2;
    std::fclose(f);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    auto cloud = [&](uint64_t rows) {
        std::vector<uint32_t> pos(m.n_vox + 1, 7);
        std::vector<double> out(rows * 3 + 3, -7.25);
        size_t temp_bytes = 0;
        if (vmap_temp_bytes(m.n_vox, &temp_bytes) != hipSuccess || temp_bytes == 0) std::exit(3);
        std::vector<uint8_t> temp(temp_bytes);
        if (vmap_cloud(m, pos.data(), out.data(), temp.data(), temp_bytes, nullptr) != hipSuccess) std::exit(3);
        if (out[rows * 3] != -7.25) std::printf("cloud: written behind its rows\n");
        wr(out.data(), rows * 24, o);
    };
    const uint32_t before[4] = {mh.status, m.n_vox, (uint32_t)points, 0};
    // removal at `origin`
    int32_t origin[3];
    for (int k = 0; k < 3; ++k) origin[k] = (int32_t)std::floor(par[3 + k] * m.inv);
    std::vector<uint32_t> keep(m.n_vox + 1, 7), keep_pos(m.n_vox + 1, 7), gone(m.n_vox + 1, 7), gone_pos(m.n_vox + 1, 7);
    VMapFarArgs far{};
    far.hdr = &mh, far.keep = keep.data(), far.keep_pos = keep_pos.data(), far.gone = gone.data(), far.gone_pos = gone_pos.data();
    std::memcpy(far.origin, origin, sizeof origin);
    far.max_voxel_dist = (int64_t)std::ceil(par[1] * m.inv) + 1;
    mh = m.n_vox ? stale_header() : VMapHeader{};   // an empty map has nothing to remove and no step that would reset the header
    uint32_t kept = m.n_vox;
    std::vector<double> extracted;
    if (m.n_vox) {
        size_t temp_bytes = 0;
        if (vmap_temp_bytes(m.n_vox, &temp_bytes) != hipSuccess || temp_bytes == 0) return 3;
        std::vector<uint8_t> temp(temp_bytes);
        if (vmap_far_prepare(m, far, temp.data(), temp_bytes, nullptr) != hipSuccess) return 3;
        kept = mh.n_keep;
        extracted.assign((size_t)mh.n_evicted * 3 + 3, -7.25);
        far.out = extracted.data();
    }
    const uint32_t head[4] = {before[0], before[1], before[2], kept};
    wr(head, sizeof head, o);
    cloud(points);
    if (m.n_vox) {
        const VMapSet to{cell[1].data(), count[1].data(), pts[1].data()};
        if (vmap_far_commit(m, to, far, nullptr) != hipSuccess) return 3;
        m.s = to, m.n_vox = mh.n_keep, points -= mh.n_evicted;
        if (vmap_rebuild(m, &mh, nullptr) != hipSuccess) return 3;   // over the table of the old ids: the reset is vmap_rebuild's
        if (extracted[(size_t)mh.n_evicted * 3] != -7.25) std::printf("extract: written behind its rows\n");
    }
    const uint32_t ev[2] = {mh.n_evicted, mh.status};
    wr(ev, sizeof ev, o);
    wr(extracted.data(), (size_t)mh.n_evicted * 24, o);
    cloud(points);
    std::vector<double> nn((size_t)nq * 3 + 3, -7.25), d2(nq + 1, -7.25);
    VMapClosestArgs q{};
    q.queries = queries.data(), q.stride = 3, q.q = nq, q.max_distance_sq = par[2], q.out_points = nn.data(), q.out_dist_sq = d2.data();
    if (vmap_closest(m, q, nullptr) != hipSuccess) return 3;
    if (nn[(size_t)nq * 3] != -7.25 || d2[nq] != -7.25) std::printf("closest: written behind its rows\n");
    wr(nn.data(), (size_t)nq * 24, o);
    wr(d2.data(), (size_t)nq * 8, o);
    std::fclose(o);
    std::printf("voxel_map_lanes: done\n");
    return 0;
}
