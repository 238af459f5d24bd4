// voxel_map_lanes.cpp -- k_vmap_find, k_vmap_publish, k_vmap_admit, k_vmap_far, k_vmap_compact, k_vmap_rebuild, k_vmap_closest and
// k_vmap_cloud of csrc/k_voxel_map.hip compiled for the CPU (tests/cpp/host_lanes/hip/hip_runtime.h: one thread per lane), over the
// call-local grid k_voxel.hip's own kernels build; the scans and the stable sort rocPRIM does on the device are std:: here.  Built
// and run by tests/test_voxel_map_lanes_cpu.py, which compares every output with tests/voxel_map_model.py bit for bit.
//   voxel_map_lanes <case file> <result file>
// case file: u32 n_calls P n_queries cap, f64 voxel_size max_distance bound_sq origin[3]; per call u32 n, pad, f64 rows [n][3]; f64
// queries [n_queries][3].  The map has room for `cap` voxels and 2 * cap slots (a power of two) from the start: it never grows.
// result file: u32 status voxels points kept, f64 cloud [points][3] after the last add, then (after removal at `origin`) u32
// evicted_rows pad, f64 extracted [evicted_rows][3], f64 cloud [points - evicted_rows][3], f64 nn [n_queries][3], f64 d2 [n_queries].
#include "host_lanes/voxel_lanes_atomics.h"

inline unsigned long long atomicAdd(unsigned long long* address, unsigned long long val) {
    std::atomic_ref<unsigned long long> r(*address);
    return r.fetch_add(val);
}
#define __constant__ static const

#include "../../ouster_sdk_amd/csrc/k_voxel.hip"
#include "../../ouster_sdk_amd/csrc/k_voxel_map.hip"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

using namespace ouster_hip_dev;

static bool rd(void* p, size_t bytes, FILE* f) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
static void wr(const void* p, size_t bytes, FILE* f) {
    if (bytes) std::fwrite(p, 1, bytes, f);
}
static void scan(const uint32_t* in, uint32_t* out, size_t n) {
    uint32_t run = 0;
    for (size_t i = 0; i < n; ++i) out[i] = run, run += in[i];
}
static dim3 blocks(uint64_t n) { return dim3((unsigned)((n + VOXEL_WG - 1) / VOXEL_WG)); }
// the stand-in's launch takes one argument: a kernel of several goes in as a closure, called once per lane
template <class F>
static void run(dim3 grid, F f) {
    hipLaunchKernelGGL(+[](F* g) { (*g)(); }, grid, dim3(VOXEL_WG), 0, nullptr, &f);
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
    std::vector<int32_t> table(slots, VOXEL_EMPTY);
    VMapDev m;
    m.s = VMapSet{cell[0].data(), count[0].data(), pts[0].data()};
    m.table = table.data(), m.table_mask = slots - 1, m.cap = cap, m.P = P;
    m.voxel_size = par[0], m.inv = 1.0 / par[0], m.resolution_sq = par[0] * par[0] / (double)P;
    VMapHeader mh{};
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
        VoxelHeader vh{};
        std::vector<VoxelKey> keys(n);
        std::vector<int32_t> local((size_t)a.table_mask + 1, VOXEL_EMPTY);
        std::vector<uint32_t> slot(n), first(n), first_id(n), vid(n), idx(n), svid(n), sidx(n), seg_begin(n), seg_end(n), found(n), is_new(n), new_pos(n);
        a.hdr = &vh, a.keys = keys.data(), a.table = local.data(), a.slot = slot.data(), a.first = first.data(), a.first_id = first_id.data();
        a.vid = vid.data(), a.idx = idx.data(), a.svid = svid.data(), a.sidx = sidx.data(), a.seg_begin = seg_begin.data(), a.seg_end = seg_end.data();
        if (launch_voxel_keys(a, nullptr) != hipSuccess || launch_voxel_insert(a, nullptr) != hipSuccess || launch_voxel_first(a, nullptr) != hipSuccess) return 3;
        scan(first.data(), first_id.data(), n);
        if (launch_voxel_ids(a, nullptr) != hipSuccess) return 3;
        std::vector<uint32_t> order(n);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return vid[x] < vid[y]; });
        for (uint32_t i = 0; i < n; ++i) svid[i] = vid[order[i]], sidx[i] = idx[order[i]];
        if (launch_voxel_segments(a, nullptr) != hipSuccess) return 3;
        VMapAddArgs x{&mh, found.data(), is_new.data(), new_pos.data()};
        mh = VMapHeader{};
        run(blocks(n), [&] { k_vmap_find(a, m, x); });
        scan(is_new.data(), new_pos.data(), n);
        mh.n_new = new_pos[n - 1] + is_new[n - 1];
        if (vh.status || m.n_vox + mh.n_new > cap) return 4;
        run(blocks(n), [&] { k_vmap_publish(a, m, x); });
        run(blocks(n), [&] { k_vmap_admit<double>(a, m, x); });
        m.n_vox += mh.n_new, points += mh.n_admitted;
        if (mh.status) return 5;
    }
    std::vector<double> queries((size_t)nq * 3);
    if (!rd(queries.data(), queries.size() * 8, f)) return 2;
    std::fclose(f);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    auto cloud = [&](uint64_t rows) {
        std::vector<uint32_t> pos(m.n_vox + 1);
        std::vector<double> out(rows * 3 + 3, -7.25);
        scan(m.s.count, pos.data(), m.n_vox);
        if (m.n_vox) run(blocks((uint64_t)m.n_vox * P), [&] { k_vmap_cloud(m, pos.data(), out.data()); });
        if (out[rows * 3] != -7.25) std::printf("cloud: written behind its rows\n");
        wr(out.data(), rows * 24, o);
    };
    const uint32_t before[4] = {mh.status, m.n_vox, (uint32_t)points, 0};
    // removal at `origin`
    int32_t origin[3];
    for (int k = 0; k < 3; ++k) origin[k] = (int32_t)std::floor(par[3 + k] * m.inv);
    std::vector<uint32_t> keep(m.n_vox + 1), keep_pos(m.n_vox + 1), gone(m.n_vox + 1), gone_pos(m.n_vox + 1);
    VMapFarArgs far{};
    far.hdr = &mh, far.keep = keep.data(), far.keep_pos = keep_pos.data(), far.gone = gone.data(), far.gone_pos = gone_pos.data();
    std::memcpy(far.origin, origin, sizeof origin);
    far.max_voxel_dist = (int64_t)std::ceil(par[1] * m.inv) + 1;
    mh = VMapHeader{};
    uint32_t kept = m.n_vox;
    std::vector<double> extracted;
    if (m.n_vox) {
        run(blocks(m.n_vox), [&] { k_vmap_far(m, far); });
        scan(keep.data(), keep_pos.data(), m.n_vox);
        scan(gone.data(), gone_pos.data(), m.n_vox);
        mh.n_keep = keep_pos[m.n_vox - 1] + keep[m.n_vox - 1], mh.n_evicted = gone_pos[m.n_vox - 1] + gone[m.n_vox - 1];
        kept = mh.n_keep;
        extracted.assign((size_t)mh.n_evicted * 3 + 3, -7.25);
        far.out = extracted.data();
    }
    const uint32_t head[4] = {before[0], before[1], before[2], kept};
    wr(head, sizeof head, o);
    cloud(points);
    if (m.n_vox) {
        const VMapSet to{cell[1].data(), count[1].data(), pts[1].data()};
        run(blocks((uint64_t)m.n_vox * P), [&] { k_vmap_compact(m, to, far); });
        m.s = to, m.n_vox = mh.n_keep, points -= mh.n_evicted;
        std::fill(table.begin(), table.end(), VOXEL_EMPTY);
        if (m.n_vox) run(blocks(m.n_vox), [&] { k_vmap_rebuild(m, &mh); });
        if (extracted[(size_t)mh.n_evicted * 3] != -7.25) std::printf("extract: written behind its rows\n");
    }
    const uint32_t ev[2] = {mh.n_evicted, mh.status};
    wr(ev, sizeof ev, o);
    wr(extracted.data(), (size_t)mh.n_evicted * 24, o);
    cloud(points);
    std::vector<double> nn((size_t)nq * 3 + 3, -7.25), d2(nq + 1, -7.25);
    VMapClosestArgs q{};
    q.queries = queries.data(), q.stride = 3, q.q = nq, q.max_distance_sq = par[2], q.out_points = nn.data(), q.out_dist_sq = d2.data();
    if (nq) run(blocks(nq), [&] { k_vmap_closest<double>(m, q); });
    if (nn[(size_t)nq * 3] != -7.25 || d2[nq] != -7.25) std::printf("closest: written behind its rows\n");
    wr(nn.data(), (size_t)nq * 24, o);
    wr(d2.data(), (size_t)nq * 8, o);
    std::fclose(o);
    std::printf("voxel_map_lanes: done\n");
    return 0;
}
