// registration_lanes.cpp -- the source of k_reg_pass's thread (reg_thread_rows: load, apply, the map's query, flag, weight, terms, the
// fold of the thread's rows) and of k_reg_fold (reg_fold_chunks) of csrc/k_registration.hip compiled for the CPU
// (tests/cpp/host_lanes/hip/hip_runtime.h: one thread per lane).  The wave butterfly of block_sums is device only (__shfl_xor); this
// program restates it over the threads' accumulators -- the same shape: xor offsets 32 .. 1 within a wave of 64, lane 0 of each wave,
// the 4 waves in order -- and the chunks go through the kernel's own fold.  Built and run by
// tests/test_registration_lanes_cpu.py, which compares with tests/registration_model.py.
//   registration_lanes <case file> <result file>
// case file: u32 n P apply f32 stride n_vox pad pad; f64 voxel_size max_distance kernel_scale; f64 estimate[7]; per voxel i32 cell[3],
// u32 count; f64 points [n_vox][P][3]; the rows [n][stride] of f32 / f64.  The map is laid out from the model's state, its table
// filled by linear probing from voxel_hash.
// result file: f64 moved [n][3]; f64 neighbours [n][3]; f64 dist_sq [n]; f64 terms [n][16]; f64 thread_acc [chunks * 256][16]; f64
// sums [16]; u64 count; u32 thread_count [chunks * 256]; u8 flags [n].
#include "../../ouster_sdk_amd/csrc/k_registration.hip"

#include "host_lanes/lanes_util.h"

using namespace ouster_hip_dev;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    uint32_t hd[8];
    double par[3], est[7];
    if (!f || !rd(hd, sizeof hd, f) || !rd(par, sizeof par, f) || !rd(est, sizeof est, f)) return 2;
    const uint32_t n = hd[0], P = hd[1], apply = hd[2], f32 = hd[3], stride = hd[4], n_vox = hd[5];
    if (n == 0 || stride < 3 || P == 0) return 2;
    std::vector<VoxelKey> cell(n_vox + 1);
    std::vector<uint32_t> held(n_vox + 1);
    for (uint32_t v = 0; v < n_vox; ++v) {
        int32_t c[3];
        if (!rd(c, sizeof c, f) || !rd(&held[v], 4, f)) return 2;
        cell[v] = VoxelKey{c[0], c[1], c[2], 1};
    }
    std::vector<double> pts((size_t)n_vox * P * 3 + 3);
    if (!rd(pts.data(), (size_t)n_vox * P * 24, f)) return 2;
    std::vector<uint8_t> raw((size_t)n * stride * (f32 ? 4 : 8));
    if (!rd(raw.data(), raw.size(), f)) return 2;
    std::fclose(f);
    uint32_t slots = 2;
    while (slots < 2 * n_vox) slots <<= 1;
    std::vector<int32_t> table(slots, VOXEL_EMPTY);
    for (uint32_t v = 0; v < n_vox; ++v) {
        uint32_t s = voxel_hash(cell[v]) & (slots - 1);
        while (table[s] != VOXEL_EMPTY) s = (s + 1) & (slots - 1);
        table[s] = (int32_t)v;
    }
    VMapDev m;
    m.s = VMapSet{cell.data(), held.data(), pts.data()};
    m.table = table.data(), m.table_mask = slots - 1, m.n_vox = n_vox, m.cap = n_vox, m.P = P;
    m.voxel_size = par[0], m.inv = 1.0 / par[0], m.resolution_sq = par[0] * par[0] / (double)P;

    const uint32_t chunks = reg_chunks(n), threads = chunks * ICP_WG;
    const double guard = -7.25;
    std::vector<double> moved((size_t)n * 3 + 3, guard), nn((size_t)n * 3 + 3, guard), d2(n + 1, guard), terms((size_t)n * REG_NS + 1, guard);
    std::vector<uint8_t> flags(n + 1, 7);
    std::vector<double> acc((size_t)threads * REG_NS), partials((size_t)chunks * REG_NS);
    std::vector<uint32_t> tcount(threads), counts(chunks);
    RegHeader hdr{};
    RegPassArgs a{};
    a.src = raw.data(), a.stride = stride, a.n = n, a.apply = (int32_t)apply;
    for (int k = 0; k < 4; ++k) a.q[k] = est[k];
    for (int k = 0; k < 3; ++k) a.t[k] = est[4 + k];
    a.max_d2 = par[1] * par[1], a.k = par[2];
    a.moved = moved.data(), a.partials = partials.data(), a.counts = counts.data(), a.hdr = &hdr;
    a.flags = flags.data(), a.neighbours = nn.data(), a.dist_sq = d2.data(), a.terms = terms.data();
    run_lanes(dim3(chunks), dim3(ICP_WG), [&] {
        double mine[REG_NS];
        uint32_t c;
        if (f32) reg_thread_rows<float>(m, a, blockIdx.x, threadIdx.x, mine, c);
        else reg_thread_rows<double>(m, a, blockIdx.x, threadIdx.x, mine, c);
        const size_t t = (size_t)blockIdx.x * ICP_WG + threadIdx.x;
        std::memcpy(&acc[t * REG_NS], mine, sizeof mine);
        tcount[t] = c;
    });
    if (moved[(size_t)n * 3] != guard || nn[(size_t)n * 3] != guard || d2[n] != guard || terms[(size_t)n * REG_NS] != guard || flags[n] != 7) {
        std::printf("written behind its rows\n");
        return 3;
    }
    // block_sums restated: the butterfly within each wave, lane 0, the waves in order
    for (uint32_t b = 0; b < chunks; ++b) {
        std::vector<double> v(acc.begin() + (size_t)b * ICP_WG * REG_NS, acc.begin() + (size_t)(b + 1) * ICP_WG * REG_NS);
        std::vector<uint32_t> c(tcount.begin() + (size_t)b * ICP_WG, tcount.begin() + (size_t)(b + 1) * ICP_WG);
        for (uint32_t off = 32; off >= 1; off >>= 1) {
            const std::vector<double> old = v;
            const std::vector<uint32_t> oldc = c;
            for (uint32_t l = 0; l < ICP_WG; ++l) {
                for (int s = 0; s < REG_NS; ++s) v[l * REG_NS + s] = old[l * REG_NS + s] + old[(l ^ off) * REG_NS + s];
                c[l] = oldc[l] + oldc[l ^ off];
            }
        }
        for (int s = 0; s < REG_NS; ++s) {
            double p = v[s];
            for (uint32_t w = 1; w < ICP_WG / 64; ++w) p = p + v[(size_t)w * 64 * REG_NS + s];
            partials[(size_t)b * REG_NS + s] = p;
        }
        uint32_t pc = c[0];
        for (uint32_t w = 1; w < ICP_WG / 64; ++w) pc = pc + c[w * 64];
        counts[b] = pc;
    }
    run_lanes(dim3(1), dim3(64), [&] { reg_fold_chunks(a, chunks, threadIdx.x); });

    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    wr(moved.data(), (size_t)n * 24, o);
    wr(nn.data(), (size_t)n * 24, o);
    wr(d2.data(), (size_t)n * 8, o);
    wr(terms.data(), (size_t)n * REG_NS * 8, o);
    wr(acc.data(), acc.size() * 8, o);
    wr(hdr.sums, sizeof hdr.sums, o);
    wr(&hdr.count, 8, o);
    wr(tcount.data(), tcount.size() * 4, o);
    wr(flags.data(), n, o);
    std::fclose(o);
    std::printf("registration_lanes: done\n");
    return 0;
}
