// icp_target_ref_main.cpp -- the plain C++ helpers of the many-source ICP route (csrc/host/icp_util.cpp: the chunk-table builder
// and the argument checks of ouster_hip_icp_target_*) in a program of its own, built with -fsanitize=address,undefined by
// tests/cpp/Makefile (`make -C tests/cpp sanitized` runs it) and run directly.  No GPU, no library.  The chunk tables go into
// buffers of exactly the size asked for, so a write past a table's end is an ASan report; the table is checked against its
// definition: every source cut into runs of 1024 rows from its own row 0, sources in order, a source of 0 rows without a chunk.
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../ouster_sdk_amd/csrc/icp_host.h"

using namespace ouster_hip_dev;

namespace ouster_hip_dev {
int fail_msg(int code, const char*) { return code; }   // the C ABI's error channel: not this program's business
}  // namespace ouster_hip_dev

static int failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) std::printf("line %d: %s\n", __LINE__, #cond), ++failures; \
    } while (0)

static void check_table(const std::vector<uint64_t>& rows) {
    const uint32_t n = static_cast<uint32_t>(rows.size());
    const uint64_t count = icp_chunk_table(rows.data(), n, nullptr, 0, nullptr, nullptr);
    std::vector<IcpChunk> chunks(count);
    std::vector<uint64_t> first_row(n), first_chunk(n);
    CHECK(icp_chunk_table(rows.data(), n, chunks.data(), count, first_row.data(), first_chunk.data()) == count);
    uint64_t at = 0, row = 0;
    for (uint32_t k = 0; k < n; ++k) {
        CHECK(first_row[k] == row && first_chunk[k] == at);
        for (uint64_t first = 0; first < rows[k]; first += ICP_CHUNK_ROWS, ++at) {
            CHECK(at < count);
            if (at >= count) return;
            const uint64_t want = rows[k] - first < ICP_CHUNK_ROWS ? rows[k] - first : ICP_CHUNK_ROWS;
            CHECK(chunks[at].source == k && chunks[at].first == first && chunks[at].rows == want);
        }
        row += rows[k];
    }
    CHECK(at == count);
    // a table that is too small is filled as far as it goes and the count is still the whole
    if (count > 1) {
        std::vector<IcpChunk> half(count / 2);
        CHECK(icp_chunk_table(rows.data(), n, half.data(), half.size(), nullptr, nullptr) == count);
        CHECK(std::memcmp(half.data(), chunks.data(), half.size() * sizeof(IcpChunk)) == 0);
    }
}

static std::string refusal(bool plane, const std::vector<ouster_hip_icp_source>& s, int32_t dtype, double angle, int* code) {
    char msg[40];   // shorter than the longest message: it must be cut, not overrun
    msg[0] = 0;
    *code = icp_sources_validate(plane, s.data(), static_cast<uint32_t>(s.size()), dtype, angle, msg, sizeof msg);
    return msg;
}

int main() {
    check_table({});
    for (uint64_t n : {0ull, 20ull, 1023ull, 1024ull, 1025ull, 2049ull}) check_table({n});
    check_table({20, 1023, 1024, 1025, 2049});
    check_table({2049, 0, 20, 0, 1024, 1025, 0});
    check_table(std::vector<uint64_t>(300, 1025));

    static const double rows3[90] = {};
    ouster_hip_icp_source a{};
    a.points = rows3, a.n = 30;
    ouster_hip_icp_source b = a;
    b.normals = rows3, b.n_normals = 30;
    int code = 0;
    CHECK(refusal(false, {a, a}, OUSTER_HIP_F64, 20.0, &code).empty() && code == OUSTER_HIP_OK);
    CHECK(refusal(true, {b, b}, OUSTER_HIP_F32, 180.0, &code).empty() && code == OUSTER_HIP_OK);
    CHECK(refusal(false, {}, OUSTER_HIP_F64, 20.0, &code).empty() && code == OUSTER_HIP_OK);
    CHECK(refusal(true, {b}, OUSTER_HIP_F64, std::numeric_limits<double>::quiet_NaN(), &code) == std::string("max_normal_angle_deg must be finite and in [0, 180]").substr(0, 39));
    CHECK(code == OUSTER_HIP_ERR_INVALID_ARGUMENT);
    ouster_hip_icp_source c = b;
    c.n_normals = 29;
    CHECK(refusal(true, {b, c}, OUSTER_HIP_F64, 20.0, &code) == std::string("source_points and source_normals must have the same number of rows").substr(0, 39));
    CHECK(refusal(false, {a, b}, OUSTER_HIP_F64, 20.0, &code) == std::string("icp_target: source 1 has normals and the target has none").substr(0, 39));
    CHECK(refusal(true, {a, b}, OUSTER_HIP_F64, 20.0, &code) == std::string("icp_target: source 0 has no normals and the target has them").substr(0, 39));
    CHECK(refusal(false, {a}, 12345, 20.0, &code) == "dtype must be F32 or F64" && code == OUSTER_HIP_ERR_INVALID_ARGUMENT);
    ouster_hip_icp_source d = a;
    d.stride = 2;
    CHECK(refusal(false, {d}, OUSTER_HIP_F64, 20.0, &code) == "a row stride is smaller than 3");
    d = a, d.points = nullptr;
    CHECK(refusal(false, {d}, OUSTER_HIP_F64, 20.0, &code) == "NULL pointer");
    CHECK(refusal(false, std::vector<ouster_hip_icp_source>(ICP_MAX_SOURCES + 1, a), OUSTER_HIP_F64, 20.0, &code) ==
          std::string("icp_target: more than 65535 sources").substr(0, 39));
    CHECK(code == OUSTER_HIP_ERR_UNSUPPORTED);
    d = a, d.n = (1ull << 29) + 1;   // nothing is read: the limits come from the counts alone
    CHECK(refusal(false, {d, d}, OUSTER_HIP_F64, 20.0, &code) == "icp: more than 2^30 rows" && code == OUSTER_HIP_ERR_UNSUPPORTED);

    ouster_hip_icp_target_desc t{};
    t.points = rows3, t.n = 30, t.dtype = OUSTER_HIP_F64, t.max_corr_dist = 0.25;
    CHECK(icp_target_validate(&t) == nullptr);
    t.flags = 1;
    CHECK(std::string(icp_target_validate(&t)) == "flags must be 0");
    t.flags = 0, t.normals = rows3, t.n_normals = 29;
    CHECK(std::string(icp_target_validate(&t)) == "target_points and target_normals must have the same number of rows");
    t.max_corr_dist = 0.0;
    CHECK(std::string(icp_target_validate(&t)) == "max_corr_dist must be finite and greater than zero");

    if (failures) return 1;
    std::printf("icp_target_ref_main: ok\n");
    return 0;
}
