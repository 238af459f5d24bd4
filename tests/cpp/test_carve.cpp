// The workspace carver (ouster_sdk_amd/csrc/carve.h) on mixed layouts: g++ only, no HIP.  A layout is a list of piece sizes in
// bytes; it is measured over no base, then assigned over a buffer (or, where a piece is too large to own, over an address that
// is never touched).  Every piece must be 256-byte aligned, pieces must not overlap, the last one must end within `total`, and
// the two passes must agree on `total`.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ouster_sdk_amd/csrc/carve.h"

using ouster_hip_dev::Carver;

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

struct Wide {   // an element type wider than a byte: sizes below are counts of it where `wide` is set
    double v[3];
};

// the layout under test, written once: piece i has sizes[i] elements of uint8_t, or of Wide where i is odd and `wide` is set
static size_t layout(void* base, const std::vector<size_t>& sizes, bool wide, std::vector<uintptr_t>& at) {
    Carver c(base);
    at.clear();
    for (size_t i = 0; i < sizes.size(); ++i)
        at.push_back(wide && i % 2 ? reinterpret_cast<uintptr_t>(c.take<Wide>(sizes[i])) : reinterpret_cast<uintptr_t>(c.take<uint8_t>(sizes[i])));
    return c.total;
}

// touch: the buffer is real, write every byte of every piece with its own mark and read all of them back
static void run(const std::vector<size_t>& sizes, bool wide, bool touch) {
    std::vector<uintptr_t> at;
    const size_t total = layout(nullptr, sizes, wide, at);
    for (uintptr_t p : at) CHECK(p == 0);   // measuring hands out no address
    CHECK(total % 256 == 0);
    void* buf = nullptr;
    uintptr_t base = 256 * 4096;            // an address that is only compared, never followed
    if (touch) {
        buf = std::aligned_alloc(256, total ? total : 256);
        CHECK(buf != nullptr);
        if (!buf) return;
        base = reinterpret_cast<uintptr_t>(buf);
    }
    CHECK(layout(reinterpret_cast<void*>(base), sizes, wide, at) == total);
    uintptr_t end = base;
    for (size_t i = 0; i < sizes.size(); ++i) {
        const size_t bytes = sizes[i] * (wide && i % 2 ? sizeof(Wide) : 1);
        CHECK(at[i] % 256 == 0);
        CHECK(at[i] >= end);                // after everything before it: no overlap
        end = at[i] + bytes;
        CHECK(end - base <= total);
        if (touch) std::memset(reinterpret_cast<void*>(at[i]), (int)(i + 1), bytes);
    }
    if (touch)
        for (size_t i = 0; i < sizes.size(); ++i) {
            const size_t bytes = sizes[i] * (wide && i % 2 ? sizeof(Wide) : 1);
            const uint8_t* p = reinterpret_cast<const uint8_t*>(at[i]);
            for (size_t k = 0; k < bytes; ++k)
                if (p[k] != (uint8_t)(i + 1)) {
                    CHECK(!"a piece was overwritten by another");
                    break;
                }
        }
    std::free(buf);
}

int main() {
    run({}, false, true);
    run({0}, false, true);
    run({1}, false, true);
    run({0, 0, 1, 0}, false, true);
    run({1, 255, 256, 257}, false, true);
    run({257, 0, 256, 1, 255, 0}, false, true);
    run({256, 1, 0, 11, 255, 43, 1, 0}, true, true);          // odd pieces count 24-byte elements
    run({1, (1ull << 31) + 1, 255, 0, 257}, false, false);   // 2^31 + 1 bytes: counted, never touched
    run({0, ((1ull << 31) + 1 + 23) / 24, 1}, true, false);   // the same through a wide element type
    {   // the figures themselves, once: 1 | 255 | 256 | 257 bytes take 256 | 256 | 256 | 512
        std::vector<uintptr_t> at;
        CHECK(layout(nullptr, {1, 255, 256, 257}, false, at) == 1280);
        CHECK(layout(reinterpret_cast<void*>(uintptr_t(4096)), {1, 255, 256, 257}, false, at) == 1280);
        CHECK(at.size() == 4 && at[0] == 4096 && at[1] == 4352 && at[2] == 4608 && at[3] == 4864);
        CHECK(layout(nullptr, {(1ull << 31) + 1}, false, at) == (1ull << 31) + 256);
    }
    if (failures) return std::fprintf(stderr, "%d checks failed\n", failures), 1;
    std::puts("carve: ok");
    return 0;
}
