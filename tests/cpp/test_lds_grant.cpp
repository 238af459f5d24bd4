// The dynamic-LDS grant (ouster_sdk_amd/csrc/lds_grant.h) with the runtime replaced by a counter: g++ only, no HIP.  What is
// checked is when the runtime is asked -- never at or below 48 KB, once per (kernel, device) for a limit, again only for a
// larger one -- and that a device outside the table is asked every time and never reads or writes another device's slot.
#include <cstdio>
#include <initializer_list>

#include "../../ouster_sdk_amd/csrc/lds_grant.h"

using ouster_hip_dev::LdsGrant;

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

static int asked = 0;      // calls that reached the "runtime"
static int answer = 0;     // what it returns (0: success)
static int ensure(LdsGrant& g, size_t lds, int device) {
    return g.ensure(lds, device, [] { ++asked; return answer; });
}

int main() {
    constexpr size_t KB = 1024;
    {   // at or below 48 KB nothing is asked and nothing is remembered
        LdsGrant g;
        CHECK(ensure(g, 0, 0) == 0 && ensure(g, 1, 0) == 0 && ensure(g, 48 * KB, 0) == 0 && ensure(g, 48 * KB, 16) == 0);
        CHECK(asked == 0);
        for (auto& b : g.bytes) CHECK(b.load() == 0);
    }
    {   // the first request above it asks; an equal or smaller one after it does not; a larger one asks again
        LdsGrant g;
        asked = 0;
        CHECK(ensure(g, 48 * KB + 1, 0) == 0 && asked == 1);
        CHECK(ensure(g, 48 * KB + 1, 0) == 0 && asked == 1);
        CHECK(ensure(g, 96 * KB, 0) == 0 && asked == 2);
        CHECK(ensure(g, 96 * KB, 0) == 0 && ensure(g, 64 * KB, 0) == 0 && ensure(g, 48 * KB + 1, 0) == 0 && asked == 2);
        CHECK(ensure(g, 160 * KB, 0) == 0 && asked == 3);
        CHECK(g.bytes[0].load() == 160 * KB);
        // devices 0 and 1 are independent, and so is the last slot of the table
        CHECK(ensure(g, 64 * KB, 1) == 0 && asked == 4 && g.bytes[1].load() == 64 * KB && g.bytes[0].load() == 160 * KB);
        CHECK(ensure(g, 64 * KB, 1) == 0 && asked == 4);
        CHECK(ensure(g, 64 * KB, 15) == 0 && asked == 5 && g.bytes[15].load() == 64 * KB);
        CHECK(ensure(g, 64 * KB, 15) == 0 && asked == 5);
    }
    {   // devices 16 and -1 are never remembered and never read device 0's slot (nor 15's): asked every time
        LdsGrant g;
        asked = 0;
        CHECK(ensure(g, 160 * KB, 0) == 0 && ensure(g, 160 * KB, 15) == 0 && asked == 2);
        for (int dev : {16, -1, 17, 32, 1 << 20, -16}) {
            const int before = asked;
            CHECK(ensure(g, 64 * KB, dev) == 0 && asked == before + 1);
            CHECK(ensure(g, 64 * KB, dev) == 0 && asked == before + 2);
        }
        for (int d = 0; d < LdsGrant::MAX_DEVICES; ++d) CHECK(g.bytes[d].load() == (d == 0 || d == 15 ? 160 * KB : 0));
        LdsGrant h;   // and they write no slot either: device 0 still has to ask
        asked = 0;
        CHECK(ensure(h, 64 * KB, 16) == 0 && ensure(h, 64 * KB, -1) == 0 && asked == 2);
        CHECK(ensure(h, 64 * KB, 0) == 0 && asked == 3);
    }
    {   // a refusal is handed back and not remembered
        LdsGrant g;
        asked = 0;
        answer = 1;
        CHECK(ensure(g, 64 * KB, 0) == 1 && asked == 1 && g.bytes[0].load() == 0);
        answer = 0;
        CHECK(ensure(g, 64 * KB, 0) == 0 && asked == 2);
        CHECK(ensure(g, 64 * KB, 0) == 0 && asked == 2);
    }
    if (failures) return 1;
    std::printf("lds_grant: ok\n");
    return 0;
}
