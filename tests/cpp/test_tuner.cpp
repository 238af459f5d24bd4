// The decode's variant tuner (ouster_sdk_amd/csrc/decode_tuner.h) with the clocks replaced by an array of floats: g++ only, no
// HIP.  What is checked is what decides a verdict (cold and warm samples, ties, candidates without a usable sample), the
// sequence of a workload's calls, the text of the cache file and what the tuner does with it, the bound on the table, that
// every route by which an entry goes destroys its samples, and that another candidate list under the same key starts over.
#include <stdlib.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../ouster_sdk_amd/csrc/decode_tuner.h"

using namespace ouster_hip_dev;

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

// the samples of one workload: times the test writes, and whether each has "landed"
struct Fake {
    static int made, live, asked;
    float t[TUNE_SAMPLES];
    bool done[TUNE_SAMPLES];
    Fake() {
        ++made, ++live;
        for (float& x : t) x = 1.0f;
        for (bool& d : done) d = false;
    }
    Fake(const Fake&) = delete;
    Fake& operator=(const Fake&) = delete;
    ~Fake() { --live; }
    bool landed(int n) const {
        ++asked;
        for (int i = 0; i < n; ++i)
            if (!done[i]) return false;
        return true;
    }
    float ms(int i) const { return ++asked, t[i]; }
};
int Fake::made = 0, Fake::live = 0, Fake::asked = 0;
using Tuner = DecodeTuner<Fake>;
constexpr int R = TUNE_ROUNDS;

static bool is(const Tuner::Step& s, int variant, int slot, const char* source) {
    return s.variant == variant && s.slot == slot && (slot >= 0) == (s.record != nullptr) && !strcmp(s.source, source);
}

// the nc * R measuring calls of a fresh key, sample i taking ms[i] (1.0 without) and landing at once; -> the call after them
static Tuner::Step measure(Tuner& t, uint64_t key, const int* cand, int nc, const float* ms = nullptr) {
    for (int i = 0; i < nc * R; ++i) {
        const Tuner::Step s = t.step(key, cand, nc);
        CHECK(is(s, cand[i / R], i, "measuring"));
        if (!s.record) return s;
        s.record->t[i] = ms ? ms[i] : 1.0f;
        s.record->done[i] = true;
    }
    return t.step(key, cand, nc);
}

static std::vector<std::string> lines_of(const std::string& path) {
    std::vector<std::string> out;
    std::ifstream f(path);
    for (std::string ln; std::getline(f, ln);) out.push_back(ln);
    return out;
}
static void write_file(const std::string& path, const std::string& text) { std::ofstream(path, std::ios::trunc) << text; }

static void test_sequence() {
    const int cand[3] = {256, 128, 1256};
    Tuner t;
    Fake* f = nullptr;
    for (int i = 0; i < 12; ++i) {
        const Tuner::Step s = t.step(7, cand, 3);
        CHECK(is(s, cand[i / 4], i, "measuring"));
        f = s.record;
        f->t[i] = i / 4 == 1 ? 0.5f : 1.0f;   // 128 is the fastest
        f->done[i] = i != 7;
    }
    CHECK(is(t.step(7, cand, 3), 256, -1, "measuring"));   // every sample queued, sample 7 not landed: the default, no slot
    CHECK(is(t.step(7, cand, 3), 256, -1, "measuring"));
    f->done[7] = true;
    CHECK(is(t.step(7, cand, 3), 128, -1, "measured"));    // the verdict, in the call that finds them landed
    Fake::asked = 0;
    for (int i = 0; i < 100; ++i) CHECK(is(t.step(7, cand, 3), 128, -1, "measured"));
    CHECK(Fake::asked == 0);                               // the steady state asks the clock nothing
}

static void test_verdict() {
    const int cand[3] = {256, 128, 0};
    {   // the smallest number of the table is a cold sample of a candidate whose warm samples are the largest: it loses
        const float ms[12] = {0.1f, 9, 9, 9, /**/ 5, 2, 3, 4, /**/ 5, 2.5f, 2.5f, 2.5f};
        const TuneVerdict v = tune_verdict(ms, cand, 3);
        CHECK(v.variant == 128 && v.ms == 2);
    }
    {   // only its cold sample usable: that sample competes
        const float ms[12] = {5, 4, 4, 4, /**/ 3, 0, -1, 0, /**/ 5, 3.5f, 6, 6};
        const TuneVerdict v = tune_verdict(ms, cand, 3);
        CHECK(v.variant == 128 && v.ms == 3);
        const float ms2[12] = {5, 4, 4, 4, /**/ 4.5f, 0, -1, 0, /**/ 5, 4.25f, 6, 6};
        CHECK(tune_verdict(ms2, cand, 3).variant == 256);
    }
    {   // nothing usable: cannot win, even listed first
        const float ms[12] = {0, -1, 0, -2, /**/ 5, 4, 4, 4, /**/ 5, 6, 6, 6};
        const TuneVerdict v = tune_verdict(ms, cand, 3);
        CHECK(v.variant == 128 && v.ms == 4);
    }
    {   // two equal best times: the earlier candidate
        const float ms[12] = {5, 4, 4, 4, /**/ 5, 3, 4, 4, /**/ 1, 4, 3, 4};
        const TuneVerdict v = tune_verdict(ms, cand, 3);
        CHECK(v.variant == 128 && v.ms == 3);
    }
    {   // everything unusable: the default and a time of 0
        const float ms[12] = {0, 0, 0, 0, /**/ -1, -1, -1, -1, /**/ 0, -3, 0, 0};
        const TuneVerdict v = tune_verdict(ms, cand, 3);
        CHECK(v.variant == 256 && v.ms == 0);
        const int other[2] = {128, 0};   // ... also where the default is not among the candidates
        CHECK(tune_verdict(ms, other, 2).variant == 256);
    }
    {   // the tuner takes its verdict by the same function, over the samples of this list
        const float ms[12] = {0.1f, 9, 9, 9, /**/ 5, 2, 3, 4, /**/ 5, 1.5f, 2.5f, 2.5f};
        Tuner t;
        CHECK(is(measure(t, 1, cand, 3, ms), 0, -1, "measured"));
    }
}

static void test_cache_text(const std::string& dir) {
    const std::string id = tune_cache_id("gfx950:sramecc+:xnack-", 256, "AMD Instinct\tMI355X", "ouster_hip 0.4 (gfx950)");
    CHECK(id == "gfx950:sramecc+:xnack-:256:AMD_Instinct_MI355X:ouster_hip_0.4_(gfx950)");
    CHECK(id.find(' ') == std::string::npos && id.find('\t') == std::string::npos);
    char line[TUNE_LINE];
    for (uint64_t key : {(uint64_t)0, (uint64_t)1, ~(uint64_t)0}) {
        const int n = tune_cache_format(line, id, key, 1128, 0.53127f);
        CHECK(n > 0 && (size_t)n == strlen(line) && line[n - 1] == '\n');
        uint64_t k = 5;
        int v = -1;
        CHECK(tune_cache_parse(line, id, &k, &v) && k == key && v == 1128);
    }
    tune_cache_format(line, id, 0xabcull, 128, 1.25f);
    CHECK(std::string(line) == "v1 " + id + " 0000000000000abc 128 1.2500\n");
    CHECK(tune_cache_format(line, std::string(600, 'x'), 1, 128, 1.0f) == 0);   // does not fit: not written

    uint64_t k = 0;
    int v = 0;
    const std::string good = "v1 " + id + " 0000000000000abc 128 1.2500\n";
    CHECK(tune_cache_parse(good.c_str(), id, &k, &v));
    const std::string tail = "abc 128 1.2500";
    const std::string long_line = "v1 " + id + " " + std::string(600 - 4 - id.size() - tail.size(), '0') + tail;   // 600 characters
    CHECK(long_line.size() == 600);
    const std::string bad[] = {
        "v2 " + id + " 0000000000000abc 128 1.2500\n",          // another version
        "v1 some_other_gpu:1:x:v0 0000000000000abc 128 1.2500\n",   // another device or library
        "v1 " + id + " 0000000000000abc 128\n",                 // four fields
        "v1 " + id + " xyz 128 1.2500\n",                       // the key is not hexadecimal
        long_line + "\n",
    };
    for (const std::string& b : bad) CHECK(!tune_cache_parse(b.c_str(), id, &k, &v));

    // loading: every bad line is passed over, whatever surrounds it, and the last line of a key wins
    const int cand[3] = {256, 128, 0};
    const std::string path = dir + "/text.cache";
    for (const std::string& b : bad) {
        write_file(path, b + b);
        Tuner t;
        t.set_cache(path, id);
        CHECK(is(t.step(0xabc, cand, 3), 256, 0, "measuring"));
    }
    write_file(path, bad[4] + good + bad[0] + "v1 " + id + " 0000000000000abc 0 0.9000\n" + bad[1]);
    Tuner t;
    t.set_cache(path, id);
    CHECK(is(t.step(0xabc, cand, 3), 0, -1, "cache"));
}

static void test_cache_behaviour(const std::string& dir) {
    const std::string id = tune_cache_id("gfx950", 256, "a b", "v");
    const int cand[3] = {256, 128, 0};
    const std::string path = dir + "/tuning.cache";
    const float ms[12] = {5, 4, 4, 4, /**/ 5, 3, 4, 4, /**/ 5, 6, 6, 6};
    {   // a measuring tuner appends its verdict as exactly one line of the stated form
        Tuner t;
        t.set_cache(path, id);
        CHECK(is(measure(t, 0x11, cand, 3, ms), 128, -1, "measured"));
        CHECK(is(t.step(0x11, cand, 3), 128, -1, "measured"));
        const auto lines = lines_of(path);
        CHECK(lines.size() == 1 && lines[0] == "v1 gfx950:256:a_b:v 0000000000000011 128 3.0000");
    }
    {   // the next tuner takes it from call one, is handed no slot ever, and appends nothing
        Tuner t;
        t.set_cache(path, id);
        Fake::asked = 0;
        for (int i = 0; i < 30; ++i) CHECK(is(t.step(0x11, cand, 3), 128, -1, "cache"));
        CHECK(Fake::asked == 0 && lines_of(path).size() == 1);
    }
    {   // a cached variant that is not among the call's candidates is not launched: it measures
        const int others[2] = {256, 0};
        Tuner t;
        t.set_cache(path, id);
        CHECK(is(t.step(0x11, others, 2), 256, 0, "measuring"));
    }
    {   // under another id the file says nothing
        Tuner t;
        t.set_cache(path, id + "x");
        CHECK(is(t.step(0x11, cand, 3), 256, 0, "measuring"));
    }
    {   // retune: the same key measures again and appends a second line; so does what came from the file
        Tuner t;
        t.set_cache(path, id);
        CHECK(is(t.step(0x11, cand, 3), 128, -1, "cache"));
        t.forget();
        CHECK(is(measure(t, 0x11, cand, 3, ms), 128, -1, "measured"));
        CHECK(lines_of(path).size() == 2 && lines_of(path)[1] == lines_of(path)[0]);
        t.forget();
        CHECK(is(measure(t, 0x11, cand, 3, ms), 128, -1, "measured"));
        CHECK(lines_of(path).size() == 3);
    }
    {   // nothing usable: the default, and a line that ends in 0.0000
        const float none[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        Tuner t;
        t.set_cache(path, id);
        CHECK(is(measure(t, 0x12, cand, 3, none), 256, -1, "measured"));
        CHECK(lines_of(path).back() == "v1 gfx950:256:a_b:v 0000000000000012 256 0.0000");
    }
    {   // a path in a directory that does not exist: the same calls, no file; an empty path: no cache at all
        const std::string nowhere = dir + "/no_such_dir/tuning.cache";
        for (const std::string& p : {nowhere, std::string()}) {
            Tuner t;
            t.set_cache(p, id);
            CHECK(is(measure(t, 0x11, cand, 3, ms), 128, -1, "measured"));
            CHECK(is(t.step(0x11, cand, 3), 128, -1, "measured"));
        }
        struct stat st;
        CHECK(stat(nowhere.c_str(), &st) != 0 && stat((dir + "/no_such_dir").c_str(), &st) != 0);
    }
}

static void test_bound_and_lifetime() {
    const int cand[3] = {256, 128, 0};
    Fake::made = Fake::live = 0;
    {
        Tuner t;
        // the table holds what it held before: a new key that finds more than 64 entries forgets them all, itself excepted
        for (uint64_t key = 1; key <= 65; ++key) {
            CHECK(is(t.step(key, cand, 3), 256, 0, "measuring"));   // one sample queued each
            CHECK(Fake::live == (int)key);
        }
        CHECK(is(t.step(3, cand, 3), 256, 1, "measuring") && Fake::live == 65);   // a key it knows is no new key
        CHECK(is(t.step(66, cand, 3), 256, 0, "measuring"));
        CHECK(Fake::live == 1 && Fake::made == 66 && t.size() == 1);
        CHECK(is(t.step(3, cand, 3), 256, 0, "measuring") && Fake::live == 2);    // forgotten: from the start
        // retune in the middle of a measurement leaves none
        for (int i = 1; i < 5; ++i) CHECK(is(t.step(3, cand, 3), cand[i / R], i, "measuring"));
        t.forget();
        CHECK(Fake::live == 0 && t.size() == 0);
        CHECK(is(t.step(3, cand, 3), 256, 0, "measuring") && is(t.step(4, cand, 3), 256, 0, "measuring") && Fake::live == 2);
    }
    CHECK(Fake::live == 0);   // nor does the tuner's end
}

static void test_changed_list() {
    const int before[3] = {256, 128, 0}, after[2] = {256, 0};
    Fake::made = Fake::live = 0;
    Tuner t;
    for (int i = 0; i < 5; ++i) CHECK(is(t.step(9, before, 3), before[i / R], i, "measuring"));
    CHECK(Fake::made == 1 && Fake::live == 1);
    // sample 4 was a launch of 128: under the new list slot 4 belongs to variant 0.  The entry starts over.
    const float ms[8] = {5, 4, 4, 4, /**/ 5, 3, 4, 4};
    CHECK(is(measure(t, 9, after, 2, ms), 0, -1, "measured"));   // slots 0 .. 7 of the new list, then its verdict
    CHECK(Fake::made == 2 && Fake::live == 1);                   // the first samples are gone
    // a verdict does not outlive its list either
    CHECK(is(t.step(9, before, 3), 256, 0, "measuring") && Fake::made == 3 && Fake::live == 1);
}

int main() {
    char tmpl[] = "/tmp/test_tuner.XXXXXX";
    const char* made = mkdtemp(tmpl);
    if (!made) return std::perror("mkdtemp"), 1;
    const std::string dir = made;
    test_sequence();
    test_verdict();
    test_cache_text(dir);
    test_cache_behaviour(dir);
    test_bound_and_lifetime();
    test_changed_list();
    for (const char* name : {"/text.cache", "/tuning.cache"}) unlink((dir + name).c_str());
    rmdir(dir.c_str());
    if (failures) return 1;
    std::printf("tuner: ok\n");
    return 0;
}
