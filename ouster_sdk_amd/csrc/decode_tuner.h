// decode_tuner.h -- the variant tuner of the fused decode: which of a workload's candidate kernels
// ouster_hip_decode launches, learnt by timing each candidate on the first calls, and the text file its verdicts persist in.
// No HIP include: what a sample is belongs to the owner (`Samples`; the library's holds pairs of events, capi_internal.h), and
// tests/cpp/test_tuner.cpp runs every rule below on the CPU.
//
// Four launches of each candidate, back to back (a launch that follows a different variant is not representative of the
// steady state: alternating the candidates made the 64-column kernel look 8 % faster than it then ran).  Single launches
// vary by ~10 %, mostly upwards, and the candidates can be within 1-5 % of each other: each candidate's fastest sample
// counts, its first one (cold code, cold TLB, another variant's write-backs still draining) only when nothing else landed.
// The clocks are polled, never waited for: until all samples have landed the default variant runs.
#pragma once
#include <fcntl.h>
#include <stdint.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

namespace ouster_hip_dev {
#pragma GCC visibility push(hidden)   // the library's dynamic symbols stay what they were

constexpr int TUNE_ROUNDS = 4, TUNE_NCAND = 5, TUNE_SAMPLES = TUNE_NCAND * TUNE_ROUNDS;
constexpr int TUNE_DEFAULT = 256;   // the variant that runs while nothing is known: k_decode_wide's 256-column tiles

// ---- the verdict --------------------------------------------------------------------------------------------------------
// ms[0 .. nc * TUNE_ROUNDS): sample i belongs to candidate i / TUNE_ROUNDS and is its cold one when i % TUNE_ROUNDS == 0; a
// time <= 0 is a sample that cannot be used.  A candidate's time is its fastest warm sample, its cold one when no warm one is
// usable; the fastest candidate wins, the earlier one on a tie, and one without any usable sample cannot.
struct TuneVerdict {
    int variant = TUNE_DEFAULT;
    float ms = 0;   // 0: nothing usable
};
inline TuneVerdict tune_verdict(const float* ms, const int* cand, int nc) {
    TuneVerdict v;
    for (int k = 0; k < nc; ++k) {
        const float* s = ms + k * TUNE_ROUNDS;
        float t = 0;
        for (int r = 1; r < TUNE_ROUNDS; ++r)
            if (s[r] > 0 && (t == 0 || s[r] < t)) t = s[r];
        if (t == 0 && s[0] > 0) t = s[0];
        if (t > 0 && (v.ms == 0 || t < v.ms)) v = {cand[k], t};
    }
    return v;
}

// ---- the cache file's text ----------------------------------------------------------------------------------------------
// One line per verdict: "v1 <device and library id> <workload key, hex> <variant> <its fastest sample, ms>".  Lines are
// appended with one write() each (O_APPEND: ranks of one job may share the file), the last line of a key wins at load.
constexpr int TUNE_LINE = 512;   // bytes of a line with its newline and terminator: a longer one is neither written nor read

inline std::string tune_cache_id(const char* arch, int cus, const char* name, const char* version) {
    std::string id = std::string(arch) + ":" + std::to_string(cus) + ":" + name + ":" + version;
    for (char& ch : id)
        if (ch == ' ' || ch == '\t') ch = '_';
    return id;
}
// -> characters written to line[TUNE_LINE]; 0: it does not fit
inline int tune_cache_format(char* line, const std::string& id, uint64_t key, int variant, float ms) {
    const int n = snprintf(line, TUNE_LINE, "v1 %s %016llx %d %.4f\n", id.c_str(), (unsigned long long)key, variant, ms);
    return n > 0 && n < TUNE_LINE ? n : 0;
}
// a line of this version, written for this device and library
inline bool tune_cache_parse(const char* line, const std::string& id, uint64_t* key, int* variant) {
    char ver[8], dev[320];
    unsigned long long k = 0;
    float ms = 0;
    if (strlen(line) >= (size_t)TUNE_LINE) return false;
    if (sscanf(line, "%7s %319s %llx %d %f", ver, dev, &k, variant, &ms) != 5 || strcmp(ver, "v1") || id != dev) return false;
    *key = (uint64_t)k;
    return true;
}

// ---- the tuner ----------------------------------------------------------------------------------------------------------
// Samples holds the clocks of one workload's nc * TUNE_ROUNDS timed launches:
//   bool landed(int n)   have the first n samples completed (asked once per call, and only while a verdict is due)
//   float ms(int i)      the time of sample i; <= 0: not usable
// and its destructor frees what it holds, so that no route by which an entry goes -- the bound on the table, forget(), another
// candidate list, the tuner's own end -- leaves anything behind.
template <class Samples>
class DecodeTuner {
public:
    static constexpr size_t MAX_KEYS = 64;
    // What this call launches: a verdict ("measured", or an earlier process's: "cache"), the next sample of a candidate
    // (`record` / `slot`: where the owner puts its clocks), or the default variant while samples are in flight.
    struct Step {
        int variant = TUNE_DEFAULT;
        Samples* record = nullptr;
        int slot = -1;
        const char* source = "none";
    };

    // cand[0 .. nc): what plan_candidates offers this call, nc <= TUNE_NCAND.  Once a key has its verdict a call costs one
    // look-up and asks Samples nothing.
    Step step(uint64_t key, const int* cand, int nc) {
        auto it = entries_.find(key);
        if (it != entries_.end() && !(it->second.nc == nc && std::equal(cand, cand + nc, it->second.cand))) {
            entries_.erase(it);   // its samples were of other variants: measure this list
            it = entries_.end();
        }
        if (it == entries_.end()) {
            if (entries_.size() > MAX_KEYS) entries_.clear();   // bounded: forget everything, re-learn
            it = entries_.try_emplace(key).first;
            Entry& e = it->second;
            e.nc = nc;
            std::copy(cand, cand + nc, e.cand);
            // an earlier process (or rank) has timed this workload on this device: launch its choice from call 1
            const auto hit = cached_.find(key);
            if (hit != cached_.end() && std::find(cand, cand + nc, hit->second) != cand + nc) e.best = hit->second, e.from_cache = true;
        }
        Entry& e = it->second;
        const int ns = nc * TUNE_ROUNDS;
        if (e.best == MEASURING && e.calls >= ns && e.samples.landed(ns)) {   // every sample is queued: have they landed?
            float ms[TUNE_SAMPLES];
            for (int i = 0; i < ns; ++i) ms[i] = e.samples.ms(i);
            const TuneVerdict v = tune_verdict(ms, cand, nc);
            e.best = v.variant;
            append(key, v);
        }
        if (e.best != MEASURING) return {e.best, nullptr, -1, e.from_cache ? "cache" : "measured"};
        if (e.calls >= ns) return {TUNE_DEFAULT, nullptr, -1, "measuring"};
        const int slot = e.calls++;
        return {cand[slot / TUNE_ROUNDS], &e.samples, slot, "measuring"};
    }

    // knob `retune`: what was learnt and what the cache file said are void; the next verdicts are appended anew
    void forget() {
        entries_.clear();
        cached_.clear();
    }

    // Verdicts persist in `path` under `id` (tune_cache_id); an empty path switches that off.  A file that cannot be read, or
    // later written, is not an error of the decode.
    void set_cache(const std::string& path, const std::string& id) {
        cached_.clear();
        path_ = path;
        id_ = id;
        FILE* f = path.empty() ? nullptr : fopen(path.c_str(), "r");
        if (!f) return;
        char line[TUNE_LINE];
        bool tail = false;   // this piece continues a line longer than the buffer
        while (fgets(line, sizeof line, f)) {
            const bool whole = strchr(line, '\n') || feof(f);
            uint64_t key = 0;
            int variant = 0;
            if (whole && !tail && tune_cache_parse(line, id_, &key, &variant)) cached_[key] = variant;
            tail = !whole;
        }
        fclose(f);
    }

    size_t size() const { return entries_.size(); }

private:
    static constexpr int MEASURING = -2;
    struct Entry {
        int best = MEASURING;   // else 0: narrow; 128 / 256: wide; 1000 + tile width: the persistent kernel
        int calls = 0;
        bool from_cache = false;   // `best` was read from the cache file, not timed by this tuner
        int nc = 0, cand[TUNE_NCAND] = {};   // the list the samples belong to
        Samples samples;
    };
    void append(uint64_t key, const TuneVerdict& v) {
        if (path_.empty()) return;
        cached_[key] = v.variant;
        char line[TUNE_LINE];
        const int n = tune_cache_format(line, id_, key, v.variant, v.ms);
        if (!n) return;
        const int fd = open(path_.c_str(), O_WRONLY | O_APPEND | O_CREAT, 0644);
        if (fd < 0) return;
        (void)!write(fd, line, (size_t)n);
        close(fd);
    }
    std::map<uint64_t, Entry> entries_;
    std::string path_, id_;
    std::map<uint64_t, int> cached_;   // key -> variant, as loaded and as appended
};

#pragma GCC visibility pop
}  // namespace ouster_hip_dev
