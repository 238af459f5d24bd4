// What the *_lanes.cpp programs share besides the stand-in headers: reading a case file, writing a result file, and launching a
// closure once per lane (for a device function that is not a kernel of its own, such as reg_thread_rows).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>

static inline bool rd(void* p, size_t bytes, FILE* f) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
static inline void wr(const void* p, size_t bytes, FILE* f) {
    if (bytes) std::fwrite(p, 1, bytes, f);
}

template <class F>
static void run_lanes(dim3 grid, dim3 wg, F f) {
    hipLaunchKernelGGL(+[](F* g) { (*g)(); }, grid, wg, 0, nullptr, &f);
}
