// The integer atomics k_tm_hist uses -- an add on a workgroup's histogram and an add on the tile's global one, both on uint32_t --
// for the host-lanes build (hip/hip_runtime.h beside this file has none): lanes are real threads there, so this is a real atomic.
// Included before the kernel source by tests/cpp/tonemap_lanes.cpp.
#pragma once
#include <atomic>
#include <cstdint>

inline uint32_t atomicAdd(uint32_t* address, uint32_t val) {
    return std::atomic_ref<uint32_t>(*address).fetch_add(val);
}
