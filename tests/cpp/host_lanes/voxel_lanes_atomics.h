// The two integer atomics k_voxel_insert uses, for the host-lanes build (hip/hip_runtime.h beside this file has none): lanes are
// real threads there, so these are real atomics.  Included before the kernel source by tests/cpp/voxel_lanes.cpp.
#pragma once
#include <atomic>

inline int atomicCAS(int* address, int compare, int val) {
    std::atomic_ref<int> r(*address);
    r.compare_exchange_strong(compare, val);
    return compare;   // the value found, as on the device
}

inline int atomicMin(int* address, int val) {
    std::atomic_ref<int> r(*address);
    int old = r.load();
    while (old > val && !r.compare_exchange_weak(old, val)) {
    }
    return old;
}
