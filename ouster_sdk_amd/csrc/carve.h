// carve.h -- lays a workspace out as consecutive pieces, each 256-byte aligned.  Plain C++, no HIP (tests/cpp/test_carve.cpp).
// A layout is written once, as a function of a Carver, and run twice: over no base to learn `total`, then -- once a buffer of
// that size exists -- over its base to get the pointers.  Offsets are computed on integers; without a base take() returns NULL.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ouster_hip_dev {

struct Carver {
    uintptr_t base = 0;   // 0: measure only
    size_t total = 0;     // bytes taken so far, a multiple of 256
    explicit Carver(void* p = nullptr) : base(reinterpret_cast<uintptr_t>(p)) {}
    template <class T>
    T* take(size_t count) {
        const size_t at = total;
        total += (count * sizeof(T) + 255) & ~(size_t)255;
        return base ? reinterpret_cast<T*>(base + at) : nullptr;
    }
};

}  // namespace ouster_hip_dev
