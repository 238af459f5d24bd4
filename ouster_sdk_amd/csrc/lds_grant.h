// lds_grant.h -- "has this kernel's dynamic-LDS limit been raised on this device to at least `lds` bytes": one LdsGrant per
// kernel, remembered per device so that the steady state makes no runtime call.  No HIP include: `raise` is whatever asks the
// runtime (launch_with_lds, launch_util.h), and tests/cpp/test_lds_grant.cpp runs the bookkeeping on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <atomic>

namespace ouster_hip_dev {

struct LdsGrant {
    static constexpr size_t FREE_BYTES = 48 * 1024;   // dynamic LDS every kernel may have without asking
    static constexpr int MAX_DEVICES = 16;
    std::atomic<uint32_t> bytes[MAX_DEVICES];         // the limit granted so far, per device
    LdsGrant() { for (auto& b : bytes) b.store(0); }

    // raise() -> error code, zero for success (hipError_t).  Called when `lds` exceeds what is known to be granted; a device
    // outside the table is never remembered (asked every time: correct, merely slower) and never aliased onto another one.
    template <class Raise>
    auto ensure(size_t lds, int device, Raise&& raise) -> decltype(raise()) {
        using E = decltype(raise());
        if (lds <= FREE_BYTES) return E{};
        std::atomic<uint32_t>* have = (device >= 0 && device < MAX_DEVICES) ? &bytes[device] : nullptr;
        if (have && have->load(std::memory_order_acquire) >= lds) return E{};
        const E e = raise();
        if (e == E{} && have) have->store((uint32_t)lds, std::memory_order_release);
        return e;
    }
};

}  // namespace ouster_hip_dev
