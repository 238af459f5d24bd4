// hip_runtime.h stand-in for the *_lanes.cpp programs of tests/cpp: just enough of the HIP launch model to run a kernel's source
// -- and the library's run functions around it -- on the CPU.
// Every lane of a workgroup is a thread of its own (threadIdx / blockIdx are thread-local), __syncthreads() is a real barrier,
// __shared__ is one function-local static object -- safe only because workgroups run one after the other here, never two at
// a time --, a launch returns when its grid is done, so a stream is the order of the calls: hipMemsetAsync is a memset and an
// event records nothing.  The integer atomics are real atomics, since the lanes are real threads.  For checking
// index arithmetic, the order of the steps and the order of floating-point operations against a model without a GPU; it says
// nothing about the device's own division and square root.
// OUSTER_HOST_LANES tells csrc/k_voxel.h that rocPRIM's scan and radix sort have stand-ins here too (rocprim/device/ beside hip/).
#pragma once
#define OUSTER_HOST_LANES 1
#include <algorithm>
#include <atomic>
#include <barrier>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

struct dim3 {
    unsigned x, y, z;
    dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
inline thread_local dim3 threadIdx, blockIdx;
inline std::barrier<>* host_lanes_barrier = nullptr;
#define __syncthreads() host_lanes_barrier->arrive_and_wait()
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __shared__ static
#define __constant__ static const
using std::max;
using std::min;
typedef int hipError_t;
typedef void* hipStream_t;
typedef void* hipEvent_t;
constexpr int hipSuccess = 0, hipErrorInvalidValue = 1;
inline hipError_t hipGetLastError() { return hipSuccess; }
inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
inline hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t) {
    std::memset(dst, value, bytes);
    return hipSuccess;
}

template <class K, class... A>
void hipLaunchKernelGGL(K kernel, dim3 grid, dim3 wg, size_t, hipStream_t, A... args) {
    const unsigned n = wg.x * wg.y * wg.z;
    for (unsigned bz = 0; bz < grid.z; ++bz)
        for (unsigned by = 0; by < grid.y; ++by)
            for (unsigned bx = 0; bx < grid.x; ++bx) {
                std::barrier<> bar(n);
                host_lanes_barrier = &bar;
                std::vector<std::thread> lanes;
                for (unsigned t = 0; t < n; ++t)
                    lanes.emplace_back([=] {
                        threadIdx = dim3(t % wg.x, (t / wg.x) % wg.y, t / (wg.x * wg.y));
                        blockIdx = dim3(bx, by, bz);
                        kernel(args...);
                    });
                for (auto& l : lanes) l.join();
            }
}

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

inline uint32_t atomicAdd(uint32_t* address, uint32_t val) { return std::atomic_ref<uint32_t>(*address).fetch_add(val); }

inline unsigned long long atomicAdd(unsigned long long* address, unsigned long long val) {
    return std::atomic_ref<unsigned long long>(*address).fetch_add(val);
}

inline long long __double_as_longlong(double v) {
    long long r;
    std::memcpy(&r, &v, sizeof r);
    return r;
}
