// hip_runtime.h stand-in for tests/cpp/normals_lanes.cpp: just enough of the HIP launch model to run a kernel's source on the CPU.
// Every lane of a workgroup is a thread of its own (threadIdx / blockIdx are thread-local), __syncthreads() is a real barrier,
// __shared__ is one function-local static object -- safe only because workgroups run one after the other here, never two at
// a time --, a launch returns when its grid is done.  For checking
// index arithmetic and the order of floating-point operations against a model without a GPU; it says nothing about the device's
// own division and square root.
#pragma once
#include <algorithm>
#include <barrier>
#include <cmath>
#include <cstddef>
#include <cstdint>
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
using std::max;
using std::min;
typedef int hipError_t;
typedef void* hipStream_t;
constexpr int hipSuccess = 0, hipErrorInvalidValue = 1;
inline hipError_t hipGetLastError() { return hipSuccess; }

template <class K, class A>
void hipLaunchKernelGGL(K kernel, dim3 grid, dim3 wg, size_t, hipStream_t, A args) {
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
                        kernel(args);
                    });
                for (auto& l : lanes) l.join();
            }
}
