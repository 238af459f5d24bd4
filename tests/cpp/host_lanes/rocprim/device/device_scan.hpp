// Stand-in for the one rocPRIM scan the run functions of csrc call -- rocprim::exclusive_scan with rocprim::plus -- for the
// host-lanes build (hip/hip_runtime.h beside this directory).  The calling convention is rocPRIM's: temp == nullptr asks for the
// bytes of temporary storage, anything else runs the scan and wants that many.
#pragma once
#include <hip/hip_runtime.h>

namespace rocprim {

constexpr size_t host_lanes_temp_bytes = 64;   // small and not zero: a caller that skips the size query is refused

template <class T>
struct plus {
    T operator()(const T& a, const T& b) const { return a + b; }
};

template <class In, class Out, class T, class Op>
hipError_t exclusive_scan(void* temp, size_t& bytes, In in, Out out, T initial, size_t n, Op op, hipStream_t = nullptr) {
    if (!temp) {
        bytes = host_lanes_temp_bytes;
        return hipSuccess;
    }
    if (bytes < host_lanes_temp_bytes) return hipErrorInvalidValue;
    T run = initial;
    for (size_t i = 0; i < n; ++i) {
        const T v = in[i];   // read first: in and out may be one array
        out[i] = run;
        run = op(run, v);
    }
    return hipSuccess;
}

}  // namespace rocprim
