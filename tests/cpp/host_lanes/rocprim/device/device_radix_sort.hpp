// Stand-in for the one rocPRIM sort the run functions of csrc call -- rocprim::radix_sort_pairs -- for the host-lanes build
// (hip/hip_runtime.h beside this directory).  Like the device's: stable, ascending, and blind to every bit of a key outside
// [begin_bit, end_bit) -- a caller that passes too few bits gets the order that mistake gives on the device.
#pragma once
#include <hip/hip_runtime.h>

#include <numeric>

#include "device_scan.hpp"

namespace rocprim {

template <class Key, class Value>
hipError_t radix_sort_pairs(void* temp, size_t& bytes, const Key* keys_in, Key* keys_out, const Value* values_in, Value* values_out,
                            size_t n, unsigned begin_bit = 0, unsigned end_bit = 8 * sizeof(Key), hipStream_t = nullptr) {
    if (!temp) {
        bytes = host_lanes_temp_bytes;
        return hipSuccess;
    }
    if (bytes < host_lanes_temp_bytes || begin_bit >= end_bit || end_bit > 8 * sizeof(Key)) return hipErrorInvalidValue;
    const unsigned width = end_bit - begin_bit;
    const Key mask = width == 8 * sizeof(Key) ? ~Key(0) : (Key)((Key(1) << width) - 1);
    auto digits = [&](size_t i) { return (Key)((keys_in[i] >> begin_bit) & mask); };
    std::vector<size_t> order(n);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return digits(x) < digits(y); });
    for (size_t p = 0; p < n; ++p) keys_out[p] = keys_in[order[p]], values_out[p] = values_in[order[p]];
    return hipSuccess;
}

}  // namespace rocprim
