/* Stand-in for <cub/cub.cuh>: the two device-wide primitives the rasterizer calls, on the host.
 * Both follow CUB's calling convention: a first call with d_temp_storage == nullptr only reports a size. */
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <vector>
#include "../ref_shim.h"

namespace cub {
struct DeviceScan {
    template <class In, class Out>
    static cudaError_t InclusiveSum(void* d_temp_storage, size_t& temp_storage_bytes, In d_in, Out d_out, int num_items)
    {
        if (d_temp_storage == nullptr) { temp_storage_bytes = 1; return cudaSuccess; }
        std::remove_cv_t<std::remove_reference_t<decltype(d_out[0])>> run = 0;
        for (int i = 0; i < num_items; i++) { run += d_in[i]; d_out[i] = run; }
        return cudaSuccess;
    }
};
struct DeviceRadixSort {
    /* stable, ascending, on key bits [begin_bit, end_bit) only */
    template <class K, class V>
    static cudaError_t SortPairs(void* d_temp_storage, size_t& temp_storage_bytes, const K* d_keys_in, K* d_keys_out,
                                 const V* d_values_in, V* d_values_out, int num_items, int begin_bit = 0,
                                 int end_bit = sizeof(K) * 8)
    {
        if (d_temp_storage == nullptr) { temp_storage_bytes = 1; return cudaSuccess; }
        const int bits = end_bit - begin_bit;
        const K mask = bits >= (int)sizeof(K) * 8 ? ~K(0) : (K(1) << bits) - 1;
        std::vector<int> order(num_items);
        for (int i = 0; i < num_items; i++) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
            return ((d_keys_in[a] >> begin_bit) & mask) < ((d_keys_in[b] >> begin_bit) & mask);
        });
        for (int i = 0; i < num_items; i++) { d_keys_out[i] = d_keys_in[order[i]]; d_values_out[i] = d_values_in[order[i]]; }
        return cudaSuccess;
    }
};
}  // namespace cub
