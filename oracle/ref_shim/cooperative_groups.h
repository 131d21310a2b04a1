/* Stand-in for <cooperative_groups.h>: the grid's thread rank and the thread block of the fiber that is running. */
#pragma once
#include "ref_shim.h"

namespace cooperative_groups {
struct grid_group {
    unsigned long long thread_rank() const
    {
        const ref_shim::Position& p = ref_shim::pos;
        const unsigned long long block = ((unsigned long long)p.blockIdx.z * p.gridDim.y + p.blockIdx.y) * p.gridDim.x + p.blockIdx.x;
        return block * ((unsigned long long)p.blockDim.x * p.blockDim.y * p.blockDim.z) + ref_shim::thread_rank_in_block();
    }
};
struct thread_block {
    void sync() const { ref_shim::barrier(); }
    unsigned int thread_rank() const { return ref_shim::thread_rank_in_block(); }
    dim3 group_index() const { return ref_shim::pos.blockIdx; }
    dim3 thread_index() const { return ref_shim::pos.threadIdx; }
};
inline grid_group this_grid() { return grid_group(); }
inline thread_block this_thread_block() { return thread_block(); }
}  // namespace cooperative_groups

/* The compositor's exponential.  The rasterizer's sources include this header after glm and after the standard headers,
 * so the function-like macros below reach only the rasterizer's own unqualified calls: exp / expf of a float go to the
 * fixed-sequence expf the oracle and the HIP kernels share, which is what lets the forward be compared bit for bit. */
#define exp(x) ref_shim::exp_(x)
#define expf(x) ref_shim::exp_((float)(x))
