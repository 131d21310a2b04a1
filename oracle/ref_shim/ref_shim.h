/*
 * ref_shim.h -- TEST INFRASTRUCTURE ONLY.  Our own code: the slice of the CUDA runtime that a tile rasterizer written for
 * nvcc needs in order to be compiled by a host C++ compiler and RUN on one OS thread (oracle/ref_build.py, oracle/ref_glue.cpp).
 *
 *   - vector types, dim3, the mixed-sign min / max overloads of CUDA's math headers, atomicAdd, cudaMemcpy / cudaMemset;
 *   - launch(kernel, grid, block, args...): the ordinary call that `kernel<<<grid, block>>>(args...)` is rewritten into.
 *     A grid runs one block at a time, a block's threads are fibers (ucontext) that run in thread-rank order; a barrier
 *     hands over to the next fiber and everybody resumes once every live fiber has arrived (a fiber that returned counts
 *     as arrived).  One thread, one block at a time: `__shared__` is `static`, atomicAdd is a plain add, every run gives
 *     the same bits.
 *   - exp on float is the fixed-sequence expf of oracle/sks_oracle.c (set through ref_shim_set_expf); sqrt, division and
 *     ceil are the host's IEEE ones.  Build with -ffp-contract=off -fno-fast-math.
 */
#pragma once
#include <math.h>   /* (the C++ wrapper: ::sqrt(float), ::ceil(float) ... as in CUDA, not only the double ones) */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <ucontext.h>

#include <functional>
#include <tuple>
#include <utility>

#define __global__ static
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(...)

struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
struct int2 { int x, y; };
struct uint2 { unsigned int x, y; };
struct dim3 {
    unsigned int x, y, z;
    dim3(unsigned int x_ = 1, unsigned int y_ = 1, unsigned int z_ = 1) : x(x_), y(y_), z(z_) {}
};

enum cudaError_t { cudaSuccess = 0 };
enum cudaMemcpyKind { cudaMemcpyHostToHost, cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost, cudaMemcpyDeviceToDevice };
inline cudaError_t cudaDeviceSynchronize() { return cudaSuccess; }
inline const char* cudaGetErrorString(cudaError_t) { return "no error"; }
inline cudaError_t cudaMemcpy(void* dst, const void* src, size_t n, cudaMemcpyKind) { memcpy(dst, src, n); return cudaSuccess; }
inline cudaError_t cudaMemset(void* dst, int v, size_t n) { memset(dst, v, n); return cudaSuccess; }
inline void __trap() { abort(); }

/* CUDA's min / max: fminf / fmaxf on floats, and an unsigned result whenever one side is unsigned. */
inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }
inline unsigned int min(unsigned int a, unsigned int b) { return a < b ? a : b; }
inline unsigned int max(unsigned int a, unsigned int b) { return a > b ? a : b; }
inline unsigned int min(unsigned int a, int b) { return min(a, (unsigned int)b); }
inline unsigned int min(int a, unsigned int b) { return min((unsigned int)a, b); }
inline unsigned int max(unsigned int a, int b) { return max(a, (unsigned int)b); }
inline unsigned int max(int a, unsigned int b) { return max((unsigned int)a, b); }
inline float min(float a, float b) { return fminf(a, b); }
inline float max(float a, float b) { return fmaxf(a, b); }
inline double min(double a, double b) { return fmin(a, b); }
inline double max(double a, double b) { return fmax(a, b); }

/* One thread, one block at a time: nothing to be atomic against. */
inline float atomicAdd(float* address, float val) { const float old = *address; *address = old + val; return old; }

extern "C" void ref_shim_set_expf(float (*f)(float));

namespace ref_shim {

struct Position { dim3 gridDim, blockDim, blockIdx, threadIdx; };

constexpr int MAX_BLOCK_THREADS = 1024;
constexpr size_t FIBER_STACK_BYTES = 256 * 1024;

struct Fiber { ucontext_t uc; dim3 threadIdx; bool live; };

/* one scheduler for all translation units (C++17 inline variables) */
inline Position pos;
inline float (*expf_impl)(float) = nullptr;
inline Fiber* fibers = nullptr;
inline char* stacks = nullptr;
inline ucontext_t scheduler_uc;
inline int running = -1;
inline const std::function<void()>* body = nullptr;
inline int votes = 0, votes_result = 0;

inline float exp_(float x)
{
    if (!expf_impl) { fprintf(stderr, "ref_shim: ref_shim_set_expf was not called\n"); abort(); }
    return expf_impl(x);
}
inline double exp_(double x) { return ::exp(x); }

inline unsigned int thread_rank_in_block()
{
    return (pos.threadIdx.z * pos.blockDim.y + pos.threadIdx.y) * pos.blockDim.x + pos.threadIdx.x;
}

/* block.sync(): arrive, run everybody else up to the same point, go on */
inline void barrier() { swapcontext(&fibers[running].uc, &scheduler_uc); }

/* __syncthreads_count: a barrier that also returns how many arrivals brought a non-zero predicate.
 * Assumes what CUDA demands of the call: every live fiber of the block reaches the SAME __syncthreads_count in the same pass.
 * A plain sync() mixed into that pass, or a fiber that returned before it, would not vote and would change the count in
 * silence (CUDA leaves both undefined); the rasterizer's renderCUDA, its only caller, does neither. */
inline int barrier_count(int predicate)
{
    votes += predicate != 0;
    barrier();
    return votes_result;   /* set by the scheduler when the pass that collected the votes ended */
}

inline void fiber_main()
{
    (*body)();
    fibers[running].live = false;   /* uc_link returns to the scheduler */
}

inline void run_block(const std::function<void()>& f)
{
    const int n = (int)(pos.blockDim.x * pos.blockDim.y * pos.blockDim.z);
    if (n > MAX_BLOCK_THREADS) { fprintf(stderr, "ref_shim: block of %d threads\n", n); abort(); }
    if (!fibers) {
        fibers = new Fiber[MAX_BLOCK_THREADS];
        stacks = (char*)malloc(FIBER_STACK_BYTES * MAX_BLOCK_THREADS);
        if (!stacks) abort();
    }
    body = &f;
    votes = votes_result = 0;
    int i = 0;
    for (unsigned z = 0; z < pos.blockDim.z; z++)
        for (unsigned y = 0; y < pos.blockDim.y; y++)
            for (unsigned x = 0; x < pos.blockDim.x; x++, i++) {
                Fiber& fb = fibers[i];
                getcontext(&fb.uc);
                fb.uc.uc_stack.ss_sp = stacks + FIBER_STACK_BYTES * (size_t)i;
                fb.uc.uc_stack.ss_size = FIBER_STACK_BYTES;
                fb.uc.uc_link = &scheduler_uc;
                makecontext(&fb.uc, fiber_main, 0);
                fb.threadIdx = dim3(x, y, z);
                fb.live = true;
            }
    /* One pass resumes every live fiber once, in rank order; each runs to its next barrier or to its end.  When the pass
     * is over every live fiber has arrived, so the next pass is the release. */
    for (int live = n; live > 0;) {
        live = 0;
        for (i = 0; i < n; i++) {
            if (!fibers[i].live) continue;
            running = i;
            pos.threadIdx = fibers[i].threadIdx;
            swapcontext(&scheduler_uc, &fibers[i].uc);
            live += fibers[i].live;
        }
        votes_result = votes;
        votes = 0;
    }
    running = -1;
    body = nullptr;
}

/* `kernel<<<grid, block>>>(args...)` */
template <class... Params, class... Args>
void launch(void (*kernel)(Params...), dim3 grid, dim3 block, Args&&... args)
{
    std::tuple<Params...> params(std::forward<Args>(args)...);   /* the conversions a call would make */
    const std::function<void()> f = [&] { std::apply(kernel, params); };
    pos.gridDim = grid;
    pos.blockDim = block;
    for (unsigned z = 0; z < grid.z; z++)
        for (unsigned y = 0; y < grid.y; y++)
            for (unsigned x = 0; x < grid.x; x++) {
                pos.blockIdx = dim3(x, y, z);
                run_block(f);
            }
}

}  // namespace ref_shim

inline int __syncthreads_count(int predicate) { return ref_shim::barrier_count(predicate); }
inline void __syncthreads() { ref_shim::barrier(); }
