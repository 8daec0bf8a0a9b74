// The fixed-order reductions of the bandwidth-bound kernels: butterfly inside a wave, one hop through LDS, the waves' results
// combined in a STATED order.  The order is what the bit-identity of repeated runs (and of a refactor) rests on, so the two orders
// in use have two names: CHAIN, red[0] + red[1] + ..., and TREE (four waves), (red[0] + red[1]) + (red[2] + red[3]).
// DESIGN.md ("Fixed-order reductions") lists which kernel uses which.
// Device only; the library is built with -fno-gpu-rdc: everything here is in an anonymous namespace and each including file gets
// its own instance.
#pragma once
#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ float max2(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ unsigned max2(unsigned a, unsigned b) { return max(a, b); }

// ---- inside a wave: the 32, 16, ..., 1 xor butterfly at width 64; every lane ends with the wave's result
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max2(v, __shfl_xor(v, off, 64));
    return v;
}

// ---- across the waves of a workgroup: lane 0 of every wave puts the wave's result into red[wave] ...
template <typename T>
__device__ __forceinline__ void wave_store(T v, T* red) {
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
}
// ... and, behind a barrier, any thread combines the NW results in one of the two orders
template <int NW, typename T>
__device__ __forceinline__ T chain_sum(const T* red) {
    T s = red[0];
#pragma unroll
    for (int k = 1; k < NW; ++k) s += red[k];
    return s;
}
template <typename T>
__device__ __forceinline__ T tree_sum4(const T* red) { return (red[0] + red[1]) + (red[2] + red[3]); }
template <typename T>
__device__ __forceinline__ T tree_max4(const T* red) { return max2(max2(red[0], red[1]), max2(red[2], red[3])); }

// ---- store, barrier, combine in one call, for a value that is already the wave's result; the same value in every thread.
// red is free for the next reduction once every thread has passed another barrier.  (Two values that share one barrier use
// wave_store twice, __syncthreads() and the combine of their choice.)
template <int NW, typename T>
__device__ __forceinline__ T block_chain_sum(T wave_v, T* red) {
    wave_store(wave_v, red);
    __syncthreads();
    return chain_sum<NW>(red);
}
template <typename T>
__device__ __forceinline__ T block_tree_sum4(T wave_v, T* red) {
    wave_store(wave_v, red);
    __syncthreads();
    return tree_sum4(red);
}
template <typename T>
__device__ __forceinline__ T block_tree_max4(T wave_v, T* red) {
    wave_store(wave_v, red);
    __syncthreads();
    return tree_max4(red);
}

// Sum of v over the NT threads of a workgroup, CHAIN order, the same value in every thread.  red: NT / 64 elements of LDS; two
// calls may share it (the leading barrier protects the previous call's reads).
template <typename T, int NT>
__device__ __forceinline__ T block_sum(T v, T* red) {
    v = wave_sum(v);
    __syncthreads();
    return block_chain_sum<NT / 64>(v, red);
}

}  // namespace
