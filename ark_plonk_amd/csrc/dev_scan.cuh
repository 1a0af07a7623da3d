// Exclusive scan of an integer vector on the device, defined once (lookup.hip: bucket parities and offsets; compile.hip: the digit counts
// of a radix pass): chunk sums, the scan of the sums by one workgroup, then every chunk on top of its sum.  A chunk is THREADS * ITEMS
// consecutive values, ITEMS per lane; the caller picks the geometry.
#pragma once
#include "zk_common.h"

namespace {

template <class T, uint32_t THREADS>
ZK_D T scan_block_inclusive(T x, T* sh) {
    const uint32_t t = threadIdx.x;
    sh[t] = x;
    __syncthreads();
    for (uint32_t d = 1; d < THREADS; d <<= 1) {
        const T v = t >= d ? sh[t - d] : T(0);
        __syncthreads();
        x += v;
        sh[t] = x;
        __syncthreads();
    }
    return x;
}
// exclusive scan of in[base, base + THREADS * ITEMS) (clipped to len) on top of `carry`, to the same places of out; returns the chunk's sum
template <class T, uint32_t THREADS, uint32_t ITEMS>
ZK_D T scan_chunk(const T* in, T* out, uint64_t base, uint64_t len, T carry, T* sh, bool write) {
    const uint32_t t = threadIdx.x;
    T v[ITEMS], s = 0;
#pragma unroll
    for (uint32_t i = 0; i < ITEMS; ++i) {
        const uint64_t idx = base + (uint64_t)t * ITEMS + i;
        v[i] = idx < len ? in[idx] : T(0);
        s += v[i];
    }
    const T incl = scan_block_inclusive<T, THREADS>(s, sh);
    const T total = sh[THREADS - 1];
    __syncthreads();                                       // sh is reused by the caller's next chunk
    if (write) {
        T run = carry + incl - s;
#pragma unroll
        for (uint32_t i = 0; i < ITEMS; ++i) {
            const uint64_t idx = base + (uint64_t)t * ITEMS + i;
            if (idx < len) out[idx] = run;
            run += v[i];
        }
    }
    return total;
}
template <class T, uint32_t THREADS, uint32_t ITEMS>
__global__ void __launch_bounds__(THREADS) scan_sums(const T* in, uint64_t len, T* sums) {
    __shared__ T sh[THREADS];
    const T total = scan_chunk<T, THREADS, ITEMS>(in, nullptr, (uint64_t)blockIdx.x * THREADS * ITEMS, len, T(0), sh, false);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// one workgroup, chunk after chunk: any number of sums
template <class T, uint32_t THREADS, uint32_t ITEMS>
__global__ void __launch_bounds__(THREADS) scan_top(T* sums, uint64_t n_chunks, T* total) {
    __shared__ T sh[THREADS];
    T carry = 0;
    for (uint64_t base = 0; base < n_chunks; base += THREADS * ITEMS)
        carry += scan_chunk<T, THREADS, ITEMS>(sums, sums, base, n_chunks, carry, sh, true);
    if (total && threadIdx.x == 0) *total = carry;
}
template <class T, uint32_t THREADS, uint32_t ITEMS>
__global__ void __launch_bounds__(THREADS) scan_apply(const T* in, T* out, uint64_t len, const T* sums) {
    __shared__ T sh[THREADS];
    scan_chunk<T, THREADS, ITEMS>(in, out, (uint64_t)blockIdx.x * THREADS * ITEMS, len, sums[blockIdx.x], sh, true);
}

// n >= 1.  out[i] = in[0] + ... + in[i - 1], i < n; *total (unless null) = the sum of all n.  in == out is allowed: a chunk is read whole by the
// workgroup that writes it.  sums: one T per chunk.  The caller reads hipGetLastError.
template <class T, uint32_t THREADS, uint32_t ITEMS>
void scan_excl(const T* in, T* out, uint64_t n, T* sums, T* total, hipStream_t st) {
    const uint64_t n_chunks = (n + THREADS * ITEMS - 1) / (THREADS * ITEMS);
    hipLaunchKernelGGL((scan_sums<T, THREADS, ITEMS>), dim3((unsigned)n_chunks), dim3(THREADS), 0, st, in, n, sums);
    hipLaunchKernelGGL((scan_top<T, THREADS, ITEMS>), dim3(1), dim3(THREADS), 0, st, sums, n_chunks, total);
    hipLaunchKernelGGL((scan_apply<T, THREADS, ITEMS>), dim3((unsigned)n_chunks), dim3(THREADS), 0, st, in, out, n, (const T*)sums);
}

}  // namespace
