// wave.h — the cross-lane building blocks of the device modules, one definition each: wave reductions and scan, the wave- and
// workgroup-aggregated append, the workgroup sum and scan and the ordered (deterministic) fp64 grid reduction.  Wave64,
// one-dimensional workgroups of whole waves.  scan.h builds the one-workgroup scan of the chunk sums on the workgroup scan.  The
// stage kernels keep their own code and do not include this file; lsm_comm.hip keeps its own sum and scan of chunk counts.
#pragma once
#include <hip/hip_runtime.h>

namespace lsm {

// ---- reductions over the wave, the result in every lane: the xor butterfly from offset 32 down to 1.  The order is fixed; it is
// what makes the fp64 sums bitwise reproducible.  Every lane of the wave calls these.
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
template <class T>
__device__ __forceinline__ T wave_or(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off, 64);
    return v;
}
// NaN-dropping where the other operand is a number (the comparisons are false for NaN): callers reduce an "any NaN" flag separately
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// inclusive prefix sum over the wave: lane l gets v_0 + … + v_l.  Every lane of the wave calls this.
template <class T>
__device__ __forceinline__ T wave_incl_scan(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(v, d, 64);
        if (lane >= d) v += y;
    }
    return v;
}

// the sum of v over a workgroup of NWAVES waves, in every thread: one barrier, no atomics.  wsum: NWAVES words of LDS, which the
// caller leaves alone until the workgroup's next barrier.  Every thread of the workgroup calls this.
template <int NWAVES, class T>
__device__ __forceinline__ T block_sum(T v, T* wsum) {
    const T s = wave_sum(v);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    T total = 0;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) total += wsum[w];
    return total;
}

// exclusive prefix sum of v over a workgroup of NWAVES waves, and its total in every thread.  wsum as for block_sum.  Every
// thread of the workgroup calls this.
template <int NWAVES, class T>
__device__ __forceinline__ T block_excl_scan(T v, T* wsum, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T incl = wave_incl_scan(v);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    T excl = incl - v;
    total = 0;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) {
        const T s = wsum[w];
        if (w < wave) excl += s;
        total += s;
    }
    return excl;
}

// ---- appends to a list whose length is *counter.  The keeping lanes among those active at the call take consecutive slots, in
// lane order, behind ONE atomic per wave (done by the first of them; none where no lane keeps).  Returns the slot of a keeping
// lane; the value means nothing in the others.
__device__ __forceinline__ unsigned wave_append(bool keep, unsigned* counter) {
    const unsigned long long bal = __ballot(keep);
    if (!bal) return 0u;
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)bal) - 1;
    unsigned base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned)__popcll(bal));
    return __shfl(base, leader, 64) + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
}
// The two-level form: the waves append to a counter in LDS, and ONE atomic per workgroup reaches *counter.  EVERY thread of the
// workgroup of THREADS threads must call this (it holds barriers), whole waves active.
template <int THREADS>
__device__ __forceinline__ unsigned block_append(bool keep, unsigned* counter) {
    static_assert(THREADS % 64 == 0, "whole waves");
    __shared__ unsigned blk_n, blk_base;
    const unsigned long long bal = __ballot(keep);
    const int lane = threadIdx.x & 63;
    if (threadIdx.x == 0) blk_n = 0;
    __syncthreads();
    unsigned wbase = 0;
    if (bal && lane == 0) wbase = atomicAdd(&blk_n, (unsigned)__popcll(bal));
    wbase = __shfl(wbase, 0, 64);
    __syncthreads();
    if (threadIdx.x == 0 && blk_n) blk_base = atomicAdd(counter, blk_n);
    __syncthreads();
    return blk_base + wbase + __popcll(bal & ((1ull << lane) - 1ull));
}

// ---- the grid's sum of K fp64 values per thread, deterministic: one partial per workgroup (partial: K · gridDim.x words), and the
// last workgroup to draw a ticket sums the partials in workgroup order.  Returns true in that workgroup only, with the totals in
// v in every thread of it; *ticket is zero on entry and is left zero.  Every thread of the grid's workgroups of THREADS threads
// calls this.
// Memory ordering: thread 0 publishes its workgroup's partials, then takes a ticket — an agent-scope release fence before the
// relaxed add, with the stores drained before and after it; the workgroup that draws the last ticket has therefore every other
// workgroup's partials behind its acquire fence, and only then reads them.
template <int K, int THREADS>
__device__ bool block_reduce_ordered(double (&v)[K], double* partial, unsigned* ticket) {
    static_assert(THREADS == 256, "the wave totals are paired as (0 + 1) + (2 + 3)");
    __shared__ double red[K][THREADS / 64];
    __shared__ int last;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = wave_sum(v[k]);
        if (lane == 0) red[k][wave] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) partial[k * gridDim.x + blockIdx.x] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
        // publish the partials, then take a ticket (agent-scope release before the relaxed add; acquire in the last one)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned tk = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = tk == gridDim.x - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!last) return false;
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        acc[k] = 0.0;
        for (unsigned b = threadIdx.x; b < gridDim.x; b += blockDim.x) acc[k] += partial[k * gridDim.x + b];
    }
    __syncthreads();   // red is reused
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = wave_sum(acc[k]);
        if (lane == 0) red[k][wave] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}

}  // namespace lsm
