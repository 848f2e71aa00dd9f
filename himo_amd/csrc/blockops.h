// blockops.h -- the ONE statement of the kernels' fixed-order reductions, scans and segment search (device code only).
//
// The order of the float64 additions below is part of several stages' written rules -- it is what "the same inputs give the same
// bytes on every run" rests on ("The fixed summation orders and the segment search", lists the stages): change a loop
// here and those stages change their bytes.  Nothing in this file multiplies -- the helpers add, compare and shuffle -- so they mean
// the same under every -ffp-contract setting.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace himo {

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// largest k in [0, n) with offsets[k] <= i   (i < offsets[n]): the segment (sweep, cluster) that owns packed row i; segments
// without rows are passed over
__device__ inline int segment_of(const int64_t* __restrict__ offsets, int n, int64_t i) {
    int lo = 0, hi = n;   // invariant: offsets[lo] <= i < offsets[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- one wave ------------------------------------------------------------------------------------------------------------------
// sum over the wave as an xor butterfly 32, 16, ... 1: every lane ends with the same bits (the additions of a stage are the same
// pairs whichever lane makes them), on every launch.  int, unsigned, the 64-bit integers and double.
template <typename T> __device__ inline T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// two sums at once, stage by stage (the two shuffles of a stage are independent and issue back to back)
template <typename A, typename B> __device__ inline void wave_sum2(A& a, B& b) {
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off, 64); b += __shfl_xor(b, off, 64); }
}

__device__ inline unsigned long long shfl_xor_u64(unsigned long long v, int m) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, m, 64);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), m, 64);
    return ((unsigned long long)hi << 32) | lo;
}

// maximum of 64-bit keys over the wave, in every lane (also of non-negative doubles, whose bit patterns order as they do)
__device__ inline unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
        const unsigned long long o = shfl_xor_u64(v, w);
        v = o > v ? o : v;
    }
    return v;
}

// lane l: the sum of lanes 0 .. l
__device__ inline int wave_inclusive_scan(int v) {
    const int lane = threadIdx.x & 63;
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(v, off, 64);
        if (lane >= off) v += y;
    }
    return v;
}

// the first wave of a block (threads 0 .. 63 call it): the sum of the tile totals before this block's, and of all gridDim.x of them
__device__ inline void tiles_before_and_all(const int* __restrict__ tile_sum, int& before, int& all) {
    before = 0; all = 0;
    for (int t = threadIdx.x; t < (int)gridDim.x; t += 64) {
        const int x = tile_sum[t];
        all += x;
        if (t < (int)blockIdx.x) before += x;
    }
    wave_sum2(before, all);
}

// ---- one block -----------------------------------------------------------------------------------------------------------------
// K sums over the NT threads of a block as the fixed LDS tree NT/2, NT/4, ... 1 (the same bytes on every run); thread 0 writes
// out[0 .. K).  No leading barrier: the buffer is the function's own, so a kernel calls this ONCE.
template <int NT, int K> __device__ inline void block_sum(const double (&v)[K], double* out) {
    __shared__ double red[K][NT];
#pragma unroll
    for (int k = 0; k < K; ++k) red[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
#pragma unroll
            for (int k = 0; k < K; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) out[k] = red[k][0];
}
template <int NT> __device__ inline void block_sum(double v, double* out) {
    const double one[1] = {v};
    block_sum<NT, 1>(one, out);
}

// The sum / maximum over a GROUP of NT threads, returned to every thread of it.  NT == 64: the group is a wave, the butterfly
// above, no barrier and sh unused.  Otherwise the group is the block: the same fixed tree through the caller's sh[NT], which may be
// reused from call to call -- the leading barrier is what lets the previous call's readers of sh[0] finish first.
template <int NT> __device__ inline double group_sum(double v, double* sh) {
    if constexpr (NT == 64) {
        return wave_sum(v);
    } else {
        __syncthreads();
        sh[threadIdx.x] = v;
        __syncthreads();
#pragma unroll
        for (int s = NT / 2; s >= 1; s >>= 1) {
            if ((int)threadIdx.x < s) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + s];
            __syncthreads();
        }
        return sh[0];
    }
}
template <int NT> __device__ inline unsigned long long group_max_u64(unsigned long long v, unsigned long long* sh) {
    if constexpr (NT == 64) {
        return wave_max_u64(v);
    } else {
        __syncthreads();
        sh[threadIdx.x] = v;
        __syncthreads();
#pragma unroll
        for (int s = NT / 2; s >= 1; s >>= 1) {
            if ((int)threadIdx.x < s) sh[threadIdx.x] = sh[threadIdx.x] > sh[threadIdx.x + s] ? sh[threadIdx.x] : sh[threadIdx.x + s];
            __syncthreads();
        }
        return sh[0];
    }
}

// Hillis-Steele inclusive scan of one value per thread over the NT threads of a block, through the caller's part[NT]: returns
// part[threadIdx.x] = x of threads 0 .. threadIdx.x.  Ends on a barrier, so any thread may read all of part[] afterwards; the caller
// puts a barrier before the next call.
template <int NT> __device__ inline int block_inclusive_scan(int x, int* part) {
    part[threadIdx.x] = x;
    __syncthreads();
    for (int off = 1; off < NT; off <<= 1) {
        const int y = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += y;
        __syncthreads();
    }
    return part[threadIdx.x];
}

}  // namespace himo
