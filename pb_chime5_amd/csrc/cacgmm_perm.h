// What the exhaustive permutation searches share (cacgmm_align.hip: the classes of one frequency
// against the centroid; cacgmm_link.hip: the classes of one window against the previous one): a
// fixed-order sum over a 256-thread workgroup, the decoder of the K! candidates and the tie rule.
#pragma once

#include "gss_internal.h"

constexpr int ALIGN_WG = 256;

// sum over the workgroup's 256 threads in one fixed order (DPP inside a wave, waves ascending);
// the total is returned to every thread.  `red` holds 4 doubles.
__device__ __forceinline__ double block_sum_256(double v, double *red) {
    const double w = wave_sum(v);
    __syncthreads();                         // (red may still be read from a previous use)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__host__ __device__ constexpr int align_factorial(int n) { return n <= 1 ? 1 : n * align_factorial(n - 1); }

// total of candidate `index` (lexicographic rank among the K! permutations, decoded with the
// factorial number system: digit k picks among the classes not taken yet, ascending), and the
// permutation itself when `perm` is given
template <int K>
__device__ __forceinline__ double align_candidate(int index, const double *S, int32_t *perm) {
    int rem = index;
    unsigned used = 0;
    double total = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int fact = align_factorial(K - 1 - k);
        int digit = rem / fact;
        rem -= digit * fact;
        int j = 0;
#pragma unroll
        for (int e = 0; e < K; ++e) {
            const bool is_free = ((used >> e) & 1u) == 0;
            if (is_free && digit == 0) j = e;
            if (is_free) --digit;
        }
        used |= 1u << j;
        total += S[k * K + j];
        if (perm) perm[k] = j;
    }
    return total;
}

__device__ __forceinline__ bool align_better(double ta, int ia, double tb, int ib) {
    return ta > tb || (ta == tb && ia < ib);
}

// The best of the K! candidates over S (K x K, LDS or global), searched by the workgroup's 256
// threads: thread tid takes ranks tid, tid + 256, ... ascending, so `>` keeps the smallest rank
// among equal totals; waves and then the workgroup are reduced under the same rule.  The rank is
// returned to thread 0 (only); `best_total` and `best_index` hold 4 entries each.
template <int K>
__device__ __forceinline__ int align_search(const double *S, double *best_total, int *best_index) {
    constexpr int NF = align_factorial(K);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double bt = -INFINITY;
    int bi = 0;
    for (int i = tid; i < NF; i += ALIGN_WG) {
        const double tot = align_candidate<K>(i, S, nullptr);
        if (align_better(tot, i, bt, bi)) {
            bt = tot;
            bi = i;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ot = __shfl_xor(bt, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (align_better(ot, oi, bt, bi)) {
            bt = ot;
            bi = oi;
        }
    }
    if (lane == 0) {
        best_total[wave] = bt;
        best_index[wave] = bi;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w)
            if (align_better(best_total[w], best_index[w], bt, bi)) {
                bt = best_total[w];
                bi = best_index[w];
            }
        bi = min(max(bi, 0), NF - 1);        // (non-finite scores: any permutation, but a permutation)
    }
    return bi;
}
