// Cross-window class linking (gss_cacgmm_link; include/gss_hip.h).  Two windows of a recording
// that overlap are separated independently, so class k of one is not class k of the other; on
// the L frames they share, the link finds the permutation of the current window's classes under
// which its posteriors agree with the previous window's.  The definition is
// tests/link_reference.py; with prev (F,K,T_prev) and cur (F,K,T_cur), frames prev_begin + t and
// cur_begin + t, t in [0, L):
//
//    num[a, b] = sum_f sum_t prev[f, a, t] cur[f, b, t]
//    S[a, b]   = num[a, b] / sqrt(sum_f sum_t prev[f, a, t]^2 * sum_f sum_t cur[f, b, t]^2)
//                (0 where the product of the norms is not positive)
//    mapping   = argmax_p sum_a S[a, p[a]]       (K! candidates, the lexicographically smallest
//                                                 among exact maxima: cacgmm_perm.h)
//
// Kernels, named as gss_profile_report lists them:
//
//   link_products<K>   prev, cur -> part (F, K K + 2 K)    one workgroup per frequency: the K x K
//                      products and the 2 K squared norms over the L frames
//   link_finish<K>     part -> S (K,K), mapping (K)        one workgroup: the rows added in
//                      ascending f, the scores, the search
//   link_gather        rows taken by the mapping, the same for every frequency
//                      (gss_cacgmm_link_gather)
//
// float64, no floating-point atomics, one fixed order for every sum: the same call gives the same
// bits, and two identical rows of a table give identical entries of S (an exact tie).
#include <algorithm>

#include "cacgmm_perm.h"
#include "gss_internal.h"

namespace {

constexpr int LINK_ROWS = 32;       // rows of `part` the finish kernel stages in LDS at a time

__host__ __device__ constexpr int link_entries(int K) { return K * K + 2 * K; }

template <int K>
__global__ __launch_bounds__(ALIGN_WG) void link_products_kernel(
    const double *__restrict__ prev, int64_t T_prev, int64_t prev_begin,
    const double *__restrict__ cur, int64_t T_cur, int64_t cur_begin, int64_t L,
    double *__restrict__ part) {
    constexpr int KK = K * K, NE = link_entries(K);
    __shared__ double red[4][NE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t f = blockIdx.x;
    const double *pf = prev + f * K * T_prev + prev_begin;
    const double *cf = cur + f * K * T_cur + cur_begin;

    // per-thread partials, frames tid, tid + 256, ...
    double acc[K][K], np[K], nc[K];
#pragma unroll
    for (int a = 0; a < K; ++a) {
        np[a] = 0.0;
        nc[a] = 0.0;
#pragma unroll
        for (int b = 0; b < K; ++b) acc[a][b] = 0.0;
    }
    for (int64_t t = tid; t < L; t += ALIGN_WG) {
        double p[K], c[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            p[k] = pf[(int64_t)k * T_prev + t];
            c[k] = cf[(int64_t)k * T_cur + t];
        }
#pragma unroll
        for (int a = 0; a < K; ++a) {
            np[a] = fma(p[a], p[a], np[a]);
            nc[a] = fma(c[a], c[a], nc[a]);
#pragma unroll
            for (int b = 0; b < K; ++b) acc[a][b] = fma(p[a], c[b], acc[a][b]);
        }
    }
#pragma unroll
    for (int a = 0; a < K; ++a) {
#pragma unroll
        for (int b = 0; b < K; ++b) {
            const double w = wave_sum(acc[a][b]);
            if (lane == 0) red[wave][a * K + b] = w;
        }
        const double wp = wave_sum(np[a]), wc = wave_sum(nc[a]);
        if (lane == 0) {
            red[wave][KK + a] = wp;
            red[wave][KK + K + a] = wc;
        }
    }
    __syncthreads();
    if (tid < NE)
        part[f * NE + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

template <int K>
__global__ __launch_bounds__(ALIGN_WG) void link_finish_kernel(const double *__restrict__ part,
                                                               int F,
                                                               int32_t *__restrict__ mapping,
                                                               double *__restrict__ scores) {
    constexpr int KK = K * K, NE = link_entries(K);
    __shared__ double rows[LINK_ROWS * NE];
    __shared__ double sum[NE];
    __shared__ double S[KK];
    __shared__ double best_total[4];
    __shared__ int best_index[4];
    const int tid = threadIdx.x;

    // the F rows in ascending f: LINK_ROWS of them are staged by all threads, then thread e adds
    // entry e of each, in order
    double s = 0.0;
    for (int f0 = 0; f0 < F; f0 += LINK_ROWS) {
        const int n = min(LINK_ROWS, F - f0) * NE;
        __syncthreads();                     // (the rows of the round before have been read)
        for (int i = tid; i < n; i += ALIGN_WG) rows[i] = part[(int64_t)f0 * NE + i];
        __syncthreads();
        if (tid < NE)
            for (int i = tid; i < n; i += NE) s += rows[i];
    }
    if (tid < NE) sum[tid] = s;
    __syncthreads();
    if (tid < KK) {
        const int a = tid / K, b = tid - a * K;
        // (a zero row has no direction: its scores are zero.  NaN compares false: zero as well.)
        const double den = sum[KK + a] * sum[KK + K + b];
        const double v = den > 0.0 ? sum[tid] / sqrt(den) : 0.0;
        S[tid] = v;
        scores[tid] = v;
    }
    __syncthreads();
    const int bi = align_search<K>(S, best_total, best_index);
    if (tid == 0) {
        int32_t perm[K];
        align_candidate<K>(bi, S, perm);
#pragma unroll
        for (int k = 0; k < K; ++k) mapping[k] = perm[k];
    }
}

// out[f, a, :] = in[f, mapping[a], :]; an entry outside [0, K) gives NaN and reads nothing
__global__ __launch_bounds__(ALIGN_WG) void link_gather_kernel(const double *__restrict__ gamma,
                                                               const int32_t *__restrict__ mapping,
                                                               int K, int64_t T,
                                                               double *__restrict__ out) {
    const int64_t row = blockIdx.x;                  // f * K + a
    const int j = mapping[row % K];
    const bool ok = j >= 0 && j < K;
    const double *src = gamma + (row / K * K + (ok ? j : 0)) * T;
    double *dst = out + row * T;
    for (int64_t t = (int64_t)blockIdx.y * ALIGN_WG + threadIdx.x; t < T;
         t += (int64_t)gridDim.y * ALIGN_WG)
        dst[t] = ok ? src[t] : NAN;
}

template <int K>
int launch_link(gss_ctx *ctx, const double *prev, int64_t T_prev, int64_t prev_begin,
                const double *cur, int64_t T_cur, int64_t cur_begin, int64_t L, int F,
                double *part, int32_t *mapping, double *scores) {
    {
        GSS_PROF(ctx, "link_products");
        hipLaunchKernelGGL((link_products_kernel<K>), dim3((unsigned)F), dim3(ALIGN_WG), 0,
                           ctx->stream, prev, T_prev, prev_begin, cur, T_cur, cur_begin, L, part);
        GSS_LAUNCH_CHECK(ctx, "link_products_kernel");
    }
    GSS_PROF(ctx, "link_finish");
    hipLaunchKernelGGL((link_finish_kernel<K>), dim3(1), dim3(ALIGN_WG), 0, ctx->stream, part, F,
                       mapping, scores);
    GSS_LAUNCH_CHECK(ctx, "link_finish_kernel");
    return GSS_OK;
}

}  // namespace

static double *link_blocks(Workspace &ws, int F, int K) {
    return ws.take<double>((size_t)F * link_entries(K), "link partial rows");
}

size_t cacgmm_link_workspace_bytes(int F, int K) {
    Workspace ws;
    link_blocks(ws, F, K);
    return ws.bytes + 4096;
}

int cacgmm_link_run(gss_ctx *ctx, const double *prev, int64_t T_prev, int64_t prev_begin,
                    const double *cur, int64_t T_cur, int64_t cur_begin, int64_t L, int F, int K,
                    int32_t *mapping, double *scores) {
    Workspace ws(ctx);
    double *part = link_blocks(ws, F, K);
    GSS_TRY(ws.status("cacgmm link"));
#define GSS_LINK_CASE(N)                                                                          \
    case N:                                                                                       \
        return launch_link<N>(ctx, prev, T_prev, prev_begin, cur, T_cur, cur_begin, L, F, part,   \
                              mapping, scores);
    switch (K) {
        GSS_LINK_CASE(1) GSS_LINK_CASE(2) GSS_LINK_CASE(3) GSS_LINK_CASE(4) GSS_LINK_CASE(5)
        GSS_LINK_CASE(6) GSS_LINK_CASE(7) GSS_LINK_CASE(8)
        default: return gss_fail(ctx, GSS_ERR_UNSUPPORTED, "gss_cacgmm_link: K=%d", K);
    }
#undef GSS_LINK_CASE
}

int cacgmm_link_gather_run(gss_ctx *ctx, const double *gamma, int F, int K, int64_t T,
                           const int32_t *mapping, double *out) {
    GSS_PROF(ctx, "link_gather");
    const unsigned ty = (unsigned)std::min<int64_t>((T + ALIGN_WG - 1) / ALIGN_WG, 64);
    hipLaunchKernelGGL(link_gather_kernel, dim3((unsigned)(F * K), ty), dim3(ALIGN_WG), 0,
                       ctx->stream, gamma, mapping, K, T, out);
    GSS_LAUNCH_CHECK(ctx, "link_gather_kernel");
    return GSS_OK;
}
