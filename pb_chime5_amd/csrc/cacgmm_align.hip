// Permutation alignment of per-frequency posteriors (gss_cacgmm_align, gss_cacgmm_model_permute;
// include/gss_hip.h).  A CACGMM fitted per frequency without an annotation numbers its classes
// independently in every bin; the aligner finds, per frequency, the permutation of the classes
// under which the rows gamma[f, k, :] of all bins look alike.  The definition is
// tests/align_reference.py; in short, with feat[f, j, :] = gamma[f, j, :] / |gamma[f, j, :]|:
//
//    pass over [start, end):   c[k, :] = unit(sum_f feat[f, mapping[f, k], :])
//                              S_f[k, j] = <c[k, :], feat[f, j, :]>
//                              mapping[f, :] = argmax_p sum_k S_f[k, p[k]]   (K! candidates,
//                                              the lexicographically smallest among exact maxima)
//
// Features are never written: the (F,K) table of 1 / |gamma[f, j, :]| scales the centroid's terms
// and the scores.  Kernels, named as gss_profile_report lists them:
//
//   align_norms      gamma -> inv_n (F,K)                      one workgroup per row
//   align_centroid   gamma, inv_n, mapping -> part (slices,K,T) -> c (K,T), sq (K, blocks)
//                    the column sum of cacgmm_prior.hip's prior update with a gather: slices of
//                    the range's frequencies side by side (ascending f inside), added in order;
//                    the finish kernel also leaves the squares of c summed per 256 frames
//   align_assign<K>  gamma, c, sq, inv_n -> mapping row, "changed" word   one workgroup per
//                    frequency of the range
//   align_gather / align_model_gather    rows taken by the mapping
//   (the activity is cacgmm_prior.hip's column sum over the aligned table, unchanged)
//
// No floating-point atomics and one fixed order for every sum: the same call gives the same bits.
// The early end of a plan entry ("no mapping changed") is a device-side word per pass: every
// kernel of a pass returns at once when the pass before it, in the same entry, changed nothing --
// a pass is a function of the mappings in its range, so it would change nothing either.  No sync.
#include <algorithm>

#include "cacgmm_perm.h"
#include "gss_internal.h"

namespace {

// ------------------------------------------------------------------ 1 / row norms
__global__ __launch_bounds__(ALIGN_WG) void align_norms_kernel(const double *__restrict__ gamma,
                                                               int64_t T,
                                                               double *__restrict__ inv_n) {
    __shared__ double red[4];
    const double *row = gamma + (int64_t)blockIdx.x * T;
    double s = 0.0;
    for (int64_t t = threadIdx.x; t < T; t += ALIGN_WG) s = fma(row[t], row[t], s);
    s = block_sum_256(s, red);
    // (a zero row has no direction: its features are zero.  NaN compares false: zero as well.)
    if (threadIdx.x == 0) inv_n[blockIdx.x] = s > 0.0 ? 1.0 / sqrt(s) : 0.0;
}

__global__ __launch_bounds__(ALIGN_WG) void align_identity_kernel(int32_t *__restrict__ mapping,
                                                                  int64_t FK, int K) {
    const int64_t i = (int64_t)blockIdx.x * ALIGN_WG + threadIdx.x;
    if (i < FK) mapping[i] = (int32_t)(i % K);
}

// ------------------------------------------------------------------ centroid
// part[slice, k, t] = sum over the slice's frequencies, ascending, of
//                     inv_n[f, j] gamma[f, j, t],  j = mapping[f, k]
__global__ __launch_bounds__(ALIGN_WG) void align_centroid_partial_kernel(
    const double *__restrict__ gamma, const double *__restrict__ inv_n,
    const int32_t *__restrict__ mapping, int f_begin, int f_end, int per_slice, int K, int64_t T,
    double *__restrict__ part, const int32_t *__restrict__ prev_changed) {
    if (prev_changed && *prev_changed == 0) return;
    const int64_t KT = (int64_t)K * T;
    const int64_t idx = (int64_t)blockIdx.x * ALIGN_WG + threadIdx.x;
    if (idx >= KT) return;
    const int k = (int)(idx / T);
    const int64_t t = idx - (int64_t)k * T;
    const int f0 = f_begin + blockIdx.y * per_slice, f1 = min(f0 + per_slice, f_end);
    double s = 0.0;
    for (int f = f0; f < f1; ++f) {
        const int j = mapping[f * K + k];
        s = fma(inv_n[f * K + j], gamma[((int64_t)f * K + j) * T + t], s);
    }
    part[(int64_t)blockIdx.y * KT + idx] = s;
}

// c[k, t] = the slices added in order; sq[k, block] = sum of c[k, t]^2 over the block's frames
__global__ __launch_bounds__(ALIGN_WG) void align_centroid_finish_kernel(
    const double *__restrict__ part, int nslice, int K, int64_t T, double *__restrict__ c,
    double *__restrict__ sq, const int32_t *__restrict__ prev_changed) {
    __shared__ double red[4];
    if (prev_changed && *prev_changed == 0) return;
    const int64_t KT = (int64_t)K * T;
    const int k = blockIdx.y;
    const int64_t t = (int64_t)blockIdx.x * ALIGN_WG + threadIdx.x;
    double s = 0.0;
    if (t < T) {
        const int64_t idx = (int64_t)k * T + t;
        s = part[idx];
        for (int j = 1; j < nslice; ++j) s += part[(int64_t)j * KT + idx];
        c[idx] = s;
    }
    const double tot = block_sum_256(s * s, red);
    if (threadIdx.x == 0) sq[(int64_t)k * gridDim.x + blockIdx.x] = tot;
}

// ------------------------------------------------------------------ score and assign
// (the candidates, their decoder and the tie rule: cacgmm_perm.h)
template <int K>
__global__ __launch_bounds__(ALIGN_WG) void align_assign_kernel(
    const double *__restrict__ gamma, const double *__restrict__ c, const double *__restrict__ sq,
    int nblk, const double *__restrict__ inv_n, int32_t *__restrict__ mapping, int f_begin,
    int64_t T, const int32_t *__restrict__ prev_changed, int32_t *__restrict__ changed) {
    constexpr int KK = K * K;
    __shared__ double red[4][KK];
    __shared__ double S[KK];
    __shared__ double best_total[4];
    __shared__ int best_index[4];
    if (prev_changed && *prev_changed == 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = f_begin + blockIdx.x;
    const double *gf = gamma + (int64_t)f * K * T;

    // the K x K dot products over t: per-thread partials, frames tid, tid + 256, ...
    double acc[K][K];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int j = 0; j < K; ++j) acc[k][j] = 0.0;
    for (int64_t t = tid; t < T; t += ALIGN_WG) {
        double cv[K], g[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            cv[k] = c[(int64_t)k * T + t];
            g[k] = gf[(int64_t)k * T + t];
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int j = 0; j < K; ++j) acc[k][j] = fma(cv[k], g[j], acc[k][j]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double w = wave_sum(acc[k][j]);
            if (lane == 0) red[wave][k * K + j] = w;
        }
    __syncthreads();
    if (tid < KK) {
        const int k = tid / K, j = tid - k * K;
        const double s = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        double n2 = sq[(int64_t)k * nblk];
        for (int b = 1; b < nblk; ++b) n2 += sq[(int64_t)k * nblk + b];
        const double rc = n2 > 0.0 ? 1.0 / sqrt(n2) : 0.0;      // a zero centroid row stays zero
        S[tid] = s * rc * inv_n[f * K + j];
    }
    __syncthreads();

    // the K! candidates, the smallest rank among equal totals (cacgmm_perm.h)
    const int bi = align_search<K>(S, best_total, best_index);
    if (tid == 0) {
        int32_t perm[K];
        align_candidate<K>(bi, S, perm);
        bool moved = false;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            moved |= mapping[f * K + k] != perm[k];
            mapping[f * K + k] = perm[k];
        }
        if (moved) *changed = 1;             // the same value from every workgroup: no atomic
    }
}

// ------------------------------------------------------------------ gathers and the count
// out[f, k, :] = in[f, mapping[f, k], :]; an entry outside [0, K) gives NaN and reads nothing
__global__ __launch_bounds__(ALIGN_WG) void align_gather_kernel(const double *__restrict__ gamma,
                                                                const int32_t *__restrict__ mapping,
                                                                int K, int64_t T,
                                                                double *__restrict__ out) {
    const int64_t row = blockIdx.x;                  // f * K + k
    const int j = mapping[row];
    const bool ok = j >= 0 && j < K;
    const double *src = gamma + (row / K * K + (ok ? j : 0)) * T;
    double *dst = out + row * T;
    for (int64_t t = (int64_t)blockIdx.y * ALIGN_WG + threadIdx.x; t < T;
         t += (int64_t)gridDim.y * ALIGN_WG)
        dst[t] = ok ? src[t] : NAN;
}

__global__ __launch_bounds__(ALIGN_WG) void align_model_gather_kernel(
    const cplx *__restrict__ precision, const double *__restrict__ log_det,
    const double *__restrict__ weight, const int32_t *__restrict__ mapping, int K, int DD,
    cplx *__restrict__ precision_out, double *__restrict__ log_det_out,
    double *__restrict__ weight_out) {
    const int64_t row = blockIdx.x;                  // f * K + k
    const int j = mapping[row];
    const bool ok = j >= 0 && j < K;
    const int64_t from = row / K * K + (ok ? j : 0);
    for (int e = threadIdx.x; e < DD; e += ALIGN_WG)
        precision_out[row * DD + e] = ok ? precision[from * DD + e] : c_make(NAN, NAN);
    if (threadIdx.x == 0) {
        log_det_out[row] = ok ? log_det[from] : NAN;
        weight_out[row] = ok ? weight[from] : NAN;
    }
}

// frequencies whose row is not the identity -> the context's status word (one workgroup)
__global__ __launch_bounds__(ALIGN_WG) void align_moved_kernel(const int32_t *__restrict__ mapping,
                                                               int F, int K,
                                                               int32_t *__restrict__ status) {
    __shared__ int count;
    if (threadIdx.x == 0) count = 0;
    __syncthreads();
    int mine = 0;
    for (int f = threadIdx.x; f < F; f += ALIGN_WG) {
        bool moved = false;
        for (int k = 0; k < K; ++k) moved |= mapping[f * K + k] != k;
        mine += moved ? 1 : 0;
    }
    atomicAdd(&count, mine);                         // (integers in LDS: any order, one result)
    __syncthreads();
    if (threadIdx.x == 0)
        __hip_atomic_store(status, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <int K>
int launch_assign(gss_ctx *ctx, const double *gamma, const double *c, const double *sq, int nblk,
                  const double *inv_n, int32_t *mapping, int f_begin, int f_end, int64_t T,
                  const int32_t *prev_changed, int32_t *changed) {
    hipLaunchKernelGGL((align_assign_kernel<K>), dim3(f_end - f_begin), dim3(ALIGN_WG), 0,
                       ctx->stream, gamma, c, sq, nblk, inv_n, mapping, f_begin, T, prev_changed,
                       changed);
    GSS_LAUNCH_CHECK(ctx, "align_assign_kernel");
    return GSS_OK;
}

// Frequencies per slice of the centroid's column sum: a function of (n, K, T) only.  About 1024
// workgroups in all, at most PRIOR_MAX_SLICES slices (the rule of the prior update).
int centroid_per_slice(int n, int K, int64_t T) {
    const int64_t blocks = ((int64_t)K * T + ALIGN_WG - 1) / ALIGN_WG;
    int64_t want = (1024 + blocks - 1) / blocks;
    want = std::min<int64_t>(std::min<int64_t>(want, PRIOR_MAX_SLICES), n);
    if (want < 1) want = 1;
    return (int)((n + want - 1) / want);
}

int64_t plan_passes(const gss_align_plan *plan) {
    int64_t passes = 0;
    for (int e = 0; e < plan->entries; ++e) passes += plan->iterations[e];
    return passes;
}

}  // namespace

struct AlignWork {
    double *inv_n;      // (F,K) 1 / row norms
    double *c;          // (K,T) centroid
    double *part;       // slices of a column sum
    double *sq;         // squares of the centroid per block of frames
    int32_t *changed;   // one word per pass
    double *aligned;    // own_aligned: the aligned table the activity is formed from
};
static AlignWork align_blocks(Workspace &ws, int F, int K, int64_t T, const gss_align_plan *plan,
                              bool own_aligned) {
    const size_t KT = (size_t)K * T, nblk = (size_t)((T + ALIGN_WG - 1) / ALIGN_WG);
    AlignWork k;
    k.inv_n = ws.take<double>((size_t)F * K, "align inv_n");
    k.c = ws.take<double>(KT, "align centroid");
    k.part = ws.take<double>((size_t)PRIOR_MAX_SLICES * KT, "align slices");
    k.sq = ws.take<double>((size_t)K * nblk, "align squares");
    k.changed = ws.take<int32_t>((size_t)plan_passes(plan), "align changed");
    k.aligned = own_aligned ? ws.take<double>((size_t)F * KT, "align aligned") : nullptr;
    return k;
}

size_t cacgmm_align_workspace_bytes(int F, int K, int64_t T, const gss_align_plan *plan,
                                    bool own_aligned) {
    Workspace ws;
    align_blocks(ws, F, K, T, plan, own_aligned);
    return ws.bytes + 4096;
}

int cacgmm_align_run(gss_ctx *ctx, const double *gamma, int F, int K, int64_t T,
                     const gss_align_plan *plan, int32_t *mapping, double *aligned,
                     double *activity) {
    const int64_t KT = (int64_t)K * T;
    const int nblk = (int)((T + ALIGN_WG - 1) / ALIGN_WG);
    const int64_t passes = plan_passes(plan);
    Workspace ws(ctx);
    const AlignWork k = align_blocks(ws, F, K, T, plan, activity && !aligned);
    GSS_TRY(ws.status("cacgmm align"));
    double *inv_n = k.inv_n, *c = k.c, *part = k.part, *sq = k.sq;
    int32_t *changed = k.changed;
    if (k.aligned) aligned = k.aligned;

    {
        GSS_PROF(ctx, "align_norms");
        hipLaunchKernelGGL(align_norms_kernel, dim3((unsigned)(F * K)), dim3(ALIGN_WG), 0,
                           ctx->stream, gamma, T, inv_n);
        GSS_LAUNCH_CHECK(ctx, "align_norms_kernel");
        hipLaunchKernelGGL(align_identity_kernel,
                           dim3((unsigned)(((int64_t)F * K + ALIGN_WG - 1) / ALIGN_WG)),
                           dim3(ALIGN_WG), 0, ctx->stream, mapping, (int64_t)F * K, K);
        GSS_LAUNCH_CHECK(ctx, "align_identity_kernel");
        GSS_HIP_CHECK(ctx, hipMemsetAsync(changed, 0, sizeof(int32_t) * (size_t)passes, ctx->stream));
    }

    int64_t pass = 0;
    for (int e = 0; e < plan->entries && K > 1; ++e) {       // (K = 1: the identity is the answer)
        const int f_begin = plan->start[e], f_end = plan->end[e], n = f_end - f_begin;
        const int per = centroid_per_slice(n, K, T), nslice = (n + per - 1) / per;
        for (int it = 0; it < plan->iterations[e]; ++it, ++pass) {
            const int32_t *prev = it > 0 ? changed + pass - 1 : nullptr;
            {
                GSS_PROF(ctx, "align_centroid");
                hipLaunchKernelGGL(align_centroid_partial_kernel,
                                   dim3((unsigned)((KT + ALIGN_WG - 1) / ALIGN_WG), nslice),
                                   dim3(ALIGN_WG), 0, ctx->stream, gamma, inv_n, mapping, f_begin,
                                   f_end, per, K, T, part, prev);
                GSS_LAUNCH_CHECK(ctx, "align_centroid_partial_kernel");
                hipLaunchKernelGGL(align_centroid_finish_kernel, dim3(nblk, K), dim3(ALIGN_WG), 0,
                                   ctx->stream, part, nslice, K, T, c, sq, prev);
                GSS_LAUNCH_CHECK(ctx, "align_centroid_finish_kernel");
            }
            GSS_PROF(ctx, "align_assign");
#define GSS_ALIGN_CASE(N)                                                                        \
    case N:                                                                                      \
        GSS_TRY(launch_assign<N>(ctx, gamma, c, sq, nblk, inv_n, mapping, f_begin, f_end, T, prev, \
                                 changed + pass));                                               \
        break;
            switch (K) {
                GSS_ALIGN_CASE(2) GSS_ALIGN_CASE(3) GSS_ALIGN_CASE(4) GSS_ALIGN_CASE(5)
                GSS_ALIGN_CASE(6) GSS_ALIGN_CASE(7) GSS_ALIGN_CASE(8)
                default: return gss_fail(ctx, GSS_ERR_UNSUPPORTED, "gss_cacgmm_align: K=%d", K);
            }
#undef GSS_ALIGN_CASE
        }
    }

    hipLaunchKernelGGL(align_moved_kernel, dim3(1), dim3(ALIGN_WG), 0, ctx->stream, mapping, F, K,
                       ctx->status_dev + GSS_STATUS_ALIGN_MOVED);
    GSS_LAUNCH_CHECK(ctx, "align_moved_kernel");
    if (aligned) {
        GSS_PROF(ctx, "align_gather");
        const unsigned ty = (unsigned)std::min<int64_t>((T + ALIGN_WG - 1) / ALIGN_WG, 64);
        hipLaunchKernelGGL(align_gather_kernel, dim3((unsigned)(F * K), ty), dim3(ALIGN_WG), 0,
                           ctx->stream, gamma, mapping, K, T, aligned);
        GSS_LAUNCH_CHECK(ctx, "align_gather_kernel");
    }
    if (activity) {
        // activity[k, t] = (1 / F) sum_f aligned[f, k, t]: the prior update's column sum as it is
        const EmPriorWork w{aligned, activity, part, nullptr};
        GSS_TRY(cacgmm_prior_update_run(ctx, w, F, K, T));
    }
    return GSS_OK;
}

int cacgmm_model_permute_run(gss_ctx *ctx, const EmModel &in, int F, int K, int D,
                             const int32_t *mapping, const EmModel &out) {
    GSS_PROF(ctx, "align_model_gather");
    hipLaunchKernelGGL(align_model_gather_kernel, dim3((unsigned)(F * K)), dim3(ALIGN_WG), 0,
                       ctx->stream, in.precision, in.log_det, in.weight, mapping, K, D * D,
                       out.precision, out.log_det, out.weight);
    GSS_LAUNCH_CHECK(ctx, "align_model_gather_kernel");
    return GSS_OK;
}
