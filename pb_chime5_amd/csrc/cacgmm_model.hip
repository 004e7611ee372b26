// The fitted CACGMM as an object (gss_cacgmm_fit / gss_cacgmm_predict, include/gss_hip.h):
// conversions between the public dense model and the EM's packed one, and the log-likelihood of
// frames under a model.
//
// The EM (cacgmm.hip) keeps  Mq (F, NE, K): the upper triangle of B_k^-1, row-major packed,
// off-diagonals doubled, the class index fastest (a wave reads the K values of an entry with one
// scalar load).  The public form is the dense Hermitian B_k^-1 (F, K, D, D) with both triangles.
// Going from one to the other is a factor 2 on the off-diagonals -- exact in binary floating
// point -- so export followed by import gives back the bits the EM left.
#include "cacgmm_estep.h"

namespace {

// thread = one (f, k, d1, d2) of the dense matrix
__global__ __launch_bounds__(256) void model_import_kernel(const cplx *__restrict__ P,
                                                           const double *__restrict__ ld_in,
                                                           const double *__restrict__ w_in, int F,
                                                           int K, int D, cplx *__restrict__ Mq,
                                                           double *__restrict__ logdet,
                                                           double *__restrict__ pi) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)F * K * D * D;
    if (idx < (int64_t)F * K) {
        logdet[idx] = ld_in[idx];
        pi[idx] = w_in[idx];
    }
    if (idx >= total) return;
    const int d2 = (int)(idx % D), d1 = (int)(idx / D % D);
    if (d1 > d2) return;                     // the lower triangle is the conjugate: not read
    const int64_t fk = idx / ((int64_t)D * D);
    const int k = (int)(fk % K);
    const int64_t f = fk / K;
    cplx v = P[idx];
    if (d1 == d2) {
        v.y = 0.0;
    } else {
        v.x *= 2.0;
        v.y *= 2.0;
    }
    Mq[(f * tri_count(D) + tri_index(d1, d2, D)) * K + k] = v;
}

__global__ __launch_bounds__(256) void model_export_kernel(const cplx *__restrict__ Mq,
                                                           const double *__restrict__ logdet,
                                                           const double *__restrict__ pi, int F,
                                                           int K, int D, cplx *__restrict__ P,
                                                           double *__restrict__ ld_out,
                                                           double *__restrict__ w_out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)F * K * D * D;
    if (idx < (int64_t)F * K) {
        ld_out[idx] = logdet[idx];
        w_out[idx] = pi[idx];
    }
    if (idx >= total) return;
    const int d2 = (int)(idx % D), d1 = (int)(idx / D % D);
    const int64_t fk = idx / ((int64_t)D * D);
    const int k = (int)(fk % K);
    const int64_t f = fk / K;
    const int lo = d1 < d2 ? d1 : d2, hi = d1 < d2 ? d2 : d1;
    cplx v = Mq[(f * tri_count(D) + tri_index(lo, hi, D)) * K + k];
    if (d1 == d2) {
        v.y = 0.0;
    } else {
        v.x *= 0.5;
        v.y *= d1 < d2 ? 0.5 : -0.5;
    }
    P[idx] = v;
}

// ------------------------------------------------------------------ log-likelihood
// ln sum_k pi_k m_kt exp(-D ln q_kt - ln det B_k) per frame.  One lane per frame, one wave per
// workgroup; the frame comes from the unit-normalised (F, D, T) copy (coalesced loads) and goes
// through quad_forms_lds (cacgmm_estep.h), the entry order of every E-step.  Every frame is
// written by exactly one lane: no atomics, the same call gives the same bits.
template <int K>
__global__ __launch_bounds__(64) void cacgmm_loglik_kernel(
        const cplx *__restrict__ Yn, const cplx *__restrict__ Mq, const double *__restrict__ logdet,
        const double *__restrict__ pi, const uint8_t *__restrict__ act, int64_t act_stride,
        int64_t act_fstride, int masked, int F, int64_t T, int D, double *__restrict__ loglik) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cplx *ys = reinterpret_cast<cplx *>(smem);      // D * 64
    const int ntile = (int)((T + 63) / 64);
    int f, tile;
    if (!xcd_group_map(ntile, F, f, tile)) return;
    const int lane = threadIdx.x;
    const int64_t t = (int64_t)tile * 64 + lane;
    const bool valid = t < T;
    const int64_t tc = valid ? t : T - 1;
    const cplx *yf = Yn + (int64_t)f * D * T + tc;
    for (int d = 0; d < D; ++d) ys[d * 64 + lane] = yf[(int64_t)d * T];

    double q[K];
    quad_forms_lds<K>(ys, lane, D, Mq + (int64_t)f * tri_count(D) * K, q);
    // max-shifted log-sum-exp, the shift over the classes that are on: a class the mask turns off
    // may exceed every active one by more than exp() can span (floored eigenvalues at D = 24)
    double lp[K], mx = -INFINITY;
    bool on[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        on[k] = !masked || act[(int64_t)f * act_fstride + (int64_t)k * act_stride + tc] != 0;
        lp[k] = -(double)D * log(fmax(fabs(q[k]), GSS_TINY)) - logdet[f * K + k];
        if (on[k]) mx = fmax(mx, lp[k]);
    }
    double ssum = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) ssum += on[k] ? exp(lp[k] - mx) * pi[f * K + k] : 0.0;
    if (valid) loglik[(int64_t)f * T + t] = mx + log(ssum);      // every class off: -inf + ln 0
}

template <int K>
int launch_loglik(gss_ctx *ctx, const cplx *Yn, const cplx *Mq, const double *logdet,
                  const double *pi, const uint8_t *act, int64_t act_stride, int64_t act_fstride,
                  int masked, int F, int64_t T, int D, double *loglik) {
    GSS_PROF(ctx, "em_loglik");
    const size_t lds = sizeof(cplx) * 64 * (size_t)D;
    hipLaunchKernelGGL(cacgmm_loglik_kernel<K>, dim3(xcd_grid((int)((T + 63) / 64), F)), dim3(64), lds,
                       ctx->stream, Yn, Mq, logdet, pi, act, act_stride, act_fstride, masked, F, T, D,
                       loglik);
    GSS_LAUNCH_CHECK(ctx, "cacgmm_loglik_kernel");
    return GSS_OK;
}

unsigned model_grid(int F, int K, int D) {
    return (unsigned)(((int64_t)F * K * D * D + 255) / 256);
}

}  // namespace

int cacgmm_model_import(gss_ctx *ctx, const EmModel &m, int F, int K, int D, cplx *Mq,
                        double *logdet, double *pi) {
    GSS_PROF(ctx, "em_model_import");
    hipLaunchKernelGGL(model_import_kernel, dim3(model_grid(F, K, D)), dim3(256), 0, ctx->stream,
                       m.precision, m.log_det, m.weight, F, K, D, Mq, logdet, pi);
    GSS_LAUNCH_CHECK(ctx, "model_import_kernel");
    return GSS_OK;
}

int cacgmm_model_export(gss_ctx *ctx, const cplx *Mq, const double *logdet, const double *pi, int F,
                        int K, int D, const EmModel &m) {
    GSS_PROF(ctx, "em_model_export");
    hipLaunchKernelGGL(model_export_kernel, dim3(model_grid(F, K, D)), dim3(256), 0, ctx->stream, Mq,
                       logdet, pi, F, K, D, m.precision, m.log_det, m.weight);
    GSS_LAUNCH_CHECK(ctx, "model_export_kernel");
    return GSS_OK;
}

int cacgmm_loglik_run(gss_ctx *ctx, const cplx *Yn, const cplx *Mq, const double *logdet,
                      const double *pi, const uint8_t *act, int64_t act_stride,
                      int64_t act_fstride, int masked, int F, int64_t T, int D, int K,
                      double *loglik) {
    return dispatch_classes(ctx, K, [&](auto k) {
        return launch_loglik<decltype(k)::value>(ctx, Yn, Mq, logdet, pi, act, act_stride,
                                                 act_fstride, masked, F, T, D, loglik);
    });
}
