// CACGMM with a frequency-shared prior (gss_cacgmm_shared_prior, include/gss_hip.h): pb_bss's
// weight_constant_axis=-3.  The mixture weight is not pi[f, k] (constant over time, one per
// frequency) but prior[k, t]: one value per class and FRAME for all frequencies, the mean over f
// of the affiliations (Ito et al., frequency-independent source-presence priors).  It ties the
// frequencies together -- class k is the same speaker in every bin -- which is what lets the EM
// start without an annotation.
//
// Two pieces that the per-frequency EM (cacgmm.hip) does not have:
//   em_estep_prior_kernel   the E-step that multiplies by prior[k, t] and hands the M-step three
//   (and its register form) things: W = gamma / max(q, 10 tiny), the gamma itself (the prior
//                           update reads it) and the per-(f, tile, k) sums of gamma (em_chol's
//                           denominator), built from the pieces of cacgmm_estep.h;
//   prior_partial_kernel /  prior[k, t] = (1 / F) sum_f gamma[f, k, t]: a column sum over an
//   prior_finish_kernel     (F, K T) array, slices of frequencies summed side by side and then
//                           added in order.
// The M-step and the model update are the kernels of cacgmm.hip, unchanged; the pi[f, k] the
// model update still writes is not read by anything here.
#include <algorithm>

#include "cacgmm_estep.h"

namespace {

// ------------------------------------------------------------------ E-step with a per-frame prior
// One lane per frame, one wave per workgroup; the frame comes from the unit-normalised (F, D, T)
// copy (coalesced loads) and goes through quad_forms_lds (cacgmm_estep.h).  The K prior values of
// a frame are prior[k * T + t]: coalesced over the lanes.  The softmax is the log form of
// em_estep_kernel (max over ALL classes, as pb_bss takes it before the mask is multiplied in), in
// registers.
//   EM_PRIOR_FIRST    the initialisation as the affiliation (q = 1): W = gamma = init[f, k, t],
//                     or where(mask, 1, 1e-10) / sum_k when only a mask is given; no model read
//   EM_PRIOR_FIT      W, gamma and the sums of gamma
//   EM_PRIOR_PREDICT  the posteriors only
// Sums of gamma: one record per (f, 64-frame tile), Sg[(f * ntile + tile) * K + k] -- the layout
// em_chol_kernel / em_eigh_kernel read with sg_nch = ntile.
template <int K, int MODE>
__global__ __launch_bounds__(64) void em_estep_prior_kernel(EmPriorArgs a,
                                                            const cplx *__restrict__ Yn,
                                                            const cplx *__restrict__ Mq,
                                                            const double *__restrict__ logdet,
                                                            const double *__restrict__ prior) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cplx *ys = reinterpret_cast<cplx *>(smem);      // D * 64
    const int64_t T = a.T;
    const int D = a.D;
    const int ntile = (int)((T + 63) / 64);
    int f, tile;
    if (!xcd_group_map(ntile, a.F, f, tile)) return;
    const int lane = threadIdx.x;
    const int64_t t = (int64_t)tile * 64 + lane;
    const bool valid = t < T;
    const int64_t tc = valid ? t : T - 1;
    const uint8_t *actf = a.act + (int64_t)f * a.act_fstride + tc;
    double *Sgf = a.Sg + ((int64_t)f * ntile + tile) * K;
    bool on[K];
    double q[K], v[K];

    if (MODE == EM_PRIOR_FIRST) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            on[k] = actf[(int64_t)k * a.act_stride] != 0;
            q[k] = 1.0;                              // the quadratic form of the first iteration
        }
        // W = G = the affiliations as they are: estep_finish with norm = 1, q = 1 and no clip
        // divides by 1.0 and by max(1, 10 tiny) = 1.0, both exact for every double
        first_affiliations<K>(a.init ? a.init + (int64_t)f * a.init_fstride + tc : nullptr,
                              a.init_stride, on, v);
        estep_finish<K, false, false, true>(v, 1.0, q, q, 0.0, valid, lane, T, (int64_t)f * K, t,
                                            a.W, a.G, Sgf);
        return;
    }

    const cplx *yf = Yn + (int64_t)f * D * T + tc;
    for (int d = 0; d < D; ++d) ys[d * 64 + lane] = yf[(int64_t)d * T];
    quad_forms_lds<K>(ys, lane, D, Mq + (int64_t)f * tri_count(D) * K, q);
    double mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        q[k] = fmax(fabs(q[k]), GSS_TINY);
        v[k] = -(double)D * log(q[k]) - logdet[f * K + k];
        mx = fmax(mx, v[k]);
    }
    double ssum = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        v[k] = exp(v[k] - mx) * prior[(int64_t)k * T + tc];
        if (a.masked) v[k] *= actf[(int64_t)k * a.act_stride] ? 1.0 : 0.0;
        ssum += v[k];
    }
    estep_finish<K, MODE == EM_PRIOR_PREDICT, false, true>(
            v, fmax(ssum, GSS_TINY), q, q, a.aff_eps, valid, lane, T, (int64_t)f * K, t,
            MODE == EM_PRIOR_PREDICT ? a.gamma : a.W, a.G, Sgf);
}

// ------------------------------------------------------------------ the same, register form
// For the shapes of estep_reg_supported the frame's D values stay in registers and the walk is
// quad_forms_reg (cacgmm_estep.h), one wave per workgroup.  The LDS form above holds D KB per
// wave, six waves on a CU at D = 24, and exposes every scalar load (cacgmm_loglik_kernel, the
// same shape, takes 4.4 E-step launches for an E-step's arithmetic).  The softmax is the ratio
// form of posterior_ratio,  (q_min / q_k)^D exp(ln det_min - ln det_k) prior[k, t],  with the
// log form where every term underflows, and the epilogue that of estep_finish -- both in this
// kernel's own text: through the shared functions the D = 4 instantiations were 3 % slower
// (DESIGN.md, section 28).
template <int K, int D, int MODE>
__global__ __launch_bounds__(64) void em_estep_prior_reg_kernel(EmPriorArgs a,
                                                                 const cplx *__restrict__ Yn,
                                                                 const cplx *__restrict__ Mq,
                                                                 const double *__restrict__ logdet,
                                                                 const double *__restrict__ prior) {
    constexpr int NE = D * (D + 1) / 2;
    const int64_t T = a.T;
    const int ntile = (int)((T + 63) / 64);
    int f, tile;
    if (!xcd_group_map(ntile, a.F, f, tile)) return;
    const int lane = threadIdx.x;
    const int64_t t = (int64_t)tile * 64 + lane;
    const bool valid = t < T;
    const int64_t tc = valid ? t : T - 1;
    const cplx *yf = Yn + (int64_t)f * D * T + tc;

    estep_priority<3>();
    cplx y[D];
#pragma unroll
    for (int d = 0; d < D; ++d) y[d] = yf[(int64_t)d * T];
    double q[K];
    quad_forms_reg<K, D>(y, Mq + (int64_t)f * NE * K, q);

    int64_t tcl = tc;
    int kk = lane < K ? lane : K - 1;
    hold_below_walk(q[0], tcl, kk);
    // lane k: ln det_k and exp(ln det_min - ln det_k), handed to all lanes through SGPR pairs
    double els, ldl;
    {
        ldl = logdet[f * K + kk];
        double ldmin = INFINITY;
#pragma unroll
        for (int k = 0; k < K; ++k) ldmin = fmin(ldmin, lane_bcast(ldl, k));
        els = exp(ldmin - ldl);
    }
    double qmin = INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        q[k] = fmax(fabs(q[k]), GSS_TINY);
        qmin = fmin(qmin, q[k]);
    }
    double pk[K];
    bool on[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        pk[k] = prior[(int64_t)k * T + tcl];
        // (always readable and always read: no branch)
        on[k] = a.act[(int64_t)f * a.act_fstride + (int64_t)k * a.act_stride + tcl] != 0;
    }
    double v[K], iq[K], ssum = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        iq[k] = 1.0 / q[k];
        const double r = qmin * iq[k];
        double p = 1.0, b = r;            // r^D by squaring
#pragma unroll
        for (int bit = D; bit > 0; bit >>= 1) {
            if (bit & 1) p = p * b;
            b = b * b;
        }
        v[k] = p * lane_bcast(els, k) * pk[k];
        v[k] = (!a.masked || on[k]) ? v[k] : 0.0;
        ssum += v[k];
    }
    if (ssum < 1e-280) {
        double lp[K], mx = -INFINITY;
        ssum = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            lp[k] = -(double)D * log(q[k]) - lane_bcast(ldl, k);
            mx = fmax(mx, lp[k]);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            v[k] = exp(lp[k] - mx) * pk[k];
            v[k] = (!a.masked || on[k]) ? v[k] : 0.0;
            ssum += v[k];
        }
    }
    const double is = 1.0 / fmax(ssum, GSS_TINY);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double gam = v[k] * is;
        if (a.aff_eps != 0.0) gam = fmin(fmax(gam, a.aff_eps), 1.0 - a.aff_eps);
        if (MODE == EM_PRIOR_PREDICT) {
            if (valid) a.gamma[((int64_t)f * K + k) * T + t] = gam;
        } else {
            if (valid) {
                a.W[((int64_t)f * K + k) * T + t] =
                    gam * (q[k] < 10.0 * GSS_TINY ? 1.0 / (10.0 * GSS_TINY) : iq[k]);
                a.G[((int64_t)f * K + k) * T + t] = gam;
            }
            const double tot = wave_sum(valid ? gam : 0.0);
            if (lane == 0) a.Sg[((int64_t)f * ntile + tile) * K + k] = tot;
        }
    }
}

template <int K, int D>
int launch_estep_prior_reg(gss_ctx *ctx, const EmPriorArgs &a, int mode) {
    const dim3 grid(xcd_grid((int)((a.T + 63) / 64), a.F)), block(64);
    if (mode == EM_PRIOR_FIT) {
        GSS_PROF(ctx, "em_estep_prior");
        hipLaunchKernelGGL((em_estep_prior_reg_kernel<K, D, EM_PRIOR_FIT>), grid, block, 0,
                           ctx->stream, a, a.Yn, a.Mq, a.logdet, a.prior);
    } else {
        GSS_PROF(ctx, "em_predict_prior");
        hipLaunchKernelGGL((em_estep_prior_reg_kernel<K, D, EM_PRIOR_PREDICT>), grid, block, 0,
                           ctx->stream, a, a.Yn, a.Mq, a.logdet, a.prior);
    }
    GSS_LAUNCH_CHECK(ctx, "em_estep_prior_reg_kernel");
    return GSS_OK;
}

template <int K>
int launch_estep_prior(gss_ctx *ctx, const EmPriorArgs &a, int mode) {
    const size_t lds = sizeof(cplx) * 64 * (size_t)a.D;
    const dim3 grid(xcd_grid((int)((a.T + 63) / 64), a.F)), block(64);
    if (mode == EM_PRIOR_FIRST) {
        GSS_PROF(ctx, "em_estep_prior");
        hipLaunchKernelGGL((em_estep_prior_kernel<K, EM_PRIOR_FIRST>), grid, block, 0, ctx->stream,
                           a, a.Yn, a.Mq, a.logdet, a.prior);
    } else if (mode == EM_PRIOR_FIT) {
        GSS_PROF(ctx, "em_estep_prior");
        hipLaunchKernelGGL((em_estep_prior_kernel<K, EM_PRIOR_FIT>), grid, block, lds, ctx->stream,
                           a, a.Yn, a.Mq, a.logdet, a.prior);
    } else {
        GSS_PROF(ctx, "em_predict_prior");
        hipLaunchKernelGGL((em_estep_prior_kernel<K, EM_PRIOR_PREDICT>), grid, block, lds,
                           ctx->stream, a, a.Yn, a.Mq, a.logdet, a.prior);
    }
    GSS_LAUNCH_CHECK(ctx, "em_estep_prior_kernel");
    return GSS_OK;
}

// ------------------------------------------------------------------ the prior update
// prior[k, t] = (1 / nf) sum_f G[f, k, t]: a column sum over an (nf, K T) array, t fastest.  One
// thread per (k, t) and slice of frequencies, ascending f (consecutive threads read consecutive
// addresses); the slices are the second grid dimension, so that K T = 4705 columns do not leave
// the chip empty.  A second short kernel adds the slices in order and divides.  No atomics.
// (At most PRIOR_MAX_SLICES slices, gss_internal.h: the aligner's activity shares the kernels.)

__global__ __launch_bounds__(256) void prior_partial_kernel(const double *__restrict__ G, int nf,
                                                            int per_slice, int64_t KT,
                                                            double *__restrict__ part) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= KT) return;
    const int f0 = blockIdx.y * per_slice, f1 = min(f0 + per_slice, nf);
    double s = 0.0;
    for (int f = f0; f < f1; ++f) s += G[(int64_t)f * KT + idx];
    part[(int64_t)blockIdx.y * KT + idx] = s;
}

__global__ __launch_bounds__(256) void prior_finish_kernel(const double *__restrict__ part,
                                                           int nslice, int nf, int64_t KT,
                                                           double *__restrict__ prior) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= KT) return;
    double s = part[idx];
    for (int j = 1; j < nslice; ++j) s += part[(int64_t)j * KT + idx];
    prior[idx] = s / (double)nf;
}

}  // namespace

// Frequencies per slice of the column sum: a function of (nf, K, T) only.  About 1024 workgroups
// in all, at most PRIOR_MAX_SLICES slices.
static int prior_per_slice(int nf, int K, int64_t T) {
    const int64_t blocks = ((int64_t)K * T + 255) / 256;
    int64_t want = (1024 + blocks - 1) / blocks;
    want = std::min<int64_t>(std::min<int64_t>(want, PRIOR_MAX_SLICES), nf);
    if (want < 1) want = 1;
    return (int)((nf + want - 1) / want);
}

EmPriorWork cacgmm_prior_alloc(Workspace &ws, int F, int64_t T, int K, bool own_prior) {
    EmPriorWork w;
    w.G = ws.take<double>((size_t)F * K * T, "shared prior G");
    w.prior = own_prior ? ws.take<double>((size_t)K * T, "shared prior") : nullptr;
    w.part = ws.take<double>((size_t)PRIOR_MAX_SLICES * K * T, "shared prior slices");
    w.Sg = ws.take<double>((size_t)F * ((T + 63) / 64) * K, "shared prior Sg");
    return w;
}

size_t cacgmm_prior_workspace_bytes(int F, int64_t T, int K) {
    Workspace ws;
    cacgmm_prior_alloc(ws, F, T, K, true);
    return ws.bytes + 4096;
}

int cacgmm_prior_estep_run(gss_ctx *ctx, const EmPriorArgs &a, int K, int mode) {
    // (GSS_VARIANT=estep_lds: the LDS form at every shape, as for the per-frequency E-step)
    if (mode != EM_PRIOR_FIRST && estep_reg_supported(a.D, K) && !gss_variant_set("estep_lds"))
        return dispatch_reg_shape(ctx, a.D, K, [&](auto d, auto k) {
            return launch_estep_prior_reg<decltype(k)::value, decltype(d)::value>(ctx, a, mode);
        });
    GSS_REQUIRE(ctx, sizeof(cplx) * 64 * (size_t)a.D <= 64 * 1024, GSS_ERR_UNSUPPORTED,
                "cacgmm (shared prior): D=%d", a.D);
    return dispatch_classes(ctx, K, [&](auto k) {
        return launch_estep_prior<decltype(k)::value>(ctx, a, mode);
    });
}

int cacgmm_prior_update_run(gss_ctx *ctx, const EmPriorWork &w, int nf, int K, int64_t T) {
    GSS_PROF(ctx, "em_prior_update");
    const int64_t KT = (int64_t)K * T;
    const int per = prior_per_slice(nf, K, T), nslice = (nf + per - 1) / per;
    const unsigned blocks = (unsigned)((KT + 255) / 256);
    hipLaunchKernelGGL(prior_partial_kernel, dim3(blocks, nslice), dim3(256), 0, ctx->stream, w.G,
                       nf, per, KT, w.part);
    GSS_LAUNCH_CHECK(ctx, "prior_partial_kernel");
    hipLaunchKernelGGL(prior_finish_kernel, dim3(blocks), dim3(256), 0, ctx->stream, w.part, nslice,
                       nf, KT, w.prior);
    GSS_LAUNCH_CHECK(ctx, "prior_finish_kernel");
    return GSS_OK;
}
