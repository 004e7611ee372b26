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
//                           denominator);
//   prior_partial_kernel /  prior[k, t] = (1 / F) sum_f gamma[f, k, t]: a column sum over an
//   prior_finish_kernel     (F, K T) array, slices of frequencies summed side by side and then
//                           added in order.
// The M-step and the model update are the kernels of cacgmm.hip, unchanged; the pi[f, k] the
// model update still writes is not read by anything here.
#include <algorithm>

#include "gss_internal.h"

namespace {

// ------------------------------------------------------------------ E-step with a per-frame prior
// One lane per frame, one wave per workgroup, no barrier and no exchange between lanes before the
// sums of gamma -- the form of cacgmm_loglik_kernel: a lane parks the D values of its frame (from
// the unit-normalised (F, D, T) copy: coalesced loads) in its own 16-byte column of LDS, because
// the channel index of the walk is a run-time value and registers cannot be indexed; consecutive
// lanes sit on consecutive slots (conflict free as ds_read_b128).  The walk over the packed
// triangle is the E-step's: P_de = y_d conj(y_e), 4 real FMAs per (entry, class) against the
// doubled off-diagonals, the K model values of an entry wave-uniform (scalar loads through the
// __restrict__ pointer).  The K prior values of a frame are prior[k * T + t]: coalesced over the
// lanes.  The softmax is the log form of em_estep_kernel (max over ALL classes, as pb_bss takes
// it before the mask is multiplied in), in registers.
//   EM_PRIOR_FIRST    the initialisation as the affiliation (q = 1): W = gamma = init[f, k, t],
//                     or where(mask, 1, 1e-10) / sum_k when only a mask is given; no model read
//   EM_PRIOR_FIT      W, gamma and the sums of gamma
//   EM_PRIOR_PREDICT  the posteriors only
// Sums of gamma: one record per (f, 64-frame tile), Sg[(f * ntile + tile) * K + k] -- the layout
// em_chol_kernel / em_eigh_kernel read with sg_nch = ntile.  Every element is written by exactly
// one lane: no atomics, the same call gives the same bits.
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

    if (MODE == EM_PRIOR_FIRST) {
        double g[K];
        if (a.init != nullptr) {
            // fit(initialization=array): the affiliations as given, not renormalised
            const double *initf = a.init + (int64_t)f * a.init_fstride + tc;
#pragma unroll
            for (int k = 0; k < K; ++k) g[k] = initf[(int64_t)k * a.init_stride];
        } else {
            // GSS initialisation (core.py:156-160): where(act == 0, 1e-10, act) / sum_k
            double ssum = 0.0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                g[k] = actf[(int64_t)k * a.act_stride] ? 1.0 : 1e-10;
                ssum += g[k];
            }
#pragma unroll
            for (int k = 0; k < K; ++k) g[k] = g[k] / ssum;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (valid) {
                a.W[((int64_t)f * K + k) * T + t] = g[k];        // quadratic form = 1
                a.G[((int64_t)f * K + k) * T + t] = g[k];
            }
            const double tot = wave_sum(valid ? g[k] : 0.0);
            if (lane == 0) Sgf[k] = tot;
        }
        return;
    }

    const cplx *yf = Yn + (int64_t)f * D * T + tc;
    for (int d = 0; d < D; ++d) ys[d * 64 + lane] = yf[(int64_t)d * T];

    double q[K];
#pragma unroll
    for (int k = 0; k < K; ++k) q[k] = 0.0;
    const cplx *mrow = Mq + (int64_t)f * tri_count(D) * K;
    for (int d1 = 0; d1 < D; ++d1) {
        const cplx y1 = ys[d1 * 64 + lane];
        {
            const double pr = y1.x * y1.x + y1.y * y1.y;
#pragma unroll
            for (int k = 0; k < K; ++k) q[k] = fma(mrow[k].x, pr, q[k]);
            mrow += K;
        }
        for (int d2 = d1 + 1; d2 < D; ++d2) {
            const cplx y2 = ys[d2 * 64 + lane];
            const double pr = y1.x * y2.x + y1.y * y2.y;
            const double pim = y1.y * y2.x - y1.x * y2.y;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const cplx m = mrow[k];
                q[k] = fma(m.x, pr, q[k]);
                q[k] = fma(m.y, pim, q[k]);
            }
            mrow += K;
        }
    }
    double v[K], mx = -INFINITY;
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
    ssum = fmax(ssum, GSS_TINY);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double gam = v[k] / ssum;
        if (a.aff_eps != 0.0) gam = fmin(fmax(gam, a.aff_eps), 1.0 - a.aff_eps);
        if (MODE == EM_PRIOR_PREDICT) {
            if (valid) a.gamma[((int64_t)f * K + k) * T + t] = gam;
        } else {
            if (valid) {
                a.W[((int64_t)f * K + k) * T + t] = gam / fmax(q[k], 10.0 * GSS_TINY);
                a.G[((int64_t)f * K + k) * T + t] = gam;
            }
            const double tot = wave_sum(valid ? gam : 0.0);
            if (lane == 0) Sgf[k] = tot;
        }
    }
}

// ------------------------------------------------------------------ the same, register form
// For the channel counts of the corpus (D = 24, 20, 12, 10, 4) and 2 <= K <= 6 -- the shapes for
// which the per-frequency EM has em_estep_reg_kernel -- the frame's D values stay in registers
// and the packed triangle is walked fully unrolled: the walk of em_estep_reg_kernel (a ring of
// model rows requested two entries ahead as scalar loads, a scheduling barrier per entry, wave
// priority falling with progress), one wave per workgroup.  The LDS form above holds D KB per
// wave, six waves on a CU at D = 24, and exposes every scalar load (cacgmm_loglik_kernel, the
// same shape, takes 4.4 E-step launches for an E-step's arithmetic).  The softmax is the
// ratio form of that kernel,  (q_min / q_k)^D exp(ln det_min - ln det_k) prior[k, t]  -- the
// common factor cancels in the normalisation --, with the log form where every term underflows.
// The epilogue's loads are ordered after the walk (see `tcl` below) so that the compiler cannot
// move them above it, where they would spill its ring, and the epilogue is one basic block.
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
    const cplx *Mf = Mq + (int64_t)f * NE * K;
    const cplx *yf = Yn + (int64_t)f * D * T + tc;

    __builtin_amdgcn_s_setprio(3);
    cplx y[D];
#pragma unroll
    for (int d = 0; d < D; ++d) y[d] = yf[(int64_t)d * T];

    double q[K];
#pragma unroll
    for (int k = 0; k < K; ++k) q[k] = 0.0;
    constexpr int P = 2, RING = P + 1;
    cplx ring[RING][K];
#pragma unroll
    for (int j = 0; j < P; ++j)
#pragma unroll
        for (int k = 0; k < K; ++k) ring[j][k] = Mf[j * K + k];
    int e = 0;
#pragma unroll
    for (int d1 = 0; d1 < D; ++d1) {
#pragma unroll
        for (int d2 = d1; d2 < D; ++d2) {
            if (e + P < NE) {
#pragma unroll
                for (int k = 0; k < K; ++k) ring[(e + P) % RING][k] = Mf[(e + P) * K + k];
            }
            const double pr = y[d1].x * y[d2].x + y[d1].y * y[d2].y;
            if (d1 == d2) {
#pragma unroll
                for (int k = 0; k < K; ++k) q[k] = fma(ring[e % RING][k].x, pr, q[k]);
            } else {
                const double pim = y[d1].y * y[d2].x - y[d1].x * y[d2].y;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const cplx m = ring[e % RING][k];
                    q[k] = fma(m.x, pr, q[k]);
                    q[k] = fma(m.y, pim, q[k]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            ++e;
            if (e == NE / 4) __builtin_amdgcn_s_setprio(2);
            if (e == NE / 2) __builtin_amdgcn_s_setprio(1);
            if (e == 3 * NE / 4) __builtin_amdgcn_s_setprio(0);
        }
    }
    // (the indices of the epilogue's loads pass through an empty statement that also names the
    // walk's result: their values are untouched, and nothing that uses them can move above it)
    int64_t tcl = tc;
    int kk = lane < K ? lane : K - 1;
    asm volatile("" : "+v"(tcl), "+v"(kk) : "v"(q[0]));
    auto lane_bcast = [](double x, int k) {
        const unsigned long long u = __double_as_longlong(x);
        const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)u, k);
        const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)(u >> 32), k);
        return __longlong_as_double(((unsigned long long)hi << 32) | lo);
    };
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
        // (always readable and always read: a branch here splits the epilogue into blocks and the
        // walk's scalar loads are then all hoisted to the top -- thousands of SGPR spills)
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

template <int D>
int launch_estep_prior_reg_k(gss_ctx *ctx, const EmPriorArgs &a, int K, int mode) {
    switch (K) {
        case 2: return launch_estep_prior_reg<2, D>(ctx, a, mode);
        case 3: return launch_estep_prior_reg<3, D>(ctx, a, mode);
        case 4: return launch_estep_prior_reg<4, D>(ctx, a, mode);
        case 5: return launch_estep_prior_reg<5, D>(ctx, a, mode);
        case 6: return launch_estep_prior_reg<6, D>(ctx, a, mode);
    }
    return gss_fail(ctx, GSS_ERR_UNSUPPORTED, "cacgmm: K=%d", K);
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
    if (mode != EM_PRIOR_FIRST && K >= 2 && K <= 6 && !gss_variant_set("estep_lds")) {
        switch (a.D) {
            case 24: return launch_estep_prior_reg_k<24>(ctx, a, K, mode);
            case 20: return launch_estep_prior_reg_k<20>(ctx, a, K, mode);
            case 12: return launch_estep_prior_reg_k<12>(ctx, a, K, mode);
            case 10: return launch_estep_prior_reg_k<10>(ctx, a, K, mode);
            case 4: return launch_estep_prior_reg_k<4>(ctx, a, K, mode);
        }
    }
    GSS_REQUIRE(ctx, sizeof(cplx) * 64 * (size_t)a.D <= 64 * 1024, GSS_ERR_UNSUPPORTED,
                "cacgmm (shared prior): D=%d", a.D);
#define GSS_PRIOR_CASE(N) \
    case N: return launch_estep_prior<N>(ctx, a, mode);
    switch (K) {
        GSS_PRIOR_CASE(1) GSS_PRIOR_CASE(2) GSS_PRIOR_CASE(3) GSS_PRIOR_CASE(4) GSS_PRIOR_CASE(5)
        GSS_PRIOR_CASE(6) GSS_PRIOR_CASE(7) GSS_PRIOR_CASE(8) GSS_PRIOR_CASE(9) GSS_PRIOR_CASE(10)
        GSS_PRIOR_CASE(11) GSS_PRIOR_CASE(12) GSS_PRIOR_CASE(13) GSS_PRIOR_CASE(14)
        GSS_PRIOR_CASE(15) GSS_PRIOR_CASE(16) GSS_PRIOR_CASE(17) GSS_PRIOR_CASE(18)
        GSS_PRIOR_CASE(19)
    }
#undef GSS_PRIOR_CASE
    return gss_fail(ctx, GSS_ERR_UNSUPPORTED, "cacgmm: K=%d", K);
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
