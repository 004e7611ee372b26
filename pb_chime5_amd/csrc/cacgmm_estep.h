// The pieces of the CACGMM E-step that its kernels share: the walk over the packed triangle
// (register form and run-time-D form), the posterior in ratio form with its log-form fall-back,
// the epilogue (clip, M-step weight, sums of gamma), the first-iteration affiliations, and the
// dispatch from run-time (D, K) to the compiled shapes.  Each kernel keeps its own thread mapping,
// loads and stores:
//   em_estep_kernel            (cacgmm.hip)        first_affiliations; its own four-wave walk
//   em_estep_reg_kernel        (cacgmm.hip)        quad_forms_reg, posterior_ratio, estep_finish
//   em_estep_prior_kernel      (cacgmm_prior.hip)  first_affiliations, quad_forms_lds, estep_finish
//   em_estep_prior_reg_kernel  (cacgmm_prior.hip)  quad_forms_reg; its own posterior and epilogue
//   cacgmm_loglik_kernel       (cacgmm_model.hip)  quad_forms_lds
// (em_onchip4_kernel keeps its own first iteration.)
#pragma once
#include <type_traits>
#include <utility>

#include "gss_internal.h"

#ifndef GSS_ESTEP_PRIO
#define GSS_ESTEP_PRIO 1      // wave priority falling with progress in the register-form E-step
#endif

// a step of the register-form E-step's wave priority (a kernel starts at 3 before it loads its
// frame, quad_forms_reg lowers it)
template <int P>
__device__ __forceinline__ void estep_priority() {
#if GSS_ESTEP_PRIO
    __builtin_amdgcn_s_setprio(P);
#endif
}

// ------------------------------------------------------------------ quadratic forms
// q_k = sum_{d <= e} Re(Mq_k,de) Re(P_de) + Im(Mq_k,de) Im(P_de),  P_de = y_d conj(y_e): 4 real FMAs
// per (entry, class) against the doubled off-diagonals, entries in packed (row-major) order, the K
// model values of an entry wave-uniform (scalar loads through the __restrict__ pointer, so the
// model costs no LDS or vector-memory bandwidth).  (The imaginary parts of a diagonal entry and
// of its product are zero: skipping them changes no bit of q.)

// The frame in registers, the triangle fully unrolled.  A ring of model rows: the row of entry
// e + P is requested before entry e is evaluated, and a scheduling barrier per entry keeps the
// compiler from hoisting every row of the unrolled triangle to the top (which would spill
// thousands of SGPRs).  Priority falls with the wave's progress: the waves of a SIMD converge
// instead of finishing oldest first, and the end of the launch is not a row of single waves
// finishing alone.
template <int K, int D>
__device__ __forceinline__ void quad_forms_reg(const cplx (&y)[D], const cplx *__restrict__ Mf,
                                               double (&q)[K]) {
    constexpr int NE = D * (D + 1) / 2;
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
            if (e == NE / 4) estep_priority<2>();
            if (e == NE / 2) estep_priority<1>();
            if (e == 3 * NE / 4) estep_priority<0>();
        }
    }
}

// The walk sits at the 128 registers of four waves per SIMD and at the SGPR limit, and nothing
// orders the epilogue's loads after it: activity bytes, ln det, weights -- or the lane masks made
// of them -- were moved above the walk and spilled its ring of model rows lane by lane (5 x
// slower).  So the indices of those loads pass through an empty statement that also names the
// walk's result: their values are untouched, and nothing that uses them can move above it.
__device__ __forceinline__ void hold_below_walk(double q0, int64_t &t, int &k) {
    asm volatile("" : "+v"(t), "+v"(k) : "v"(q0));
}

// A run-time channel count: registers cannot be indexed, so the lane has parked the D values of
// its frame in its own 16-byte column of LDS, ys[d * 64 + lane] (consecutive lanes on consecutive
// slots: conflict free as ds_read_b128).  No barrier, no exchange between lanes.
template <int K>
__device__ __forceinline__ void quad_forms_lds(const cplx *ys, int lane, int D,
                                               const cplx *__restrict__ mrow, double (&q)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) q[k] = 0.0;
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
}

// ------------------------------------------------------------------ posterior, ratio form
// pi_k exp(-D ln q_k - ln det_k) / sum  without a logarithm per frame: relative to the class with
// the smallest q it is  (q_min / q_k)^D c_k  with  c_k = pi_k exp(ln det_min - ln det_k)  -- the
// common factor cancels in the normalisation.  c_k is one exponential per class and WAVE (lane k
// computes it, an SGPR pair hands it to all lanes) instead of K logarithms and K exponentials per
// FRAME: the transcendental functions were 600 of the register kernel's 5200 instructions per
// wave, and the integer power is the more accurate form (24 roundings against the 1e-13 of
// exp(500 +- ...)).  One reciprocal per class (iq) serves the ratio and the M-step weight
// gamma / q, one more (returned) the normalisation: gamma_k = v_k * returned.  A frame whose
// terms all underflow (sum < 1e-280: the classes' ln det hundreds apart AND the q ratios against
// them) takes the log form, which is also the form of em_estep_kernel: the max over ALL classes,
// as pb_bss takes it before the mask is multiplied in.
//   q         in: the walk's result; out: max(|q|, tiny)
//   ldl, pil  lane k holds ln det_k and pi_k (lanes >= K: any class's)
//   on        the activity of the lane's frame, used when `masked`
// One basic block but for the fall-back: a branch per class would split it, and the walk's scalar
// loads are then all hoisted to the top -- thousands of SGPR spills.
// One caller, em_estep_reg_kernel.  em_estep_prior_reg_kernel has the same steps with prior[k, t]
// multiplied in after the coefficient and in the fall-back, in its own text: sharing this one
// through a flag cost its D = 4 instantiations 1 % of the shared-prior call.
template <int K, int D>
__device__ __forceinline__ double posterior_ratio(double (&q)[K], double (&iq)[K], double (&v)[K],
                                                  double ldl, double pil, const bool (&on)[K],
                                                  int masked) {
    double cls;
    {
        double ldmin = INFINITY;
#pragma unroll
        for (int k = 0; k < K; ++k) ldmin = fmin(ldmin, lane_bcast(ldl, k));
        cls = pil * exp(ldmin - ldl);
    }
    double qmin = INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        q[k] = fmax(fabs(q[k]), GSS_TINY);
        qmin = fmin(qmin, q[k]);
    }
    double ssum = 0.0;
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
        v[k] = p * lane_bcast(cls, k);
        v[k] = (!masked || on[k]) ? v[k] : 0.0;
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
            v[k] = exp(lp[k] - mx) * lane_bcast(pil, k);
            v[k] = (!masked || on[k]) ? v[k] : 0.0;
            ssum += v[k];
        }
    }
    return 1.0 / fmax(ssum, GSS_TINY);
}

// ------------------------------------------------------------------ epilogue
// gamma_k = v_k * norm (RECIP) or v_k / norm, clipped to [aff_eps, 1 - aff_eps]; then
//   PREDICT   out[k T] = gamma_k
//   otherwise out[k T] = W = gamma_k / max(q_k, 10 tiny) -- RECIP: by the reciprocal iq_k the
//             ratio form already has --, G[k T] = gamma_k (WITH_G: the shared prior's update
//             reads it), and Sg[k] = the sum of gamma_k over the wave's valid lanes.
// out and G are (F, K, T) arrays, row = f K the frequency's first row in them and t the lane's
// frame; Sg points at the caller's record of K sums.
// Every element is written by exactly one lane: no atomics, the same call gives the same bits.
template <int K, bool PREDICT, bool RECIP, bool WITH_G>
__device__ __forceinline__ void estep_finish(const double (&v)[K], double norm,
                                             const double (&q)[K], const double (&iq)[K],
                                             double aff_eps, bool valid, int lane, int64_t T,
                                             int64_t row, int64_t t, double *out, double *G,
                                             double *Sg) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double gam = RECIP ? v[k] * norm : v[k] / norm;
        if (aff_eps != 0.0) gam = fmin(fmax(gam, aff_eps), 1.0 - aff_eps);
        if (PREDICT) {
            if (valid) out[(row + k) * T + t] = gam;
        } else {
            if (valid) {
                out[(row + k) * T + t] =
                        RECIP ? gam * (q[k] < 10.0 * GSS_TINY ? 1.0 / (10.0 * GSS_TINY) : iq[k])
                              : gam / fmax(q[k], 10.0 * GSS_TINY);
                if (WITH_G) G[(row + k) * T + t] = gam;
            }
            const double tot = wave_sum(valid ? gam : 0.0);
            if (lane == 0) Sg[k] = tot;
        }
    }
}

// ------------------------------------------------------------------ first iteration
// The affiliations the EM starts from, for one frame: init[k * init_stride] as given, not
// renormalised (fit(initialization=array)), or, with init == NULL, the GSS initialisation
// (core.py:156-160)  where(act == 0, 1e-10, act) / sum_k.
template <int K>
__device__ __forceinline__ void first_affiliations(const double *init, int64_t init_stride,
                                                   const bool (&on)[K], double (&g)[K]) {
    if (init != nullptr) {
#pragma unroll
        for (int k = 0; k < K; ++k) g[k] = init[(int64_t)k * init_stride];
    } else {
        double ssum = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            g[k] = on[k] ? 1.0 : 1e-10;
            ssum += g[k];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) g[k] = g[k] / ssum;
    }
}

// ------------------------------------------------------------------ dispatch
// Run-time counts to compile-time ones: fn(std::integral_constant<int, N>{}) for the N of the
// list that equals n; false when none does.
template <int... Ns, class Fn>
bool dispatch_int(int n, std::integer_sequence<int, Ns...>, int &rc, Fn &&fn) {
    return ((n == Ns && (rc = fn(std::integral_constant<int, Ns>{}), true)) || ...);
}
// K = 1 .. 19 (pb_bss: assert K < 20, CACGMMTrainer.fit)
template <class Fn>
int dispatch_classes(gss_ctx *ctx, int K, Fn &&fn) {
    int rc = GSS_OK;
    if (dispatch_int(K, std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14,
                                              15, 16, 17, 18, 19>{}, rc, fn))
        return rc;
    return gss_fail(ctx, GSS_ERR_UNSUPPORTED, "cacgmm: K=%d", K);
}
// The shapes with a register-form E-step: D = 4 x arrays (all microphones), 2 x arrays (outer
// microphones) or 4 (reference array) for the 5 and 6 array sessions of the corpus, 2 - 6 classes.
using EstepRegChannels = std::integer_sequence<int, 24, 20, 12, 10, 4>;
using EstepRegClasses = std::integer_sequence<int, 2, 3, 4, 5, 6>;
template <int... Ns>
bool contains(int n, std::integer_sequence<int, Ns...>) {
    return ((n == Ns) || ...);
}
inline bool estep_reg_supported(int D, int K) {
    return contains(D, EstepRegChannels{}) && contains(K, EstepRegClasses{});
}
// fn(integral_constant D, integral_constant K) for such a shape
template <class Fn>
int dispatch_reg_shape(gss_ctx *ctx, int D, int K, Fn &&fn) {
    int rc = GSS_OK;
    bool hit = false;
    dispatch_int(D, EstepRegChannels{}, rc, [&](auto d) {
        int r = GSS_OK;
        hit = dispatch_int(K, EstepRegClasses{}, r, [&](auto k) { return fn(d, k); });
        return r;
    });
    return hit ? rc : gss_fail(ctx, GSS_ERR_UNSUPPORTED, "cacgmm: K=%d", K);
}
