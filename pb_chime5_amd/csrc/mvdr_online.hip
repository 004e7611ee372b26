// Online MVDR: Souden's mask-based MVDR (optionally with blind analytic normalisation) whose
// statistics are exponentially forgetting running sums and whose filter is recomputed at every
// frame (include/gss_hip.h: gss_mvdr_online).  Per frequency, for every
// frame t in order, with y = Y[f,t,:], a = mask_x[f,t], b = mask_n[f,t]:
//   Phi_X <- beta Phi_X + a y y^H,   Phi_N <- beta Phi_N + b y y^H
//   Phi_N = U^H U (a pivot that is not > 0 or not finite: a FALLBACK frame -- w = 0, X = 0, the
//   frame is counted, the update above stays)
//   w = (Phi_N^-1 Phi_X)[:, ref] / max(Re trace(Phi_N^-1 Phi_X), 1e-10)
//   ban:  v = Phi_N w,  w <- w sqrt(v^H v) / |w^H v|   (w^H v = 0, a zero filter: w stays 0)
//   X[f,t] = w^H y                       (the sums include frame t: look-ahead L, default 0 --
//                                         L >= 1: the look-ahead kernels further down)
// Only the two running sums are a recurrence in time, but the factorisation of frame t needs the
// sums of frame t, so one persistent wave per frequency walks the frames of the call with both
// matrices in LDS.  Per frame: the rank-one update on the 8 x 8 lane grid, chol_inverse_sweep
// (dense_wave.h; U and W = U^-H = L^-1 in one register-resident pass of D steps), then with
// Phi_N^-1 = W^H W
//   B  = W Phi_X (lower triangle and column ref only),  tr = sum_{i >= k} Re(B_ik conj(W_ik)),
//   w  = W^H B[:, ref] / max(tr, 1e-10)
// -- no explicit Psi and no triangular substitutions.  The form (the template argument NR =
// ceil(D / 8), the leading dimension 8 NR + 1) and every order of summation depend on D alone,
// never on T, F or where a call begins: a recording fed in blocks gives the bits of one call.
// Both sums keep the FULL Hermitian matrix; (i, j) and (j, i) are updated with operations that
// commute with conjugation (c_outer, real scalings), so the lower triangle stays the exact
// conjugate of the upper one and the diagonal exactly real.  No floating-point atomics.
//
// The frame is written once, mol_frame<NR>; the kernels below are the I/O around it.
#include "dense_wave.h"

namespace {

// ---- look-ahead L (gss_mvdr_online_lookahead*) --------------------------
// Frame g is filtered with the filter of frame g + L.  mol_frame takes the frame that enters the
// sums from LDS (s.yb) and the frame the filter is applied to as a register argument, so with
// L > 0 the two kernels hand it two different frames and the frame body, the sums and every filter
// keep their bits.  A wave then walks the sequence "the h frames the line holds, then the T frames
// of the call": at step t frame t of the call enters, element j = h + t - L of the sequence is
// filtered into output row j (j < 0: the line is still filling, the result is dropped).
//
// The line of one (target, frequency): the held frames (L, D) oldest first, their target-mask
// values (L) and the filter of the last frame that entered (D).  Every wave reads and writes only
// its own line.
struct MolHold {
    cplx *frames;    // (F, L, D)
    double *mask;    // (F, L)
    cplx *filter;    // (F, D)
};

struct MolLine {
    const cplx *Yf;      // the call's frames of this frequency (T, D)
    const double *mf;    // their target-mask values (T)
    cplx *Hf;            // the held frames (L, D)
    double *hm;          // their target-mask values (L)
    cplx *wl;            // the last filter (D)
    int64_t T;
    int h, L, D;
    __device__ __forceinline__ cplx frame(int64_t i, int lane) const {
        return i < h ? Hf[i * D + lane] : Yf[(i - h) * D + lane];
    }
    __device__ __forceinline__ double mask(int64_t i) const { return i < h ? hm[i] : mf[i - h]; }
};

// After the call's frames: the last filter, and the new line -- the last n = min(L, h + T)
// elements of the sequence.  With T < L the line shifts in place: slot i takes element
// i + (h + T - n) >= i, every lane moves its own channel in ascending i (lane 0 the mask values),
// so a value is read before its slot is written.
__device__ __forceinline__ void mol_line_store(const MolLine &q, cplx w, int lane) {
    const int64_t total = q.h + q.T;
    const int n = (int)(total < q.L ? total : q.L);
    const int64_t base = total - n;
    if (lane < q.D) {
        q.wl[lane] = w;
        for (int i = 0; i < n; ++i) {
            const cplx v = q.frame(base + i, lane);
            q.Hf[i * q.D + lane] = v;
        }
    }
    if (lane == 0)
        for (int i = 0; i < n; ++i) {
            const double v = q.mask(base + i);
            q.hm[i] = v;
        }
}

struct MolArgs {
    const cplx *Y;           // (F, T, D)
    const double *mx, *mn;   // (F, T)
    cplx *phi_x, *phi_n;     // (F, D, D)
    cplx *X;                 // element (f, t) at [f xs_f + t xs_t]
    int64_t xs_f, xs_t;
    cplx *W;                 // (F, T, D) or NULL
    const int32_t *ref_dev;  // the reference channel of a whole-window pass, NULL: `ref`
    int32_t *fallbacks;      // the call's device counter
    int32_t *status;         // status word of the reference channel
    int32_t *ref_out;        // the reference channel used, or NULL
    int64_t T;
    int D, ref, ban;
    double beta;
    MolHold hold;            // the delay line; read only with L > 0
    int64_t R;               // rows of W per frequency: T without a look-ahead
    int L, held;             // the look-ahead and the frames the line holds; L = 0: none
};

// p_f = mean |Y[f]|^2 over the T D values handed in (1 when there are none or the mean is 0),
// Phi_X = 0, Phi_N = loading p_f I.  Thread j sums the values j, j + 256, ... in ascending
// order, the 256 partial sums are added by a fixed tree.
__global__ __launch_bounds__(256) void mvdr_online_init_kernel(const cplx *__restrict__ Y, int64_t T,
                                                               int D, double loading,
                                                               cplx *__restrict__ phi_x,
                                                               cplx *__restrict__ phi_n) {
    __shared__ double part[256];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int64_t total = Y ? T * D : 0;
    double acc = 0.0;
    for (int64_t i = tid; i < total; i += 256) {
        const cplx v = Y[(int64_t)f * total + i];
        acc = fma(v.x, v.x, acc);
        acc = fma(v.y, v.y, acc);
    }
    part[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) part[tid] += part[tid + s];
        __syncthreads();
    }
    double p = total > 0 ? part[0] / (double)total : 1.0;
    if (p == 0.0) p = 1.0;
    const double delta = loading * p;
    for (int idx = tid; idx < D * D; idx += 256) {
        const int r = idx / D, c = idx - r * D;
        phi_x[(int64_t)f * D * D + idx] = c_make(0.0, 0.0);
        phi_n[(int64_t)f * D * D + idx] = c_make(r == c ? delta : 0.0, 0.0);
    }
}

// The LDS of one wave: Phi_X, Phi_N and the sweep's rows M, each D rows of ld = 8 NR + 1 complex
// values (odd: the lanes that walk a column fall on different 16-byte slots), y, B[:, ref], w and
// the sweep's 1 / U_jj (mol_lds_bytes).
template <int NR>
struct MolLds {
    static constexpr int ld = 8 * NR + 1;
    cplx *PX, *PN, *M, *yb, *cb, *wb;
    double *dinv;
    __device__ __forceinline__ MolLds(char *smem, int D) {
        PX = reinterpret_cast<cplx *>(smem);
        PN = PX + D * ld;
        M = PN + D * ld;
        yb = M + D * ld;      // 8 NR each
        cb = yb + 8 * NR;
        wb = cb + 8 * NR;
        dinv = reinterpret_cast<double *>(wb + 8 * NR);
    }
};

// A state handed in is read from its upper triangle and the real part of its diagonal.
__device__ __forceinline__ void mol_load(const cplx *__restrict__ g, cplx *m, int D, int ld, int lane) {
    for (int idx = lane; idx < D * D; idx += 64) {
        const int r = idx / D, c = idx - r * D;
        cplx v = r <= c ? g[idx] : c_conj(g[c * D + r]);
        if (r == c) v.y = 0.0;
        m[r * ld + c] = v;
    }
}

// The two sums after the call's frames -> the state, the full matrices.
template <int NR>
__device__ __forceinline__ void mol_store(const MolLds<NR> &s, cplx *__restrict__ gx,
                                          cplx *__restrict__ gn, int D, int lane) {
    constexpr int ld = MolLds<NR>::ld;
    for (int idx = lane; idx < D * D; idx += 64) {
        const int r = idx / D, c = idx - r * D;
        gx[idx] = s.PX[r * ld + c];
        gn[idx] = s.PN[r * ld + c];
    }
}

// One frame of one wave: y (lane < D holds y[lane]; also in s.yb, published by a wave_sync) with
// the mask values ma, mb -> the filter w (lane < D holds w[lane]) and x = w^H y.  Lane (ty, tx) =
// (lane >> 3, lane & 7) owns the entries (ty + 8 a, tx + 8 b) of both sums and of the sweep's
// register tile.  false: a fallback frame, w = 0 and x = 0, the sums advanced all the same.
template <int NR>
__device__ __forceinline__ bool mol_frame(const MolLds<NR> &s, cplx y, double ma, double mb,
                                          double beta, int ref, int ban, int D, int lane, int tx,
                                          int ty, cplx &w, cplx &x) {
    constexpr int ld = MolLds<NR>::ld;
    cplx *const PX = s.PX, *const PN = s.PN, *const M = s.M;
    cplx *const yb = s.yb, *const cb = s.cb, *const wb = s.wb;
    double *const dinv = s.dinv;
    const bool row = lane < D;
    const cplx zero = c_make(0.0, 0.0);
    // the two running sums; the sweep's tile is the upper triangle of the new Phi_N
    cplx reg[NR][NR];
#pragma unroll
    for (int ai = 0; ai < NR; ++ai)
#pragma unroll
        for (int bi = 0; bi < NR; ++bi) {
            const int i = ty + 8 * ai, k = tx + 8 * bi;
            reg[ai][bi] = zero;
            if (i < D && k < D) {
                const cplx o = c_outer(yb[i], yb[k]);
                const cplx px = PX[i * ld + k], pn = PN[i * ld + k];
                PX[i * ld + k] = c_make(fma(beta, px.x, ma * o.x), fma(beta, px.y, ma * o.y));
                const cplx nn = c_make(fma(beta, pn.x, mb * o.x), fma(beta, pn.y, mb * o.y));
                PN[i * ld + k] = nn;
                if (k >= i) reg[ai][bi] = nn;
            }
        }
    wave_sync();
    const bool ok = chol_inverse_sweep<8, NR, true>(reg, D, M, ld, dinv, tx, ty);
    w = zero, x = zero;
    if (ok) {   // decided by the pivots alone, the same in every lane
        // M: row i holds W[i][k] / dinv[i] for k < i; W[i][i] = dinv[i].
        // B[i][k] = dinv[i] (sum_{j<i} M[i][j] Phi_X[j][k] + Phi_X[i][k])
        double trp = 0.0;
#pragma unroll
        for (int ai = 0; ai < NR; ++ai) {
            const int i = ty + 8 * ai;
            if (i < D) {
                cplx acc[NR];
#pragma unroll
                for (int bi = 0; bi <= ai; ++bi) acc[bi] = zero;
                for (int j = 0; j < i; ++j) {
                    const cplx m = M[i * ld + j];
#pragma unroll
                    for (int bi = 0; bi <= ai; ++bi) c_fma(acc[bi], m, PX[j * ld + min(tx + 8 * bi, D - 1)]);
                }
                const double d2 = dinv[i] * dinv[i];
#pragma unroll
                for (int bi = 0; bi <= ai; ++bi) {
                    const int k = tx + 8 * bi;
                    if (k <= i) {
                        const cplx bu = c_add(acc[bi], PX[i * ld + k]);
                        const cplx m = k < i ? M[i * ld + k] : c_make(1.0, 0.0);
                        trp = fma(d2, fma(bu.x, m.x, bu.y * m.y), trp);
                    }
                }
            }
        }
        // cb[i] = dinv[i] B[i][ref]
        if (row) {
            cplx acc = zero;
            for (int j = 0; j < lane; ++j) c_fma(acc, M[lane * ld + j], PX[j * ld + ref]);
            acc = c_add(acc, PX[lane * ld + ref]);
            cb[lane] = c_scale(acc, dinv[lane] * dinv[lane]);
        }
        const double tr = wave_sum(trp);
        wave_sync();
        // w[k] = sum_{i >= k} conj(W[i][k]) B[i][ref] / max(tr, eps)
        if (row) {
            cplx acc = cb[lane];
            for (int i = lane + 1; i < D; ++i) c_cfma(acc, M[i * ld + lane], cb[i]);
            w = c_scale(acc, 1.0 / fmax(tr, 1e-10));
        }
        if (ban) {
            if (row) wb[lane] = w;
            wave_sync();
            cplx v = zero;     // (Phi_N w)[i], from column i of the Hermitian matrix
            if (row)
                for (int k = 0; k < D; ++k) c_cfma(v, PN[k * ld + lane], wb[k]);
            const double vv = wave_sum(fma(v.x, v.x, v.y * v.y));
            cplx wv = zero;
            c_cfma(wv, w, v);
            const double wr = wave_sum(wv.x), wi = wave_sum(wv.y);
            // eps = 0 as upstream, but a filter that is exactly zero (no target mass yet: the
            // context frames of every window) stays zero where upstream divides 0 by 0
            const double den = hypot(wr, wi);
            w = c_scale(w, den == 0.0 ? 0.0 : sqrt(vv) / den);
        }
        cplx p = zero;
        c_cfma(p, w, y);
        x = c_make(wave_sum(p.x), wave_sum(p.y));
    }
    return ok;
}

// One wave per frequency.  The masks are the caller's, X is strided, the reference channel may
// come from a whole-window pass (ref_dev; none found: NaN, the state untouched).  y and the two
// mask values of frame t + 1 are fetched while frame t's dependent chain runs.  With a look-ahead
// (L > 0) the frame that enters and the frame the filter is applied to differ: the second one,
// element j + 1 of the line's sequence, has an address known a step ahead and is fetched beside
// the first, off the dependent chain.  The walk is compiled twice, LOOK = false being the loop
// without a line -- one frame fetched, the filter applied to it, no row index, no line -- and the
// kernel picks one by a.L, the same in every wave of the grid.
template <int NR, bool LOOK>
__device__ __forceinline__ void mol_walk(const MolArgs &a, char *smem) {
    const int D = a.D;
    const MolLds<NR> s(smem, D);
    const int f = blockIdx.x, lane = threadIdx.x;
    const int tx = lane & 7, ty = lane >> 3;
    const bool row = lane < D;
    const int64_t T = a.T;
    const cplx zero = c_make(0.0, 0.0);
    const cplx *Yf = a.Y + (int64_t)f * T * D;
    const double *mxf = a.mx + (int64_t)f * T, *mnf = a.mn + (int64_t)f * T;
    cplx *Xf = a.X + (int64_t)f * a.xs_f;
    cplx *Wf = a.W ? a.W + (int64_t)f * a.R * D : nullptr;
    cplx *gx = a.phi_x + (int64_t)f * D * D, *gn = a.phi_n + (int64_t)f * D * D;
    const int L = LOOK ? a.L : 0, h = LOOK ? a.held : 0;
    const MolLine q{Yf, mxf, a.hold.frames + (int64_t)f * L * D, a.hold.mask + (int64_t)f * L,
                    a.hold.filter + (int64_t)f * D, T, h, L, D};   // LOOK only

    const int ref = a.ref_dev ? a.ref_dev[0] : a.ref;
    if (f == 0 && lane == 0) {
        __hip_atomic_store(a.status, ref < 0 ? -1 : ref, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (a.ref_out) a.ref_out[0] = ref < 0 ? -1 : ref;
    }
    if (ref < 0) {   // the whole-window pass found no finite SNR: as mvdr_apply_kernel, state untouched
        const double qnan = __longlong_as_double(0x7ff8000000000000LL);
        for (int64_t t = lane; t < T; t += 64) Xf[t * a.xs_t] = c_make(qnan, qnan);
        if (Wf)
            for (int64_t i = lane; i < T * D; i += 64) Wf[i] = c_make(qnan, qnan);
        return;
    }
    mol_load(gx, s.PX, D, s.ld, lane);
    mol_load(gn, s.PN, D, s.ld, lane);
    wave_sync();

    const double beta = a.beta;
    int64_t j = (int64_t)h - L;      // LOOK: the element of the sequence step t filters
    cplx y_next = zero;
    if (row) y_next = Yf[lane];
    cplx d_next = zero;              // LOOK: the delayed frame
    if constexpr (LOOK)
        if (row && j >= 0) d_next = q.frame(j, lane);
    double ma_next = mxf[0], mb_next = mnf[0];
    int nfall = 0;
    cplx wl = zero;                  // LOOK: the last filter
    for (int64_t t = 0; t < T; ++t) {
        const cplx e = y_next;
        const double ma = ma_next, mb = mb_next;
        if (row) s.yb[lane] = e;
        if (t + 1 < T) {
            if (row) y_next = Yf[(t + 1) * D + lane];
            ma_next = mxf[t + 1];
            mb_next = mnf[t + 1];
        }
        cplx w, x;
        if constexpr (LOOK) {
            const cplx y = d_next;
            if (t + 1 < T && row && j + 1 >= 0) d_next = q.frame(j + 1, lane);
            wave_sync();
            if (!mol_frame<NR>(s, y, ma, mb, beta, ref, a.ban, D, lane, tx, ty, w, x)) ++nfall;
            if (j >= 0) {            // j < 0: the line is still filling, the result is dropped
                if (lane == 0) Xf[j * a.xs_t] = x;
                if (Wf && row) Wf[j * D + lane] = w;
            }
            wl = w;
            ++j;
        } else {
            wave_sync();
            if (!mol_frame<NR>(s, e, ma, mb, beta, ref, a.ban, D, lane, tx, ty, w, x)) ++nfall;
            if (lane == 0) Xf[t * a.xs_t] = x;
            if (Wf && row) Wf[t * D + lane] = w;
        }
    }
    wave_sync();
    mol_store<NR>(s, gx, gn, D, lane);
    if constexpr (LOOK) mol_line_store(q, wl, lane);
    if (lane == 0 && nfall) atomicAdd(a.fallbacks, nfall);
}

template <int NR>
__global__ __launch_bounds__(64) void mvdr_online_kernel(MolArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (a.L > 0) mol_walk<NR, true>(a, smem);
    else mol_walk<NR, false>(a, smem);
}

// S targets of one stream (gss_mvdr_online_targets).
struct MolTargetsArgs {
    const cplx *Y;           // (F, T, D)
    const double *gamma;     // (F, K, T): the posteriors, the masks are formed here
    cplx *phi_x[GSS_CACGMM_ONLINE_MAX_CLASSES], *phi_n[GSS_CACGMM_ONLINE_MAX_CLASSES];  // (F, D, D) each
    int32_t target[GSS_CACGMM_ONLINE_MAX_CLASSES];
    double *mx, *mn;         // (S, F, T) or NULL: the masks, for the debug taps only
    cplx *X;                 // (S, T, F)
    cplx *W;                 // (S, F, T, D) or NULL
    int32_t *fallbacks;      // (S, F): the fallback frames of every wave
    int32_t *status;         // status word of the reference channel
    int32_t *ref_out;        // (S,) the reference channel used, or NULL
    int64_t T;
    int F, D, K, ref, ban, postfilter;
    double beta;
    MolHold hold[GSS_CACGMM_ONLINE_MAX_CLASSES];   // the delay lines; read only with L > 0
    int64_t R, Xrows;        // rows of W, and of X, per target: T without a look-ahead
    int L, held;             // the look-ahead and the frames every line holds; L = 0: none
    int release;             // the end of the lines: nothing enters, the held frames leave
};

// grid (F, S): one wave per (frequency, target), no LDS and no barrier shared between the waves
// of a frequency.  The frame is mol_frame, the one mvdr_online_kernel runs: target s has the bits
// of that kernel on the masks of class target[s].  What differs is around it: the masks come from
// the posteriors -- a = gamma[target], b = the sum over k != target in ascending k from 0.0,
// masks_kernel's expressions --, whose K values of frame t + 1 are fetched while frame t's chain
// runs; the postfilter 'mask_mul' (re a, im a: mask_mul_kernel's product) is applied to the
// stored value; X is (S, T, F); every wave has a count word of its own.  With a look-ahead the
// walk is mvdr_online_kernel's, the postfilter takes the target mask the line carries with the
// output frame, and X is (S, Xrows, F); `release` ends the lines: nothing enters and no sum is
// touched, the held frames leave with the filter of the last frame that entered.
template <int NR, bool LOOK>
__device__ __forceinline__ void mol_walk_targets(const MolTargetsArgs &a, char *smem) {
    constexpr int KMAX = GSS_CACGMM_ONLINE_MAX_CLASSES;
    const int D = a.D, K = a.K, F = a.F;
    const MolLds<NR> l(smem, D);
    const int f = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
    const int tx = lane & 7, ty = lane >> 3;
    const bool row = lane < D;
    const int64_t T = a.T;
    const cplx zero = c_make(0.0, 0.0);
    const int target = a.target[s], ref = a.ref;
    const cplx *Yf = a.Y + (int64_t)f * T * D;
    const double *gf = a.gamma + (int64_t)f * K * T;
    const int64_t sf = (int64_t)s * F + f;
    double *mxf = a.mx ? a.mx + sf * T : nullptr, *mnf = a.mn ? a.mn + sf * T : nullptr;
    cplx *Xs = a.X + (int64_t)s * a.Xrows * F + f;
    cplx *Wf = a.W ? a.W + sf * a.R * D : nullptr;
    const int L = LOOK ? a.L : 0, h = LOOK ? a.held : 0;
    const MolHold &line = a.hold[LOOK ? s : 0];                     // LOOK only
    const MolLine q{Yf, gf + (int64_t)target * T, line.frames + (int64_t)f * L * D,
                    line.mask + (int64_t)f * L, line.filter + (int64_t)f * D, T, h, L, D};
    if (LOOK && a.release) {   // the held frames with the last filter: mol_frame's product and sum
        cplx w = zero;
        if (row) w = q.wl[lane];
        for (int i = 0; i < h; ++i) {
            cplx y = zero, p = zero;
            if (row) y = q.Hf[i * D + lane];
            c_cfma(p, w, y);
            const cplx x = c_make(wave_sum(p.x), wave_sum(p.y));
            if (lane == 0) Xs[(int64_t)i * F] = a.postfilter ? c_scale(x, q.hm[i]) : x;
            if (Wf && row) Wf[i * D + lane] = w;
        }
        return;
    }
    cplx *gx = a.phi_x[s] + (int64_t)f * D * D, *gn = a.phi_n[s] + (int64_t)f * D * D;

    if (f == 0 && lane == 0) {
        if (s == 0) __hip_atomic_store(a.status, ref, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (a.ref_out) a.ref_out[s] = ref;
    }
    mol_load(gx, l.PX, D, l.ld, lane);
    mol_load(gn, l.PN, D, l.ld, lane);
    wave_sync();

    const double beta = a.beta;
    int64_t j = (int64_t)h - L;      // LOOK: the element of the sequence step t filters
    cplx y_next = zero;
    if (row) y_next = Yf[lane];
    cplx d_next = zero;              // LOOK: the delayed frame and its target mask
    double p_next = 0.0;
    if constexpr (LOOK)
        if (j >= 0) {
            if (row) d_next = q.frame(j, lane);
            p_next = q.mask(j);
        }
    double g_next[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) g_next[k] = k < K ? gf[(int64_t)k * T] : 0.0;
    int nfall = 0;
    cplx wl = zero;                  // LOOK: the last filter
    for (int64_t t = 0; t < T; ++t) {
        const cplx e = y_next;
        double ma = 0.0, mb = 0.0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) {
                if (k == target) ma = g_next[k];
                else mb += g_next[k];
            }
        if (row) l.yb[lane] = e;
        if (t + 1 < T) {
            if (row) y_next = Yf[(t + 1) * D + lane];
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (k < K) g_next[k] = gf[(int64_t)k * T + t + 1];
        }
        cplx w, x;
        if constexpr (LOOK) {
            const cplx y = d_next;
            const double pm = p_next;
            if (t + 1 < T && j + 1 >= 0) {
                if (row) d_next = q.frame(j + 1, lane);
                p_next = q.mask(j + 1);
            }
            wave_sync();
            if (!mol_frame<NR>(l, y, ma, mb, beta, ref, a.ban, D, lane, tx, ty, w, x)) ++nfall;
            if (lane == 0) {
                // the postfilter takes the target mask of the OUTPUT frame j, which the line carries
                if (j >= 0) Xs[j * F] = a.postfilter ? c_scale(x, pm) : x;
                if (mxf) mxf[t] = ma;
                if (mnf) mnf[t] = mb;
            }
            if (Wf && row && j >= 0) Wf[j * D + lane] = w;
            wl = w;
            ++j;
        } else {
            wave_sync();
            if (!mol_frame<NR>(l, e, ma, mb, beta, ref, a.ban, D, lane, tx, ty, w, x)) ++nfall;
            if (lane == 0) {
                Xs[t * F] = a.postfilter ? c_scale(x, ma) : x;
                if (mxf) mxf[t] = ma;
                if (mnf) mnf[t] = mb;
            }
            if (Wf && row) Wf[t * D + lane] = w;
        }
    }
    wave_sync();
    mol_store<NR>(l, gx, gn, D, lane);
    if constexpr (LOOK) mol_line_store(q, wl, lane);
    if (lane == 0) a.fallbacks[sf] = nfall;   // every wave writes its own word: no atomic, no memset
}

template <int NR>
__global__ __launch_bounds__(64) void mvdr_online_targets_kernel(MolTargetsArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (a.L > 0) mol_walk_targets<NR, true>(a, smem);
    else mol_walk_targets<NR, false>(a, smem);
}

// counts (S, F) -> words[1 + s] = the sum over f of target s, words[0] = the sum over the targets.
// One workgroup: thread j sums the values j, j + 256, ... of a target, a fixed tree adds the 256
// partial sums.
__global__ __launch_bounds__(256) void mvdr_online_targets_count_kernel(
    const int32_t *__restrict__ counts, int F, int S, int32_t *__restrict__ words) {
    __shared__ int32_t part[256];
    const int tid = threadIdx.x;
    int32_t total = 0;
    for (int s = 0; s < S; ++s) {
        int32_t acc = 0;
        for (int f = tid; f < F; f += 256) acc += counts[(int64_t)s * F + f];
        part[tid] = acc;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if (tid < h) part[tid] += part[tid + h];
            __syncthreads();
        }
        if (tid == 0) {
            words[1 + s] = part[0];
            total += part[0];
        }
        __syncthreads();
    }
    if (tid == 0) words[0] = total;
}

size_t mol_lds_bytes(int D) {
    const size_t nr = (size_t)(D + 7) / 8, ld = 8 * nr + 1;
    return sizeof(cplx) * (3 * (size_t)D * ld + 3 * 8 * nr) + sizeof(double) * 8 * nr;
}

// One wave per workgroup of `grid` with the LDS of D channels, the form NR = ceil(D / 8) of
// `kernels` = {<1>, <2>, <3>, <4>}.
template <typename Args>
int mol_launch(gss_ctx *ctx, void (*const (&kernels)[4])(Args), dim3 grid, int D, const Args &a) {
    const size_t lds = mol_lds_bytes(D);
    void (*const kernel)(Args) = kernels[(D - 1) / 8];
    if (lds > 48 * 1024)
        GSS_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, grid, dim3(64), lds, ctx->stream, a);
    return GSS_OK;
}
#define GSS_MOL_KERNELS(kernel) {kernel<1>, kernel<2>, kernel<3>, kernel<4>}

}  // namespace

// the counter and, for a thrown-away state, its two matrices
struct MolWork {
    int32_t *words;         // [0]: fallback counter, [1]: the window's ref
    cplx *phi_x, *phi_n;
};
static MolWork mol_blocks(Workspace &ws, int F, int D, bool fresh) {
    MolWork k;
    k.words = ws.take<int32_t>(4, "online mvdr words");
    k.phi_x = fresh ? ws.take<cplx>((size_t)F * D * D, "online mvdr phi_x") : nullptr;
    k.phi_n = fresh ? ws.take<cplx>((size_t)F * D * D, "online mvdr phi_n") : nullptr;
    return k;
}
// ref_channel = -1, above a mark: the output of the whole-window pass, which nobody asked for
static cplx *mol_window_blocks(Workspace &ws, int F, int64_t T) {
    return ws.take<cplx>((size_t)F * T, "online mvdr window X");
}

size_t mvdr_online_workspace_bytes(int F, int64_t T, int D, bool fresh, bool window_ref) {
    Workspace ws;
    mol_blocks(ws, F, D, fresh);
    if (window_ref) mol_window_blocks(ws, F, T);
    return ws.bytes + (window_ref ? mvdr_workspace_bytes(F, T, D) : 0) + 4096;
}

int mvdr_online_init_run(gss_ctx *ctx, int F, int D, const cplx *Y, int64_t T, double loading,
                         cplx *phi_x, cplx *phi_n) {
    GSS_PROF(ctx, "mvdr_online_init");
    hipLaunchKernelGGL(mvdr_online_init_kernel, dim3(F), dim3(256), 0, ctx->stream,
                       T > 0 ? Y : nullptr, T, D, loading, phi_x, phi_n);
    GSS_LAUNCH_CHECK(ctx, "mvdr_online_init_kernel");
    return GSS_OK;
}

// phi_x, phi_n: the caller's state, advanced in place; both NULL: a fresh state from the arena,
// initialised from Y with `loading`, thrown away.  X: element (f, t) at [f xs_f + t xs_t].
// ref < 0: the reference channel of the whole-window beamformer over the call's frames;
// ref_out: receives the channel used.  The
// arguments have been validated by the entry point (T >= 1).
int mvdr_online_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D, const double *mx,
                    const double *mn, int ban, double beta, double loading, int ref, cplx *phi_x,
                    cplx *phi_n, cplx *X, int64_t xs_f, int64_t xs_t, cplx *W,
                    int32_t *ref_out) {
    Workspace ws(ctx);
    const MolWork k = mol_blocks(ws, F, D, !phi_x);
    GSS_TRY(ws.status("online mvdr"));
    int32_t *words = k.words;
    if (!phi_x) {
        phi_x = k.phi_x, phi_n = k.phi_n;
        GSS_TRY(mvdr_online_init_run(ctx, F, D, Y, T, loading, phi_x, phi_n));
    }
    ctx->last_targets = 0;
    GSS_HIP_CHECK(ctx, hipMemsetAsync(words, 0, sizeof(int32_t) * 4, ctx->stream));
    const int32_t *ref_dev = nullptr;
    if (ref < 0) {
        const size_t mark = ctx->arena_off;
        cplx *Xw = mol_window_blocks(ws, F, T);
        GSS_TRY(ws.status("online mvdr window"));
        GSS_TRY(mvdr_run(ctx, Y, F, T, D, mx, mn, ban, Xw, words + 1));
        GSS_TRY(arena_release(ctx, mark));
        ref_dev = words + 1;
    }
    const MolArgs a{Y, mx, mn, phi_x, phi_n, X, xs_f, xs_t, W, ref_dev, words, ctx->status_dev,
                    ref_out, T, D, ref, ban, beta, MolHold{}, T, 0, 0};
    {
        GSS_PROF(ctx, "mvdr_online");
        GSS_TRY(mol_launch(ctx, GSS_MOL_KERNELS(mvdr_online_kernel), dim3(F), D, a));
        GSS_LAUNCH_CHECK(ctx, "mvdr_online_kernel");
    }
    // the count of this call -> the context's status word
    GSS_HIP_CHECK(ctx, hipMemcpyAsync(ctx->status_host + GSS_STATUS_MVDR_ONLINE_FALLBACKS, words,
                                      sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    return GSS_OK;
}

// the counters of a targets call: one word per wave, and their sums: [0] over everything,
// [1 + s] of target s
struct MolTargetsWork {
    int32_t *counts, *words;
};
static MolTargetsWork mol_targets_blocks(Workspace &ws, int F, int S) {
    MolTargetsWork k;
    k.counts = ws.take<int32_t>((size_t)S * F, "online mvdr targets counts");
    k.words = ws.take<int32_t>(1 + GSS_CACGMM_ONLINE_MAX_CLASSES, "online mvdr targets words");
    return k;
}

// the per-wave counts -> the context's status words: the sum where the one-target call leaves
// its count, then one word per target
static int mol_counts_to_status(gss_ctx *ctx, const MolTargetsWork &k, int F, int S) {
    hipLaunchKernelGGL(mvdr_online_targets_count_kernel, dim3(1), dim3(256), 0, ctx->stream, k.counts,
                       F, S, k.words);
    GSS_LAUNCH_CHECK(ctx, "mvdr_online_targets_count_kernel");
    GSS_HIP_CHECK(ctx, hipMemcpyAsync(ctx->status_host + GSS_STATUS_MVDR_ONLINE_FALLBACKS, k.words,
                                      sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    GSS_HIP_CHECK(ctx, hipMemcpyAsync(ctx->status_host + GSS_STATUS_MVDR_ONLINE_TARGETS, k.words + 1,
                                      sizeof(int32_t) * S, hipMemcpyDeviceToHost, ctx->stream));
    return GSS_OK;
}

size_t mvdr_online_targets_workspace_bytes(int F, int S) {
    Workspace ws;
    mol_targets_blocks(ws, F, S);
    return ws.bytes + 4096;
}

// S targets (1 <= S <= GSS_CACGMM_ONLINE_MAX_CLASSES) from the posteriors gamma (F,K,T), each
// with the caller's state, advanced in place.  X (S,T,F); mx / mn (S,F,T) or NULL; W (S,F,T,D)
// or NULL; ref_out (S,) or NULL.  The arguments have been validated by the entry point (T >= 1,
// ref >= 0), which also records S for gss_last_mvdr_online_fallbacks_targets where the call is
// one of S targets for its caller (the one-target stream block runs this with S = 1).
int mvdr_online_targets_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D,
                            const double *gamma, int K, const int32_t *targets, int S, int ban,
                            double beta, int ref, cplx *const *phi_x, cplx *const *phi_n,
                            int postfilter, double *mx, double *mn, cplx *X, cplx *W,
                            int32_t *ref_out) {
    Workspace ws(ctx);
    const MolTargetsWork k = mol_targets_blocks(ws, F, S);
    GSS_TRY(ws.status("online mvdr targets"));
    ctx->last_targets = 0;
    MolTargetsArgs a{};
    a.Y = Y, a.gamma = gamma, a.mx = mx, a.mn = mn, a.X = X, a.W = W;
    a.fallbacks = k.counts, a.status = ctx->status_dev, a.ref_out = ref_out;
    a.T = T, a.F = F, a.D = D, a.K = K, a.ref = ref, a.ban = ban, a.postfilter = postfilter;
    a.beta = beta, a.R = T, a.Xrows = T;
    for (int s = 0; s < S; ++s) a.phi_x[s] = phi_x[s], a.phi_n[s] = phi_n[s], a.target[s] = targets[s];
    {
        GSS_PROF(ctx, "mvdr_online_targets");
        GSS_TRY(mol_launch(ctx, GSS_MOL_KERNELS(mvdr_online_targets_kernel), dim3(F, S), D, a));
        GSS_LAUNCH_CHECK(ctx, "mvdr_online_targets_kernel");
        GSS_TRY(mol_counts_to_status(ctx, k, F, S));
    }
    return GSS_OK;
}

// ---- look-ahead: the runs ------------------------------------------------------------------
size_t mvdr_online_lookahead_workspace_bytes(int F, int S) {
    return mvdr_online_targets_workspace_bytes(F, S);
}

static MolHold mol_hold(const gss_mvdr_online_hold &h) {
    return MolHold{reinterpret_cast<cplx *>(h.frames), h.mask, reinterpret_cast<cplx *>(h.filter)};
}

int64_t mvdr_online_lookahead_rows(const gss_mvdr_online_hold *hold, int64_t T) {
    const int64_t r = (int64_t)hold->held + T - hold->L;
    return r > 0 ? r : 0;
}

// the line's host counter after T more frames
static void mol_hold_advance(gss_mvdr_online_hold *holds, int S, int64_t T) {
    for (int s = 0; s < S; ++s) {
        const int64_t total = (int64_t)holds[s].held + T;
        holds[s].held = (int32_t)(total < holds[s].L ? total : holds[s].L);
    }
}

int mvdr_online_hold_init_run(gss_ctx *ctx, gss_mvdr_online_hold *hold) {
    const size_t F = (size_t)hold->F, L = (size_t)hold->L, D = (size_t)hold->D;
    GSS_HIP_CHECK(ctx, hipMemsetAsync(hold->frames, 0, sizeof(cplx) * F * L * D, ctx->stream));
    GSS_HIP_CHECK(ctx, hipMemsetAsync(hold->mask, 0, sizeof(double) * F * L, ctx->stream));
    GSS_HIP_CHECK(ctx, hipMemsetAsync(hold->filter, 0, sizeof(cplx) * F * D, ctx->stream));
    hold->held = 0;
    return GSS_OK;
}

int mvdr_online_lookahead_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D, const double *mx,
                              const double *mn, int ban, double beta, int ref, cplx *phi_x,
                              cplx *phi_n, gss_mvdr_online_hold *hold, cplx *X, cplx *W) {
    Workspace ws(ctx);
    const MolWork k = mol_blocks(ws, F, D, false);
    GSS_TRY(ws.status("online mvdr look-ahead"));
    ctx->last_targets = 0;
    GSS_HIP_CHECK(ctx, hipMemsetAsync(k.words, 0, sizeof(int32_t) * 4, ctx->stream));
    const int64_t R = mvdr_online_lookahead_rows(hold, T);
    const MolArgs a{Y, mx, mn, phi_x, phi_n, X, R, 1, W, nullptr, k.words, ctx->status_dev, nullptr,
                    T, D, ref, ban, beta, mol_hold(*hold), R, hold->L, hold->held};
    {
        GSS_PROF(ctx, "mvdr_online_lookahead");
        GSS_TRY(mol_launch(ctx, GSS_MOL_KERNELS(mvdr_online_kernel), dim3(F), D, a));
        GSS_LAUNCH_CHECK(ctx, "mvdr_online_kernel");
    }
    GSS_HIP_CHECK(ctx, hipMemcpyAsync(ctx->status_host + GSS_STATUS_MVDR_ONLINE_FALLBACKS, k.words,
                                      sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    mol_hold_advance(hold, 1, T);
    return GSS_OK;
}

int mvdr_online_lookahead_targets_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D,
                                      const double *gamma, int K, const int32_t *targets, int S,
                                      int ban, double beta, int ref, cplx *const *phi_x,
                                      cplx *const *phi_n, gss_mvdr_online_hold *holds, int postfilter,
                                      double *mx, double *mn, cplx *X, int64_t Xrows, cplx *W,
                                      int32_t *ref_out) {
    Workspace ws(ctx);
    const MolTargetsWork k = mol_targets_blocks(ws, F, S);
    GSS_TRY(ws.status("online mvdr look-ahead targets"));
    ctx->last_targets = 0;
    MolTargetsArgs a{};
    a.Y = Y, a.gamma = gamma, a.mx = mx, a.mn = mn, a.X = X, a.W = W;
    a.fallbacks = k.counts, a.status = ctx->status_dev, a.ref_out = ref_out;
    a.T = T, a.R = mvdr_online_lookahead_rows(holds, T), a.Xrows = Xrows;
    a.F = F, a.D = D, a.K = K, a.ref = ref, a.ban = ban, a.postfilter = postfilter;
    a.L = holds[0].L, a.held = holds[0].held, a.beta = beta;
    for (int s = 0; s < S; ++s) {
        a.phi_x[s] = phi_x[s], a.phi_n[s] = phi_n[s], a.target[s] = targets[s];
        a.hold[s] = mol_hold(holds[s]);
    }
    {
        GSS_PROF(ctx, "mvdr_online_lookahead_targets");
        GSS_TRY(mol_launch(ctx, GSS_MOL_KERNELS(mvdr_online_targets_kernel), dim3(F, S), D, a));
        GSS_LAUNCH_CHECK(ctx, "mvdr_online_targets_kernel");
        GSS_TRY(mol_counts_to_status(ctx, k, F, S));
    }
    mol_hold_advance(holds, S, T);
    return GSS_OK;
}

int mvdr_online_release_run(gss_ctx *ctx, gss_mvdr_online_hold *holds, int S, int postfilter, cplx *X,
                            int64_t Xrows, cplx *W) {
    const int h = holds[0].held;
    if (h > 0) {
        MolTargetsArgs a{};
        for (int s = 0; s < S; ++s) a.hold[s] = mol_hold(holds[s]);
        a.X = X, a.W = W, a.Xrows = Xrows, a.R = h;
        a.F = holds[0].F, a.D = holds[0].D, a.L = holds[0].L, a.held = h, a.postfilter = postfilter;
        a.release = 1;
        GSS_PROF(ctx, "mvdr_online_release");
        GSS_TRY(mol_launch(ctx, GSS_MOL_KERNELS(mvdr_online_targets_kernel), dim3(a.F, S), a.D, a));
        GSS_LAUNCH_CHECK(ctx, "mvdr_online_targets_kernel");
    }
    for (int s = 0; s < S; ++s) holds[s].held = 0;
    return GSS_OK;
}
