// Mask post-processing and mask-based MVDR (Souden) beamforming with blind
// analytic normalisation:
//   enhance_observation mask handling            core.py:537-554
//   beamform_mvdr_souden_from_masks / _Beamformer speech_enhancement/beamforming_wrapper.py:11-124
//   -> pb_bss.extraction.beamformer.{get_power_spectral_density_matrix,
//      get_mvdr_vector_souden(eps=1e-10), blind_analytic_normalization,
//      apply_beamforming_vector}
#include "dense_wave.h"
#include "gss_internal.h"
#include "jacobi.h"

namespace {

constexpr int PSD_TILE = 64;

// gamma (F,K,T) -> target (F,T), distortion (F,T); Python slice semantics for the
// zeroed context frames (masks[:, :start] = 0; if end > 0: masks[:, -end:] = 0).
__global__ void masks_kernel(const double *__restrict__ gamma, int F, int K, int64_t T,
                             int target, int64_t zero_lo_end, int64_t zero_hi_begin,
                             double *__restrict__ mx, double *__restrict__ mn) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)F * T) return;
    const int f = idx / T;
    const int64_t t = idx - (int64_t)f * T;
    double x = 0.0, n = 0.0;
    if (t >= zero_lo_end && t < zero_hi_begin) {
        const double *g = gamma + (int64_t)f * K * T + t;
        x = g[(int64_t)target * T];
        for (int k = 0; k < K; ++k)
            if (k != target) n += g[(int64_t)k * T];
    }
    mx[idx] = x;
    mn[idx] = n;
}

// S targets at once: gamma (F,K,T) -> mx, mn (S,F,T), one thread per (f, t) for every target.
// Each target's values are masks_kernel's expressions (the distortion sum in the same k
// order), with that target's own context range.
__global__ void masks_targets_kernel(const double *__restrict__ gamma, int F, int K, int64_t T,
                                     TargetMaskArgs a, double *__restrict__ mx,
                                     double *__restrict__ mn) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)F * T) return;
    const int f = idx / T;
    const int64_t t = idx - (int64_t)f * T;
    const double *g = gamma + (int64_t)f * K * T + t;
    for (int s = 0; s < a.S; ++s) {
        const int target = a.target[s];
        double x = 0.0, n = 0.0;
        if (t >= a.zero_lo_end[s] && t < a.zero_hi_begin[s]) {
            x = g[(int64_t)target * T];
            for (int k = 0; k < K; ++k)
                if (k != target) n += g[(int64_t)k * T];
        }
        mx[(int64_t)s * F * T + idx] = x;
        mn[(int64_t)s * F * T + idx] = n;
    }
}

// Pack ROWS masks into the (F, ROWS, T) weight layout of the shared covariance kernel
// (cacgmm.hip: wcov_kernel) and sum them over time: two rows [target, distortion] for the MVDR,
// three [target, interferer, noise] for the LCMV.  grid (F, S), block 256: target blockIdx.y
// packs its own (F,T) masks into its own (F, ROWS, T) block and (F, ROWS) sums.
template <int ROWS>
struct MaskRows {
    const double *m[ROWS];     // (S,F,T) each
};
template <int ROWS>
__global__ __launch_bounds__(256) void mask_pack_kernel(MaskRows<ROWS> rows, int64_t T,
                                                        double *__restrict__ Wr,
                                                        double *__restrict__ msum) {
    __shared__ double red[4 * ROWS];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int64_t F = gridDim.x, s = blockIdx.y;
    Wr += s * F * ROWS * T;
    msum += s * F * ROWS;
    double sum[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) sum[r] = 0.0;
    for (int64_t t = tid; t < T; t += blockDim.x) {
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const double a = rows.m[r][(s * F + f) * T + t];
            Wr[((int64_t)f * ROWS + r) * T + t] = a;
            sum[r] += a;
        }
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) sum[r] = wave_sum(sum[r]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int r = 0; r < ROWS; ++r) red[4 * r + (tid >> 6)] = sum[r];
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
            msum[f * ROWS + r] = (red[4 * r] + red[4 * r + 1]) + (red[4 * r + 2] + red[4 * r + 3]);
    }
}

__device__ __forceinline__ cplx c_div(cplx a, cplx b) {
    // Smith's algorithm (what NumPy uses for complex division)
    if (fabs(b.x) >= fabs(b.y)) {
        if (b.x == 0.0 && b.y == 0.0) return c_make(a.x / fabs(b.x), a.y / fabs(b.x));
        const double r = b.y / b.x, den = b.x + b.y * r;
        return c_make((a.x + a.y * r) / den, (a.y - a.x * r) / den);
    }
    const double r = b.x / b.y, den = b.x * r + b.y;
    return c_make((a.x * r + a.y) / den, (a.y * r - a.x) / den);
}

// ------------------------------------------------------------------ the solve of a beamformer
// The steps mvdr_solve_kernel and lcmv_solve_kernel are made of (gev_solve_kernel takes the first
// few).  One workgroup of MVDR_NT threads per frequency works on an LDS block `aug` of D rows with
// leading dimension ld (2 D or 3 D) of which `used` columns are in use: the D x D matrix, then
// D-wide right-hand blocks.  Every element of every step is computed by exactly the expressions a
// single wave used until round 5 (the rank-1 update of an LU step, the products of the SNR terms
// are element-wise), so the result does not depend on the thread count: four waves take the
// 23 x 47 element update of the first step in 5 trips instead of 17 -- the kernel was one wave's
// latency chain per frequency (120 us for ~10 000 instructions), not work.  Pivot search, back
// substitution (one right-hand side per lane) and the Jacobi fallback stay with wave 0.
// The build contracts within a statement (-ffp-contract=on): an arithmetic statement below is
// not to be split, merged or reordered, and no sum changes its order.
#ifndef GSS_MVDR_NT
#define GSS_MVDR_NT 256        // (tools/build_variant.sh NAME -DGSS_MVDR_NT=64: the same bits from one wave)
#endif
constexpr int MVDR_NT = GSS_MVDR_NT;

// Element e of the ROWS packed matrices of frequency f, each summed over the nch chunks in
// ascending order: part (F, nch, ROWS, NE), the partial sums of the PSD pass.
template <int ROWS>
__device__ __forceinline__ void partials_sum(const cplx *__restrict__ part, int f, int nch, int NE,
                                             int e, cplx (&v)[ROWS]) {
#pragma unroll
    for (int r = 0; r < ROWS; ++r) v[r] = c_make(0.0, 0.0);
    for (int c = 0; c < nch; ++c) {
        const cplx *pp = part + ((int64_t)f * nch + c) * ROWS * NE;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) v[r] = c_add(v[r], pp[r * NE + e]);
    }
}

// Element e = (d1, d2) of Phi_X and Phi_N from the two-row partial sums: S / max(s, 1e-10) with
// an exactly real diagonal.
__device__ __forceinline__ void phi_pair(const cplx *__restrict__ part, int f, int nch, int NE,
                                         int e, bool diagonal, double dx, double dn, cplx &vx,
                                         cplx &vn) {
    cplx v[2];
    partials_sum<2>(part, f, nch, NE, e, v);
    vx = c_make(v[0].x / dx, v[0].y / dx);
    vn = c_make(v[1].x / dn, v[1].y / dn);
    if (diagonal) {
        vx.y = 0.0;
        vn.y = 0.0;
    }
}

// v to (d1, d2) and its conjugate to (d2, d1) of a Hermitian matrix (in this order: a diagonal
// element ends as conj(v))
__device__ __forceinline__ void herm_store(cplx *M, int ld, int d1, int d2, cplx v) {
    M[d1 * ld + d2] = v;
    M[d2 * ld + d1] = c_conj(v);
}

// Largest `best` of the 64 lanes with its index `bi`, the lowest index among equal values; the
// result in every lane.
__device__ __forceinline__ void wave_argmax_first(double &best, int &bi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) {
            best = ob;
            bi = oi;
        }
    }
}

// LU with partial pivoting (pivot by |re| + |im| like LAPACK izamax) of the left D x D block,
// applied to all `used` columns: [M | R] -> [U | Z], the multipliers below the diagonal.
// flags[0]: the pivot row of a step; flags[1]: set on a zero or NaN pivot, where the elimination
// stops -- the caller zeroes it in front of the barrier that ends its fill.  Returns "singular".
__device__ __forceinline__ bool lu_eliminate(cplx *aug, int ld, int used, int D, int *flags) {
    constexpr int NT = MVDR_NT;
    const int tid = threadIdx.x, lane = tid & 63;
    const bool wave0 = tid < 64;                   // (D <= 32: one wave holds a column)
    int &s_piv = flags[0];
    int &s_singular = flags[1];
    for (int j = 0; j < D; ++j) {
        if (wave0) {
            double best = -1.0;
            int bi = j;
            if (lane >= j && lane < D) {
                const cplx v = aug[lane * ld + j];
                best = fabs(v.x) + fabs(v.y);
                bi = lane;
            }
            wave_argmax_first(best, bi);
            if (lane == 0) {
                s_piv = bi;
                if (!(best > 0.0)) s_singular = 1;   // zero or NaN pivot
            }
        }
        __syncthreads();
        if (s_singular) break;
        const int p = s_piv;
        if (p != j) {
            for (int col = tid; col < used; col += NT) {
                const cplx t = aug[j * ld + col];
                aug[j * ld + col] = aug[p * ld + col];
                aug[p * ld + col] = t;
            }
        }
        __syncthreads();
        const cplx piv = aug[j * ld + j];
        const int rows = D - j - 1, cols = used - j - 1;
        // multipliers first (column j), then the rank-1 update
        for (int i = tid; i < rows; i += NT) {
            const int r = j + 1 + i;
            aug[r * ld + j] = c_div(aug[r * ld + j], piv);
        }
        __syncthreads();
        for (int it = tid; it < rows * cols; it += NT) {
            const int i = it / cols, cidx = it - i * cols;
            const int r = j + 1 + i, col = j + 1 + cidx;
            const cplx l = aug[r * ld + j], u = aug[j * ld + col];
            cplx v = aug[r * ld + col];
            v.x -= l.x * u.x - l.y * u.y;
            v.y -= l.x * u.y + l.y * u.x;
            aug[r * ld + col] = v;
        }
        __syncthreads();
    }
    return s_singular != 0;
}

// Back substitution U X = Z in place, one right-hand side per lane (nrhs <= 58: wave 0).
__device__ __forceinline__ void back_substitute(cplx *aug, int ld, int D, int nrhs) {
    const int tid = threadIdx.x;
    if (tid < nrhs) {
        const int col = D + tid;
        for (int j = D - 1; j >= 0; --j) {
            cplx v = aug[j * ld + col];
            for (int k = j + 1; k < D; ++k) {
                const cplx u = aug[j * ld + k], x = aug[k * ld + col];
                v.x -= u.x * x.x - u.y * x.y;
                v.y -= u.x * x.y + u.y * x.x;
            }
            aug[j * ld + col] = c_div(v, aug[j * ld + j]);
        }
    }
    __syncthreads();
}

// np.linalg.lstsq(M, R) for an exactly singular M: the minimum-norm solution via the Hermitian
// eigendecomposition, singular values below eps * D * max dropped.  The block holds [M | R] as
// filled (the elimination has overwritten it: the caller fills it again, with a barrier, before
// this); every right-hand block is replaced by its solution, the left block is used up.
// JA, JV: m x m each (m = D rounded up to even); *s_cut: a double in LDS.
__device__ __forceinline__ void min_norm_solve(cplx *aug, int ld, int used, int D, int m, cplx *JA,
                                               cplx *JV, double *s_cut) {
    constexpr int NT = MVDR_NT;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int idx = tid; idx < m * m; idx += NT) {
        const int i = idx / m, jx = idx - i * m;
        JA[idx] = (i < D && jx < D) ? aug[i * ld + jx] : c_make(0.0, 0.0);
    }
    __syncthreads();
    if (tid < 64) {
        jacobi_eigh_wave(JA, JV, m, lane, 20);
        double lmax = 0.0;
        for (int i = lane; i < D; i += 64) lmax = fmax(lmax, fabs(JA[i * m + i].x));
        lmax = wave_max(lmax);
        if (lane == 0) *s_cut = 2.220446049250313e-16 * (double)D * lmax;
    }
    __syncthreads();
    const double cut = *s_cut;
    // each right-hand side R in turn: tmp = diag(1/l) V^H R -> the left block, V tmp -> R
    for (int c0 = D; c0 < used; c0 += D) {
        for (int it = tid; it < D * D; it += NT) {
            const int j = it / D, col = it - j * D;
            cplx v = c_make(0.0, 0.0);
            for (int i = 0; i < D; ++i) c_cfma(v, JV[i * m + j], aug[i * ld + c0 + col]);
            const double l = JA[j * m + j].x;
            const double il = fabs(l) > cut ? 1.0 / l : 0.0;
            aug[j * ld + col] = c_scale(v, il);
        }
        __syncthreads();
        for (int it = tid; it < D * D; it += NT) {
            const int i = it / D, col = it - i * D;
            cplx v = c_make(0.0, 0.0);
            for (int j = 0; j < D; ++j) c_fma(v, JV[i * m + j], aug[j * ld + col]);
            aug[i * ld + c0 + col] = v;
        }
        __syncthreads();
    }
}

// W = Psi / max(Re tr Psi, eps), Psi the D x D block at column c0: to the left block (where the
// SNR terms read it) and to Wf (D,D) in global memory.  *s_den: a double in LDS.
// (every thread reads its elements of Psi before anyone overwrites the left block: the two are
// disjoint)
__device__ __forceinline__ void trace_normalise(cplx *aug, int ld, int c0, int D, double eps,
                                                double *s_den, cplx *__restrict__ Wf) {
    constexpr int NT = MVDR_NT;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 64) {
        double tr = 0.0;
        for (int i = lane; i < D; i += 64) tr += aug[i * ld + c0 + i].x;
        tr = wave_sum(tr);
        if (lane == 0) *s_den = fmax(tr, eps);
    }
    __syncthreads();
    const double dentr = *s_den;
    for (int it = tid; it < D * D; it += NT) {
        const int i = it / D, col = it - i * D;
        const cplx v = aug[i * ld + c0 + col];
        const cplx wv = c_make(v.x / dentr, v.y / dentr);
        aug[i * ld + col] = wv;
        Wf[it] = wv;
    }
}

// SNR terms per reference channel r: w_r^H Phi_X w_r and w_r^H Phi_D w_r -> snr_f (D,2), W in
// the left block (behind a barrier of the caller's).  The products T_X = Phi_X W (-> the block
// at column cx) and T_D = Phi_D W (-> JA) are spread over the whole workgroup; the sums over e
// and then over d run in the same order as one lane per r would take them.
// (reads: W in the left block, Phi_X / Phi_D in global memory; writes: the block at cx and JA --
// disjoint, no barrier inside the first loop)
__device__ __forceinline__ void snr_terms(cplx *aug, int ld, int cx, int D, int m, cplx *JA,
                                          const cplx *PhiX, const cplx *PhiD,
                                          cplx *__restrict__ snr_f) {
    constexpr int NT = MVDR_NT;
    const int tid = threadIdx.x;
    for (int it = tid; it < D * D; it += NT) {
        const int d = it / D, r = it - d * D;
        cplx tx = c_make(0.0, 0.0), tn = c_make(0.0, 0.0);
        for (int e = 0; e < D; ++e) {
            const cplx we = aug[e * ld + r];
            c_fma(tx, PhiX[d * D + e], we);
            c_fma(tn, PhiD[d * D + e], we);
        }
        aug[d * ld + cx + r] = tx;
        JA[d * m + r] = tn;
    }
    __syncthreads();
    if (tid < D) {
        const int r = tid;
        cplx num = c_make(0.0, 0.0), den = c_make(0.0, 0.0);
        for (int d = 0; d < D; ++d) {
            const cplx wd = aug[d * ld + r];
            c_cfma(num, wd, aug[d * ld + cx + r]);
            c_cfma(den, wd, JA[d * m + r]);
        }
        snr_f[r * 2] = num;
        snr_f[r * 2 + 1] = den;
    }
}

// Per frequency: Phi_X, Phi_N from the partial sums; Psi = solve(Phi_N, Phi_X) by LU with partial
// pivoting, pseudo-inverse (lstsq) fallback on an exactly singular Phi_N; W = Psi / max(Re tr Psi,
// eps); per-reference-channel SNR terms.
__global__ __launch_bounds__(MVDR_NT) void mvdr_solve_kernel(
    const cplx *__restrict__ part, const double *__restrict__ msum, int nch, int D, double eps,
    cplx *__restrict__ Phi /* (F,2,D,D) */, cplx *__restrict__ W /* (F,D,D) */,
    cplx *__restrict__ snr /* (F,D,2) */) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NT = MVDR_NT;
    {   // grid (F, S): target blockIdx.y works on its own block of every array
        const int64_t F = gridDim.x, s = blockIdx.y, NEs = tri_count(D);
        part += s * F * nch * 2 * NEs;
        msum += s * F * 2;
        Phi += s * F * 2 * D * D;
        W += s * F * D * D;
        snr += s * F * D * 2;
    }
    const int m = D + (D & 1);
    const int NE = tri_count(D);
    const int W2 = 2 * D;
    cplx *aug = reinterpret_cast<cplx *>(smem);   // D x 2D : [Phi_N | Phi_X] -> [U | Z] -> Psi
    cplx *JA = aug + D * W2;                       // m * m
    cplx *JV = JA + m * m;                         // m * m
    // flags live in the dynamic region too: a static __shared__ in front of it
    // would break its 16-byte alignment
    int *flags = reinterpret_cast<int *>(JV + m * m);        // lu_eliminate's two
    double *s_val = reinterpret_cast<double *>(flags + 2);   // the cut, then the denominator
    const int f = blockIdx.x, tid = threadIdx.x;

    const double sx = msum[f * 2], sn = msum[f * 2 + 1];
    const double dx = fmax(sx, 1e-10), dn = fmax(sn, 1e-10);
    cplx *PhiX = Phi + (int64_t)f * 2 * D * D;
    cplx *PhiN = PhiX + D * D;
    // (called again on a singular matrix: the elimination has overwritten the block by then)
    auto fill = [&]() {
        for (int e = tid; e < NE; e += NT) {
            int d1, d2;
            tri_unpack(e, D, d1, d2);
            cplx vx, vn;
            phi_pair(part, f, nch, NE, e, d1 == d2, dx, dn, vx, vn);
            herm_store(PhiX, D, d1, d2, vx);
            herm_store(PhiN, D, d1, d2, vn);
            herm_store(aug, W2, d1, d2, vn);
            herm_store(aug + D, W2, d1, d2, vx);
        }
    };
    fill();
    if (tid == 0) flags[1] = 0;
    __syncthreads();
    if (!lu_eliminate(aug, W2, W2, D, flags)) {
        back_substitute(aug, W2, D, D);
    } else {
        fill();
        __syncthreads();
        min_norm_solve(aug, W2, W2, D, m, JA, JV, s_val);
    }
    // Psi = aug[:, D:2D]
    trace_normalise(aug, W2, D, D, eps, s_val, W + (int64_t)f * D * D);
    __syncthreads();
    snr_terms(aug, W2, D, D, m, JA, PhiX, PhiN, snr + (int64_t)f * D * 2);
}

// GEV beamformer (beamforming_wrapper.py:77-89 -> pb_bss get_gev_vector): principal
// generalised eigenvector of (Phi_X, Phi_N), normalised like the generalised
// Hermitian eigensolvers do (w^H Phi_N w = 1; the phase is arbitrary, as upstream).
//   Phi_N = L L^H,  C = L^-1 Phi_X L^-H,  C u = lambda_max u,  w = L^-H u
// One wave per frequency; w is written to column 0 of W so that mvdr_apply (with
// ref = 0) does the BAN and the filtering.  A Phi_N that is not positive definite makes
// scipy.linalg.eigh -- and with it the reference -- raise LinAlgError: the frequency is
// recorded (ref[0] = -2, ref[1] = the lowest such frequency; the host presets 0 and a
// large number), mvdr_apply fills Xhat with NaN and the host raises.
__global__ __launch_bounds__(64) void gev_solve_kernel(const cplx *__restrict__ part,
                                                       const double *__restrict__ msum, int nch,
                                                       int D, cplx *__restrict__ Phi,
                                                       cplx *__restrict__ W,
                                                       int32_t *__restrict__ ref) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    {   // grid (F, S): target blockIdx.y works on its own block of every array, status ref[4 s]
        const int64_t F = gridDim.x, s = blockIdx.y, NEs = tri_count(D);
        part += s * F * nch * 2 * NEs;
        msum += s * F * 2;
        Phi += s * F * 2 * D * D;
        W += s * F * D * D;
        ref += 4 * s;
    }
    const int m = D + (D & 1);
    const int NE = tri_count(D);
    cplx *Ln = reinterpret_cast<cplx *>(smem);    // m * m : Phi_N -> L -> L^-1
    cplx *JA = Ln + m * m;                         // m * m : C
    cplx *JV = JA + m * m;                         // m * m : eigenvectors
    cplx *Tm = JV + m * m;                         // m * m : Linv Phi_X
    const int f = blockIdx.x, lane = threadIdx.x;

    const double dx = fmax(msum[f * 2], 1e-10), dn = fmax(msum[f * 2 + 1], 1e-10);
    cplx *PhiX = Phi + (int64_t)f * 2 * D * D;
    cplx *PhiN = PhiX + D * D;
    for (int idx = lane; idx < m * m; idx += 64) {
        Ln[idx] = c_make(0.0, 0.0);
        JA[idx] = c_make(0.0, 0.0);
    }
    __syncthreads();
    for (int e = lane; e < NE; e += 64) {
        int d1, d2;
        tri_unpack(e, D, d1, d2);
        cplx vx, vn;
        phi_pair(part, f, nch, NE, e, d1 == d2, dx, dn, vx, vn);
        herm_store(PhiX, D, d1, d2, vx);
        herm_store(PhiN, D, d1, d2, vn);
        Ln[d2 * m + d1] = c_conj(vn);          // lower triangle
        if (d1 == d2) Ln[d1 * m + d1] = vn;
    }
    __syncthreads();
    cplx *Wf = W + (int64_t)f * D * D;
    if (!cholesky_lower_wave(Ln, D, m, lane)) {
        for (int idx = lane; idx < D * D; idx += 64) Wf[idx] = c_make(NAN, NAN);
        if (lane == 0) {
            atomicMin(&ref[0], -2);
            atomicMin(&ref[1], f);
        }
        return;
    }
    invert_lower_wave(Ln, D, m, lane);          // Ln = L^-1 (lower)
    // Tm = Linv Phi_X
    for (int idx = lane; idx < D * D; idx += 64) {
        const int i = idx / D, j = idx - i * D;
        cplx v = c_make(0.0, 0.0);
        for (int k = 0; k <= i; ++k) c_fma(v, Ln[i * m + k], PhiX[k * D + j]);
        Tm[i * m + j] = v;
    }
    __syncthreads();
    // C = Tm Linv^H  (Hermitian)
    for (int idx = lane; idx < D * D; idx += 64) {
        const int i = idx / D, j = idx - i * D;
        cplx v = c_make(0.0, 0.0);
        for (int k = 0; k <= j; ++k) c_fmac(v, Tm[i * m + k], Ln[j * m + k]);
        JA[i * m + j] = v;
    }
    __syncthreads();
    // exact Hermitian symmetry for the Jacobi sweeps
    for (int idx = lane; idx < D * D; idx += 64) {
        const int i = idx / D, j = idx - i * D;
        if (i < j) {
            const cplx a = JA[i * m + j], b = JA[j * m + i];
            const cplx h = c_make(0.5 * (a.x + b.x), 0.5 * (a.y - b.y));
            Tm[i * m + j] = h;
            Tm[j * m + i] = c_conj(h);
        } else if (i == j) {
            Tm[i * m + i] = c_make(JA[i * m + i].x, 0.0);
        }
    }
    __syncthreads();
    for (int idx = lane; idx < m * m; idx += 64) {
        const int i = idx / m, j = idx - i * m;
        JA[idx] = (i < D && j < D) ? Tm[idx] : c_make(0.0, 0.0);
    }
    __syncthreads();
    jacobi_eigh_wave(JA, JV, m, lane, 20);
    // largest eigenvalue (first index on ties)
    double best = lane < D ? JA[lane * m + lane].x : -INFINITY;
    int bi = lane < D ? lane : 1 << 30;
    wave_argmax_first(best, bi);
    // w = Linv^H u :  w[d] = sum_{i >= d} conj(Linv[i][d]) u[i]
    for (int idx = lane; idx < D * D; idx += 64) {
        const int d = idx / D, col = idx - d * D;
        cplx v = c_make(0.0, 0.0);
        if (col == 0)
            for (int i = d; i < D; ++i) c_cfma(v, Ln[i * m + d], JV[i * m + bi]);
        Wf[idx] = v;
    }
}

// get_optimal_reference_channel: one reference channel for all frequencies.
// forced >= 0: the caller names the channel (pb_bss get_mvdr_vector_souden(ref_channel=...)).
// A non-finite SNR makes the reference abort the utterance (`assert np.all(np.isfinite(SNR))`):
// the channel becomes -1, mvdr_apply fills Xhat with NaN and the host raises.
constexpr int MVDR_REF_NT = 1024, MVDR_REF_CHUNK = 64;     // frequencies staged per round
__global__ __launch_bounds__(MVDR_REF_NT) void mvdr_ref_kernel(const cplx *__restrict__ snr, int F,
                                                              int D, double eps, int forced,
                                                              int32_t *__restrict__ ref) {
    // snr (F, D, 2) is one contiguous run: the whole workgroup copies MVDR_REF_CHUNK frequencies
    // of it to LDS at a time (coalesced, every load independent), then lane r of wave 0 adds its
    // channel's terms in ascending frequency -- the order one lane walking global memory took
    // until round 5 (64 dependent round trips to L2: 37 us for 25 000 numbers).
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cplx *buf = reinterpret_cast<cplx *>(smem);            // MVDR_REF_CHUNK * D * 2
    const int tid = threadIdx.x, lane = tid & 63;
    snr += (int64_t)blockIdx.x * F * D * 2;                 // grid (S): one workgroup per target
    ref += 4 * blockIdx.x;
    if (forced >= 0) {
        if (tid == 0) ref[0] = forced;
        return;
    }
    double val = -INFINITY;
    bool isnan_ = false;
    bool bad = false;
    cplx num = c_make(0.0, 0.0), den = c_make(0.0, 0.0);
    for (int f0 = 0; f0 < F; f0 += MVDR_REF_CHUNK) {
        const int nf = min(MVDR_REF_CHUNK, F - f0);
        const int total = nf * D * 2;
        __syncthreads();
        for (int i = tid; i < total; i += MVDR_REF_NT) buf[i] = snr[(int64_t)f0 * D * 2 + i];
        __syncthreads();
        if (tid < D) {
            for (int f = 0; f < nf; ++f) {
                num = c_add(num, buf[(f * D + tid) * 2]);
                den = c_add(den, buf[(f * D + tid) * 2 + 1]);
            }
        }
    }
    if (tid >= 64) return;
    if (lane < D) {
    // np.maximum(den, eps) on complex: lexicographic (real, then imag)
        if (!(den.x > eps || (den.x == eps && den.y > 0.0))) den = c_make(eps, 0.0);
        const cplx q = c_div(num, den);
        val = q.x;
        isnan_ = val != val;
        bad = !(isfinite(q.x) && isfinite(q.y));
    }
    const bool any_bad = __any(bad);
    // np.argmax: first maximum, NaN counts as maximum
    double best = val;
    int bi = lane < D ? lane : 1 << 30;
    bool bn = isnan_;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        const bool on = __shfl_xor((int)bn, o, 64) != 0;
        bool take;
        if (on != bn) take = on;
        else if (on) take = oi < bi;
        else take = ob > best || (ob == best && oi < bi);
        if (take) {
            best = ob;
            bi = oi;
            bn = on;
        }
    }
    if (lane == 0) ref[0] = any_bad ? -1 : bi;
}

// w = W[:, ref] (optionally BAN-normalised), Xhat[t][f] = w^H y_t.  grid (chunks, F)
// SEGMENTS (mvdr_segments_run): W (B,F,D,D) and Phi (B,F,2,D,D) hold one filter per segment
// of seg_frames frames; chunk_frames divides seg_frames, so a workgroup's frames lie in one
// segment and it takes that segment's w and Phi_N.  `fallbacks`: the call's device counter of
// (segment, frequency) pairs that fell back, copied to its status word.  Without SEGMENTS
// both arguments are unused: the whole-window instantiation is the kernel it always was.
template <bool SEGMENTS>
__global__ __launch_bounds__(256) void mvdr_apply_kernel(
    const cplx *__restrict__ Y, const cplx *__restrict__ W, const cplx *__restrict__ Phi,
    const int32_t *__restrict__ ref, int F, int64_t T, int D, int ban, int chunk_frames,
    cplx *__restrict__ Xhat, int32_t *__restrict__ ref_out, int32_t *__restrict__ status,
    int64_t seg_frames, const int32_t *__restrict__ fallbacks) {
    __shared__ cplx w[GSS_MAX_CHANNELS];
    __shared__ cplx t1[GSS_MAX_CHANNELS];
    __shared__ cplx t2[GSS_MAX_CHANNELS];
    __shared__ double s_norm;
    const int f = blockIdx.y, tid = threadIdx.x;
    const int r = ref[0];
    if (blockIdx.x == 0 && f == 0 && tid == 0) {
        // -1: non-finite SNR (MVDR); -2 - f: Phi_N of frequency f not positive definite (GEV)
        const int code = r == -2 ? -2 - ref[1] : r;
        if (ref_out) ref_out[0] = code;
        if (status) __hip_atomic_store(status, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (SEGMENTS)
            __hip_atomic_store(status + GSS_STATUS_SEGMENT_FALLBACKS, fallbacks[0], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
    }
    const int64_t c0 = (int64_t)blockIdx.x * chunk_frames;
    const int64_t c1 = c0 + chunk_frames < T ? c0 + chunk_frames : T;
    if (SEGMENTS) {   // this workgroup's (segment, frequency) block of W and Phi
        const int64_t blk = (c0 / seg_frames) * F;
        W += blk * D * D;
        Phi += blk * 2 * D * D;
    }
    if (r < 0) {   // the reference raises (see above), nothing meaningful to write
        const double qnan = __longlong_as_double(0x7ff8000000000000LL);
        for (int64_t t = c0 + tid; t < c1; t += blockDim.x) Xhat[t * F + f] = c_make(qnan, qnan);
        return;
    }
    if (tid < D) w[tid] = W[((int64_t)f * D + tid) * D + r];
    __syncthreads();
    if (ban) {
        const cplx *PhiN = Phi + ((int64_t)f * 2 + 1) * D * D;
        if (tid < D) {
            cplx v = c_make(0.0, 0.0);
            for (int e = 0; e < D; ++e) c_fma(v, PhiN[tid * D + e], w[e]);
            t1[tid] = v;   // Phi_N w
            cplx u = c_make(0.0, 0.0);   // (w^H Phi_N)_a = sum_d conj(w_d) Phi_N[d][a], a = tid
            for (int d = 0; d < D; ++d) c_cfma(u, w[d], PhiN[d * D + tid]);
            t2[tid] = u;
        }
        __syncthreads();
        if (tid == 0) {
            // nominator = w^H Phi_N Phi_N w ; denominator = w^H Phi_N w
            cplx nom = c_make(0.0, 0.0), den = c_make(0.0, 0.0);
            for (int a = 0; a < D; ++a) {
                c_fma(nom, t2[a], t1[a]);
                c_cfma(den, w[a], t1[a]);
            }
            const double n = sqrt(hypot(nom.x, nom.y));   // |sqrt(z)|
            const double dd = hypot(den.x, den.y);
            s_norm = n / dd;   // eps = 0 upstream: 0/0 -> NaN like the reference
        }
        __syncthreads();
        if (tid < D) w[tid] = c_scale(w[tid], s_norm);
        __syncthreads();
    }
    const cplx *Yf = Y + (int64_t)f * T * D;
    for (int64_t t = c0 + tid; t < c1; t += blockDim.x) {
        const cplx *y = Yf + t * D;
        cplx v = c_make(0.0, 0.0);
        for (int d = 0; d < D; ++d) c_cfma(v, w[d], y[d]);
        Xhat[t * F + f] = v;
    }
}

// mvdr_apply for S <= SB targets in one pass over Y.  grid (chunks, F), block 256.  Target s
// takes w = W_s[:, ref_s] (its own blocks of W / Phi / ref, see mvdr_solve_kernel), BAN-normalised
// with mvdr_apply_kernel's expressions; every observation vector y_t is loaded once and
// Xhat_s[t][f] = w_s^H y_t is accumulated over d in mvdr_apply_kernel's order for each target.
// ref_out[s] / status[s]: the target's status word; *status0: target 0's (gss_last_ref_channel).
template <int SB>
__global__ __launch_bounds__(256) void mvdr_apply_targets_kernel(
    const cplx *__restrict__ Y, const cplx *__restrict__ W, const cplx *__restrict__ Phi,
    const int32_t *__restrict__ ref, int F, int64_t T, int D, int S, int ban, int chunk_frames,
    cplx *__restrict__ Xhat, int32_t *__restrict__ ref_out, int32_t *__restrict__ status,
    int32_t *__restrict__ status0) {
    __shared__ cplx w[SB][GSS_MAX_CHANNELS];
    __shared__ cplx t1[SB][GSS_MAX_CHANNELS];
    __shared__ cplx t2[SB][GSS_MAX_CHANNELS];
    __shared__ double s_norm[SB];
    __shared__ int s_ref[SB];
    const int f = blockIdx.y, tid = threadIdx.x;
    if (tid < S) {
        const int r = ref[4 * tid];
        s_ref[tid] = r;
        if (blockIdx.x == 0 && f == 0) {
            const int code = r == -2 ? -2 - ref[4 * tid + 1] : r;
            if (ref_out) ref_out[tid] = code;
            if (status) __hip_atomic_store(status + tid, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (status0 && tid == 0)
                __hip_atomic_store(status0, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    __syncthreads();
    // (slots s >= S and failed targets hold w = 0: the accumulation below runs over all SB slots
    // without a branch, and only the S live rows are stored)
    for (int i = tid; i < SB * D; i += blockDim.x) {
        const int s = i / D, d = i - s * D;
        const int r = s < S ? s_ref[s] : -1;
        w[s][d] = r >= 0 ? W[(((int64_t)s * F + f) * D + d) * D + r] : c_make(0.0, 0.0);
    }
    __syncthreads();
    if (ban) {
        for (int i = tid; i < S * D; i += blockDim.x) {
            const int s = i / D, a = i - s * D;
            if (s_ref[s] < 0) continue;
            const cplx *PhiN = Phi + (((int64_t)s * F + f) * 2 + 1) * D * D;
            cplx v = c_make(0.0, 0.0);
            for (int e = 0; e < D; ++e) c_fma(v, PhiN[a * D + e], w[s][e]);
            t1[s][a] = v;   // Phi_N w
            cplx u = c_make(0.0, 0.0);   // (w^H Phi_N)_a
            for (int d = 0; d < D; ++d) c_cfma(u, w[s][d], PhiN[d * D + a]);
            t2[s][a] = u;
        }
        __syncthreads();
        if (tid < S && s_ref[tid] >= 0) {
            const int s = tid;
            cplx nom = c_make(0.0, 0.0), den = c_make(0.0, 0.0);
            for (int a = 0; a < D; ++a) {
                c_fma(nom, t2[s][a], t1[s][a]);
                c_cfma(den, w[s][a], t1[s][a]);
            }
            const double n = sqrt(hypot(nom.x, nom.y));
            const double dd = hypot(den.x, den.y);
            s_norm[s] = n / dd;
        }
        __syncthreads();
        for (int i = tid; i < S * D; i += blockDim.x) {
            const int s = i / D, d = i - s * D;
            if (s_ref[s] >= 0) w[s][d] = c_scale(w[s][d], s_norm[s]);
        }
        __syncthreads();
    }
    const int64_t c0 = (int64_t)blockIdx.x * chunk_frames;
    const int64_t c1 = c0 + chunk_frames < T ? c0 + chunk_frames : T;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    const cplx *Yf = Y + (int64_t)f * T * D;
    for (int64_t t = c0 + tid; t < c1; t += blockDim.x) {
        const cplx *y = Yf + t * D;
        cplx v[SB];
#pragma unroll
        for (int s = 0; s < SB; ++s) v[s] = c_make(0.0, 0.0);
        for (int d = 0; d < D; ++d) {
            const cplx yd = y[d];
#pragma unroll
            for (int s = 0; s < SB; ++s) c_cfma(v[s], w[s][d], yd);
        }
#pragma unroll
        for (int s = 0; s < SB; ++s)
            if (s < S)
                Xhat[((int64_t)s * T + t) * F + f] = s_ref[s] >= 0 ? v[s] : c_make(qnan, qnan);
    }
}

// ------------------------------------------------------------------ segment-wise MVDR
// mask_pack_kernel with the mask sums per segment of seg_frames frames: grid (B, F), block
// 256.  W2 (F, 2, T) as there; msum (F, B, 2).
__global__ __launch_bounds__(256) void mask_pack_segments_kernel(
    const double *__restrict__ mx, const double *__restrict__ mn, int64_t T, int64_t seg_frames,
    double *__restrict__ W2, double *__restrict__ msum) {
    __shared__ double red[8];
    const int b = blockIdx.x, B = gridDim.x, f = blockIdx.y, tid = threadIdx.x;
    const int64_t t0 = (int64_t)b * seg_frames;
    const int64_t t1 = t0 + seg_frames < T ? t0 + seg_frames : T;
    double sx = 0.0, sn = 0.0;
    for (int64_t t = t0 + tid; t < t1; t += blockDim.x) {
        const double a = mx[(int64_t)f * T + t], c = mn[(int64_t)f * T + t];
        W2[((int64_t)f * 2) * T + t] = a;
        W2[((int64_t)f * 2 + 1) * T + t] = c;
        sx += a;
        sn += c;
    }
    sx = wave_sum(sx);
    sn = wave_sum(sn);
    if ((tid & 63) == 0) {
        red[tid >> 6] = sx;
        red[4 + (tid >> 6)] = sn;
    }
    __syncthreads();
    if (tid == 0) {
        msum[((int64_t)f * B + b) * 2] = (red[0] + red[1]) + (red[2] + red[3]);
        msum[((int64_t)f * B + b) * 2 + 1] = (red[4] + red[5]) + (red[6] + red[7]);
    }
}

// Statistics window of segment b at frequency f: the unnormalised sums of the PSD partials and
// of the mask sums over segments max(0, b - ctx_seg) .. min(B - 1, b + ctx_seg), in ascending
// order (a segment's partials are its nsub chunks of `part`, ascending).  A window whose target
// or distortion mass is below min_mass takes the whole-window sums of its frequency instead
// (`whole_*`, made by a first launch of this kernel with grid (F, 1), ctx_seg = B, min_mass = 0,
// whole_part = NULL) and is counted in *fallbacks.  Output in the layout mvdr_solve_kernel
// reads for "targets" b = 0 .. gridDim.y - 1 with one chunk each: wpart (B, F, 2, NE),
// wmsum (B, F, 2).  grid (F, B or 1), block 256.
__global__ __launch_bounds__(256) void mvdr_window_segments_kernel(
    const cplx *__restrict__ part /* (F, nch, 2, NE) */,
    const double *__restrict__ msum /* (F, B, 2) */, int nch, int nsub, int B, int ctx_seg, int NE,
    double min_mass, const cplx *__restrict__ whole_part /* (F, 2, NE) */,
    const double *__restrict__ whole_msum /* (F, 2) */, cplx *__restrict__ wpart,
    double *__restrict__ wmsum, int32_t *__restrict__ fallbacks) {
    __shared__ int s_fall;
    const int f = blockIdx.x, b = blockIdx.y, F = gridDim.x, tid = threadIdx.x;
    const int lo = b - ctx_seg > 0 ? b - ctx_seg : 0;
    const int hi = b + ctx_seg < B - 1 ? b + ctx_seg : B - 1;
    const int64_t out = (int64_t)b * F + f;
    if (tid == 0) {
        double sx = 0.0, sn = 0.0;
        for (int s = lo; s <= hi; ++s) {
            sx += msum[((int64_t)f * B + s) * 2];
            sn += msum[((int64_t)f * B + s) * 2 + 1];
        }
        const bool fall = whole_part && (sx < min_mass || sn < min_mass);
        if (fall) {
            sx = whole_msum[f * 2];
            sn = whole_msum[f * 2 + 1];
            atomicAdd(fallbacks, 1);
        }
        wmsum[out * 2] = sx;
        wmsum[out * 2 + 1] = sn;
        s_fall = fall;
    }
    __syncthreads();
    cplx *dst = wpart + out * 2 * NE;
    if (s_fall) {
        for (int e = tid; e < 2 * NE; e += blockDim.x) dst[e] = whole_part[(int64_t)f * 2 * NE + e];
        return;
    }
    const int ch0 = lo * nsub, ch1 = (hi + 1) * nsub < nch ? (hi + 1) * nsub : nch;
    for (int e = tid; e < 2 * NE; e += blockDim.x) {
        cplx v = c_make(0.0, 0.0);
        for (int c = ch0; c < ch1; ++c) v = c_add(v, part[((int64_t)f * nch + c) * 2 * NE + e]);
        dst[e] = v;
    }
}

// The SNR terms of mvdr_solve_kernel summed over the frequencies of one segment: snr (B, F, D, 2)
// -> part (B, D, 2), block b its own segment, in mvdr_ref_kernel's way (MVDR_REF_CHUNK
// frequencies staged in LDS at a time, lane r adds its channel's terms in ascending frequency).
// mvdr_ref_kernel then adds the B partial sums in ascending order and picks the channel: one
// workgroup walking all B F terms was the longest kernel of a call with many segments.
__global__ __launch_bounds__(MVDR_REF_NT) void mvdr_snr_segments_kernel(
    const cplx *__restrict__ snr, int F, int D, cplx *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cplx *buf = reinterpret_cast<cplx *>(smem);            // MVDR_REF_CHUNK * D * 2
    const int tid = threadIdx.x;
    snr += (int64_t)blockIdx.x * F * D * 2;
    cplx num = c_make(0.0, 0.0), den = c_make(0.0, 0.0);
    for (int f0 = 0; f0 < F; f0 += MVDR_REF_CHUNK) {
        const int nf = min(MVDR_REF_CHUNK, F - f0);
        const int total = nf * D * 2;
        __syncthreads();
        for (int i = tid; i < total; i += MVDR_REF_NT) buf[i] = snr[(int64_t)f0 * D * 2 + i];
        __syncthreads();
        if (tid < D) {
            for (int f = 0; f < nf; ++f) {
                num = c_add(num, buf[(f * D + tid) * 2]);
                den = c_add(den, buf[(f * D + tid) * 2 + 1]);
            }
        }
    }
    if (tid < D) {
        part[((int64_t)blockIdx.x * D + tid) * 2] = num;
        part[((int64_t)blockIdx.x * D + tid) * 2 + 1] = den;
    }
}

// ------------------------------------------------------------------ interferer-nulling LCMV
// Per-frequency mass of every class over the frames the context zeroing keeps: gamma (F,K,T)
// -> fmass (F,K).  grid (F, K), block 256; mask_pack_kernel's summation order.
__global__ __launch_bounds__(256) void lcmv_mass_kernel(const double *__restrict__ gamma, int K,
                                                        int64_t T, int64_t zero_lo_end,
                                                        int64_t zero_hi_begin,
                                                        double *__restrict__ fmass) {
    __shared__ double red[4];
    const int f = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    const double *g = gamma + ((int64_t)f * K + k) * T;
    double s = 0.0;
    for (int64_t t = zero_lo_end + tid; t < zero_hi_begin; t += blockDim.x) s += g[t];
    s = wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) fmass[(int64_t)f * K + k] = (red[0] + red[1]) + (red[2] + red[3]);
}

// The interferer of a call: forced >= 0 names it; otherwise the candidate class (bit k of
// `candidates`, the target's bit ignored) of largest mass, the masses of lcmv_mass_kernel added
// in ascending frequency, equal masses to the lower index; -1 without a candidate or when the
// largest mass is 0.  One wave; pick[0] receives the class.
__global__ __launch_bounds__(64) void lcmv_pick_kernel(const double *__restrict__ fmass, int F,
                                                       int K, int target, uint32_t candidates,
                                                       int forced, int32_t *__restrict__ pick) {
    const int lane = threadIdx.x;
    if (forced >= 0) {
        if (lane == 0) pick[0] = forced;
        return;
    }
    const bool cand = lane < K && lane != target && (candidates >> lane & 1u);
    double best = -1.0;
    int bi = 1 << 30;
    if (cand) {
        double s = 0.0;
        for (int f = 0; f < F; ++f) s += fmass[(int64_t)f * K + lane];
        // (a NaN mass never wins: the class is no candidate)
        if (s == s) {
            best = s;
            bi = lane;
        }
    }
    wave_argmax_first(best, bi);
    if (lane == 0) pick[0] = best > 0.0 ? bi : -1;
}

// gamma (F,K,T) -> target, interferer and noise masks (F,T): X = gamma[target], I =
// gamma[pick[0]] (zero for -1), N = the remaining classes added in ascending k; all zero on the
// context frames (masks_kernel's rule).  The first thread reports the interferer.
__global__ void masks3_kernel(const double *__restrict__ gamma, int F, int K, int64_t T, int target,
                              const int32_t *__restrict__ pick, int64_t zero_lo_end,
                              int64_t zero_hi_begin, double *__restrict__ mx,
                              double *__restrict__ mi, double *__restrict__ mn,
                              int32_t *__restrict__ interferer_out, int32_t *__restrict__ status) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int interferer = pick[0];
    if (idx == 0) {
        if (interferer_out) interferer_out[0] = interferer;
        __hip_atomic_store(status + GSS_STATUS_LCMV_INTERFERER, interferer, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (idx >= (int64_t)F * T) return;
    const int f = idx / T;
    const int64_t t = idx - (int64_t)f * T;
    double x = 0.0, i = 0.0, n = 0.0;
    if (t >= zero_lo_end && t < zero_hi_begin) {
        const double *g = gamma + (int64_t)f * K * T + t;
        x = g[(int64_t)target * T];
        if (interferer >= 0) i = g[(int64_t)interferer * T];
        for (int k = 0; k < K; ++k)
            if (k != target && k != interferer) n += g[(int64_t)k * T];
    }
    mx[idx] = x;
    mi[idx] = i;
    mn[idx] = n;
}

// Souden's LCMV with one null (Souden, Benesty, Affes 2010, eq. 51), per frequency (one
// workgroup of MVDR_NT threads, made of the steps mvdr_solve_kernel is made of):
//   Phi_m = S_m / max(s_m, 1e-10) for m in {X, I, N};  A = solve(Phi_N, Phi_I),
//   B = solve(Phi_N, Phi_X) from ONE factorisation of the D x 3D block [Phi_N | Phi_I | Phi_X];
//   g_in = tr A,  g = g_in tr B - tr(A B),  W = (g_in B - A B) / max(Re g, eps);
//   distortion matrix Phi_D = Phi_I + Phi_N.
// A frequency whose interferer mask sums to less than min_mass takes the MVDR of the merged
// mask instead: Phi_D = (S_I + S_N) / max(s_I + s_N, 1e-10), the D x 2D block [Phi_D | Phi_X],
// W = Psi / max(Re tr Psi, eps) -- the functions mvdr_solve_kernel calls, on the same block --
// and is counted in *fallbacks.  s_I is known before the factorisation: a frequency factors one
// matrix.  Out: Phi (F,2,D,D) = [Phi_X, Phi_D], W (F,D,D), snr (F,D,2): what mvdr_ref_kernel and
// mvdr_apply_kernel read.
__global__ __launch_bounds__(MVDR_NT) void lcmv_solve_kernel(
    const cplx *__restrict__ part /* (F,nch,3,NE) */, const double *__restrict__ msum /* (F,3) */,
    int nch, int D, double eps, double min_mass, cplx *__restrict__ Phi, cplx *__restrict__ W,
    cplx *__restrict__ snr, int32_t *__restrict__ fallbacks) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NT = MVDR_NT;
    const int m = D + (D & 1);
    const int NE = tri_count(D);
    const int W3 = 3 * D;
    cplx *aug = reinterpret_cast<cplx *>(smem);   // D x 3D : [Phi_N | Phi_I | Phi_X] -> [U | A | B]
    cplx *JA = aug + D * W3;                       // m * m
    cplx *JV = JA + m * m;                         // m * m
    int *flags = reinterpret_cast<int *>(JV + m * m);   // (in the dynamic region: its alignment)
    double *s_val = reinterpret_cast<double *>(flags + 2);   // 3 doubles
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63;

    const double sx = msum[f * 3], si = msum[f * 3 + 1], sn = msum[f * 3 + 2];
    const bool fall = si < min_mass;
    // the columns in use: the matrix, then one (fallback) or two D x D right-hand sides; the
    // solution for Phi_X sits at column cx
    const int used = fall ? 2 * D : 3 * D, cx = used - D, nrhs = used - D;
    const double dx = fmax(sx, 1e-10), di = fmax(si, 1e-10), dn = fmax(sn, 1e-10);
    const double dd = fmax(si + sn, 1e-10);
    cplx *PhiX = Phi + (int64_t)f * 2 * D * D;
    cplx *PhiD = PhiX + D * D;
    if (tid == 0 && fall) atomicAdd(fallbacks, 1);
    // (called again on a singular matrix: the elimination has overwritten the block by then)
    auto fill = [&]() {
        for (int e = tid; e < NE; e += NT) {
            int d1, d2;
            tri_unpack(e, D, d1, d2);
            cplx v[3];
            partials_sum<3>(part, f, nch, NE, e, v);
            cplx vx = v[0], vi = v[1], vn = v[2];
            vx = c_make(vx.x / dx, vx.y / dx);
            cplx vd;
            if (fall) {
                vn = c_add(vi, vn);
                vn = c_make(vn.x / dd, vn.y / dd);
                vd = vn;
            } else {
                vi = c_make(vi.x / di, vi.y / di);
                vn = c_make(vn.x / dn, vn.y / dn);
                vd = c_add(vi, vn);
            }
            if (d1 == d2) {
                vx.y = 0.0;
                vi.y = 0.0;
                vn.y = 0.0;
                vd.y = 0.0;
            }
            herm_store(PhiX, D, d1, d2, vx);
            herm_store(PhiD, D, d1, d2, vd);
            herm_store(aug, W3, d1, d2, vn);
            if (!fall) herm_store(aug + D, W3, d1, d2, vi);
            herm_store(aug + cx, W3, d1, d2, vx);
        }
    };
    fill();
    if (tid == 0) flags[1] = 0;
    __syncthreads();
    if (!lu_eliminate(aug, W3, used, D, flags)) {
        back_substitute(aug, W3, D, nrhs);
    } else {
        fill();
        __syncthreads();
        min_norm_solve(aug, W3, used, D, m, JA, JV, s_val);
    }
    cplx *Wf = W + (int64_t)f * D * D;
    if (fall) {
        // Psi = aug[:, D:2D]
        trace_normalise(aug, W3, D, D, eps, s_val, Wf);
    } else {
        // A = aug[:, D:2D], B = aug[:, 2D:3D]; A B -> JA, spread over the workgroup
        for (int it = tid; it < D * D; it += NT) {
            const int i = it / D, col = it - i * D;
            cplx v = c_make(0.0, 0.0);
            for (int k = 0; k < D; ++k) c_fma(v, aug[i * W3 + D + k], aug[k * W3 + 2 * D + col]);
            JA[i * m + col] = v;
        }
        __syncthreads();
        // the traces: lane i holds the i-th diagonal entries, summed over the wave in wave_sum's
        // fixed order
        if (tid < 64) {
            cplx a = c_make(0.0, 0.0), b = c_make(0.0, 0.0), ab = c_make(0.0, 0.0);
            if (lane < D) {
                a = aug[lane * W3 + D + lane];
                b = aug[lane * W3 + 2 * D + lane];
                ab = JA[lane * m + lane];
            }
            const cplx gi = c_make(wave_sum(a.x), wave_sum(a.y));
            const cplx gx = c_make(wave_sum(b.x), wave_sum(b.y));
            const double tab = wave_sum(ab.x);
            if (lane == 0) {
                s_val[0] = fmax(c_mul(gi, gx).x - tab, eps);   // max(Re g, eps)
                s_val[1] = gi.x;
                s_val[2] = gi.y;
            }
        }
        __syncthreads();
        const double den = s_val[0];
        const cplx gi = c_make(s_val[1], s_val[2]);
        // (reads the two right blocks and JA, writes the left block: disjoint)
        for (int it = tid; it < D * D; it += NT) {
            const int i = it / D, col = it - i * D;
            const cplx v = c_sub(c_mul(gi, aug[i * W3 + 2 * D + col]), JA[i * m + col]);
            const cplx wv = c_make(v.x / den, v.y / den);
            aug[i * W3 + col] = wv;
            Wf[it] = wv;
        }
    }
    __syncthreads();
    snr_terms(aug, W3, cx, D, m, JA, PhiX, PhiD, snr + (int64_t)f * D * 2);
}

int psd_chunks(int F, int64_t T, int *chunk_frames) {
    int64_t tiles = (T + PSD_TILE - 1) / PSD_TILE;
    int64_t want = (2048 + F - 1) / F;
    int64_t tpc = (tiles + want - 1) / want;
    if (tpc < 1) tpc = 1;
    *chunk_frames = (int)(tpc * PSD_TILE);
    return (int)((tiles + tpc - 1) / tpc);
}

// The frames [lo_end, hi_begin) the context zeroing keeps, by the Python slice semantics of
// masks[:, :sf] = 0; if ef > 0: masks[:, -ef:] = 0 (drop == 0: all of them).
void context_range(int64_t T, int drop, int64_t sf, int64_t ef, int64_t *lo_end,
                   int64_t *hi_begin) {
    *lo_end = 0;
    *hi_begin = T;
    if (drop) {
        *lo_end = sf >= 0 ? (sf < T ? sf : T) : (T + sf > 0 ? T + sf : 0);
        if (ef > 0) *hi_begin = T - ef > 0 ? T - ef : 0;
    }
}

// Dynamic LDS of mvdr_solve_kernel (blocks = 2) and lcmv_solve_kernel (3): the D x blocks D
// block, JA and JV (m x m each), the two flags and three doubles.
size_t solve_lds_bytes(int D, int blocks) {
    const int m = D + (D & 1);
    return (sizeof(cplx) * ((size_t)D * blocks * D + 2 * (size_t)m * m) + 32 + 15) / 16 * 16;
}

}  // namespace

int masks_from_posteriors_run(gss_ctx *ctx, const double *gamma, int F, int K, int64_t T,
                              int target, int drop, int64_t sf, int64_t ef, double *mx,
                              double *mn) {
    int64_t lo_end, hi_begin;
    context_range(T, drop, sf, ef, &lo_end, &hi_begin);
    GSS_PROF(ctx, "masks");
    const int64_t total = (int64_t)F * T;
    hipLaunchKernelGGL(masks_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       ctx->stream, gamma, F, K, T, target, lo_end, hi_begin, mx, mn);
    GSS_LAUNCH_CHECK(ctx, "masks_kernel");
    return GSS_OK;
}

int masks_targets_run(gss_ctx *ctx, const double *gamma, int F, int K, int64_t T, int S,
                      const int32_t *targets, int drop, const int64_t *sf, const int64_t *ef,
                      double *mx, double *mn) {
    TargetMaskArgs a{};
    a.S = S;
    for (int s = 0; s < S; ++s) {
        a.target[s] = targets[s];
        context_range(T, drop, sf[s], ef[s], &a.zero_lo_end[s], &a.zero_hi_begin[s]);
    }
    GSS_PROF(ctx, "masks_targets");
    const int64_t total = (int64_t)F * T;
    hipLaunchKernelGGL(masks_targets_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       ctx->stream, gamma, F, K, T, a, mx, mn);
    GSS_LAUNCH_CHECK(ctx, "masks_targets_kernel");
    return GSS_OK;
}

// The blocks of mvdr_run (rows = 2 weight rows, S targets) and of lcmv_run (rows = 3, S = 1):
// every intermediate in S consecutive per-target blocks of the one-target layout.
struct BfWork {
    cplx *part;         // (S, F, nch, rows, NE) PSD partials
    double *msum, *Wr;  // (S, F, rows) mask sums, (S, F, rows, T) packed weight rows
    cplx *Phi, *W, *snr;
    int32_t *ref;       // per target [0]: reference channel, [2]: fallback counter (LCMV)
    int nch, cf;        // the chunks of the PSD pass
};
static BfWork bf_blocks(Workspace &ws, int F, int64_t T, int D, int S, int rows) {
    const size_t NE = tri_count(D), SF = (size_t)S * F;
    BfWork k;
    k.nch = psd_chunks(F, T, &k.cf);
    k.part = ws.take<cplx>(SF * k.nch * rows * NE, "beamformer psd partials");
    k.msum = ws.take<double>(SF * rows, "beamformer mask sums");
    k.Wr = ws.take<double>(SF * rows * T, "beamformer weight rows");
    k.Phi = ws.take<cplx>(SF * 2 * D * D, "beamformer Phi");
    k.W = ws.take<cplx>(SF * D * D, "beamformer W");
    k.snr = ws.take<cplx>(SF * D * 2, "beamformer snr");
    k.ref = ws.take<int32_t>(4 * (size_t)S, "beamformer ref");
    return k;
}

size_t mvdr_workspace_bytes(int F, int64_t T, int D, int S) {
    Workspace ws;
    bf_blocks(ws, F, T, D, S, 2);
    return ws.bytes + 4096;
}

// The tail of a one-target call (mvdr_run, lcmv_run): the reference channel from the SNR terms
// (pick_ref; the GEV's solve has named column 0 already), then BAN and the filtering.
static int ref_apply_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D, const BfWork &k,
                         bool pick_ref, int forced_ref, int ban, cplx *Xhat,
                         int32_t *ref_channel) {
    if (pick_ref) {
        GSS_PROF(ctx, "mvdr_ref");
        hipLaunchKernelGGL(mvdr_ref_kernel, dim3(1), dim3(MVDR_REF_NT),
                           sizeof(cplx) * MVDR_REF_CHUNK * (size_t)D * 2, ctx->stream, k.snr, F, D,
                           1e-10, forced_ref, k.ref);
        GSS_LAUNCH_CHECK(ctx, "mvdr_ref_kernel");
    }
    GSS_PROF(ctx, "mvdr_apply");
    const int chunk = 256;
    hipLaunchKernelGGL(mvdr_apply_kernel<false>, dim3((unsigned)((T + chunk - 1) / chunk), F),
                       dim3(256), 0, ctx->stream, Y, k.W, k.Phi, k.ref, F, T, D, ban, chunk, Xhat,
                       ref_channel, ctx->status_dev, (int64_t)0, (const int32_t *)nullptr);
    GSS_LAUNCH_CHECK(ctx, "mvdr_apply_kernel");
    return GSS_OK;
}

int mvdr_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D, const double *mx,
             const double *mn, int ban, cplx *Xhat, int32_t *ref_channel, int gev,
             int forced_ref, int S, bool targets) {
    // S targets (gss_enhance_observation_targets): masks (S,F,T), Xhat (S,T,F), ref_channel (S),
    // every intermediate in S consecutive per-target blocks of the one-target layout
    Workspace ws(ctx);
    const BfWork k = bf_blocks(ws, F, T, D, S, 2);
    GSS_TRY(ws.status("mvdr"));
    const int nch = k.nch, cf = k.cf;
    cplx *part = k.part, *Phi = k.Phi, *W = k.W, *snr = k.snr;
    double *msum = k.msum, *W2 = k.Wr;
    int32_t *ref = k.ref;
    ctx->last_targets = targets ? S : 0;
    {
        GSS_PROF(ctx, targets ? "psd_targets" : "psd");
        hipLaunchKernelGGL(mask_pack_kernel<2>, dim3(F, S), dim3(256), 0, ctx->stream,
                           MaskRows<2>{{mx, mn}}, T, W2, msum);
        GSS_LAUNCH_CHECK(ctx, "mask_pack_kernel");
        GSS_TRY(psd_partials_run(ctx, Y, F, T, D, W2, 2, nch, cf, part, S));
    }
    if (gev) {
        GSS_PROF(ctx, targets ? "gev_solve_targets" : "gev_solve");
        const int m = D + (D & 1);
        const size_t lds = (sizeof(cplx) * 4 * (size_t)m * m + 15) / 16 * 16;
        GSS_TRY(raise_lds_limit(ctx, gev_solve_kernel, lds));
        if (S == 1) {
            GSS_HIP_CHECK(ctx, hipMemsetAsync(ref, 0, sizeof(int32_t), ctx->stream));
            GSS_HIP_CHECK(ctx, hipMemsetAsync(ref + 1, 0x7f, sizeof(int32_t), ctx->stream));
        } else {    // (the same two words in each target's block of four)
            GSS_HIP_CHECK(ctx, hipMemset2DAsync(ref, 4 * sizeof(int32_t), 0, sizeof(int32_t), S,
                                                ctx->stream));
            GSS_HIP_CHECK(ctx, hipMemset2DAsync(ref + 1, 4 * sizeof(int32_t), 0x7f,
                                                sizeof(int32_t), S, ctx->stream));
        }
        hipLaunchKernelGGL(gev_solve_kernel, dim3(F, S), dim3(64), lds, ctx->stream, part, msum,
                           nch, D, Phi, W, ref);
        GSS_LAUNCH_CHECK(ctx, "gev_solve_kernel");
    } else {
        GSS_PROF(ctx, targets ? "mvdr_solve_targets" : "mvdr_solve");
        const size_t lds = solve_lds_bytes(D, 2);
        GSS_TRY(raise_lds_limit(ctx, mvdr_solve_kernel, lds));
        hipLaunchKernelGGL(mvdr_solve_kernel, dim3(F, S), dim3(MVDR_NT), lds, ctx->stream, part,
                           msum, nch, D, 1e-10, Phi, W, snr);
        GSS_LAUNCH_CHECK(ctx, "mvdr_solve_kernel");
    }
    if (!targets) return ref_apply_run(ctx, Y, F, T, D, k, !gev, forced_ref, ban, Xhat, ref_channel);
    if (!gev) {
        GSS_PROF(ctx, "mvdr_ref_targets");
        hipLaunchKernelGGL(mvdr_ref_kernel, dim3(S), dim3(MVDR_REF_NT),
                           sizeof(cplx) * MVDR_REF_CHUNK * (size_t)D * 2, ctx->stream, snr, F, D, 1e-10,
                           forced_ref, ref);
        GSS_LAUNCH_CHECK(ctx, "mvdr_ref_kernel");
    }
    const int chunk = 256;
    const dim3 grid((unsigned)((T + chunk - 1) / chunk), F);
    GSS_PROF(ctx, "mvdr_apply_targets");
    int32_t *const status = ctx->status_dev + GSS_STATUS_TARGETS;
#define GSS_APPLY_TARGETS(SB)                                                                    \
    hipLaunchKernelGGL(mvdr_apply_targets_kernel<SB>, grid, dim3(256), 0, ctx->stream, Y, W, Phi, \
                       ref, F, T, D, S, ban, chunk, Xhat, ref_channel, status, ctx->status_dev)
    if (S <= 2) GSS_APPLY_TARGETS(2);
    else if (S <= 4) GSS_APPLY_TARGETS(4);
    else if (S <= 8) GSS_APPLY_TARGETS(8);
    else GSS_APPLY_TARGETS(GSS_MAX_CLASSES);
#undef GSS_APPLY_TARGETS
    GSS_LAUNCH_CHECK(ctx, "mvdr_apply_targets_kernel");
    return GSS_OK;
}

// ------------------------------------------------------------------ segment-wise MVDR
namespace {
// Segments of L frames over the PSD pass: every segment is nsub chunks of cf frames (cf a
// multiple of the 64-frame tile that divides L, at most the whole-window pass's chunk), nch
// chunks in all -- the pass over Y is the whole-window one with chunk borders on segment borders.
struct SegmentGeometry {
    int64_t L;     // segment_frames, cut to one segment when it exceeds T
    int B, nsub, nch, cf;
};
SegmentGeometry segment_geometry(int F, int64_t T, int64_t L) {
    SegmentGeometry g;
    const int64_t tiles = (T + PSD_TILE - 1) / PSD_TILE;
    g.L = L < tiles * PSD_TILE ? L : tiles * PSD_TILE;
    int cf_whole;
    psd_chunks(F, T, &cf_whole);
    const int64_t tiles_seg = g.L / PSD_TILE;
    int64_t tpc = cf_whole / PSD_TILE < tiles_seg ? cf_whole / PSD_TILE : tiles_seg;
    while (tiles_seg % tpc) --tpc;
    g.cf = (int)(tpc * PSD_TILE);
    g.nsub = (int)(tiles_seg / tpc);
    g.nch = (int)((T + g.cf - 1) / g.cf);
    g.B = (int)((T + g.L - 1) / g.L);
    return g;
}
}  // namespace

// The blocks of mvdr_segments_run for the geometry g (B segments).
struct SegWork {
    cplx *part;                     // (F, nch, 2, NE) PSD partials of the one pass over Y
    double *msum, *W2;              // (F, B, 2) mask sums, (F, 2, T) packed weights
    cplx *whole_part;               // the whole-window sums a segment falls back to
    double *whole_msum;
    cplx *wpart;                    // (B, F, 2, NE) every segment's window
    double *wmsum;
    cplx *Phi, *W, *snr, *snr_part;
    int32_t *ref;                   // [0]: reference channel, [2]: fallback counter
};
static SegWork segments_blocks(Workspace &ws, int F, int64_t T, int D, const SegmentGeometry &g) {
    const size_t NE = tri_count(D), B = g.B;
    SegWork k;
    k.part = ws.take<cplx>((size_t)F * g.nch * 2 * NE, "segments psd partials");
    k.msum = ws.take<double>((size_t)F * B * 2, "segments mask sums");
    k.W2 = ws.take<double>((size_t)F * 2 * T, "segments weight rows");
    k.whole_part = ws.take<cplx>((size_t)F * 2 * NE, "segments whole-window partials");
    k.whole_msum = ws.take<double>((size_t)F * 2, "segments whole-window mask sums");
    k.wpart = ws.take<cplx>(B * F * 2 * NE, "segments window partials");
    k.wmsum = ws.take<double>(B * F * 2, "segments window mask sums");
    k.Phi = ws.take<cplx>(B * F * 2 * D * D, "segments Phi");
    k.W = ws.take<cplx>(B * F * D * D, "segments W");
    k.snr = ws.take<cplx>(B * F * D * 2, "segments snr");
    k.snr_part = ws.take<cplx>(B * D * 2, "segments snr sums");
    k.ref = ws.take<int32_t>(4, "segments ref");
    return k;
}

size_t mvdr_segments_workspace_bytes(int F, int64_t T, int D, int64_t segment_frames) {
    Workspace ws;
    segments_blocks(ws, F, T, D, segment_geometry(F, T, segment_frames));
    return ws.bytes + 4096;
}

int mvdr_segments_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D, const double *mx,
                      const double *mn, int ban, const gss_bf_segments &seg, cplx *Xhat,
                      int32_t *ref_channel, int forced_ref) {
    const int NE = tri_count(D);
    const SegmentGeometry g = segment_geometry(F, T, seg.segment_frames);
    Workspace ws(ctx);
    const SegWork k = segments_blocks(ws, F, T, D, g);
    GSS_TRY(ws.status("mvdr segments"));
    cplx *part = k.part, *whole_part = k.whole_part, *wpart = k.wpart;
    double *msum = k.msum, *W2 = k.W2, *whole_msum = k.whole_msum, *wmsum = k.wmsum;
    cplx *Phi = k.Phi, *W = k.W, *snr = k.snr, *snr_part = k.snr_part;
    int32_t *ref = k.ref, *const fallbacks = ref + 2;
    ctx->last_targets = 0;
    GSS_HIP_CHECK(ctx, hipMemsetAsync(fallbacks, 0, sizeof(int32_t), ctx->stream));
    {
        GSS_PROF(ctx, "psd_segments");
        hipLaunchKernelGGL(mask_pack_segments_kernel, dim3(g.B, F), dim3(256), 0, ctx->stream, mx,
                           mn, T, g.L, W2, msum);
        GSS_LAUNCH_CHECK(ctx, "mask_pack_segments_kernel");
        GSS_TRY(psd_partials_run(ctx, Y, F, T, D, W2, 2, g.nch, g.cf, part));
    }
    {
        GSS_PROF(ctx, "mvdr_window_segments");
        // the whole-window sums of every frequency first (what a window falls back to) ...
        hipLaunchKernelGGL(mvdr_window_segments_kernel, dim3(F, 1), dim3(256), 0, ctx->stream, part,
                           msum, g.nch, g.nsub, g.B, g.B, NE, 0.0, (const cplx *)nullptr,
                           (const double *)nullptr, whole_part, whole_msum, fallbacks);
        GSS_LAUNCH_CHECK(ctx, "mvdr_window_segments_kernel");
        // ... then every segment's window
        const int ctx_seg = seg.context_segments < g.B ? seg.context_segments : g.B;
        hipLaunchKernelGGL(mvdr_window_segments_kernel, dim3(F, g.B), dim3(256), 0, ctx->stream,
                           part, msum, g.nch, g.nsub, g.B, ctx_seg, NE, seg.min_mass, whole_part,
                           whole_msum, wpart, wmsum, fallbacks);
        GSS_LAUNCH_CHECK(ctx, "mvdr_window_segments_kernel");
    }
    {
        // mvdr_solve_kernel's (F, S) grid with the B segments as its "targets", one chunk each
        GSS_PROF(ctx, "mvdr_solve_segments");
        const size_t lds = solve_lds_bytes(D, 2);
        GSS_TRY(raise_lds_limit(ctx, mvdr_solve_kernel, lds));
        hipLaunchKernelGGL(mvdr_solve_kernel, dim3(F, g.B), dim3(MVDR_NT), lds, ctx->stream, wpart,
                           wmsum, 1, D, 1e-10, Phi, W, snr);
        GSS_LAUNCH_CHECK(ctx, "mvdr_solve_kernel");
    }
    {
        // one reference channel for the call: the SNR terms summed over all (b, f) -- over f
        // within each segment, then mvdr_ref_kernel over the B partial sums as its "frequencies"
        GSS_PROF(ctx, "mvdr_ref_segments");
        const size_t lds = sizeof(cplx) * MVDR_REF_CHUNK * (size_t)D * 2;
        hipLaunchKernelGGL(mvdr_snr_segments_kernel, dim3(g.B), dim3(MVDR_REF_NT), lds, ctx->stream,
                           snr, F, D, snr_part);
        GSS_LAUNCH_CHECK(ctx, "mvdr_snr_segments_kernel");
        hipLaunchKernelGGL(mvdr_ref_kernel, dim3(1), dim3(MVDR_REF_NT), lds, ctx->stream, snr_part,
                           g.B, D, 1e-10, forced_ref, ref);
        GSS_LAUNCH_CHECK(ctx, "mvdr_ref_kernel");
    }
    GSS_PROF(ctx, "mvdr_apply_segments");
    const int chunk = g.L % 256 == 0 ? 256 : g.L % 128 == 0 ? 128 : 64;
    hipLaunchKernelGGL(mvdr_apply_kernel<true>, dim3((unsigned)((T + chunk - 1) / chunk), F), dim3(256), 0,
                       ctx->stream, Y, W, Phi, ref, F, T, D, ban, chunk, Xhat, ref_channel,
                       ctx->status_dev, g.L, (const int32_t *)fallbacks);
    GSS_LAUNCH_CHECK(ctx, "mvdr_apply_kernel");
    return GSS_OK;
}

// ------------------------------------------------------------------ interferer-nulling LCMV
struct LcmvMaskWork {
    double *fmass;      // (F,K) mass of every class
    int32_t *pick;      // the interferer
};
static LcmvMaskWork lcmv_masks_blocks(Workspace &ws, int F, int K) {
    LcmvMaskWork k;
    k.fmass = ws.take<double>((size_t)F * K, "lcmv masks fmass");
    k.pick = ws.take<int32_t>(4, "lcmv masks pick");
    return k;
}

size_t lcmv_masks_workspace_bytes(int F, int K) {
    Workspace ws;
    lcmv_masks_blocks(ws, F, K);
    return ws.bytes + 4096;
}

int lcmv_masks_run(gss_ctx *ctx, const double *gamma, int F, int K, int64_t T, int target,
                   const gss_bf_lcmv &bf, int drop, int64_t sf, int64_t ef, double *mx, double *mi,
                   double *mn, int32_t *interferer) {
    int64_t lo_end, hi_begin;
    context_range(T, drop, sf, ef, &lo_end, &hi_begin);
    Workspace ws(ctx);
    const LcmvMaskWork k = lcmv_masks_blocks(ws, F, K);
    GSS_TRY(ws.status("lcmv masks"));
    {
        GSS_PROF(ctx, "lcmv_pick");
        if (bf.interferer < 0) {
            hipLaunchKernelGGL(lcmv_mass_kernel, dim3(F, K), dim3(256), 0, ctx->stream, gamma, K, T,
                               lo_end, hi_begin, k.fmass);
            GSS_LAUNCH_CHECK(ctx, "lcmv_mass_kernel");
        }
        hipLaunchKernelGGL(lcmv_pick_kernel, dim3(1), dim3(64), 0, ctx->stream, k.fmass, F, K, target,
                           bf.candidates, (int)bf.interferer, k.pick);
        GSS_LAUNCH_CHECK(ctx, "lcmv_pick_kernel");
    }
    GSS_PROF(ctx, "masks3");
    const int64_t total = (int64_t)F * T;
    hipLaunchKernelGGL(masks3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       ctx->stream, gamma, F, K, T, target, k.pick, lo_end, hi_begin, mx, mi, mn,
                       interferer, ctx->status_dev);
    GSS_LAUNCH_CHECK(ctx, "masks3_kernel");
    return GSS_OK;
}

size_t lcmv_workspace_bytes(int F, int64_t T, int D) {
    Workspace ws;
    bf_blocks(ws, F, T, D, 1, 3);
    return ws.bytes + 4096;
}

int lcmv_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D, const double *mx,
             const double *mi, const double *mn, int ban, int forced_ref, double min_mass,
             cplx *Xhat, int32_t *ref_channel) {
    Workspace ws(ctx);
    const BfWork k = bf_blocks(ws, F, T, D, 1, 3);
    GSS_TRY(ws.status("lcmv"));
    int32_t *const fallbacks = k.ref + 2;
    ctx->last_targets = 0;
    GSS_HIP_CHECK(ctx, hipMemsetAsync(fallbacks, 0, sizeof(int32_t), ctx->stream));
    {
        GSS_PROF(ctx, "psd3");
        hipLaunchKernelGGL(mask_pack_kernel<3>, dim3(F), dim3(256), 0, ctx->stream,
                           MaskRows<3>{{mx, mi, mn}}, T, k.Wr, k.msum);
        GSS_LAUNCH_CHECK(ctx, "mask_pack_kernel");
        GSS_TRY(psd_partials_run(ctx, Y, F, T, D, k.Wr, 3, k.nch, k.cf, k.part));
    }
    {
        GSS_PROF(ctx, "lcmv_solve");
        const size_t lds = solve_lds_bytes(D, 3);
        GSS_TRY(raise_lds_limit(ctx, lcmv_solve_kernel, lds));
        hipLaunchKernelGGL(lcmv_solve_kernel, dim3(F), dim3(MVDR_NT), lds, ctx->stream, k.part,
                           k.msum, k.nch, D, 1e-10, min_mass, k.Phi, k.W, k.snr, fallbacks);
        GSS_LAUNCH_CHECK(ctx, "lcmv_solve_kernel");
        // the count of this call -> the context's status word
        GSS_HIP_CHECK(ctx, hipMemcpyAsync(ctx->status_host + GSS_STATUS_LCMV_FALLBACKS, fallbacks,
                                          sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    return ref_apply_run(ctx, Y, F, T, D, k, true, forced_ref, ban, Xhat, ref_channel);
}
