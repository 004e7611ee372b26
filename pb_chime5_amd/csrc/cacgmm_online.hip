// Online CACGMM: the recursive EM of the complex angular central Gaussian mixture (include/
// gss_hip.h: gss_cacgmm_online).  Per frequency the state is, per class k,
// a Hermitian running sum S_k (D,D) and a mass n_k; the model they stand for is B_k = S_k / n_k,
// pi_k = n_k / sum_j n_j.  For every frame t in order, with y = Y[f,t,:], m_kt the mask (or 1):
//   z       = y / max(||y||, tiny)
//   S_k     = U^H U;  q_k = max(n_k |U^-H z|^2, tiny),  l_k = sum_j ln pivot_j - D ln n_k
//             (a pivot that is not > 0 or not finite: a FALLBACK class for this frame, B_k = I:
//              q_k = max(||z||^2, tiny), l_k = 0, counted)
//   gamma_k = exp(lp_k - max_j lp_j) pi_k m_kt / max(sum, tiny),   lp_k = -D ln q_k - l_k
//   OUTPUT gamma[f,k,t]                 -- the model of the frames before t: causal
//   ||y|| == 0: the state stays as it is; else with g_k = clip(gamma_k, 1e-10, 1 - 1e-10)
//   S_k <- beta S_k + g_k D z z^H / max(q_k, 10 tiny),   n_k <- beta n_k + g_k
//   the rank guard: with d = max(0, max_i (S_k)_ii) of the updated S_k and p the smallest pivot
//             of the frame's factorisation, every (S_k)_ii += (1 - beta) COL_RANK_EPS d phi,
//             phi = exp(-p / (COL_RANK_GATE d))  (0 below exp(-745), without a factor, at d = 0)
//             (a class that wins almost no frame has an effective frame count below D and S_k
//              loses rank: the gate is exactly 0 on a well-conditioned class and rises smoothly
//              to 1 as p / d falls to COL_RANK_GATE, which keeps cond(S_k) near 1e11 at worst)
//   the scale pin: when the binary exponent e of the largest diagonal entry, d + its guard, is
//             outside [-COL_SCALE_BAND, COL_SCALE_BAND]: S_k <- 2^-e S_k (n_k stays: only
//             ln det B_k + D ln q_k enters gamma, and that does not see the scale of S_k)
//   Both are functions of the state and the frame alone; a maximum and a power of two are exact.
// One persistent workgroup per frequency walks the frames, one wave per class.  Wave k keeps the
// upper triangle of S_k in registers for the whole call, on the 8 x 8 lane grid of
// chol_inverse_sweep (dense_wave.h): per frame it copies the registers, runs the sweep (U and
// W = U^-H in one pass of D steps, rows through the wave's own LDS scratch) and forms
// |W z|^2 from the rows.  The K pairs (lp_k, n_k) cross the waves through a double-buffered LDS
// table behind ONE workgroup barrier per frame; every wave then forms the same softmax in
// ascending k (the same bits in every wave), wave 0 stores gamma, and every wave applies the
// rank-one update to its own registers with c_outer, so the (never stored) lower triangle is the
// exact conjugate by construction and the diagonal stays exactly real.  The form (NR = ceil(D/8),
// K waves) and every order of summation depend on D and K alone, never on T, F or where a call
// begins: blocks through one state give the bits of one call.  No floating-point atomics; the
// fallbacks of a frequency are summed through LDS and added with one integer atomic.
#include "dense_wave.h"

namespace {

// The method's constants (tests/online_cacgmm_reference.py has the same).
// Band: the exponents the parity cells, the stream cells and the pipeline scene reach without
// the pin lie in [-34, 11].
constexpr double COL_RANK_EPS = 1e-10;
constexpr double COL_RANK_GATE = 1e-9;
constexpr int COL_SCALE_BAND = 64;

// The largest of 64 values that are all >= 0, on the DPP network in wave_sum's pattern (0, which
// a lane outside a shift or a mask reads, is the identity); exact, so the same in any order.
__device__ __forceinline__ double wave_max_nonneg(double v) {
    double s = fmax(v, dpp_shifted<0x111, 0xf, 0xf>(v));     // row_shr:1
    s = fmax(s, dpp_shifted<0x112, 0xf, 0xf>(v));            // row_shr:2
    s = fmax(s, dpp_shifted<0x113, 0xf, 0xf>(v));            // row_shr:3
    s = fmax(s, dpp_shifted<0x114, 0xf, 0xe>(s));            // row_shr:4, banks 1-3
    s = fmax(s, dpp_shifted<0x118, 0xf, 0xc>(s));            // row_shr:8, banks 2-3
    s = fmax(s, dpp_shifted<0x142, 0xa, 0xf>(s));            // row_bcast:15 into rows 1, 3
    s = fmax(s, dpp_shifted<0x143, 0xc, 0xf>(s));            // row_bcast:31 into rows 2, 3
    const unsigned long long u = __double_as_longlong(s);
    const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)u, 63);
    const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)(u >> 32), 63);
    return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}

struct ColArgs {
    const cplx *Y;              // (F, T, D)
    const uint8_t *mask;        // element (f, k, t) at [f mask_f + k mask_k + t], NULL: none
    int64_t mask_f, mask_k;
    cplx *S;                    // (F, K, D, D)
    double *n;                  // (F, K)
    double *gamma;              // (F, K, T)
    int32_t *fallbacks;         // the call's device counter
    int64_t T;
    int D, K;
    double beta;
};

// the upper triangle of a (D,D) matrix and the real part of its diagonal -> the register tile
template <int NR>
__device__ __forceinline__ void col_load(const cplx *__restrict__ g, cplx (&reg)[NR][NR], int D,
                                         int tx, int ty) {
#pragma unroll
    for (int a = 0; a < NR; ++a)
#pragma unroll
        for (int b = 0; b < NR; ++b) {
            const int i = ty + 8 * a, k = tx + 8 * b;
            cplx v = c_make(0.0, 0.0);
            if (i <= k && k < D) {
                v = g[i * D + k];
                if (i == k) v.y = 0.0;
            }
            reg[a][b] = v;
        }
}

// Wave k of workgroup f owns class k.  LDS: per wave the sweep's rows M (D rows of ld = 8 NR + 1
// complex values -- odd, as in mvdr_online.hip), z (8 NR) and the sweep's 1 / U_jj (8 NR); then
// the table of the class scalars, 2 buffers x {lp, n} x 8.
template <int NR>
__global__ __launch_bounds__(512) void cacgmm_online_kernel(ColArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int ld = 8 * NR + 1;
    const int D = a.D, K = a.K;
    const int f = blockIdx.x, lane = threadIdx.x & 63, k = threadIdx.x >> 6;
    const int tx = lane & 7, ty = lane >> 3;
    const size_t per_wave = sizeof(cplx) * ((size_t)D * ld + 8 * NR) + sizeof(double) * 8 * NR;
    cplx *M = reinterpret_cast<cplx *>(smem + per_wave * k);
    cplx *zb = M + D * ld;
    double *dinv = reinterpret_cast<double *>(zb + 8 * NR);
    double *table = reinterpret_cast<double *>(smem + per_wave * K);   // [2][2][8]
    const bool row = lane < D;
    const int64_t T = a.T;
    const cplx zero = c_make(0.0, 0.0);
    const cplx *Yf = a.Y + (int64_t)f * T * D;
    const int mk = lane & 7;                       // the class whose mask value this lane fetches
    const uint8_t *mf = a.mask && mk < K ? a.mask + (int64_t)f * a.mask_f + mk * a.mask_k : nullptr;
    cplx *Sg = a.S + ((int64_t)f * K + k) * D * D;
    double *gam = a.gamma + (int64_t)f * K * T;
    const double beta = a.beta, Dd = (double)D;
    const double guard = (1.0 - beta) * COL_RANK_EPS;

    cplx reg[NR][NR];
    col_load<NR>(Sg, reg, D, tx, ty);
    double n = a.n[(int64_t)f * K + k];

    cplx y_next = row ? Yf[lane] : zero;
    double m_next = mf ? (mf[0] ? 1.0 : 0.0) : 1.0;
    int nfall = 0;
    for (int64_t t = 0; t < T; ++t) {
        const cplx y = y_next;
        const double m = m_next;
        if (t + 1 < T) {
            if (row) y_next = Yf[(t + 1) * D + lane];
            if (mf) m_next = mf[t + 1] ? 1.0 : 0.0;
        }
        const double nrm2 = wave_sum(fma(y.x, y.x, y.y * y.y));
        const double den = fmax(sqrt(nrm2), GSS_TINY);
        const cplx z = c_make(y.x / den, y.y / den);
        if (lane < 8 * NR) zb[lane] = z;
        cplx tmp[NR][NR];
#pragma unroll
        for (int ai = 0; ai < NR; ++ai)
#pragma unroll
            for (int bi = 0; bi < NR; ++bi) tmp[ai][bi] = reg[ai][bi];
        wave_sync();
        const bool ok = chol_inverse_sweep<8, NR, true>(tmp, D, M, ld, dinv, tx, ty);
        double q, l, pivot = 0.0;   // the smallest pivot, from the largest 1 / U_jj
        if (ok) {   // decided by the pivots alone, the same in every lane
            // M: row i holds W[i][j] / dinv[i] for j < i, the pivot at j = i;  W[i][i] = dinv[i]
            double r = 0.0, lg = 0.0;
            if (row) {
                cplx acc = z;
                for (int j = 0; j < lane; ++j) c_fma(acc, M[lane * ld + j], zb[j]);
                const double di = dinv[lane];
                r = fma(acc.x, acc.x, acc.y * acc.y) * (di * di);
                lg = log(M[lane * ld + lane].x);
            }
            q = fmax(n * wave_sum(r), GSS_TINY);
            const double umax = wave_max_nonneg(row ? dinv[lane] : 0.0);
            pivot = 1.0 / (umax * umax);
            l = wave_sum(lg) - Dd * log(n);
        } else {
            ++nfall;
            q = fmax(wave_sum(fma(z.x, z.x, z.y * z.y)), GSS_TINY);
            l = 0.0;
        }
        double *tb = table + (t & 1) * 16;
        if (lane == 0) {
            tb[k] = -Dd * log(q) - l;
            tb[8 + k] = n;
        }
        __syncthreads();
        // the softmax over the classes in ascending order: the same bits in every wave
        double ntot = 0.0, top = tb[0];
        for (int j = 0; j < K; ++j) {
            ntot += tb[8 + j];
            top = fmax(top, tb[j]);
        }
        double sum = 0.0, e_own = 0.0, e_out = 0.0;
        for (int j = 0; j < K; ++j) {
            const double e = exp(tb[j] - top) * (tb[8 + j] / ntot) * __shfl(m, j, 64);
            sum += e;
            if (j == k) e_own = e;
            if (j == lane) e_out = e;
        }
        const double norm = fmax(sum, GSS_TINY);
        if (k == 0 && lane < K) gam[(int64_t)lane * T + t] = e_out / norm;
        if (nrm2 != 0.0) {   // a frame of zeros leaves the state alone
            const double g = fmin(fmax(e_own / norm, 1e-10), 1.0 - 1e-10);
            const double c = g * Dd / fmax(q, 10.0 * GSS_TINY);
#pragma unroll
            for (int ai = 0; ai < NR; ++ai)
#pragma unroll
                for (int bi = ai; bi < NR; ++bi) {
                    const int i = ty + 8 * ai, kk = tx + 8 * bi;
                    if (i <= kk && kk < D) {
                        const cplx o = c_outer(zb[i], zb[kk]);
                        reg[ai][bi] = c_make(fma(beta, reg[ai][bi].x, c * o.x),
                                             fma(beta, reg[ai][bi].y, c * o.y));
                    }
                }
            n = fma(beta, n, g);
            // the rank guard and the scale pin, from the largest diagonal entry (lanes tx == ty)
            double d = 0.0;     // (a state without a positive diagonal entry gets no guard)
#pragma unroll
            for (int ai = 0; ai < NR; ++ai)
                if (tx == ty && ty + 8 * ai < D) d = fmax(d, reg[ai][ai].x);
            d = wave_max_nonneg(d);
            double phi = 0.0;
            if (ok && d > 0.0) {    // the same in every lane
                const double x = pivot / (COL_RANK_GATE * d);
                if (x < 745.0) phi = exp(-x);
            }
            const double add = guard * d * phi;
#pragma unroll
            for (int ai = 0; ai < NR; ++ai)
                if (tx == ty && ty + 8 * ai < D) reg[ai][ai].x += add;
            const double dtop = d + add;     // the bits of the largest entry after the guard
            const int ef = (int)((__double_as_longlong(dtop) >> 52) & 0x7ff);
            if (dtop > 0.0 && ef != 0 && ef != 0x7ff) {     // normal and finite
                const int e = ef - 1022;                   // frexp's exponent
                if (e > COL_SCALE_BAND || e < -COL_SCALE_BAND) {
                    const double sc = ldexp(1.0, -min(max(e, -1000), 1000));
#pragma unroll
                    for (int ai = 0; ai < NR; ++ai)
#pragma unroll
                        for (int bi = ai; bi < NR; ++bi)
                            reg[ai][bi] = c_make(reg[ai][bi].x * sc, reg[ai][bi].y * sc);
                }
            }
        }
        wave_sync();    // zb and M are rewritten by the next frame
    }
    // both triangles, lower = conj(upper)
#pragma unroll
    for (int ai = 0; ai < NR; ++ai)
#pragma unroll
        for (int bi = ai; bi < NR; ++bi) {
            const int i = ty + 8 * ai, kk = tx + 8 * bi;
            if (i <= kk && kk < D) {
                Sg[i * D + kk] = reg[ai][bi];
                if (i != kk) Sg[kk * D + i] = c_conj(reg[ai][bi]);
            }
        }
    if (lane == 0) a.n[(int64_t)f * K + k] = n;
    // one integer atomic per frequency
    __syncthreads();
    int *cnt = reinterpret_cast<int *>(table);
    if (lane == 0) cnt[k] = nfall;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int j = 0; j < K; ++j) total += cnt[j];
        if (total) atomicAdd(a.fallbacks, total);
    }
}

size_t col_lds_bytes(int D, int K) {
    const size_t nr = (size_t)(D + 7) / 8, ld = 8 * nr + 1;
    return (size_t)K * (sizeof(cplx) * ((size_t)D * ld + 8 * nr) + sizeof(double) * 8 * nr) +
           sizeof(double) * 32;
}

__global__ __launch_bounds__(256) void cacgmm_online_fresh_kernel(int64_t FK, int D, double mass,
                                                                  cplx *__restrict__ S,
                                                                  double *__restrict__ n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t dd = (int64_t)D * D;
    if (i >= FK * dd) return;
    const int64_t e = i % dd;
    S[i] = c_make(e / D == e % D ? mass : 0.0, 0.0);
    if (e == 0) n[i / dd] = mass;
}

// The two conversions between a state and a model, one wave per (frequency, class): both invert
// a Hermitian matrix A = U^H U with the sweep, A^-1 = W^H W, and hand out s A^-1 with both
// triangles (the upper one is computed, the lower one is its conjugate).
//   to_model = 0: A = precision_k, s = n_k = mass pi_k           -> S_k = n_k B_k, n_k
//   to_model = 1: A = S_k,         s = n_k                        -> precision_k = B_k^-1,
//                 log_det = sum ln pivots - D ln n_k, weight = n_k / sum_j n_j (ascending j)
// A failed pivot is counted in `failed`; the class comes out as s I (to_model: the identity model
// of a fallback class, log_det 0).
struct ColConvArgs {
    const cplx *A;        // (F, K, D, D)
    const double *scal;   // (F, K): weights (to_model = 0) or masses (to_model = 1)
    cplx *out;            // (F, K, D, D)
    double *n_out;        // to_model = 0: (F, K)
    double *log_det, *weight;   // to_model = 1: (F, K)
    int32_t *failed;
    int D, K, to_model;
    double mass;
};

template <int NR>
__global__ __launch_bounds__(64) void cacgmm_online_convert_kernel(ColConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int ld = 8 * NR + 1;
    const int D = a.D, K = a.K;
    const int fk = blockIdx.x, lane = threadIdx.x;
    const int tx = lane & 7, ty = lane >> 3;
    cplx *M = reinterpret_cast<cplx *>(smem);
    double *dinv = reinterpret_cast<double *>(M + D * ld);
    const cplx *A = a.A + (int64_t)fk * D * D;
    cplx *out = a.out + (int64_t)fk * D * D;
    cplx reg[NR][NR];
    col_load<NR>(A, reg, D, tx, ty);
    const double own = a.scal[fk];
    const double s = a.to_model ? own : a.mass * own;
    const bool ok = chol_inverse_sweep<8, NR, true>(reg, D, M, ld, dinv, tx, ty);
    double lg = 0.0;
    if (ok && lane < D) lg = log(M[lane * ld + lane].x);
    const double logdet = wave_sum(lg);
    // W in place: row r of M becomes W[r][j] for j <= r
    for (int idx = lane; idx < D * D; idx += 64) {
        const int r = idx / D, j = idx - r * D;
        if (j < r) M[r * ld + j] = c_scale(M[r * ld + j], dinv[r]);
        else if (j == r) M[r * ld + j] = c_make(dinv[r], 0.0);
    }
    wave_sync();
#pragma unroll
    for (int ai = 0; ai < NR; ++ai)
#pragma unroll
        for (int bi = ai; bi < NR; ++bi) {
            const int i = ty + 8 * ai, kk = tx + 8 * bi;
            if (i <= kk && kk < D) {
                // (W^H W)[i][kk] = sum_{r >= kk} conj(W[r][i]) W[r][kk]
                cplx acc = c_make(0.0, 0.0);
                if (ok) {
                    for (int r = kk; r < D; ++r) c_cfma(acc, M[r * ld + i], M[r * ld + kk]);
                    acc = c_scale(acc, s);
                    if (i == kk) acc.y = 0.0;
                } else if (i == kk) {
                    acc.x = a.to_model ? 1.0 : s;
                }
                out[i * D + kk] = acc;
                if (i != kk) out[kk * D + i] = c_conj(acc);
            }
        }
    if (lane == 0) {
        if (a.to_model) {
            const double *nf = a.scal + (int64_t)(fk / K) * K;
            double ntot = 0.0;
            for (int j = 0; j < K; ++j) ntot += nf[j];
            a.weight[fk] = own / ntot;
            a.log_det[fk] = ok ? logdet - (double)D * log(own) : 0.0;
        } else {
            a.n_out[fk] = s;
        }
        if (!ok) atomicAdd(a.failed, 1);
    }
}

size_t col_conv_lds_bytes(int D) {
    const size_t nr = (size_t)(D + 7) / 8, ld = 8 * nr + 1;
    return sizeof(cplx) * (size_t)D * ld + sizeof(double) * 8 * nr;
}

int col_convert(gss_ctx *ctx, const ColConvArgs &a, int F, const char *name) {
    GSS_PROF(ctx, name);
    const size_t lds = col_conv_lds_bytes(a.D);
    const dim3 grid((unsigned)(F * a.K));
    if (a.D <= 8) hipLaunchKernelGGL(cacgmm_online_convert_kernel<1>, grid, dim3(64), lds, ctx->stream, a);
    else if (a.D <= 16) hipLaunchKernelGGL(cacgmm_online_convert_kernel<2>, grid, dim3(64), lds, ctx->stream, a);
    else if (a.D <= 24) hipLaunchKernelGGL(cacgmm_online_convert_kernel<3>, grid, dim3(64), lds, ctx->stream, a);
    else hipLaunchKernelGGL(cacgmm_online_convert_kernel<4>, grid, dim3(64), lds, ctx->stream, a);
    GSS_LAUNCH_CHECK(ctx, name);
    return GSS_OK;
}

}  // namespace

// the counter and, for a thrown-away state, its sums and masses
struct ColWork {
    int32_t *words;     // [0]: fallback / failed-pivot counter
    cplx *S;
    double *n;
};
static ColWork col_blocks(Workspace &ws, int F, int K, int D, bool fresh) {
    ColWork w;
    w.words = ws.take<int32_t>(4, "online cacgmm words");
    w.S = fresh ? ws.take<cplx>((size_t)F * K * D * D, "online cacgmm S") : nullptr;
    w.n = fresh ? ws.take<double>((size_t)F * K, "online cacgmm n") : nullptr;
    return w;
}

size_t cacgmm_online_workspace_bytes(int F, int K, int D, bool fresh) {
    Workspace ws;
    col_blocks(ws, F, K, D, fresh);
    return ws.bytes + 4096;
}

int cacgmm_online_fresh_run(gss_ctx *ctx, int F, int K, int D, double mass, cplx *S, double *n) {
    GSS_PROF(ctx, "cacgmm_online_fresh");
    const int64_t total = (int64_t)F * K * D * D;
    hipLaunchKernelGGL(cacgmm_online_fresh_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       ctx->stream, (int64_t)F * K, D, mass, S, n);
    GSS_LAUNCH_CHECK(ctx, "cacgmm_online_fresh_kernel");
    return GSS_OK;
}

// n_k = mass pi_k, S_k = n_k precision_k^-1; the classes whose precision had no Cholesky factor
// are counted in status word GSS_STATUS_CACGMM_ONLINE_BAD_MODEL (the entry point turns a count
// into an error).
int cacgmm_online_from_model_run(gss_ctx *ctx, const EmModel &m, int F, int K, int D, double mass,
                                 cplx *S, double *n) {
    Workspace ws(ctx);
    const ColWork w = col_blocks(ws, F, K, D, false);
    GSS_TRY(ws.status("online cacgmm from model"));
    GSS_HIP_CHECK(ctx, hipMemsetAsync(w.words, 0, sizeof(int32_t) * 4, ctx->stream));
    ColConvArgs a{m.precision, m.weight, S, n, nullptr, nullptr, w.words, D, K, 0, mass};
    GSS_TRY(col_convert(ctx, a, F, "cacgmm_online_from_model"));
    GSS_HIP_CHECK(ctx, hipMemcpyAsync(ctx->status_host + GSS_STATUS_CACGMM_ONLINE_BAD_MODEL, w.words,
                                      sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    return GSS_OK;
}

// precision = B_k^-1 = n_k S_k^-1, log_det = ln det B_k, weight = pi_k; a class whose S_k has no
// Cholesky factor comes out as the identity model the recursion itself falls back to, and is
// counted in the fallback word.
int cacgmm_online_to_model_run(gss_ctx *ctx, const cplx *S, const double *n, int F, int K, int D,
                               const EmModel &m) {
    Workspace ws(ctx);
    const ColWork w = col_blocks(ws, F, K, D, false);
    GSS_TRY(ws.status("online cacgmm to model"));
    GSS_HIP_CHECK(ctx, hipMemsetAsync(w.words, 0, sizeof(int32_t) * 4, ctx->stream));
    ColConvArgs a{S, n, m.precision, nullptr, m.log_det, m.weight, w.words, D, K, 1, 0.0};
    GSS_TRY(col_convert(ctx, a, F, "cacgmm_online_to_model"));
    GSS_HIP_CHECK(ctx, hipMemcpyAsync(ctx->status_host + GSS_STATUS_CACGMM_ONLINE_FALLBACKS, w.words,
                                      sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    return GSS_OK;
}

// S, n: the caller's state, advanced in place; both NULL: a fresh state of mass prior_mass from
// the arena, thrown away.  The arguments have been validated by the entry point (T >= 1,
// 1 <= K <= GSS_CACGMM_ONLINE_MAX_CLASSES).
int cacgmm_online_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D, const EmGuide &guide,
                      int K, double beta, double prior_mass, cplx *S, double *n, double *gamma) {
    Workspace ws(ctx);
    const ColWork w = col_blocks(ws, F, K, D, !S);
    GSS_TRY(ws.status("online cacgmm"));
    if (!S) {
        S = w.S, n = w.n;
        GSS_TRY(cacgmm_online_fresh_run(ctx, F, K, D, prior_mass, S, n));
    }
    GSS_HIP_CHECK(ctx, hipMemsetAsync(w.words, 0, sizeof(int32_t) * 4, ctx->stream));
    ColArgs a{Y, guide.mask, guide.mask_f_stride, guide.mask_k_stride, S, n, gamma, w.words, T, D, K,
              beta};
    {
        GSS_PROF(ctx, "cacgmm_online");
        const size_t lds = col_lds_bytes(D, K);
#define GSS_COL_LAUNCH(NR)                                                                         \
    do {                                                                                           \
        if (lds > 48 * 1024)                                                                       \
            GSS_HIP_CHECK(ctx, hipFuncSetAttribute(                                                \
                                   reinterpret_cast<const void *>(cacgmm_online_kernel<NR>),       \
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));         \
        hipLaunchKernelGGL(cacgmm_online_kernel<NR>, dim3(F), dim3(64 * K), lds, ctx->stream, a);  \
    } while (0)
        if (D <= 8) GSS_COL_LAUNCH(1);
        else if (D <= 16) GSS_COL_LAUNCH(2);
        else if (D <= 24) GSS_COL_LAUNCH(3);
        else GSS_COL_LAUNCH(4);
#undef GSS_COL_LAUNCH
        GSS_LAUNCH_CHECK(ctx, "cacgmm_online_kernel");
    }
    GSS_HIP_CHECK(ctx, hipMemcpyAsync(ctx->status_host + GSS_STATUS_CACGMM_ONLINE_FALLBACKS, w.words,
                                      sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    return GSS_OK;
}
