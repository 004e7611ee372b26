// Online WPE: frame-recursive (RLS) dereverberation with a carried state, the online form of
// nara_wpe (include/gss_hip.h: gss_wpe_online).  Per problem -- one
// frequency, or one (frequency, array) pair -- with n = taps * C and L = taps + delay, for every
// frame t in order:
//   sigma = sum |frames t-L .. t|^2 / ((L+1) C)           (input only: wpe_online_sigma_kernel)
//   w     = the taps frames t-delay-taps+1 .. t-delay      (input only)
//   x_t   = y_t - G^H w                                    (the output)
//   nom   = P w;  den = alpha sigma + Re(w^H nom)
//   den > 0:  P <- (P - nom nom^H / den) / alpha,  G <- G + (nom / den) x_t^H
//   else:     P, G unchanged (the whole buffer is digital silence)
// Strictly serial in time, parallel over problems: one persistent workgroup per problem walks the
// frames of the call.  Two forms, chosen by n alone (never by T, F or A: a recording fed in
// blocks must not change form between calls):
//   on-chip (n <= 64): one wave per problem, P, G in LDS for all frames of the call;
//   memory  (n <= 512): four waves per problem, P, G stay in their HBM buffers; the update of P
//     by frame t and the product P_{t+1} w_{t+1} share one pass over the matrix.
// Both keep the FULL Hermitian matrix and update (i, j) and (j, i) with operations that commute
// with conjugation (c_outer: no fused multiply-add in the product nom_i conj(nom_j)), so the
// lower triangle stays the exact conjugate of the upper one and the diagonal exactly real -- a
// state written back is the state held, and a call continued from it continues bit for bit.
// No atomics, every sum in one fixed order: the same call gives the same bits.
#include <algorithm>

#include "gss_internal.h"

namespace {

constexpr int WOL_ONCHIP_MAX_N = 64;     // one lane per row of P
constexpr int WOL_MAX_N = 512;
constexpr int WOL_MEM_THREADS = 256;
constexpr int WOL_MEM_WAVES = WOL_MEM_THREADS / 64;
constexpr int WOL_XROWS = 16;            // memory form: row groups of the pass over G, at most

struct WolArgs {
    const cplx *Y;        // (F, T, A C)
    cplx *X;              // (F, T, A C)
    cplx *P;              // (F A, n, n)
    cplx *G;              // (F A, n, C)
    const cplx *hist;     // (F A, L, C), oldest frame first: frames -L .. -1 of the stream
    const double *sigma;  // (F A, T)
    int64_t T;
    int A, C, taps, delay, n, L;
    double alpha, inv_alpha;
};

// Channel c of frame s >= -L of the stream of problem (f, arr): the call's frames, before them
// the carried history.
__device__ __forceinline__ cplx wol_frame(const WolArgs &a, int f, int arr, int64_t s, int c) {
    if (s >= 0) return a.Y[((int64_t)f * a.T + s) * (a.A * a.C) + arr * a.C + c];
    return a.hist[((int64_t)(f * a.A + arr) * a.L + (a.L + s)) * a.C + c];
}

// (p - nom_i conj(nom_j) / den) / alpha; commutes with conjugation
__device__ __forceinline__ cplx wol_downdate(cplx p, cplx ni, cplx nj, double rden, double inv_alpha) {
    const cplx o = c_outer(ni, nj);
    return c_make(fma(-o.x, rden, p.x) * inv_alpha, fma(-o.y, rden, p.y) * inv_alpha);
}

// sigma[prob, t]: the mean power of the buffer of frame t, summed oldest frame first, channels
// ascending.  Parallel over frames; the serial kernels only read it.
__global__ __launch_bounds__(256) void wpe_online_sigma_kernel(WolArgs a, double *__restrict__ sigma) {
    const int prob = blockIdx.x, f = prob / a.A, arr = prob - f * a.A;
    const double scale = (double)(a.L + 1) * (double)a.C;
    for (int64_t t = threadIdx.x; t < a.T; t += 256) {
        double acc = 0.0;
        for (int64_t s = t - a.L; s <= t; ++s)
            for (int c = 0; c < a.C; ++c) {
                const cplx v = wol_frame(a, f, arr, s, c);
                acc = fma(v.x, v.x, acc);
                acc = fma(v.y, v.y, acc);
            }
        sigma[(int64_t)prob * a.T + t] = acc / scale;
    }
}

// The history after the call: frames T-L .. T-1 of the stream (old history where T < L), into a
// buffer of its own -- the old history is still being read.
__global__ __launch_bounds__(256) void wpe_online_history_kernel(WolArgs a, cplx *__restrict__ out) {
    const int prob = blockIdx.x, f = prob / a.A, arr = prob - f * a.A;
    const int total = a.L * a.C;
    for (int idx = threadIdx.x; idx < total; idx += 256) {
        const int l = idx / a.C, c = idx - l * a.C;
        out[(int64_t)prob * total + idx] = wol_frame(a, f, arr, a.T - a.L + l, c);
    }
}

// P = I on buffers that have been zeroed
__global__ __launch_bounds__(256) void wpe_online_identity_kernel(cplx *__restrict__ P, int n) {
    cplx *Pp = P + (int64_t)blockIdx.x * n * n;
    for (int i = threadIdx.x; i < n; i += 256) Pp[(int64_t)i * n + i] = c_make(1.0, 0.0);
}

// On-chip form: one wave per problem, lane i owns row i of P and of G.  LDS: P as (j, i) ->
// [j n + i] (lane i walks its row with consecutive lanes on consecutive 16-byte slots), G as
// (i, c) -> [i CP + c] with CP odd (the lanes of one c fall on different slots), w, nom, x.
// w, y and sigma of frame t + 1 are fetched while frame t's dependent chain runs.
__global__ __launch_bounds__(64) void wpe_online_onchip_kernel(WolArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int n = a.n, C = a.C, CP = C | 1;
    cplx *Pm = reinterpret_cast<cplx *>(smem);
    cplx *Gm = Pm + n * n;
    cplx *wb = Gm + n * CP;
    cplx *nb = wb + n;
    cplx *xb = nb + n;      // C
    cplx *yb = xb + C;      // C
    const int prob = blockIdx.x, f = prob / a.A, arr = prob - f * a.A;
    const int lane = threadIdx.x;
    const bool row = lane < n;
    const int i = row ? lane : n - 1;       // idle lanes read row n - 1 and contribute zeros
    cplx *Pg = a.P + (int64_t)prob * n * n;
    cplx *Gg = a.G + (int64_t)prob * n * C;
    // a reader takes the upper triangle and the real part of the diagonal
    for (int idx = lane; idx < n * n; idx += 64) {
        const int r = idx / n, c = idx - r * n;
        cplx v = r <= c ? Pg[idx] : c_conj(Pg[c * n + r]);
        if (r == c) v.y = 0.0;
        Pm[c * n + r] = v;
    }
    for (int idx = lane; idx < n * C; idx += 64) {
        const int r = idx / C, c = idx - r * C;
        Gm[r * CP + c] = Gg[idx];
    }
    wave_sync();

    const int tau = i / C, ch = i - tau * C;
    const int D = a.A * C;
    const double *sig = a.sigma + (int64_t)prob * a.T;
    const cplx zero = c_make(0.0, 0.0);
    cplx w_next = row ? wol_frame(a, f, arr, (int64_t)0 - a.delay - tau, ch) : zero;
    cplx y_next = lane < C ? wol_frame(a, f, arr, 0, lane) : zero;
    double sigma_next = sig[0];
    for (int64_t t = 0; t < a.T; ++t) {
        const cplx w = w_next;
        const double sigma = sigma_next;
        if (row) wb[lane] = w;
        if (lane < C) yb[lane] = y_next;
        if (t + 1 < a.T) {
            if (row) w_next = wol_frame(a, f, arr, t + 1 - a.delay - tau, ch);
            if (lane < C) y_next = wol_frame(a, f, arr, t + 1, lane);
            sigma_next = sig[t + 1];
        }
        wave_sync();
        cplx nom = zero;
        for (int j = 0; j < n; ++j) c_fma(nom, Pm[j * n + i], wb[j]);
        if (!row) nom = zero;
        const double den = fma(a.alpha, sigma, wave_sum(fma(w.x, nom.x, w.y * nom.y)));
        const bool upd = den > 0.0;
        const double rden = upd ? 1.0 / den : 0.0;
        const cplx k = c_scale(nom, rden);
        for (int c = 0; c < C; ++c) {
            cplx g = Gm[i * CP + c];
            const cplx part = row ? c_cmul(g, w) : zero;
            const double sr = wave_sum(part.x), si = wave_sum(part.y);
            const cplx y = yb[c];
            const cplx x = c_make(y.x - sr, y.y - si);      // the a-priori error
            if (lane == 0) xb[c] = x;
            if (upd && row) {
                c_fmac(g, k, x);
                Gm[i * CP + c] = g;
            }
        }
        if (upd) {
            if (row) nb[lane] = nom;
            wave_sync();
            if (row)
                for (int j = 0; j < n; ++j)
                    Pm[j * n + i] = wol_downdate(Pm[j * n + i], nom, nb[j], rden, a.inv_alpha);
        }
        wave_sync();
        if (lane < C) a.X[((int64_t)f * a.T + t) * D + arr * C + lane] = xb[lane];
    }
    wave_sync();
    for (int idx = lane; idx < n * n; idx += 64) {
        const int r = idx / n, c = idx - r * n;
        Pg[idx] = Pm[c * n + r];
    }
    for (int idx = lane; idx < n * C; idx += 64) {
        const int r = idx / C, c = idx - r * C;
        Gg[idx] = Gm[r * CP + c];
    }
}

// Memory form: four waves per problem, P and G stay in HBM.  One pass per frame over both:
//   P: wave v owns rows v, v + 4, ...; lane l the columns l, l + 64, ... of a row: read, update
//      by frame t (when den_t > 0), write, accumulate into (P_{t+1} w_{t+1})_i -- a wave sum per
//      row, and per wave the running sum of Re(conj(w_i) nom_i) for den_{t+1};
//   G: thread (r, c) owns rows r, r + R, ... of column c: read, update, write, accumulate
//      conj(G_{t+1}[i, c]) w_{t+1, i}; the R partial sums of a channel are added in ascending r.
// Every element of P and G is read and written by the same thread in every frame, so the state
// needs no visibility between threads; nom, w and the partial sums go through LDS in two
// buffers that alternate by frame, which leaves ONE workgroup barrier per frame.  The frame
// before the first (the product alone) and the last (the update alone) run the same pass with
// one half switched off: the same sums in the same order wherever a call begins or ends.
__global__ __launch_bounds__(WOL_MEM_THREADS) void wpe_online_mem_kernel(WolArgs a) {
    __shared__ cplx nomb[2][WOL_MAX_N];
    __shared__ cplx wb[2][WOL_MAX_N];
    __shared__ cplx xpart[2][WOL_MEM_THREADS];
    __shared__ double dpart[2][WOL_MEM_WAVES];
    const int n = a.n, C = a.C;
    const int prob = blockIdx.x, f = prob / a.A, arr = prob - f * a.A;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int R = min(WOL_MEM_THREADS / C, WOL_XROWS);
    const int gr = tid / C, gc = tid - gr * C;
    const bool gact = gr < R;
    const int D = a.A * C;
    cplx *Pg = a.P + (int64_t)prob * n * n;
    cplx *Gg = a.G + (int64_t)prob * n * C;
    const double *sig = a.sigma + (int64_t)prob * a.T;
    const cplx zero = c_make(0.0, 0.0);
    // a reader takes the upper triangle and the real part of the diagonal: mirror it once
    for (int idx = tid; idx < n * n; idx += WOL_MEM_THREADS) {
        const int r = idx / n, c = idx - r * n;
        if (r > c) Pg[idx] = c_conj(Pg[c * n + r]);
        else if (r == c) Pg[idx].y = 0.0;
    }
    for (int idx = tid; idx < n; idx += WOL_MEM_THREADS) {
        const int tau = idx / C;
        wb[0][idx] = wol_frame(a, f, arr, (int64_t)0 - a.delay - tau, idx - tau * C);
    }
    __syncthreads();

    cplx y_next = gact ? wol_frame(a, f, arr, 0, gc) : zero;
    double sigma_next = sig[0];
    cplx x = zero;
    double rden = 0.0;
    // t = -1: the product P_0 w_0 and G_0^H w_0 alone
    for (int64_t t = -1; t < a.T; ++t) {
        const int cur = (int)(t & 1), nxt = cur ^ 1;
        bool upd = false;
        const bool prod = t + 1 < a.T;
        if (t >= 0) {
            const cplx y = y_next;
            const double sigma = sigma_next;
            if (prod) {
                for (int idx = tid; idx < n; idx += WOL_MEM_THREADS) {
                    const int tau = idx / C;
                    wb[nxt][idx] = wol_frame(a, f, arr, t + 1 - a.delay - tau, idx - tau * C);
                }
                if (gact) y_next = wol_frame(a, f, arr, t + 1, gc);
                sigma_next = sig[t + 1];
            }
            __syncthreads();
            const double den = fma(a.alpha, sigma,
                                   ((dpart[cur][0] + dpart[cur][1]) + dpart[cur][2]) + dpart[cur][3]);
            upd = den > 0.0;
            rden = upd ? 1.0 / den : 0.0;
            if (gact) {
                cplx s = zero;
                for (int r = 0; r < R; ++r) s = c_add(s, xpart[cur][r * C + gc]);
                x = c_sub(y, s);
                if (gr == 0) a.X[((int64_t)f * a.T + t) * D + arr * C + gc] = x;
            }
        }
        double dsum = 0.0;
        for (int i = wave; i < n; i += WOL_MEM_WAVES) {
            const cplx ni = nomb[cur][i];
            cplx *rowp = Pg + (int64_t)i * n;
            cplx acc = zero;
            for (int j = lane; j < n; j += 64) {
                cplx p = rowp[j];
                if (upd) {
                    p = wol_downdate(p, ni, nomb[cur][j], rden, a.inv_alpha);
                    rowp[j] = p;
                }
                if (prod) c_fma(acc, p, wb[nxt][j]);
            }
            if (prod) {
                const double sr = wave_sum(acc.x), si = wave_sum(acc.y);
                const cplx wi = wb[nxt][i];
                dsum = fma(wi.x, sr, dsum);
                dsum = fma(wi.y, si, dsum);
                if (lane == 0) nomb[nxt][i] = c_make(sr, si);
            }
        }
        if (prod && lane == 0) dpart[nxt][wave] = dsum;
        if (gact) {
            cplx s = zero;
            for (int i = gr; i < n; i += R) {
                cplx g = Gg[i * C + gc];
                if (upd) {
                    c_fmac(g, c_scale(nomb[cur][i], rden), x);
                    Gg[i * C + gc] = g;
                }
                if (prod) c_cfma(s, g, wb[nxt][i]);
            }
            if (prod) xpart[nxt][gr * C + gc] = s;
        }
    }
}

}  // namespace

bool wpe_online_uses_memory_form(int n, bool force_mem) { return force_mem || n > WOL_ONCHIP_MAX_N; }

// sigma, then for a fresh state its buffers.  hist: the fresh state's history, or, with the
// caller's state, the new history (one element more than L C: never an empty block).
struct WolWork {
    double *sigma;
    cplx *P, *G, *hist;
};
static WolWork wol_blocks(Workspace &ws, int F, int64_t T, int A, int C, int taps, int delay,
                          bool fresh) {
    const size_t probs = (size_t)F * A, n = (size_t)taps * C, L = (size_t)taps + delay;
    WolWork k;
    k.sigma = ws.take<double>(probs * (size_t)T, "online wpe sigma");
    k.P = fresh ? ws.take<cplx>(probs * n * n, "online wpe P") : nullptr;
    k.G = fresh ? ws.take<cplx>(probs * n * C, "online wpe G") : nullptr;
    k.hist = ws.take<cplx>(probs * L * C + 1, fresh ? "online wpe history" : "online wpe new history");
    return k;
}

size_t wpe_online_workspace_bytes(int F, int64_t T, int A, int C, int taps, int delay, bool fresh) {
    Workspace ws;
    wol_blocks(ws, F, std::max<int64_t>(T, 1), A, C, taps, delay, fresh);
    return ws.bytes + 4096;
}

int wpe_online_init_run(gss_ctx *ctx, int F, int A, int C, int taps, int delay, cplx *P, cplx *G,
                        cplx *hist) {
    const size_t probs = (size_t)F * A, n = (size_t)taps * C, L = (size_t)taps + delay;
    GSS_HIP_CHECK(ctx, hipMemsetAsync(P, 0, sizeof(cplx) * probs * n * n, ctx->stream));
    GSS_HIP_CHECK(ctx, hipMemsetAsync(G, 0, sizeof(cplx) * probs * n * C, ctx->stream));
    if (L * C > 0)
        GSS_HIP_CHECK(ctx, hipMemsetAsync(hist, 0, sizeof(cplx) * probs * L * C, ctx->stream));
    hipLaunchKernelGGL(wpe_online_identity_kernel, dim3((unsigned)probs), dim3(256), 0, ctx->stream,
                       P, (int)n);
    GSS_LAUNCH_CHECK(ctx, "wpe_online_identity_kernel");
    return GSS_OK;
}

// P, G, hist: the caller's state, advanced in place; all three NULL: a fresh state from the
// arena, thrown away.  The arguments have been validated by the entry point (T >= 1).
int wpe_online_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int A, int C, int taps, int delay,
                   double alpha, cplx *P, cplx *G, cplx *hist, cplx *X, bool force_mem) {
    const int n = taps * C, L = taps + delay;
    const size_t probs = (size_t)F * A;
    const bool fresh = P == nullptr;
    Workspace ws(ctx);
    const WolWork k = wol_blocks(ws, F, T, A, C, taps, delay, fresh);
    GSS_TRY(ws.status("online wpe"));
    double *sigma = k.sigma;
    cplx *hist_new = fresh ? nullptr : k.hist;
    if (fresh) {
        P = k.P, G = k.G, hist = k.hist;
        GSS_TRY(wpe_online_init_run(ctx, F, A, C, taps, delay, P, G, hist));
    }
    WolArgs a{Y, X, P, G, hist, sigma, T, A, C, taps, delay, n, L, alpha, 1.0 / alpha};
    {
        GSS_PROF(ctx, "wpe_online_sigma");
        hipLaunchKernelGGL(wpe_online_sigma_kernel, dim3((unsigned)probs), dim3(256), 0, ctx->stream,
                           a, sigma);
        GSS_LAUNCH_CHECK(ctx, "wpe_online_sigma_kernel");
    }
    if (wpe_online_uses_memory_form(n, force_mem)) {
        GSS_PROF(ctx, "wpe_online_mem");
        hipLaunchKernelGGL(wpe_online_mem_kernel, dim3((unsigned)probs), dim3(WOL_MEM_THREADS), 0,
                           ctx->stream, a);
        GSS_LAUNCH_CHECK(ctx, "wpe_online_mem_kernel");
    } else {
        GSS_PROF(ctx, "wpe_online_onchip");
        // P, G, w, nom, x, y; at most 16 (64 * 64 + 64 * 33 + 128 + 64) bytes = 100 KB
        const size_t lds = sizeof(cplx) * ((size_t)n * n + (size_t)n * (C | 1) + 2 * (size_t)n + 2 * (size_t)C);
        if (lds > 48 * 1024)
            GSS_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(wpe_online_onchip_kernel),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(wpe_online_onchip_kernel, dim3((unsigned)probs), dim3(64), lds, ctx->stream, a);
        GSS_LAUNCH_CHECK(ctx, "wpe_online_onchip_kernel");
    }
    if (!fresh && L * C > 0) {
        hipLaunchKernelGGL(wpe_online_history_kernel, dim3((unsigned)probs), dim3(256), 0, ctx->stream,
                           a, hist_new);
        GSS_LAUNCH_CHECK(ctx, "wpe_online_history_kernel");
        GSS_HIP_CHECK(ctx, hipMemcpyAsync(hist, hist_new, sizeof(cplx) * probs * L * C,
                                          hipMemcpyDeviceToDevice, ctx->stream));
    }
    return GSS_OK;
}
