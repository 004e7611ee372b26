// Envelope-variance channel selection (Wolf & Nadeu 2014) ahead of WPE: rank the channels of
// an STFT by the variance over time of their compressed, mean-normalised sub-band envelopes
// and keep the best n.  The measure is defined by tests/channel_select_reference.py; the
// entry points are gss_channel_scores / gss_select_channels / gss_enhance_observation_select
// (include/gss_hip.h).  Four kernels, named as gss_profile_report lists them:
//
//   chsel_bands    Y (F,T,D) -> E (FS,B,T,D)   one pass over Y, FS partial sums over frequency
//   chsel_scores   E -> V (B,D) -> scores (D)  reductions over time per (band, channel), then
//                                              over channels and bands
//   chsel_pick     scores -> n channel indices, ascending (device memory + status words)
//   chsel_gather   Y (F,T,D) -> (F,T,n) with the indices read on the device
//
// No floating-point atomics anywhere: every sum has one fixed order, so a call gives the same
// bits every time.  The host never waits for the selection: n comes from the caller and shapes
// every later launch, only WHICH channels were kept is decided on the device.
#include "gss_internal.h"

#include <algorithm>
#include <cmath>

namespace {

// ------------------------------------------------------------------ band energies
// Seen as matrices, E (B, M) = W (B, F) |Y|^2 (F, M) with M = T D the contiguous (t, d) axis.
// A lane owns one column m and walks the frequencies of its block's share: every load is one
// 16-byte bin per lane, 1 KiB contiguous per wave, BANDS_LB of them in flight before the first
// is used.  The weight of (band, frequency) is the same for the whole wave -- its address
// depends on the block and the loop counters only, so it is fetched through the scalar cache
// into SGPRs -- and a run of BANDS_LB zero weights (a mel row is non-zero on a short run of
// bins) skips its FMAs on a scalar test of their bits.  Any dense table works: all B
// accumulators of a column live in registers (NB = the next compiled size >= B).
//
// M / 64 waves are too few to keep enough loads in flight (353 at 941 frames of 24 channels),
// so the frequencies are cut into FS shares (grid.y) and share s writes its own plane of E;
// chsel_scores adds the planes in order when it reads them.
constexpr int BANDS_LB = 8;

// the bits of a weight without its sign: 0 for +0.0 and -0.0 only
__device__ __forceinline__ unsigned long long weight_bits(double w) {
    return (unsigned long long)__double_as_longlong(w) << 1;
}

template <int NB>
__global__ __launch_bounds__(64) void chsel_bands_kernel(const cplx *__restrict__ Y,
                                                         const double *__restrict__ W, int F,
                                                         int64_t M, int B, int f_share,
                                                         double *__restrict__ E) {
    const int64_t m = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int share = blockIdx.y;
    const int f0 = share * f_share, f1 = min(F, f0 + f_share);
    const bool live = m < M;
    const cplx *col = Y + (live ? m : M - 1);      // (lanes past the end reread the last column)
    double acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.0;

    int f = f0;
    for (; f + BANDS_LB <= f1; f += BANDS_LB) {
        cplx v[BANDS_LB];
#pragma unroll
        for (int j = 0; j < BANDS_LB; ++j)
            v[j] = col[(int64_t)(f + j) * M];
        double p[BANDS_LB];
#pragma unroll
        for (int j = 0; j < BANDS_LB; ++j) p[j] = c_abs2(v[j]);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (b < B) {
                const double *w = W + (int64_t)b * F + f;
                double wj[BANDS_LB];
                unsigned long long any = 0ull;
#pragma unroll
                for (int j = 0; j < BANDS_LB; ++j) {
                    wj[j] = w[j];
                    any |= weight_bits(wj[j]);
                }
                if (any != 0ull) {
#pragma unroll
                    for (int j = 0; j < BANDS_LB; ++j) acc[b] = fma(wj[j], p[j], acc[b]);
                }
            }
        }
    }
    for (; f < f1; ++f) {
        const double p = c_abs2(col[(int64_t)f * M]);
#pragma unroll
        for (int b = 0; b < NB; ++b)
            if (b < B) acc[b] = fma(W[(int64_t)b * F + f], p, acc[b]);
    }
    if (live) {
        double *out = E + (int64_t)share * B * M + m;
#pragma unroll
        for (int b = 0; b < NB; ++b)
            if (b < B) out[(int64_t)b * M] = acc[b];
    }
}

// ------------------------------------------------------------------ variances
// One workgroup per band; NT threads, a multiple of D, so that a thread stays on one channel
// (element i = tid + k NT of the (T, D) slab has channel tid % D) while consecutive lanes read
// consecutive elements.  The four passes over the slab follow the definition step by step --
// maximum, mean of the logs of the floored energies, mean of C = exp(L / 3), mean of the
// squared deviations from that mean (the two-pass variance) -- and keep their intermediate
// (log E, then C) in place of E: every thread rereads only what it wrote itself.  The slab of
// a band (180 KB at 941 x 24) stays in L2 between the passes.
constexpr int VAR_THREADS = 1024;

__device__ __forceinline__ double channel_reduce(double v, bool take_max, int tid, int NT, int D,
                                                 double *red, double *stat) {
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    if (tid < D) {
        double r = red[tid];
        for (int j = tid + D; j < NT; j += D) r = take_max ? fmax(r, red[j]) : r + red[j];
        stat[tid] = r;
    }
    __syncthreads();
    return stat[tid % D];
}

__global__ __launch_bounds__(VAR_THREADS) void chsel_var_kernel(double *E, int FS, int B,
                                                                int64_t T, int D,
                                                                double floor_rel,
                                                                double *__restrict__ V) {
    __shared__ double red[VAR_THREADS];
    __shared__ double stat[GSS_MAX_CHANNELS];
    const int b = blockIdx.x, tid = threadIdx.x, NT = blockDim.x;
    const int64_t M = T * D, plane = (int64_t)B * M;
    double *e = E + (int64_t)b * M;
    const double frames = (double)T;

    // the planes of the frequency shares, added in order; m = max over t
    double mx = -INFINITY;
#pragma unroll 4
    for (int64_t i = tid; i < M; i += NT) {
        double v = e[i];
        for (int s = 1; s < FS; ++s) v += e[s * plane + i];
        if (FS > 1) e[i] = v;
        mx = fmax(mx, v);
    }
    const double m = channel_reduce(mx, true, tid, NT, D, red, stat);
    const bool dead = m == 0.0;
    const double fl = floor_rel * m;

    double sl = 0.0;
#pragma unroll 4
    for (int64_t i = tid; i < M; i += NT) {
        const double l = dead ? 0.0 : log(fmax(e[i], fl));
        e[i] = l;
        sl += l;
    }
    const double ml = channel_reduce(sl, false, tid, NT, D, red, stat) / frames;

    double sc = 0.0;
#pragma unroll 4
    for (int64_t i = tid; i < M; i += NT) {
        const double c = exp((e[i] - ml) / 3.0);
        e[i] = c;
        sc += c;
    }
    const double mc = channel_reduce(sc, false, tid, NT, D, red, stat) / frames;

    double sv = 0.0;
#pragma unroll 4
    for (int64_t i = tid; i < M; i += NT) {
        const double dv = e[i] - mc;
        sv = fma(dv, dv, sv);
    }
    const double var = channel_reduce(sv, false, tid, NT, D, red, stat) / frames;
    if (tid < D) V[(int64_t)b * D + tid] = dead ? 0.0 : var;
}

// scores[d] = sum over bands of V[b,d] / max_d' V[b,d'] (0 for a band whose maximum is 0)
__global__ __launch_bounds__(64) void chsel_score_kernel(const double *__restrict__ V, int B,
                                                         int D, double *__restrict__ scores) {
    __shared__ double v[64 * GSS_MAX_CHANNELS];
    __shared__ double band_max[64];
    const int tid = threadIdx.x;
    for (int i = tid; i < B * D; i += 64) v[i] = V[i];
    __syncthreads();
    if (tid < B) {
        double mb = v[tid * D];
        for (int d = 1; d < D; ++d) mb = fmax(mb, v[tid * D + d]);
        band_max[tid] = mb;
    }
    __syncthreads();
    if (tid < D) {
        double s = 0.0;
        for (int b = 0; b < B; ++b) {
            const double mb = band_max[b];
            s += mb > 0.0 ? v[b * D + tid] / mb : 0.0;
        }
        scores[tid] = s;
    }
}

// ------------------------------------------------------------------ pick
// Rank by counting (D <= 32, one wave): channel j comes before channel d when its score is
// higher, or equal with j < d; a non-finite score comes after every finite one.  The n first
// are kept and written in ascending channel order: the position of a kept channel is the
// number of kept channels below it.
__global__ __launch_bounds__(64) void chsel_pick_kernel(const double *__restrict__ scores, int D,
                                                        int n, int32_t *__restrict__ channels,
                                                        int32_t *__restrict__ channels_out,
                                                        int32_t *__restrict__ status) {
    __shared__ double sh[GSS_MAX_CHANNELS];
    const int tid = threadIdx.x;
    const bool in = tid < D;
    const double s = in ? scores[tid] : 0.0;
    if (in) sh[tid] = s;
    __syncthreads();
    const bool fin = isfinite(s);
    int rank = 0;
    for (int j = 0; j < D; ++j) {
        const double sj = sh[j];
        const bool fj = isfinite(sj);
        bool before;
        if (fj != fin) before = fj;
        else if (fin) before = sj > s || (sj == s && j < tid);
        else before = j < tid;
        rank += before ? 1 : 0;
    }
    const bool kept = in && rank < n;
    const unsigned long long mask = __ballot(kept);
    if (kept) {
        const int pos = __popcll(mask & ((1ull << tid) - 1ull));
        channels[pos] = tid;
        if (channels_out) channels_out[pos] = tid;
        __hip_atomic_store(status + pos, tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ------------------------------------------------------------------ gather
// out[(f T + t) n + j] = Y[(f T + t) D + channels[j]]: one 16-byte bin per lane, stores
// contiguous, loads contiguous up to the dropped channels.  A lane takes GATHER_PER bins
// 256 apart (rows * n < 2^31, checked by the entry points).
constexpr int GATHER_PER = 4;

__global__ __launch_bounds__(256) void chsel_gather_kernel(const cplx *__restrict__ Y,
                                                           unsigned total, int D, int n,
                                                           const int32_t *__restrict__ channels,
                                                           cplx *__restrict__ out) {
    __shared__ int ch[GSS_MAX_CHANNELS];
    if (threadIdx.x < n) ch[threadIdx.x] = channels[threadIdx.x];
    __syncthreads();
    const unsigned base = blockIdx.x * (256u * GATHER_PER) + threadIdx.x;
    cplx v[GATHER_PER];
#pragma unroll
    for (int k = 0; k < GATHER_PER; ++k) {
        const unsigned idx = base + k * 256u;
        if (idx < total) {
            const unsigned row = idx / (unsigned)n, j = idx - row * (unsigned)n;
            v[k] = Y[(int64_t)row * D + ch[j]];
        }
    }
#pragma unroll
    for (int k = 0; k < GATHER_PER; ++k) {
        const unsigned idx = base + k * 256u;
        if (idx < total) out[idx] = v[k];
    }
}

// Frequency shares of chsel_bands: enough waves for about one per SIMD four times over, at
// least 16 frequencies per share, at most 8 planes of E.
int bands_shares(int F, int64_t M) {
    const int64_t waves = (M + 63) / 64;
    int64_t fs = (1024 + waves - 1) / waves;
    fs = std::min<int64_t>(fs, 8);
    fs = std::min<int64_t>(fs, std::max(1, F / 16));
    return (int)std::max<int64_t>(fs, 1);
}

template <int NB>
void bands_launch(gss_ctx *ctx, const cplx *Y, const double *W, int F, int64_t M, int B, int FS,
                  double *E) {
    const int f_share = (F + FS - 1) / FS;
    hipLaunchKernelGGL(chsel_bands_kernel<NB>, dim3((unsigned)((M + 63) / 64), (unsigned)FS),
                       dim3(64), 0, ctx->stream, Y, W, F, M, B, f_share, E);
}

}  // namespace

// chsel_select_run: scores and channel indices, then the blocks of the chsel_scores_run it
// calls: the E planes and, unless the caller takes the band variances, V
struct ChselPickWork {
    double *scores;
    int32_t *idx;
};
static ChselPickWork chsel_select_blocks(Workspace &ws) {
    ChselPickWork k;
    k.scores = ws.take<double>(GSS_MAX_CHANNELS, "channel selection scores");
    k.idx = ws.take<int32_t>(GSS_MAX_CHANNELS, "channel selection indices");
    return k;
}
struct ChselScoreWork {
    double *E, *band_var;
};
static ChselScoreWork chsel_scores_blocks(Workspace &ws, int F, int64_t T, int D, int B,
                                          bool own_band_var) {
    const int64_t M = T * D;
    ChselScoreWork k;
    k.E = ws.take<double>((size_t)bands_shares(F, M) * B * M, "channel selection E");
    k.band_var = own_band_var ? ws.take<double>((size_t)B * D, "channel selection V") : nullptr;
    return k;
}

size_t chsel_workspace_bytes(int F, int64_t T, int D, int B) {
    Workspace ws;
    chsel_select_blocks(ws);
    chsel_scores_blocks(ws, F, T, D, B, true);
    return ws.bytes + 4096;
}

int chsel_scores_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D,
                     const gss_channel_select &sel, double *scores, double *band_var) {
    const int B = sel.bands;
    const int64_t M = T * D;
    const int FS = bands_shares(F, M);
    Workspace ws(ctx);
    const ChselScoreWork k = chsel_scores_blocks(ws, F, T, D, B, !band_var);
    GSS_TRY(ws.status("channel selection scores"));
    double *E = k.E;
    if (!band_var) band_var = k.band_var;
    {
        GSS_PROF(ctx, "chsel_bands");
        if (B <= 8) bands_launch<8>(ctx, Y, sel.bank_dev, F, M, B, FS, E);
        else if (B <= 16) bands_launch<16>(ctx, Y, sel.bank_dev, F, M, B, FS, E);
        else if (B <= 32) bands_launch<32>(ctx, Y, sel.bank_dev, F, M, B, FS, E);
        else if (B <= 48) bands_launch<48>(ctx, Y, sel.bank_dev, F, M, B, FS, E);
        else bands_launch<64>(ctx, Y, sel.bank_dev, F, M, B, FS, E);
        GSS_LAUNCH_CHECK(ctx, "chsel_bands_kernel");
    }
    {
        GSS_PROF(ctx, "chsel_scores");
        const int NT = VAR_THREADS / D * D;
        hipLaunchKernelGGL(chsel_var_kernel, dim3((unsigned)B), dim3((unsigned)NT), 0, ctx->stream,
                           E, FS, B, T, D, sel.floor, band_var);
        GSS_LAUNCH_CHECK(ctx, "chsel_var_kernel");
        hipLaunchKernelGGL(chsel_score_kernel, dim3(1), dim3(64), 0, ctx->stream,
                           (const double *)band_var, B, D, scores);
        GSS_LAUNCH_CHECK(ctx, "chsel_score_kernel");
    }
    return GSS_OK;
}

int chsel_select_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D,
                     const gss_channel_select &sel, cplx *Ysel, int32_t *channels) {
    const int n = sel.keep;
    Workspace ws(ctx);
    const ChselPickWork k = chsel_select_blocks(ws);
    GSS_TRY(ws.status("channel selection"));
    GSS_TRY(chsel_scores_run(ctx, Y, F, T, D, sel, k.scores, nullptr));
    {
        GSS_PROF(ctx, "chsel_pick");
        hipLaunchKernelGGL(chsel_pick_kernel, dim3(1), dim3(64), 0, ctx->stream,
                           (const double *)k.scores, D, n, k.idx, channels,
                           ctx->status_dev + GSS_STATUS_CHANNELS);
        GSS_LAUNCH_CHECK(ctx, "chsel_pick_kernel");
    }
    ctx->last_selected = n;
    if (Ysel) {
        GSS_PROF(ctx, "chsel_gather");
        const unsigned total = (unsigned)((int64_t)F * T * n);
        const unsigned per_block = 256u * GATHER_PER;
        hipLaunchKernelGGL(chsel_gather_kernel, dim3((total + per_block - 1) / per_block),
                           dim3(256), 0, ctx->stream, Y, total, D, n, (const int32_t *)k.idx, Ysel);
        GSS_LAUNCH_CHECK(ctx, "chsel_gather_kernel");
    }
    return GSS_OK;
}
