// Per-speaker frame activity from the CACGMM posteriors: the power-weighted share of every
// frame that the model gives each class,
//
//    p[f,t] = sum_d |Y[f,t,d]|^2      power[t] = sum_f w[f] p[f,t]
//    score[k,t] = sum_f w[f] gamma[f,k,t] p[f,t] / power[t]      (0 where power[t] == 0)
//
// The measure is defined by tests/posterior_activity_reference.py; the entry points are
// gss_posterior_activity / gss_enhance_observation_activity (include/gss_hip.h).  Two kernels,
// named as gss_profile_report lists them:
//
//   pact_sums     Y (F,T,D), gamma (F,K,T) -> part (FS,K+1,T)   one pass over Y and gamma, FS
//                                                              partial sums over frequency
//   pact_scores   part -> scores (K,T), power (T)              the planes added in order, divide
//
// No floating-point atomics: every sum has one fixed order (channels ascending, then the
// frequencies of a share ascending, then the shares ascending), so a call gives the same bits
// every time.
#include "gss_internal.h"

#include <algorithm>

namespace {

// ------------------------------------------------------------------ partial sums
// A workgroup is one wave and owns a tile of 64 frames for the frequencies of its share.  The
// tile's bins of one frequency, 64 D of them, are contiguous in Y (F,T,D), so the wave loads them
// lane-per-(t,d)-column: D loads of one 16-byte bin per lane, 1 KiB contiguous per wave each,
// SUMS_LB of them in flight before the first is used.  A frame's power needs the D neighbours
// of a row, which sit in D / 64-th of the lanes' registers: |y|^2 goes through LDS, written in
// load order (row = bin / D, column = bin % D, stepped without a division) and read back
// lane-per-frame, D values added in ascending d.  Rows are S = D | 1 doubles apart: an odd stride
// puts the 32 lanes of a ds_read_b64 group on 32 different bank pairs.  From there on lane t is
// frame t: the K posteriors of (f, t) are loaded coalesced along t (512 bytes per class and
// wave, issued before the pass over Y), and the K + 1 accumulators -- num[k], power -- stay
// in registers over the frequencies of the share (NK = the next compiled size >= K).
//
// The other layout, lane-per-frame loads strided by 16 D bytes, needs no LDS but makes every
// load instruction touch 64 cache lines instead of 8 and leaves coalescing to the vector cache;
// the LDS round trip here is 2 D instructions per 64 D bins, far below the rate of the loads.
//
// ceil(T / 64) waves are too few (15 at 941 frames), so the frequencies are cut into FS shares
// (grid.y) and share s writes its own plane of `part`; pact_scores adds the planes in order.
// LDS: 64 S doubles, sized by the launch (12.5 KiB at 24 channels: 12 waves per CU).
constexpr int SUMS_LB = 8;

template <int NK>
__global__ __launch_bounds__(64) void pact_sums_kernel(const cplx *__restrict__ Y,
                                                       const double *__restrict__ gamma,
                                                       const double *__restrict__ W, int F,
                                                       int64_t T, int D, int K, int f_share,
                                                       double *__restrict__ part) {
    extern __shared__ double p2[];
    const int lane = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * 64;
    const int share = blockIdx.y;
    const int f0 = share * f_share, f1 = min(F, f0 + f_share);
    const int frames = (int)min((int64_t)64, T - t0);
    const int bins = frames * D;                    // bins of the tile that exist
    const bool live = lane < frames;
    const int S = D | 1;
    const int row0 = lane / D, col0 = lane - row0 * D;
    const int step_row = 64 / D, step_col = 64 - step_row * D;

    double acc[NK], power = 0.0;
#pragma unroll
    for (int k = 0; k < NK; ++k) acc[k] = 0.0;

    for (int f = f0; f < f1; ++f) {
        const double wf = W ? W[f] : 1.0;
        double g[NK];
        const double *gr = gamma + (int64_t)f * K * T + t0 + lane;
#pragma unroll
        for (int k = 0; k < NK; ++k) g[k] = (k < K && live) ? gr[(int64_t)k * T] : 0.0;

        const cplx *src = Y + ((int64_t)f * T + t0) * D;
        int row = row0, col = col0;
        for (int j = 0; j < D; j += SUMS_LB) {
            cplx v[SUMS_LB];
#pragma unroll
            for (int i = 0; i < SUMS_LB; ++i) {
                const int e = (j + i) * 64 + lane;      // (bins past the tile's end count as 0)
                v[i] = (j + i < D && e < bins) ? src[e] : c_make(0.0, 0.0);
            }
#pragma unroll
            for (int i = 0; i < SUMS_LB; ++i) {
                if (j + i < D) {
                    p2[row * S + col] = c_abs2(v[i]);
                    row += step_row;
                    col += step_col;
                    if (col >= D) {
                        col -= D;
                        ++row;
                    }
                }
            }
        }
        __syncthreads();
        double p = 0.0;
        const double *mine = p2 + lane * S;
#pragma unroll 4
        for (int d = 0; d < D; ++d) p += mine[d];
        __syncthreads();

        const double wp = wf * p;
        power += wp;
#pragma unroll
        for (int k = 0; k < NK; ++k) acc[k] = fma(g[k], wp, acc[k]);
    }
    if (live) {
        double *out = part + (int64_t)share * (K + 1) * T + t0 + lane;
#pragma unroll
        for (int k = 0; k < NK; ++k)
            if (k < K) out[(int64_t)k * T] = acc[k];
        out[(int64_t)K * T] = power;
    }
}

// ------------------------------------------------------------------ scores
// One wave per (tile of 64 frames, class): the planes of the class and of the power added in
// ascending share order, then the division.  Class row K of the grid writes the power.
__global__ __launch_bounds__(64) void pact_scores_kernel(const double *__restrict__ part, int FS,
                                                         int K, int64_t T,
                                                         double *__restrict__ scores,
                                                         double *__restrict__ power_out) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int k = blockIdx.y;
    if (t >= T) return;
    const int64_t plane = (int64_t)(K + 1) * T;
    const double *pw = part + (int64_t)K * T + t;
    double power = 0.0;
#pragma unroll 8
    for (int s = 0; s < FS; ++s) power += pw[s * plane];
    if (k == K) {
        if (power_out) power_out[t] = power;
        return;
    }
    const double *pn = part + (int64_t)k * T + t;
    double num = 0.0;
#pragma unroll 8
    for (int s = 0; s < FS; ++s) num += pn[s * plane];
    scores[(int64_t)k * T + t] = power > 0.0 ? num / power : 0.0;
}

// Frequencies per share of pact_sums: enough shares for about eight waves per CU, at most 64
// planes of `part`, no share empty.
int sums_f_share(int F, int64_t T) {
    const int64_t waves = (T + 63) / 64;
    int64_t fs = (2048 + waves - 1) / waves;
    fs = std::max<int64_t>(1, std::min<int64_t>(fs, std::min(F, 64)));
    return (int)((F + fs - 1) / fs);
}
int sums_shares(int F, int64_t T) {
    const int f_share = sums_f_share(F, T);
    return (F + f_share - 1) / f_share;
}

template <int NK>
void sums_launch(gss_ctx *ctx, const cplx *Y, const double *gamma, const double *W, int F,
                 int64_t T, int D, int K, double *part) {
    hipLaunchKernelGGL(pact_sums_kernel<NK>,
                       dim3((unsigned)((T + 63) / 64), (unsigned)sums_shares(F, T)), dim3(64),
                       sizeof(double) * 64 * (size_t)(D | 1), ctx->stream, Y, gamma, W, F, T, D, K,
                       sums_f_share(F, T), part);
}

}  // namespace

// the partial planes (FS, K + 1, T)
static double *pact_blocks(Workspace &ws, int F, int64_t T, int K) {
    return ws.take<double>((size_t)sums_shares(F, T) * (K + 1) * T, "posterior activity partial planes");
}

size_t pact_workspace_bytes(int F, int64_t T, int K) {
    Workspace ws;
    pact_blocks(ws, F, T, K);
    return ws.bytes + 4096;
}

int pact_run(gss_ctx *ctx, const cplx *Y, const double *gamma, int F, int K, int64_t T, int D,
             const double *W, double *scores, double *power) {
    const int FS = sums_shares(F, T);
    Workspace ws(ctx);
    double *part = pact_blocks(ws, F, T, K);
    GSS_TRY(ws.status("posterior activity"));
    {
        GSS_PROF(ctx, "pact_sums");
        if (K <= 5) sums_launch<5>(ctx, Y, gamma, W, F, T, D, K, part);
        else if (K <= 12) sums_launch<12>(ctx, Y, gamma, W, F, T, D, K, part);
        else sums_launch<GSS_MAX_CLASSES>(ctx, Y, gamma, W, F, T, D, K, part);
        GSS_LAUNCH_CHECK(ctx, "pact_sums_kernel");
    }
    {
        GSS_PROF(ctx, "pact_scores");
        hipLaunchKernelGGL(pact_scores_kernel, dim3((unsigned)((T + 63) / 64), (unsigned)(K + 1)),
                           dim3(64), 0, ctx->stream, (const double *)part, FS, K, T, scores,
                           power);
        GSS_LAUNCH_CHECK(ctx, "pact_scores_kernel");
    }
    return GSS_OK;
}
