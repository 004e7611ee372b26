// WPD convolutional beamformer (weighted power minimisation distortionless response; Nakatani &
// Kinoshita 2019, Boeddeker et al. 2020) in its factorised form: per iteration
//   p_t = m_t mean_d |Y[t,d]|^2  (first iteration)  or  |xhat_t|^2  (later ones)
//   a_t = g_t / max(p_t, floor * max_{g_t = 1} p_t),  all 0 where that maximum is 0
//   one WPE step with the weights a (wpe_run with the caller's weights): Y -> Z
//   gss_mvdr_souden on Z with target mask m g and "distortion mask" a: Z -> xhat
// include/gss_hip.h (gss_wpd_souden) has the definition.  New here: the weights kernel and the
// composition; correlation, solve, filter application, PSD pass and Souden solve are the WPE's
// and the MVDR's own launches.
#include <algorithm>

#include "gss_internal.h"

namespace {

// One workgroup per frequency, like wpe_power_kernel: the maximum over the frames comes before
// the inversion.  FROM_XHAT = false: p_t = mask[f,t] * mean_d |Y[f,t,d]|^2, Y read once, 256
// frames at a time with coalesced loads through LDS; true: p_t = |xhat[t,f]|^2, which
// wpd_power_transpose_kernel has put into the output row already (xhat is (T,F): a workgroup that
// walks one frequency would pull a cache line per element).  The powers are
// parked in the output row, which every thread reads back at the frames it wrote itself.  The
// gated maximum is a butterfly over the lanes and a fixed-order max over the four waves: no
// atomics, the same call gives the same bits.  mxg (may be NULL) receives mask * gate.
constexpr int WPD_FRAMES = 256;
template <bool FROM_XHAT>
__global__ __launch_bounds__(WPD_FRAMES) void wpd_weights_kernel(
    const cplx *__restrict__ Y, const double *__restrict__ mask,
    const uint8_t *__restrict__ gate, int F, int64_t T, int D, double power_floor,
    double *__restrict__ a, double *__restrict__ mxg) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *ps = reinterpret_cast<double *>(smem);      // WPD_FRAMES * (D + 1), unused FROM_XHAT
    __shared__ double red[WPD_FRAMES / 64];
    const int f = blockIdx.x, tid = threadIdx.x;
    double *af = a + (int64_t)f * T;
    double mx = 0.0;
    if (FROM_XHAT) {
        for (int64_t t = tid; t < T; t += WPD_FRAMES) {
            if (!gate || gate[t]) mx = fmax(mx, af[t]);
        }
    } else {
        const cplx *Yf = Y + (int64_t)f * T * D;
        const double *mf = mask + (int64_t)f * T;
        const int DP = D + 1;
        for (int64_t t0 = 0; t0 < T; t0 += WPD_FRAMES) {
            const int nfr = (int)min((int64_t)WPD_FRAMES, T - t0);
            const int total = nfr * D;
            const cplx *src = Yf + t0 * D;
            __syncthreads();
            {
                // (frame, channel) of element idx advanced without dividing, eight loads in
                // flight per thread: wpe_power_kernel's staging
                constexpr int LB = 8;
                const int qf = WPD_FRAMES / D, rf = WPD_FRAMES - qf * D;
                int fr = tid / D, d = tid - fr * D;
                for (int base = tid; base < total; base += LB * WPD_FRAMES) {
                    cplx v[LB];
#pragma unroll
                    for (int j = 0; j < LB; ++j) {
                        const int idx = base + j * WPD_FRAMES;
                        v[j] = idx < total ? src[idx] : c_make(0.0, 0.0);
                    }
#pragma unroll
                    for (int j = 0; j < LB; ++j) {
                        if (base + j * WPD_FRAMES < total) ps[fr * DP + d] = c_abs2(v[j]);
                        fr += qf;
                        d += rf;
                        if (d >= D) {
                            d -= D;
                            ++fr;
                        }
                    }
                }
            }
            __syncthreads();
            if (tid < nfr) {
                const int64_t t = t0 + tid;
                double p = 0.0;
                for (int d = 0; d < D; ++d) p += ps[tid * DP + d];
                const double m = mf[t];
                p = m * (p / (double)D);
                af[t] = p;
                const bool g = !gate || gate[t];
                if (g) mx = fmax(mx, p);
                if (mxg) mxg[(int64_t)f * T + t] = g ? m : 0.0;
            }
        }
    }
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    const double lo = power_floor * mx;
    for (int64_t t = tid; t < T; t += WPD_FRAMES) {
        const bool g = !gate || gate[t];
        af[t] = (g && mx > 0.0) ? 1.0 / fmax(af[t], lo) : 0.0;
    }
}

// |xhat (T,F)|^2 -> p (F,T): 32 x 32 tiles through LDS, reads coalesced along f, writes along t.
constexpr int WPD_TILE = 32;
__global__ __launch_bounds__(WPD_TILE * 8) void wpd_power_transpose_kernel(
    const cplx *__restrict__ xhat, int F, int64_t T, double *__restrict__ p) {
    __shared__ double tile[WPD_TILE][WPD_TILE + 1];
    const int64_t t0 = (int64_t)blockIdx.x * WPD_TILE;
    const int f0 = blockIdx.y * WPD_TILE;
    const int x = threadIdx.x & (WPD_TILE - 1), y = threadIdx.x / WPD_TILE;      // y in [0, 8)
    for (int j = y; j < WPD_TILE; j += 8) {
        const int64_t t = t0 + j;
        const int f = f0 + x;
        if (t < T && f < F) tile[j][x] = c_abs2(xhat[t * F + f]);
    }
    __syncthreads();
    for (int j = y; j < WPD_TILE; j += 8) {
        const int f = f0 + j;
        const int64_t t = t0 + x;
        if (t < T && f < F) p[(int64_t)f * T + t] = tile[x][j];
    }
}

// The frame gate of the fused pipeline: 0 on the context frames that bf_drop_context zeroes
// (masks[:, :start] = 0; if end > 0: masks[:, -end:] = 0), else 1.
__global__ __launch_bounds__(256) void wpd_context_gate_kernel(int64_t T, int64_t start_frames,
                                                               int64_t end_frames,
                                                               uint8_t *__restrict__ gate) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < T) gate[t] = (t < start_frames || (end_frames > 0 && t >= T - end_frames)) ? 0 : 1;
}

}  // namespace

int wpd_weights_run(gss_ctx *ctx, const cplx *Y, const double *mask, const cplx *xhat,
                    const uint8_t *gate, int F, int64_t T, int D, double power_floor, double *a,
                    double *mxg) {
    GSS_PROF(ctx, "wpd_weights");
    if (xhat) {
        hipLaunchKernelGGL(wpd_power_transpose_kernel,
                           dim3((unsigned)((T + WPD_TILE - 1) / WPD_TILE), (F + WPD_TILE - 1) / WPD_TILE),
                           dim3(WPD_TILE * 8), 0, ctx->stream, xhat, F, T, a);
        GSS_LAUNCH_CHECK(ctx, "wpd_power_transpose_kernel");
        hipLaunchKernelGGL(wpd_weights_kernel<true>, dim3(F), dim3(WPD_FRAMES), 0, ctx->stream,
                           (const cplx *)nullptr, (const double *)nullptr, gate, F, T, D,
                           power_floor, a, (double *)nullptr);
    } else {
        // (D < 30, checked by the entry points: 256 * 30 doubles, below the 64 KB that need no
        // attribute)
        const size_t lds = sizeof(double) * WPD_FRAMES * (size_t)(D + 1);
        hipLaunchKernelGGL(wpd_weights_kernel<false>, dim3(F), dim3(WPD_FRAMES), lds, ctx->stream,
                           Y, mask, gate, F, T, D, power_floor, a, mxg);
    }
    GSS_LAUNCH_CHECK(ctx, "wpd_weights_kernel");
    return GSS_OK;
}

int wpd_context_gate_run(gss_ctx *ctx, int64_t T, int64_t start_frames, int64_t end_frames,
                         uint8_t *gate) {
    hipLaunchKernelGGL(wpd_context_gate_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0,
                       ctx->stream, T, start_frames, end_frames, gate);
    GSS_LAUNCH_CHECK(ctx, "wpd_context_gate_kernel");
    return GSS_OK;
}

// the blocks that live through the iterations; the WPE and the MVDR run above them
struct WpdWork {
    double *a, *mxg;    // (F,T) weights of the iteration, mask * gate
    cplx *Z;            // (F,T,D) dereverberated observation
};
static WpdWork wpd_blocks(Workspace &ws, int F, int64_t T, int D) {
    WpdWork k;
    k.a = ws.take<double>((size_t)F * T, "wpd a");
    k.mxg = ws.take<double>((size_t)F * T, "wpd mask gate");
    k.Z = ws.take<cplx>((size_t)F * T * D, "wpd Z");
    return k;
}

size_t wpd_workspace_bytes(int F, int64_t T, int D, int taps, int delay) {
    Workspace ws;
    wpd_blocks(ws, F, T, D);
    return ws.bytes + 4096 +
           std::max(wpe_workspace_bytes(F, T, D, taps, delay), mvdr_workspace_bytes(F, T, D));
}

int wpd_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D, const double *mask,
            const uint8_t *gate, const gss_bf_wpd &bf, int forced_ref, cplx *Xhat,
            int32_t *ref_channel) {
    Workspace ws(ctx);
    const WpdWork k = wpd_blocks(ws, F, T, D);
    GSS_TRY(ws.status("wpd"));
    const size_t mark = ctx->arena_off;
    for (int it = 0; it < bf.iterations; ++it) {
        if (it == 0)
            GSS_TRY(wpd_weights_run(ctx, Y, mask, nullptr, gate, F, T, D, bf.power_floor, k.a, k.mxg));
        else
            GSS_TRY(wpd_weights_run(ctx, nullptr, nullptr, Xhat, gate, F, T, D, bf.power_floor, k.a,
                                    nullptr));
        const WpeCallerWeights cw{k.a, GSS_STATUS_WPD_ZERO_PIVOTS, it > 0};
        GSS_TRY(wpe_run(ctx, Y, F, T, D, bf.taps, bf.delay, 1, 0, k.Z, -1, 0, &cw));
        GSS_TRY(arena_release(ctx, mark));
        // (the reference channel is chosen anew in every iteration; the last one's stays)
        GSS_TRY(mvdr_run(ctx, k.Z, F, T, D, k.mxg, k.a, bf.ban, Xhat, ref_channel, /*gev=*/0,
                         forced_ref));
        GSS_TRY(arena_release(ctx, mark));
    }
    return GSS_OK;
}
