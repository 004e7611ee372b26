// The two ends of a sample-block stream (include/gss_hip.h: gss_stft_stream, gss_istft_stream).
//
// A stream is the offline path with stft_fading = 1, cut at arbitrary sample positions.  With
// W = size, H = shift: before the first sample the history is W - H zeros (the leading fading
// pad), frame t covers the stream samples [t H - (W - H), t H + H), and after M samples
// floor(M / H) frames exist.  The analysis side carries the last W samples (and activity bytes)
// so that a frame which straddles a block border sees what the previous block left; the synthesis
// side carries the W - H partial overlap-add sums that the next frames complete.
//
// The transforms are the existing ones: the analysis lays [history | block] out as an unpadded
// signal whose frames are exactly the block's and hands it to stft_run / activity_run (the bits of
// gss_stft on the whole signal: same kernel, same channel pairing, same products); the synthesis
// takes istft_single_frames_run's frames, each transformed on its own, so that the samples do not
// depend on where the blocks were cut.
#include "gss_internal.h"

namespace {

constexpr int STAGE_THREADS = 256;
constexpr int HIST_PER_THREAD = GSS_MAX_STFT_SIZE / STAGE_THREADS;

// Sample g of the stream (g >= M - W; M samples before this block, which holds [M, M + n)):
// from the history (the samples [M - W, M), oldest first) or from the block.
template <typename TIn>
__device__ __forceinline__ double stream_sample(const double *hist, const TIn *blk, double in_scale,
                                                int64_t g, int64_t M, int W) {
    return g < M ? hist[g - (M - W)] : (double)blk[g - M] * in_scale;
}
__device__ __forceinline__ uint8_t stream_byte(const uint8_t *hist, const uint8_t *blk, int64_t g,
                                               int64_t M, int W) {
    return g < M ? hist[g - (M - W)] : (uint8_t)(blk[g - M] != 0);
}

// [history | block] of the block's frames as an unpadded signal: row r of xs (D, L) / as (K, L)
// holds the stream samples [s0, s0 + L).  grid (ceil(L / 256), D + K): rows >= D are the activity.
template <typename TIn>
__global__ __launch_bounds__(STAGE_THREADS) void stream_stage_kernel(
    const TIn *__restrict__ x, double in_scale, const uint8_t *__restrict__ act, int D, int64_t n,
    int64_t M, int64_t s0, int64_t L, int W, const double *__restrict__ x_hist,
    const uint8_t *__restrict__ act_hist, double *__restrict__ xs, uint8_t *__restrict__ as) {
    const int64_t i = (int64_t)blockIdx.x * STAGE_THREADS + threadIdx.x;
    if (i >= L) return;
    const int r = blockIdx.y;
    if (r < D)
        xs[(int64_t)r * L + i] = stream_sample(x_hist + (int64_t)r * W, x + (int64_t)r * n, in_scale,
                                               s0 + i, M, W);
    else
        as[(int64_t)(r - D) * L + i] = stream_byte(act_hist + (int64_t)(r - D) * W,
                                                   act + (int64_t)(r - D) * n, s0 + i, M, W);
}

// The history after the block: the stream samples [M + n - W, M + n).  One workgroup per row
// reads all W values into registers before any of them is written (n < W moves part of the old
// history down inside its own buffer).  grid (D + K).
template <typename TIn>
__global__ __launch_bounds__(STAGE_THREADS) void stream_history_kernel(
    const TIn *__restrict__ x, double in_scale, const uint8_t *__restrict__ act, int D, int64_t n,
    int64_t M, int W, double *x_hist, uint8_t *act_hist) {
    const int r = blockIdx.x;
    const int64_t g0 = M + n - W;
    if (r < D) {
        double *h = x_hist + (int64_t)r * W;
        double v[HIST_PER_THREAD];
#pragma unroll
        for (int j = 0; j < HIST_PER_THREAD; ++j) {
            const int i = threadIdx.x + j * STAGE_THREADS;
            v[j] = i < W ? stream_sample(h, x + (int64_t)r * n, in_scale, g0 + i, M, W) : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < HIST_PER_THREAD; ++j) {
            const int i = threadIdx.x + j * STAGE_THREADS;
            if (i < W) h[i] = v[j];
        }
    } else {
        uint8_t *h = act_hist + (int64_t)(r - D) * W;
        uint8_t v[HIST_PER_THREAD];
#pragma unroll
        for (int j = 0; j < HIST_PER_THREAD; ++j) {
            const int i = threadIdx.x + j * STAGE_THREADS;
            v[j] = i < W ? stream_byte(h, act + (int64_t)(r - D) * n, g0 + i, M, W) : (uint8_t)0;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < HIST_PER_THREAD; ++j) {
            const int i = threadIdx.x + j * STAGE_THREADS;
            if (i < W) h[i] = v[j];
        }
    }
}

// Overlap-add of the frames [t0, t0 + Tn) onto the carried tail.  Thread q takes the padded
// position p = t0 H + q, q < Tn H + (W - H): the sum starts from the tail (the partial sum of the
// frames before t0, itself started from 0.0) and takes the new frames in ascending t, as
// istft_ola_kernel does over all frames.  q < Tn H: no later frame reaches p, the sample is
// finished and goes out unless it lies in the leading fading pad (p < W - H); the others are the
// new tail, written to tail_new (tail is read by other threads).
__device__ __forceinline__ void stream_ola_sample(
    const double *__restrict__ frm, int64_t t0, int64_t Tn, int size, int shift,
    const double *__restrict__ tail, double *__restrict__ tail_new, int64_t first_out,
    double *__restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int pad = size - shift;
    if (q >= Tn * shift + pad) return;
    const int64_t p = t0 * shift + q;
    int64_t t_lo = p - size + 1;
    t_lo = t_lo <= 0 ? 0 : (t_lo + shift - 1) / shift;
    if (t_lo < t0) t_lo = t0;
    int64_t t_hi = p / shift;
    if (t_hi > t0 + Tn - 1) t_hi = t0 + Tn - 1;
    double acc = q < pad ? tail[q] : 0.0;
    for (int64_t t = t_lo; t <= t_hi; ++t) acc += frm[(t - t0) * size + (p - t * shift)];
    if (q >= Tn * shift)
        tail_new[q - Tn * shift] = acc;
    else if (p >= pad)
        out[p - pad - first_out] = acc;
}

// grid.y = s, one of S signals: frm (S,Tn,size), tail / tail_new (S, size - shift), out (S, m).
// Every signal is summed on its own rows, whatever S.
__global__ __launch_bounds__(256) void stream_ola_targets_kernel(
    const double *__restrict__ frm, int64_t t0, int64_t Tn, int size, int shift,
    const double *__restrict__ tail, double *__restrict__ tail_new, int64_t first_out, int64_t m,
    double *__restrict__ out) {
    const int64_t s = blockIdx.y;
    const int pad = size - shift;
    stream_ola_sample(frm + s * Tn * size, t0, Tn, size, shift, tail + s * pad, tail_new + s * pad,
                      first_out, out + s * m);
}

struct StreamStftWork {
    double *xs;     // (D, L)
    uint8_t *as;    // (K, L), NULL without an activity
};
// the blocks of the analysis side: the staged signal of Tn frames, L = (Tn - 1) H + W samples
StreamStftWork stream_stft_blocks(Workspace &ws, int64_t Tn, int D, int K, int size, int shift) {
    const size_t L = (size_t)(Tn - 1) * shift + size;
    StreamStftWork k;
    k.xs = ws.take<double>((size_t)D * L, "stream staged samples");
    k.as = K > 0 ? ws.take<uint8_t>((size_t)K * L, "stream staged activity") : nullptr;
    return k;
}

struct StreamIstftWork {
    double *frm;        // (S Tn, size)
    double *tail_new;   // (S, size - shift)
};
StreamIstftWork stream_istft_blocks(Workspace &ws, int64_t Tn, int size, int shift, int S) {
    StreamIstftWork k;
    k.frm = ws.take<double>((size_t)S * Tn * size, "stream istft frames");
    k.tail_new = ws.take<double>((size_t)S * (size - shift), "stream new tail");
    return k;
}

}  // namespace

size_t stream_stft_workspace_bytes(int64_t Tn, int D, int K, int size, int shift) {
    Workspace ws;
    if (Tn > 0) stream_stft_blocks(ws, Tn, D, K, size, shift);
    return ws.bytes + 4096;
}

size_t stream_istft_targets_workspace_bytes(int64_t Tn, int S, int size, int shift) {
    Workspace ws;
    if (Tn > 0) stream_istft_blocks(ws, Tn, size, shift, S);
    return ws.bytes + 4096;
}

extern "C" int64_t gss_stream_num_frames(int64_t received, int64_t n, int size, int shift) {
    return (received + n) / shift - received / shift;
}

static int64_t stream_emitted(int64_t frames, int size, int shift) {
    const int64_t m = frames * shift - (size - shift);
    return m > 0 ? m : 0;
}

extern "C" int64_t gss_stream_num_samples_out(int64_t received, int64_t n, int size, int shift) {
    return stream_emitted((received + n) / shift, size, shift) -
           stream_emitted(received / shift, size, shift);
}

extern "C" int64_t gss_stream_flush_samples(int64_t received, int size, int shift) {
    return gss_stft_num_frames(received, size, shift, 1) * shift - received;
}

int stream_init_run(gss_ctx *ctx, gss_stream_state *st) {
    const size_t W = (size_t)st->size;
    GSS_HIP_CHECK(ctx, hipMemsetAsync(st->x_hist, 0, sizeof(double) * st->D * W, ctx->stream));
    if (st->act_hist) GSS_HIP_CHECK(ctx, hipMemsetAsync(st->act_hist, 0, st->K * W, ctx->stream));
    GSS_HIP_CHECK(ctx, hipMemsetAsync(st->ola_tail, 0, sizeof(double) * (st->size - st->shift),
                                      ctx->stream));
    st->received = 0;
    st->frames_out = 0;
    return GSS_OK;
}

template <typename TIn>
static int stream_stage_launch(gss_ctx *ctx, const TIn *x, double in_scale, const uint8_t *act,
                               int64_t n, int64_t Tn, const gss_stream_state *st,
                               const StreamStftWork &k) {
    const int W = st->size, H = st->shift, D = st->D, K = act ? st->K : 0;
    const int64_t M = st->received;
    if (Tn > 0) {
        const int64_t s0 = M / H * H - (W - H), L = (Tn - 1) * H + W;
        hipLaunchKernelGGL((stream_stage_kernel<TIn>),
                           dim3((unsigned)((L + STAGE_THREADS - 1) / STAGE_THREADS), D + K),
                           dim3(STAGE_THREADS), 0, ctx->stream, x, in_scale, act, D, n, M, s0, L, W,
                           st->x_hist, st->act_hist, k.xs, k.as);
        GSS_LAUNCH_CHECK(ctx, "stream_stage_kernel");
    }
    hipLaunchKernelGGL((stream_history_kernel<TIn>), dim3(D + K), dim3(STAGE_THREADS), 0, ctx->stream,
                       x, in_scale, act, D, n, M, W, st->x_hist, st->act_hist);
    GSS_LAUNCH_CHECK(ctx, "stream_history_kernel");
    return GSS_OK;
}

int stream_stft_run(gss_ctx *ctx, const void *x, int in_type, const uint8_t *act, int64_t n,
                    gss_stream_state *st, cplx *Y, uint8_t *actf) {
    const int W = st->size, H = st->shift, D = st->D, K = act ? st->K : 0;
    const int64_t Tn = gss_stream_num_frames(st->received, n, W, H);
    Workspace ws(ctx);
    StreamStftWork k{nullptr, nullptr};
    if (Tn > 0) k = stream_stft_blocks(ws, Tn, D, K, W, H);
    GSS_TRY(ws.status("gss_stft_stream"));
    {
        GSS_PROF(ctx, "stream_stage");
        // int16 PCM times 2^-15 is exact: the history holds the float64 stream of the same values
        if (in_type == 0)
            GSS_TRY(stream_stage_launch(ctx, static_cast<const double *>(x), 1.0, act, n, Tn, st, k));
        else
            GSS_TRY(stream_stage_launch(ctx, static_cast<const int16_t *>(x), 1.0 / 32768.0, act, n,
                                        Tn, st, k));
    }
    st->received += n;
    if (Tn == 0) return GSS_OK;
    // an unpadded signal of L = (Tn - 1) H + W samples has exactly Tn frames
    const int64_t L = (Tn - 1) * H + W;
    GSS_TRY(stft_run(ctx, k.xs, 0, D, L, /*fading=*/0, Y));
    if (act) GSS_TRY(activity_run(ctx, k.as, K, L, /*fading=*/0, actf));
    return GSS_OK;
}

// The S Tn frames go through istft_single_frames_run as one batch (every frame on its own: frame
// (s, t) has the bits it has in a call of signal s alone), then one overlap-add launch.  The one
// synthesis: a one-signal stream is S = 1 with tails = st->ola_tail.
int stream_istft_targets_run(gss_ctx *ctx, const cplx *X, int64_t Tn, int S, gss_stream_state *st,
                             double *tails, double *out) {
    const int W = st->size, H = st->shift;
    const int64_t t0 = st->frames_out;
    Workspace ws(ctx);
    const StreamIstftWork k = stream_istft_blocks(ws, Tn, W, H, S);
    GSS_TRY(ws.status("gss_istft_stream_targets"));
    GSS_TRY(istft_single_frames_run(ctx, X, (int64_t)S * Tn, k.frm));
    {
        GSS_PROF(ctx, "stream_ola_targets");
        const int64_t total = Tn * H + (W - H);
        const int64_t first = stream_emitted(t0, W, H), m = stream_emitted(t0 + Tn, W, H) - first;
        hipLaunchKernelGGL(stream_ola_targets_kernel, dim3((unsigned)((total + 255) / 256), S),
                           dim3(256), 0, ctx->stream, k.frm, t0, Tn, W, H, tails, k.tail_new, first,
                           m, out);
        GSS_LAUNCH_CHECK(ctx, "stream_ola_targets_kernel");
    }
    GSS_HIP_CHECK(ctx, hipMemcpyAsync(tails, k.tail_new, sizeof(double) * S * (W - H),
                                      hipMemcpyDeviceToDevice, ctx->stream));
    st->frames_out = t0 + Tn;
    return GSS_OK;
}
