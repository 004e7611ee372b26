// Internal declarations shared by the HIP translation units of libgss_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../include/gss_hip.h"

typedef double2 cplx;  // .x = re, .y = im; bit-compatible with gss_cplx

// Kernel-variant switches for tests and A/B runs: ONE environment variable,
//     GSS_VARIANT="key=value,key,..."          (a bare key means 1)
// parsed when its text changes (tests flip it between calls), read through gss_variant().
// The keys that exist are listed in INTEGRATION.md; an unknown key is an error at the first
// library call that looks at the string (a typo must not silently run the default).
int gss_variant(const char *key, int dflt);
inline bool gss_variant_set(const char *key) { return gss_variant(key, 0) != 0; }

// Experiment builds (tools/build_variant.sh: trace instrumentation, other compile-time
// constants) must say so: none of these may leak into the library the package ships.
#if (defined(GSS_CORR_TRACE) || defined(GSS_WCOV_TRACE) || defined(GSS_EM4_TRACE) || \
     defined(GSS_CHOL_TRACE)) && !defined(GSS_EXPERIMENT_BUILD)
#error "trace instrumentation needs -DGSS_EXPERIMENT_BUILD=1 (tools/build_variant.sh)"
#endif

#define GSS_TINY 2.2250738585072014e-308  // np.finfo(np.float64).tiny

// ---------------------------------------------------------------- device math
__device__ __forceinline__ cplx c_make(double r, double i) { return make_double2(r, i); }
__device__ __forceinline__ cplx c_add(cplx a, cplx b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ cplx c_sub(cplx a, cplx b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ cplx c_mul(cplx a, cplx b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
// a * conj(b)
__device__ __forceinline__ cplx c_mulc(cplx a, cplx b) {
    return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}
// conj(a) * b
__device__ __forceinline__ cplx c_cmul(cplx a, cplx b) {
    return make_double2(a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x);
}
__device__ __forceinline__ cplx c_scale(cplx a, double s) { return make_double2(a.x * s, a.y * s); }
__device__ __forceinline__ cplx c_conj(cplx a) { return make_double2(a.x, -a.y); }
__device__ __forceinline__ double c_abs2(cplx a) { return a.x * a.x + a.y * a.y; }
// acc += a * b
__device__ __forceinline__ void c_fma(cplx &acc, cplx a, cplx b) {
    acc.x = fma(a.x, b.x, acc.x);
    acc.x = fma(-a.y, b.y, acc.x);
    acc.y = fma(a.x, b.y, acc.y);
    acc.y = fma(a.y, b.x, acc.y);
}
// acc += a * conj(b)
__device__ __forceinline__ void c_fmac(cplx &acc, cplx a, cplx b) {
    acc.x = fma(a.x, b.x, acc.x);
    acc.x = fma(a.y, b.y, acc.x);
    acc.y = fma(a.y, b.x, acc.y);
    acc.y = fma(-a.x, b.y, acc.y);
}
// acc += conj(a) * b
__device__ __forceinline__ void c_cfma(cplx &acc, cplx a, cplx b) {
    acc.x = fma(a.x, b.x, acc.x);
    acc.x = fma(a.y, b.y, acc.x);
    acc.y = fma(a.x, b.y, acc.y);
    acc.y = fma(-a.y, b.x, acc.y);
}
// a conj(b) with every product rounded on its own: c_outer(b, a) is its exact conjugate, and
// c_outer(a, a) is exactly real (the Hermitian running sums of the online WPE and MVDR).
__device__ __forceinline__ cplx c_outer(cplx a, cplx b) {
#pragma clang fp contract(off)
    const double xx = a.x * b.x, yy = a.y * b.y, yx = a.y * b.x, xy = a.x * b.y;
    return c_make(xx + yy, yx - xy);
}

// Barrier for code that is run by ONE wavefront on data in LDS (the lanes of a wave issue
// their LDS operations in order, so only the compiler has to be kept from reordering).
// In a 64-thread workgroup it is equivalent to __syncthreads(); inside a larger
// workgroup it lets single waves work independently.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Sum over the 64 lanes (all active) on the DPP network (row shifts, then row broadcasts; the
// classic GCN reduction) instead of six ds_bpermute round trips per value: 7 VALU steps, no
// LDS crossbar.  The total forms in lane 63 and is handed to every lane through an SGPR.
// It matters where many values are reduced back to back (register-form M-step: 80 sums per
// wave, a third of the kernel with the butterfly).
template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ __forceinline__ double dpp_shifted(double v) {
    const unsigned long long u = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, ROW_MASK, BANK_MASK, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, ROW_MASK, BANK_MASK, true);
    return __longlong_as_double(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
// lane k's value (k wave uniform), handed to all lanes through an SGPR pair
__device__ __forceinline__ double lane_bcast(double x, int k) {
    const unsigned long long u = __double_as_longlong(x);
    const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)u, k);
    const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)(u >> 32), k);
    return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double wave_sum(double v) {
    double s = v + dpp_shifted<0x111, 0xf, 0xf>(v);      // row_shr:1
    s += dpp_shifted<0x112, 0xf, 0xf>(v);                // row_shr:2
    s += dpp_shifted<0x113, 0xf, 0xf>(v);                // row_shr:3
    s += dpp_shifted<0x114, 0xf, 0xe>(s);                // row_shr:4, banks 1-3
    s += dpp_shifted<0x118, 0xf, 0xc>(s);                // row_shr:8, banks 2-3
    s += dpp_shifted<0x142, 0xa, 0xf>(s);                // row_bcast:15 into rows 1, 3
    s += dpp_shifted<0x143, 0xc, 0xf>(s);                // row_bcast:31 into rows 2, 3
    return lane_bcast(s, 63);
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// XCD-aware block mapping for kernels that launch `nsub` workgroups per frequency:
// the dispatcher is observed to place block b on XCD b % 8 (each XCD has its own
// L2), so the nsub workgroups of one frequency are given linear ids that are equal
// mod 8 and share that frequency's slab through one L2.  1-D grid of
// xcd_grid(nsub, F) blocks; returns false for the padding blocks.  Placement only
// affects speed, never results.
__device__ __forceinline__ bool xcd_group_map(int nsub, int F, int &f, int &sub) {
    const int L = blockIdx.x;
    const int sg = L / (8 * nsub), rem = L - sg * 8 * nsub;
    sub = rem >> 3;
    f = sg * 8 + (rem & 7);
    return f < F;
}
static inline unsigned xcd_grid(int nsub, int F) { return (unsigned)(nsub * ((F + 7) / 8 * 8)); }

// Upper-triangular packed index of (d1 <= d2) in a D x D Hermitian matrix.
__host__ __device__ __forceinline__ int tri_index(int d1, int d2, int D) {
    return d1 * D - (d1 * (d1 - 1)) / 2 + (d2 - d1);
}
__host__ __device__ __forceinline__ int tri_count(int D) { return D * (D + 1) / 2; }
// Its inverse: packed index e -> (d1 <= d2).
__device__ __forceinline__ void tri_unpack(int e, int D, int &d1, int &d2) {
    int rem = e;
    d1 = 0;
    while (rem >= D - d1) {
        rem -= D - d1;
        ++d1;
    }
    d2 = d1 + rem;
}

// ---------------------------------------------------------------- context
struct ProfEntry {
    std::string name;
    hipEvent_t start, stop;
};

struct gss_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // second stream of the frequency-blocked EM (cacgmm_run: two blocks of frequencies in
    // flight), forked from / joined to `stream` by events; created on first use
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int utterances_in_flight = 0;   // gss_set_utterances_in_flight(): exactly 1 = a call may use aux_stream
    std::string error;

    // bump arena for intermediates of one top-level call
    char *arena = nullptr;
    size_t arena_size = 0;
    size_t arena_off = 0;
    size_t arena_peak = 0;

    // Workspace debug mode (gss_debug_workspace; tests only, synchronises).  Off (-1): none of
    // the fields below is read.  On: arena and gss_dev_malloc blocks are filled with the byte
    // `debug_pattern` before use, and every arena block is followed by a guard of that byte
    // which release / reserve / report compare with the pattern.  arena_off and arena_peak stay
    // the LOGICAL offsets of the plain arena (what gss_workspace_bytes reports and the
    // *_workspace_bytes formulas bound); the blocks themselves sit at debug_phys, which also
    // counts the guards, inside the headroom arena_reserve adds for them.
    struct DebugGuard {
        int block;                      // index of the block since the last reserve
        size_t logical_off, bytes;      // the block as the plain arena would place it
        size_t guard_off, guard_bytes;  // physical: alignment slack + 256 bytes behind the block
        const char *tag;                // the name Workspace::take gave it, a string literal
        bool reported;                  // a violated guard counts once
    };
    int debug_pattern = -1;
    size_t debug_phys = 0;
    size_t debug_logical_size = 0;      // what the last reserve asked for, without the headroom
    int debug_blocks = 0;
    std::vector<DebugGuard> debug_guards;
    int64_t debug_violations = 0;
    std::string debug_first;            // text naming the first violation

    // STFT tables
    int stft_size = 0, stft_shift = 0;
    double *win_analysis = nullptr;   // device, stft_size
    double *win_synthesis = nullptr;  // device, stft_size
    cplx *twiddle = nullptr;          // device, stft_size/2: exp(-2 pi i j / size)

    // Status words (mapped host memory).  [0]: the last beamformed utterance, written by
    // mvdr_apply_kernel: the reference channel, -1 = non-finite SNR; INT32_MIN = none yet.
    // [2]: pivots zeroed by the last WPE call (copied from the device counter by wpe_run).
    // [3]: (segment, frequency) pairs of the last segment-wise MVDR that fell back to the
    // whole-window statistics (copied from the device counter by mvdr_apply_kernel).
    // [4]: the interferer class of the last LCMV mask call (masks3_kernel), -1 = none.
    // [5]: frequencies of the last LCMV beamformer that fell back to the MVDR of the merged mask
    // (copied from the device counter by lcmv_run).
    // [6]: pivots zeroed by the WPE steps of the last WPD call (wpe_run with the caller's weights).
    // [7]: frequencies whose row the last gss_cacgmm_align left off the identity (align_moved_kernel).
    // [8]: (frequency, frame) pairs of the last online MVDR call whose Phi_N had no Cholesky factor
    // (copied from the device counter by mvdr_online_run).
    // [9]: (frequency, frame, class) triples of the last online CACGMM call whose S_k had no Cholesky
    // factor (copied from the device counter by cacgmm_online_run; cacgmm_online_to_model_run counts
    // its identity classes there).  [10]: classes whose precision had none in the last
    // cacgmm_online_from_model_run.
    // [GSS_STATUS_TARGETS + s]: target s of the last targets call (mvdr_apply_targets_kernel,
    // which writes target 0's word to [0] as well).
    int32_t *status_host = nullptr;
    int32_t *status_dev = nullptr;
    int last_targets = 0;   // S of the last beamformer run when it was a targets call, else 0
    // [GSS_STATUS_MVDR_ONLINE_TARGETS + s]: fallback frames of target s of the last online MVDR
    // targets call (mvdr_online_targets_run, which leaves their sum in [8])
    int last_online_targets = 0;   // S of that call, 0 = none yet
    // [GSS_STATUS_CHANNELS + j]: the j-th channel (ascending) the last channel selection kept,
    // written by chsel_pick_kernel
    int last_selected = 0;  // n of the last channel selection on this context, 0 = none yet

    // WPE tile lists (device), rebuilt when (taps, delay, D) changes
    void *wpe_tiles = nullptr;
    int wpe_tiles_key[4] = {-1, -1, -1, -1};   // taps, delay, D, correlation tile size

    // profiling
    bool profiling = false;
    std::vector<ProfEntry> prof_pending;
    std::vector<hipEvent_t> event_pool;
    std::map<std::string, std::pair<long, double>> prof_acc;
    std::string prof_filter;   // time only this kernel (empty: all)
};

#define GSS_STATUS_SEGMENT_FALLBACKS 3                           // see gss_ctx::status_host
#define GSS_STATUS_LCMV_INTERFERER 4
#define GSS_STATUS_LCMV_FALLBACKS 5
#define GSS_STATUS_WPD_ZERO_PIVOTS 6                             // pivots zeroed by the last WPD call
#define GSS_STATUS_ALIGN_MOVED 7                                 // rows the last alignment left off the identity
#define GSS_STATUS_MVDR_ONLINE_FALLBACKS 8                        // fallback frames of the last online MVDR call
#define GSS_STATUS_CACGMM_ONLINE_FALLBACKS 9                      // fallback (frequency, frame, class) triples of the last online CACGMM call
#define GSS_STATUS_CACGMM_ONLINE_BAD_MODEL 10                     // classes of the last model -> state conversion without a Cholesky factor
#define GSS_STATUS_TARGETS 16                                   // first per-target word
#define GSS_STATUS_CHANNELS 40                                   // first selected-channel word
#define GSS_STATUS_MVDR_ONLINE_TARGETS (GSS_STATUS_CHANNELS + GSS_MAX_CHANNELS)   // fallback frames per target of the last online MVDR targets call
#define GSS_STATUS_BYTES (4 * (GSS_STATUS_MVDR_ONLINE_TARGETS + GSS_CACGMM_ONLINE_MAX_CLASSES))
static_assert(GSS_STATUS_TARGETS + GSS_MAX_CLASSES + 1 <= GSS_STATUS_CHANNELS, "status words overlap");

int gss_fail(gss_ctx *ctx, int code, const char *fmt, ...);

#define GSS_HIP_CHECK(ctx, expr)                                                   \
    do {                                                                           \
        hipError_t _e = (expr);                                                    \
        if (_e != hipSuccess)                                                      \
            return gss_fail((ctx), GSS_ERR_HIP, "%s failed: %s (%s:%d)", #expr,    \
                            hipGetErrorString(_e), __FILE__, __LINE__);            \
    } while (0)

#define GSS_REQUIRE(ctx, cond, code, ...)                      \
    do {                                                       \
        if (!(cond)) return gss_fail((ctx), (code), __VA_ARGS__); \
    } while (0)

#define GSS_TRY(expr)              \
    do {                           \
        int _s = (expr);           \
        if (_s != GSS_OK) return _s; \
    } while (0)

// Arena: reserve() makes sure `bytes` are available for the coming top-level call
// (may synchronise + reallocate); alloc() bumps.  reset() starts a new call.
// release() rewinds to a mark taken from ctx->arena_off: everything allocated after the mark is
// given back (the stages of a fused call work in each other's bytes).  Nothing that lived before
// a reserve() survives it, nothing above a mark survives its release().
int arena_reserve(gss_ctx *ctx, size_t bytes);
void arena_reset(gss_ctx *ctx);
void *arena_alloc(gss_ctx *ctx, size_t bytes, const char *tag);   // through a Workspace only
int arena_release_debug(gss_ctx *ctx, size_t mark);
static inline int arena_release(gss_ctx *ctx, size_t mark) {
    if (ctx->debug_pattern >= 0) return arena_release_debug(ctx, mark);
    ctx->arena_off = mark;
    return GSS_OK;
}
static inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// The blocks of a stage, written once: a stage's list function take()s them from a Workspace,
// and the same list serves the run (Workspace(ctx): every take is an arena_alloc, in order) and
// the stage's *_workspace_bytes() (Workspace(): take returns NULL and adds the block's aligned
// size to `bytes`).  The measured sum bounds what the list bumps the arena by at whatever offset
// the stage starts above a mark, up to the alignment of its first block (the pad every sizing
// function adds).  A list takes an optional block by an option of its own; a sizing function
// that is not told the option measures with the block taken.
struct Workspace {
    gss_ctx *ctx = nullptr;   // NULL: measuring
    size_t bytes = 0;         // measuring: sum of the aligned block sizes
    bool failed = false;      // allocating: a block came back NULL
    Workspace() = default;
    explicit Workspace(gss_ctx *c) : ctx(c) {}
    template <typename T>
    T *take(size_t count, const char *tag) {
        if (!ctx) {
            bytes += align_up(count * sizeof(T));
            return nullptr;
        }
        T *p = reinterpret_cast<T *>(arena_alloc(ctx, count * sizeof(T), tag));
        failed |= !p;
        return p;
    }
    // allocating mode, after the list: the reserve of the entry point was too small for `stage`
    int status(const char *stage) const {
        return failed ? gss_fail(ctx, GSS_ERR_NOMEM, "%s: workspace sizing bug", stage) : GSS_OK;
    }
};

// Profiling scope: records HIP events around a launch when enabled.
struct ProfScope {
    gss_ctx *ctx;
    ProfEntry e;
    bool active;
    ProfScope(gss_ctx *c, const char *name);
    ~ProfScope();
};
#define GSS_PROF(ctx, name) ProfScope _prof_scope_##__LINE__((ctx), (name))

// Post-launch error check.
#define GSS_LAUNCH_CHECK(ctx, name)                                               \
    do {                                                                          \
        hipError_t _e = hipGetLastError();                                        \
        if (_e != hipSuccess)                                                     \
            return gss_fail((ctx), GSS_ERR_HIP, "launch of %s failed: %s", (name), \
                            hipGetErrorString(_e));                               \
    } while (0)

// A kernel that asks for more than 64 KB of dynamic LDS has to be told so before its launch.
template <typename Kern>
int raise_lds_limit(gss_ctx *ctx, Kern kern, size_t lds) {
    if (lds > 64 * 1024)
        GSS_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                               hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)lds));
    return GSS_OK;
}

// ---------------------------------------------------------------- stage launchers
// (device pointers, workspace from the arena, asynchronous on ctx->stream)
size_t wpe_workspace_bytes(int F, int64_t T, int D, int taps, int delay);
size_t wpe_inverse_power_workspace_bytes(int F, int64_t T);
int wpe_inverse_power_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D, int psd_context,
                          double *w);
// part: -1 = the whole call; 0 / 1 = one of two sets of frequencies that run side by side on
// ctx->stream / ctx->aux_stream (gss_enhance_observation, GSS_VARIANT wpe_halves): part 0 zeroes
// the pivot counter and records ctx->ev_fork behind it, neither part copies the count to the
// host, each has its own correlation work queues.
// array_bins > 0: the call is (part of) a per-array WPE stage over array_bins virtual bins of
// one array each (picks the correlation geometry for the whole stage; 0 = joint WPE).
// cw: ONE iteration whose weights w (F,T) come from the caller instead of wpe_power_kernel
// (gss_wpe_weighted, the WPD): no power pass, every other launch and argument as without it.  The
// pivot count goes to status word `status_word`; `accumulate`: it continues the count of the
// preceding call instead of starting at 0 (the iterations of one WPD call).
struct WpeCallerWeights {
    const double *w;
    int status_word;
    bool accumulate;
};
int wpe_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D, int taps, int delay,
            int iterations, int psd_context, cplx *X, int part = -1, int array_bins = 0,
            const WpeCallerWeights *cw = nullptr);
// the pivot count of the last wpe_run parts -> the context's status word (after the join)
int wpe_copy_zero_pivots(gss_ctx *ctx);
// per-array WPE: (F, T, A C) -> (F A, T, C) (to_arrays) or back; src and dst must not alias
int wpe_arrays_regroup_run(gss_ctx *ctx, const cplx *src, int F, int64_t T, int A, int C,
                           bool to_arrays, cplx *dst);
// second stream + fork / join events of a context, created on first use
int aux_stream_ready(gss_ctx *ctx);

size_t cacgmm_workspace_bytes(int F, int64_t T, int D, int K, bool one_block = false);
// What guides the mixture model (gss_guidance on the device side): initial affiliations and
// source activity mask, element (f, k, t) at [f * f_stride + k * k_stride + t]; f stride 0 =
// one (K, T) table for every frequency.  init NULL: the initialisation is derived from the mask
// (core.py:156-160); mask NULL: every step is unmasked.
struct EmGuide {
    const double *init;
    const uint8_t *mask;
    int64_t init_f_stride, init_k_stride, mask_f_stride, mask_k_stride;
};
// the (K, act_stride) frame activity of the unweighted calls
static inline EmGuide em_guide_from_activity(const uint8_t *act, int64_t act_stride) {
    return EmGuide{nullptr, act, 0, 0, 0, act_stride};
}
int cacgmm_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D, const EmGuide &guide, int K,
               int iterations, int iterations_post, double *gamma);

// A fitted model in the public dense form (gss_cacgmm_model): precision (F,K,D,D), ln det and
// weights (F,K).  The EM's own form is Mq (F,NE,K): the upper triangle of the precision with the
// off-diagonals doubled.
struct EmModel {
    cplx *precision;
    double *log_det, *weight;
};
// The steps of one EM run, in the order they are enqueued: import, `iterations` M-steps from the
// guidance's initialisation (fit(initialization=array), masked where the guide has a mask),
// `model_iterations` E-step + M-step pairs from the current model (fit(initialization=model)),
// export, predict, log-likelihood.  cacgmm_run is {iterations, post - 1 unmasked, predict} with
// the one-launch kernel allowed; the model calls (gss_cacgmm_fit / gss_cacgmm_predict) are
// the other combinations, always on the multi-launch path.
struct EmSchedule {
    int iterations = 0;
    int model_iterations = 0;
    bool model_masked = false;       // the model iterations multiply the mask in (if there is one)
    bool predict_masked = false;     // so do the predict step and the log-likelihood
    double *gamma = nullptr;         // (F,K,T) posteriors of the predict step, NULL = no predict
    double *loglik = nullptr;        // (F,T), NULL = none
    const EmModel *import_model = nullptr, *export_model = nullptr;
    bool onchip_allowed = false;
    // One prior[k, t] for all frequencies in place of pi[f, k] (gss_cacgmm_shared_prior; pb_bss
    // weight_constant_axis=-3): the multi-launch path as ONE block of frequencies on one stream,
    // E-steps from cacgmm_prior.hip; no model import / export and no log-likelihood.  `prior`
    // (K,T) receives the prior of the last M-step -- the one the predict step used -- or is NULL.
    bool shared_prior = false;
    double *prior = nullptr;
};
int cacgmm_schedule_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D, const EmGuide &guide,
                        int K, const EmSchedule &s);
// cacgmm_model.hip: the conversions between the two forms (lossless: a factor 2) and the
// log-likelihood of the frames under a model
int cacgmm_model_import(gss_ctx *ctx, const EmModel &m, int F, int K, int D, cplx *Mq,
                        double *logdet, double *pi);
int cacgmm_model_export(gss_ctx *ctx, const cplx *Mq, const double *logdet, const double *pi, int F,
                        int K, int D, const EmModel &m);
int cacgmm_loglik_run(gss_ctx *ctx, const cplx *Yn, const cplx *Mq, const double *logdet,
                      const double *pi, const uint8_t *act, int64_t act_stride,
                      int64_t act_fstride, int masked, int F, int64_t T, int D, int K,
                      double *loglik);

// cacgmm_prior.hip: the E-step with a per-frame prior shared by the frequencies and the prior
// update.  The workspace the mode adds to cacgmm_workspace_bytes has its own term.
enum { EM_PRIOR_FIRST = 0, EM_PRIOR_FIT = 1, EM_PRIOR_PREDICT = 2 };
struct EmPriorWork {
    double *G;       // (F,K,T) clipped affiliations of the last fit E-step
    double *prior;   // (K,T)
    double *part;    // (slices,K,T) of the column sum
    double *Sg;      // (F, ceil(T / 64), K) sums of gamma per 64-frame tile
};
struct EmPriorArgs {
    const cplx *Yn;             // (F,D,T) unit-normalised observation
    const cplx *Mq;             // (F,NE,K)
    const double *logdet;       // (F,K)
    const double *prior;        // (K,T)
    const uint8_t *act;         // mask, element (f, k, t) at [f * act_fstride + k * act_stride + t];
    int64_t act_stride, act_fstride;    // always readable, used when `masked` (or init == NULL)
    const double *init;         // EM_PRIOR_FIRST: initial affiliations, NULL = derived from the mask
    int64_t init_stride, init_fstride;
    double *W, *G, *Sg;         // EM_PRIOR_FIRST / FIT: (F,K,T), (F,K,T), (F, ceil(T / 64), K)
    double *gamma;              // EM_PRIOR_PREDICT: (F,K,T)
    int64_t T;
    int F, D;
    int masked;
    double aff_eps;             // clip, 0 = none
};
constexpr int PRIOR_MAX_SLICES = 32;    // slices of the column sum: `part` holds this many (K,T) planes
size_t cacgmm_prior_workspace_bytes(int F, int64_t T, int K);
// the block list of the mode (own_prior false: the caller's table, w.prior is left NULL for it)
EmPriorWork cacgmm_prior_alloc(Workspace &ws, int F, int64_t T, int K, bool own_prior);
int cacgmm_prior_estep_run(gss_ctx *ctx, const EmPriorArgs &a, int K, int mode);
// prior = mean over the first nf frequencies of w.G (nf = 1: a frequency-independent table, copied)
int cacgmm_prior_update_run(gss_ctx *ctx, const EmPriorWork &w, int nf, int K, int64_t T);

// cacgmm_align.hip: permutation alignment of per-frequency posteriors (include/gss_hip.h:
// gss_cacgmm_align, gss_cacgmm_model_permute).  The plan has been validated by the entry point
// and is read during the call; the workspace has its own term (own_aligned: the activity is
// wanted but the caller takes no aligned table, so one comes from the arena).  The count of
// moved rows goes to status word GSS_STATUS_ALIGN_MOVED.
size_t cacgmm_align_workspace_bytes(int F, int K, int64_t T, const gss_align_plan *plan,
                                    bool own_aligned);
int cacgmm_align_run(gss_ctx *ctx, const double *gamma, int F, int K, int64_t T,
                     const gss_align_plan *plan, int32_t *mapping, double *aligned,
                     double *activity);
int cacgmm_model_permute_run(gss_ctx *ctx, const EmModel &in, int F, int K, int D,
                             const int32_t *mapping, const EmModel &out);

// cacgmm_link.hip: cross-window class linking (include/gss_hip.h: gss_cacgmm_link,
// gss_cacgmm_link_gather).  The frame ranges have been validated by the entry point; the partial
// rows come from the arena (cacgmm_link_workspace_bytes).
size_t cacgmm_link_workspace_bytes(int F, int K);
int cacgmm_link_run(gss_ctx *ctx, const double *prev, int64_t T_prev, int64_t prev_begin,
                    const double *cur, int64_t T_cur, int64_t cur_begin, int64_t L, int F, int K,
                    int32_t *mapping, double *scores);
int cacgmm_link_gather_run(gss_ctx *ctx, const double *gamma, int F, int K, int64_t T,
                           const int32_t *mapping, double *out);

// PSD pass of the beamformers: `rows` weight rows per frequency, 2 [target, distortion] or 3
// [target, interferer, noise] (the LCMV): Wr (F, rows, T) -> part (F, nch, rows, NE).
// S > 1: S targets' weights (S, F, rows, T) -> partials (S, F, nch, rows, NE), one launch
int psd_partials_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D, const double *Wr,
                     int rows, int nch, int chunk_frames, cplx *part, int S = 1);

size_t mvdr_workspace_bytes(int F, int64_t T, int D, int S = 1);
// targets: the multi-target tail of gss_enhance_observation_targets -- masks (S,F,T) in,
// Xhat (S,T,F) and ref_channel (S) out, the per-target status words of the context written
// (the one-target path passes S = 1, targets = false and keeps its own kernels)
int mvdr_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D, const double *mx,
             const double *mn, int ban, cplx *Xhat, int32_t *ref_channel, int gev = 0,
             int forced_ref = -1, int S = 1, bool targets = false);
// Segment-wise (piecewise time-invariant) MVDR-Souden, include/gss_hip.h: gss_mvdr_souden_segments.
// One pass over Y for the PSD partials of all segments, mvdr_solve_kernel on a (F, B) grid, one
// reference channel over all (segment, frequency) pairs (forced_ref >= 0: the caller's), apply
// with each segment's filter.  `seg` has been validated by the entry point.
size_t mvdr_segments_workspace_bytes(int F, int64_t T, int D, int64_t segment_frames);
int mvdr_segments_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D, const double *mx,
                      const double *mn, int ban, const gss_bf_segments &seg, cplx *Xhat,
                      int32_t *ref_channel, int forced_ref = -1);
// Interferer-nulling LCMV (Souden), include/gss_hip.h: gss_lcmv_souden.  Three masks (F,T) ->
// three-row PSD pass, lcmv_solve_kernel (per frequency the LCMV, or the MVDR of the merged mask
// where the interferer mask sums to less than min_mass), then the MVDR's reference-channel and
// apply kernels.  The fallback count goes to the context's status word.
size_t lcmv_workspace_bytes(int F, int64_t T, int D);
int lcmv_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D, const double *mx,
             const double *mi, const double *mn, int ban, int forced_ref, double min_mass,
             cplx *Xhat, int32_t *ref_channel);
// gamma (F,K,T) -> target, interferer and noise masks; the interferer is bf.interferer or the
// candidate of largest mass (device int32 `interferer`, may be NULL, and the status word)
size_t lcmv_masks_workspace_bytes(int F, int K);
int lcmv_masks_run(gss_ctx *ctx, const double *gamma, int F, int K, int64_t T, int target,
                   const gss_bf_lcmv &bf, int drop, int64_t start_frames, int64_t end_frames,
                   double *mx, double *mi, double *mn, int32_t *interferer);
// The targets of masks_targets_kernel (by value): target class and zeroed context frames
struct TargetMaskArgs {
    int S;
    int target[GSS_MAX_CLASSES];
    int64_t zero_lo_end[GSS_MAX_CLASSES], zero_hi_begin[GSS_MAX_CLASSES];
};
// gamma (F,K,T) -> mx, mn (S,F,T) for targets[s] with context frames sf[s] / ef[s] (host arrays)
int masks_targets_run(gss_ctx *ctx, const double *gamma, int F, int K, int64_t T, int S,
                      const int32_t *targets, int drop, const int64_t *sf, const int64_t *ef,
                      double *mx, double *mn);
int masks_from_posteriors_run(gss_ctx *ctx, const double *gamma, int F, int K, int64_t T,
                              int target, int drop, int64_t start_frames,
                              int64_t end_frames, double *mx, double *mn);

size_t stft_workspace_bytes(int64_t T, int size);
int stft_run(gss_ctx *ctx, const void *x, int in_type, int D, int64_t N, int fading, cplx *Y);
// S signals: X (S,T,F) -> x (S, gss_istft_num_samples(T)), one launch per kernel
int istft_run(gss_ctx *ctx, const cplx *X, int64_t T, int fading, double *x, int S = 1);
int activity_run(gss_ctx *ctx, const uint8_t *act, int K, int64_t N, int fading,
                 uint8_t *out);
// X (T,F) -> frm (T, size) windowed inverse frames, one transform per frame: a frame's samples do
// not depend on its neighbours in the call (istft_run pairs frames 2b and 2b + 1)
int istft_single_frames_run(gss_ctx *ctx, const cplx *X, int64_t T, double *frm);
int channel_pick_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D, int mode,
                     cplx *Xhat);  // mode 1: 'ch2', 2: 'sum'
int mask_mul_run(gss_ctx *ctx, cplx *Xhat, const double *mask_ft, int F, int64_t T);
// S targets: dst[s] (T,F) = src + s * src_stride (T,F), times mask mx[s] (F,T) when apply_mask
// (src_stride 0: one X_hat for every target; src == dst with stride F T: in place)
int mask_mul_targets_run(gss_ctx *ctx, const cplx *src, int64_t src_stride, cplx *dst,
                         const double *mx, int F, int64_t T, int S, int apply_mask);

// Envelope-variance channel selection (chsel.hip; include/gss_hip.h: gss_channel_select).  `sel`
// has been validated by the entry point; workspace from the arena (chsel_workspace_bytes).
// scores_run: Y (F,T,D) -> scores (D), band variances (B,D) into band_var when given.
// select_run: scores, then the sel.keep best channels in ascending order -> channels (device,
// may be NULL) and the context's status words; Ysel (F,T,keep) gathered unless NULL.
size_t chsel_workspace_bytes(int F, int64_t T, int D, int B);
int chsel_scores_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D,
                     const gss_channel_select &sel, double *scores, double *band_var);
int chsel_select_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D,
                     const gss_channel_select &sel, cplx *Ysel, int32_t *channels);

// Posterior activity (posterior_activity.hip; include/gss_hip.h: gss_posterior_activity): Y (F,T,D)
// and gamma (F,K,T) -> scores (K,T) and, unless NULL, power (T); W (F,) frequency weights or NULL
// for ones.  The partial planes come from the arena (pact_workspace_bytes).
size_t pact_workspace_bytes(int F, int64_t T, int K);
int pact_run(gss_ctx *ctx, const cplx *Y, const double *gamma, int F, int K, int64_t T, int D,
             const double *W, double *scores, double *power);

// WPD convolutional beamformer (wpd.hip; include/gss_hip.h: gss_wpd_souden).  weights_run: the
// weights a (F,T) of one iteration from Y (F,T,D) and the mask (F,T), or (xhat != NULL) from
// |xhat (T,F)|^2; gate (T) or NULL; mxg (F,T), may be NULL, receives mask * gate (first form).
// wpd_run: `bf` has been validated by the entry point, forced_ref as in mvdr_run; the pivots its
// WPE steps zero go to status word GSS_STATUS_WPD_ZERO_PIVOTS, the WPE stage's word is untouched.
size_t wpd_workspace_bytes(int F, int64_t T, int D, int taps, int delay);
int wpd_weights_run(gss_ctx *ctx, const cplx *Y, const double *mask, const cplx *xhat,
                    const uint8_t *gate, int F, int64_t T, int D, double power_floor, double *a,
                    double *mxg);
int wpd_context_gate_run(gss_ctx *ctx, int64_t T, int64_t start_frames, int64_t end_frames,
                         uint8_t *gate);
int wpd_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D, const double *mask,
            const uint8_t *gate, const gss_bf_wpd &bf, int forced_ref, cplx *Xhat,
            int32_t *ref_channel);

// Online WPE (wpe_online.hip; include/gss_hip.h: gss_wpe_online).  Y (F,T,A C) -> X (F,T,A C), the
// state (P (F A,n,n), G (F A,n,C), hist (F A,L,C)) advanced in place; P == G == hist == NULL: a
// fresh state from the arena, thrown away.  force_mem: the memory form at any n (GSS_VARIANT
// wpe_online_mem, read by the entry points).  Arguments validated by the entry point, T >= 1.
size_t wpe_online_workspace_bytes(int F, int64_t T, int A, int C, int taps, int delay, bool fresh);
bool wpe_online_uses_memory_form(int n, bool force_mem);
int wpe_online_init_run(gss_ctx *ctx, int F, int A, int C, int taps, int delay, cplx *P, cplx *G,
                        cplx *hist);
int wpe_online_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int A, int C, int taps, int delay,
                   double alpha, cplx *P, cplx *G, cplx *hist, cplx *X, bool force_mem);

// Online MVDR (mvdr_online.hip; include/gss_hip.h: gss_mvdr_online).  Y (F,T,D), masks (F,T) ->
// X, element (f, t) at [f xs_f + t xs_t], and the filters W (F,T,D) or NULL; phi_x, phi_n (F,D,D)
// the caller's state, advanced in place, both NULL: a fresh one from the arena, initialised from Y
// with `loading` and thrown away.  ref < 0: the reference channel of mvdr_run over the call's
// frames (window_ref in the workspace formula).  The fallback frames go to status word
// GSS_STATUS_MVDR_ONLINE_FALLBACKS, the reference channel to word 0.  Arguments validated by the
// entry point, T >= 1.
size_t mvdr_online_workspace_bytes(int F, int64_t T, int D, bool fresh, bool window_ref);
int mvdr_online_init_run(gss_ctx *ctx, int F, int D, const cplx *Y, int64_t T, double loading,
                         cplx *phi_x, cplx *phi_n);
int mvdr_online_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D, const double *mx,
                    const double *mn, int ban, double beta, double loading, int ref, cplx *phi_x,
                    cplx *phi_n, cplx *X, int64_t xs_f, int64_t xs_t, cplx *W,
                    int32_t *ref_out = nullptr);
// S targets of one stream from the posteriors gamma (F,K,T): phi_x / phi_n the S callers' states,
// X (S,T,F), the masks mx / mn (S,F,T) or NULL, W (S,F,T,D) or NULL, ref_out (S,) or NULL.
// postfilter: X times the target mask.  The fallback frames go to the words
// GSS_STATUS_MVDR_ONLINE_TARGETS + s, their sum to GSS_STATUS_MVDR_ONLINE_FALLBACKS.  T >= 1,
// ref >= 0, 1 <= S <= GSS_CACGMM_ONLINE_MAX_CLASSES.
size_t mvdr_online_targets_workspace_bytes(int F, int S);
int mvdr_online_targets_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D,
                            const double *gamma, int K, const int32_t *targets, int S, int ban,
                            double beta, int ref, cplx *const *phi_x, cplx *const *phi_n,
                            int postfilter, double *mx, double *mn, cplx *X, cplx *W,
                            int32_t *ref_out);
// Look-ahead L (gss_mvdr_online_lookahead*): the two calls above with frame g filtered by the
// filter of frame g + L through the caller's delay line(s).  A call of T >= 1 frames writes
// R = mvdr_online_lookahead_rows() rows: X (F,R) and W (F,R,D) of the masks form, rows [0, R) of
// every target of X (S,Xrows,F) and W (S,F,R,D) of the posteriors form.  release: the held frames
// with the last filter -> rows [0, held) of X (S,Xrows,F), W (S,F,held,D); the sums untouched.
// The runs advance the lines' host counter `held`.  The fallback frames go where the calls above
// leave them.  The S lines have the call's F, D, one L and one `held` (validated by the entry).
size_t mvdr_online_lookahead_workspace_bytes(int F, int S);
int64_t mvdr_online_lookahead_rows(const gss_mvdr_online_hold *hold, int64_t T);
int mvdr_online_hold_init_run(gss_ctx *ctx, gss_mvdr_online_hold *hold);
int mvdr_online_lookahead_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D, const double *mx,
                              const double *mn, int ban, double beta, int ref, cplx *phi_x,
                              cplx *phi_n, gss_mvdr_online_hold *hold, cplx *X, cplx *W);
int mvdr_online_lookahead_targets_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D,
                                      const double *gamma, int K, const int32_t *targets, int S,
                                      int ban, double beta, int ref, cplx *const *phi_x,
                                      cplx *const *phi_n, gss_mvdr_online_hold *holds, int postfilter,
                                      double *mx, double *mn, cplx *X, int64_t Xrows, cplx *W,
                                      int32_t *ref_out);
int mvdr_online_release_run(gss_ctx *ctx, gss_mvdr_online_hold *holds, int S, int postfilter, cplx *X,
                            int64_t Xrows, cplx *W);

// Online CACGMM (cacgmm_online.hip; include/gss_hip.h: gss_cacgmm_online).  Y (F,T,D), the mask of
// `guide` (its initialisation is not read) -> gamma (F,K,T); S (F,K,D,D), n (F,K) the caller's
// state, advanced in place, both NULL: a fresh one of mass prior_mass from the arena, thrown away.
// The fallback count goes to status word GSS_STATUS_CACGMM_ONLINE_FALLBACKS.  Arguments validated
// by the entry point, T >= 1, K <= GSS_CACGMM_ONLINE_MAX_CLASSES.
size_t cacgmm_online_workspace_bytes(int F, int K, int D, bool fresh);
int cacgmm_online_fresh_run(gss_ctx *ctx, int F, int K, int D, double mass, cplx *S, double *n);
int cacgmm_online_from_model_run(gss_ctx *ctx, const EmModel &m, int F, int K, int D, double mass,
                                 cplx *S, double *n);
int cacgmm_online_to_model_run(gss_ctx *ctx, const cplx *S, const double *n, int F, int K, int D,
                               const EmModel &m);
int cacgmm_online_run(gss_ctx *ctx, const cplx *Y, int F, int64_t T, int D, const EmGuide &guide,
                      int K, double beta, double prior_mass, cplx *S, double *n, double *gamma);

// Sample-block stream (stream.hip; include/gss_hip.h: gss_stft_stream, gss_istft_stream).  The
// state and the arguments have been validated by the entry point; the host counters of the state
// are advanced by the run.  stft: n >= 1 samples -> Tn = gss_stream_num_frames() frames Y (F,Tn,D)
// and, with an activity, actf (K,Tn).  istft: X (S,Tn,F), Tn >= 1 -> out (S,m), m =
// gss_stream_num_samples_out() samples of each of the S signals of one stream, with the caller's
// overlap-add tails (S, size - shift); st->frames_out advances once, st->ola_tail is touched only
// where it is handed in as the tails (S = 1: the synthesis of a one-signal stream).  Workspace
// from the arena (stream_*_workspace_bytes).
size_t stream_stft_workspace_bytes(int64_t Tn, int D, int K, int size, int shift);
int stream_init_run(gss_ctx *ctx, gss_stream_state *st);
int stream_stft_run(gss_ctx *ctx, const void *x, int in_type, const uint8_t *act, int64_t n,
                    gss_stream_state *st, cplx *Y, uint8_t *actf);
size_t stream_istft_targets_workspace_bytes(int64_t Tn, int S, int size, int shift);
int stream_istft_targets_run(gss_ctx *ctx, const cplx *X, int64_t Tn, int S, gss_stream_state *st,
                             double *tails, double *out);

int selftest_mfma_run(gss_ctx *ctx);

// Shared device routine: cyclic-Jacobi eigendecomposition of Hermitian matrices
// held in LDS (see jacobi.h).
