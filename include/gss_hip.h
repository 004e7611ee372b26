/*
 * gss_hip.h -- C ABI of libgss_hip.so: the MI355X (gfx950) implementation of the
 * pb_chime5 guided-source-separation hot path
 *
 *     STFT -> WPE -> CACGMM (guided EM) -> MVDR-Souden (+BAN) -> iSTFT
 *
 * i.e. everything /root/reference/pb_chime5/core.py:514-571
 * (Enhancer.enhance_observation) executes per utterance.  The reference has no
 * FFI layer of its own: its boundary is a set of Python callables that hand NumPy
 * arrays to nara_wpe / pb_bss.  Each entry point below names the reference call
 * it replaces (file:line).  The Python host package (pb_chime5_amd) binds this
 * header with ctypes and keeps the reference's Python signatures on top of it.
 *
 * Conventions
 *  - every function returns 0 on success or a negative gss_status; the message
 *    for the last failure on a context is available from gss_last_error().
 *  - no C++ types, no exceptions, no torch types cross this boundary.
 *  - one gss_ctx per GPU (per host thread); a context is not thread-safe,
 *    different contexts are independent.  All work of a context is ordered on
 *    one HIP stream (its own, or one adopted with gss_set_stream()); a second
 *    stream the fused pipeline may use inside a call is forked from and joined to
 *    it by events (gss_set_utterances_in_flight()).
 *  - the caller owns every buffer it passes in.  Pointers named *_dev are device
 *    pointers valid on the context's GPU (from gss_dev_malloc(), or any other
 *    allocator of the same process, e.g. torch); pointers named *_host are host
 *    pointers.  Device entry points are asynchronous on the context's stream and
 *    never retain caller pointers after the work they enqueue has run.
 *  - arithmetic type: float64 / complex128 end to end, like the reference
 *    ("gss_cplx" = interleaved {re, im} doubles).
 *
 * Canonical device layouts (row-major, last index fastest)
 *    time signal   x      (D, N)      double
 *    STFT tensor   Y      (F, T, D)   gss_cplx      "FTD"; F = size/2 + 1
 *    activity      act    (K, N)      uint8  (time)  /  (K, T) uint8 (frames)
 *    posteriors    gamma  (F, K, T)   double
 *    masks         m      (F, T)      double
 *    beamformed    Xhat   (T, F)      gss_cplx       (the reference's layout)
 * The reference's (D, T, F) / (K, T, F) / (T, F) layouts are produced / consumed
 * with the gss_layout_* helpers.
 */
#ifndef GSS_HIP_H
#define GSS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gss_ctx gss_ctx;
typedef struct { double re, im; } gss_cplx;

typedef enum {
    GSS_OK = 0,
    GSS_ERR_INVALID = -1,      /* bad argument (-> AssertionError / ValueError)   */
    GSS_ERR_HIP = -2,          /* HIP runtime failure                              */
    GSS_ERR_NOMEM = -3,        /* device allocation failed                         */
    GSS_ERR_UNSUPPORTED = -4   /* configuration outside the built kernels          */
                               /* (-> NotImplementedError)                         */
} gss_status;

/* Limits of the built kernels. */
#define GSS_MAX_CHANNELS 32    /* reference asserts D < 30 (beamforming_wrapper.py:44) */
#define GSS_MAX_CLASSES 19     /* pb_bss asserts K < 20 (CACGMMTrainer.fit); CHiME-5/6: K <= 5 */
#define GSS_MAX_STFT_SIZE 4096 /* any even length; powers of two take the FFT kernels, others a direct DFT */

/* ABI revision of this header.  Bumped whenever an entry point changes its argument list
 * or a struct its layout (round 2 added `psd_context` to gss_wpe and `wpe_psd_context` to
 * gss_params: revision 2; rounds 3, 4 and 5 added entry points only: revisions 3, 4, 5;
 * revision 7 appended `wpe_arrays` to gss_params and added gss_wpe_arrays).  The entry points
 * gss_enhance_observation_targets(_pcm16) and gss_last_ref_channels came later and, unlike the
 * additions of rounds 3 - 5, did not bump the revision: revision 7 is pinned by the test suite
 * of the per-array WPE.  A library of revision 7 may therefore lack them; the Python binding
 * checks for every symbol it declares and asks for a rebuild when one is missing.  A binder
 * compares gss_abi_version() with the GSS_ABI_VERSION it was written against before any other
 * call (and, for these three, looks the symbols up).  gss_cacgmm_guided and
 * gss_enhance_observation_guided (with the gss_guidance descriptor) were added the same way:
 * entry points only, no struct or argument list of an existing one changed, revision still 7.
 * So were gss_mvdr_souden_segments, gss_enhance_observation_segments and
 * gss_last_segment_fallbacks with the gss_bf_segments descriptor (gss_params keeps its layout:
 * the segment settings travel in a descriptor of their own).  So were gss_channel_scores,
 * gss_select_channels, gss_last_selected_channels and gss_enhance_observation_select(_pcm16)
 * with the gss_channel_select descriptor: entry points only, gss_params and gss_debug_taps keep
 * their layouts, revision still 7.  So were gss_cacgmm_fit and gss_cacgmm_predict with the
 * gss_cacgmm_model descriptor.  So were gss_lcmv_souden, gss_lcmv_masks_from_posteriors,
 * gss_enhance_observation_lcmv, gss_last_lcmv_interferer and gss_last_lcmv_fallbacks with the
 * gss_bf_lcmv descriptor.  So were gss_posterior_activity and gss_enhance_observation_activity.
 * So were gss_wpe_weighted, gss_wpd_weights, gss_wpd_souden, gss_last_wpd_zero_pivots and
 * gss_enhance_observation_wpd with the gss_bf_wpd descriptor.  So was gss_cacgmm_shared_prior
 * (it takes the gss_guidance descriptor as it is).  So were gss_wpe_online_init, gss_wpe_online and
 * gss_enhance_observation_wpe_online with the gss_wpe_online_state and gss_wpe_online_cfg
 * descriptors.  So were gss_cacgmm_align, gss_cacgmm_model_permute and gss_last_align_moved with
 * the gss_align_plan descriptor.  So were gss_mvdr_online_init, gss_mvdr_online,
 * gss_last_mvdr_online_fallbacks and gss_enhance_observation_bf_online with the
 * gss_mvdr_online_state and gss_bf_online descriptors.  So were gss_cacgmm_online_init,
 * gss_cacgmm_online, gss_cacgmm_online_model, gss_last_cacgmm_online_fallbacks and
 * gss_enhance_observation_gss_online with the gss_cacgmm_online_state and gss_em_online
 * descriptors.  So were gss_stream_init, gss_stream_num_frames, gss_stream_num_samples_out,
 * gss_stream_flush_samples, gss_stft_stream, gss_istft_stream and gss_stream_block with the
 * gss_stream_state and gss_stream_cfg descriptors.  So were gss_mvdr_online_targets,
 * gss_last_mvdr_online_fallbacks_targets, gss_istft_stream_targets and gss_stream_block_targets
 * (they take the existing descriptors as they are).  So were gss_mvdr_online_hold_init,
 * gss_mvdr_online_lookahead, gss_mvdr_online_lookahead_targets, gss_mvdr_online_release and
 * gss_stream_block_lookahead with the gss_mvdr_online_hold descriptor. */
#define GSS_ABI_VERSION 7
int gss_abi_version(void);

/* ---- context ----------------------------------------------------------- */
/* Number of visible HIP devices (0 if none / no driver).  Ranks of a node pick
 * LOCAL_RANK % gss_device_count() (pb_chime5_amd.parallel, replacing dlp_mpi's
 * rank handling at core.py:363-381). */
int gss_device_count(void);
/* PCI address of a device ("0000:c1:00.0", NUL-terminated, `len` >= 16 bytes): the host side
 * reads /sys/bus/pci/devices/<address>/{numa_node,local_cpulist} to run a rank's threads on
 * the socket its GPU hangs off (the reference leaves placement to mpiexec, README.md:108-111). */
int gss_device_pci_bus_id(int device_id, char *buf, int len);
int gss_create(int device_id, gss_ctx **ctx);
int gss_destroy(gss_ctx *ctx);
const char *gss_last_error(gss_ctx *ctx);
const char *gss_version(void);
/* Adopt an existing hipStream_t (e.g. torch's current stream); NULL restores the
 * context's own stream. */
int gss_set_stream(gss_ctx *ctx, void *hip_stream);
/* How many utterances the caller keeps in flight on this context's GPU (over all of its
 * contexts); 0 = not said (the default).  Exactly 1 -- one utterance at a time, the loop of
 * Enhancer.enhance_example, /root/reference/pb_chime5/core.py:363-392 -- lets
 * gss_enhance_observation*() run the two halves of the frequencies of the WPE stage side by
 * side on a second, internal stream: one half's solve under the other's correlation, the same
 * bits, the utterance ~1.5 % sooner.  With two or more utterances in flight (the session
 * driver) they already fill each other's idle time; with 0 the call stays on the context's
 * stream alone as well (and per-kernel timings mean what they say).  GSS_ERR_INVALID for n < 0. */
int gss_set_utterances_in_flight(gss_ctx *ctx, int n);
int gss_synchronize(gss_ctx *ctx);

/* ---- device memory plumbing (for hosts that have no allocator) ---------- */
int gss_dev_malloc(gss_ctx *ctx, size_t bytes, void **dev_ptr);
int gss_dev_free(gss_ctx *ctx, void *dev_ptr);
int gss_memcpy_h2d(gss_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int gss_memcpy_d2h(gss_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
int gss_memset(gss_ctx *ctx, void *dst_dev, int value, size_t bytes);
/* Page-locked host memory and copies that return at once (ordered on the context's stream;
 * the host buffer must stay untouched until gss_synchronize() or a later synchronous call
 * returns).  With pageable memory the *_async forms behave like the plain ones.  The session
 * driver reads WAV samples straight into such a block (replaces the reference's soundfile
 * read + float64 conversion + np.array stacking, io/audioread.py:34-226, core.py:427-470).
 * gss_host_malloc / gss_host_free touch no context state (the context only names the GPU
 * and receives the error message) and may be called from any thread.  gss_host_free does not
 * wait for the context's stream itself -- no copy from / to the block may be in flight -- but
 * hipHostFree underneath waits for the WHOLE device on ROCm: free page-locked blocks when a
 * session ends, not between utterances (the session driver parks outgrown blocks until then). */
int gss_host_malloc(gss_ctx *ctx, size_t bytes, void **host_ptr);
int gss_host_free(gss_ctx *ctx, void *host_ptr);
int gss_memcpy_h2d_async(gss_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int gss_memcpy_d2h_async(gss_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);

/* ---- per-kernel timing (HIP events on the context's stream) -------------- */
int gss_profile_enable(gss_ctx *ctx, int on);
/* Restrict the timing to one kernel name (NULL or "" = all).  Two events per timed
 * launch sit in the stream, which costs about 4 us of stream time each on MI355X:
 * timing all ~260 launches of an utterance slows it by 6 %, timing one kernel does not. */
int gss_profile_filter(gss_ctx *ctx, const char *kernel);
int gss_profile_reset(gss_ctx *ctx);
/* Writes a JSON object {"kernel": {"calls": n, "ms": total}, ...} (synchronises). */
int gss_profile_report(gss_ctx *ctx, char *buf, size_t buf_size);

/* ---- STFT geometry ------------------------------------------------------- */
/* Number of frames of nara_wpe.utils.stft(..., pad=True) (core.py:305-312). */
int64_t gss_stft_num_frames(int64_t num_samples, int size, int shift, int fading);
/* Output length of nara_wpe.utils.istft (core.py:314-321). */
int64_t gss_istft_num_samples(int64_t num_frames, int size, int shift, int fading);
/* nara_wpe.utils._samples_to_stft_frames (core.py:224-237). */
int64_t gss_samples_to_stft_frames(int64_t samples, int size, int shift, int fading);

/* Analysis / synthesis windows (host pointers, `size` doubles each).  The host
 * computes them exactly like nara_wpe (periodic Blackman, biorthogonal synthesis
 * window) so the library holds no window policy of its own. */
int gss_set_windows(gss_ctx *ctx, int size, int shift,
                    const double *analysis_host, const double *synthesis_host);

/* ---- stage entry points (device pointers, asynchronous) ------------------ */

/* A1  Enhancer.stft -> nara_wpe.utils.stft (core.py:305-312).
 * x (D,N) -> Y (F,T,D), T = gss_stft_num_frames(N,...). */
int gss_stft(gss_ctx *ctx, const double *x_dev, int D, int64_t N,
             int fading, gss_cplx *Y_dev);

/* A9  Enhancer.istft -> nara_wpe.utils.istft (core.py:314-321).
 * X (T,F) -> x (gss_istft_num_samples(T,...)). */
int gss_istft(gss_ctx *ctx, const gss_cplx *X_dev, int64_t T, int fading,
              double *x_dev);

/* A5' activity_time_to_frequency (database/chime5/database.py:409-472),
 * stft_pad=True.  act (K,N) uint8 -> (K,T) uint8.  Bit-exact. */
int gss_activity_time_to_frequency(gss_ctx *ctx, const uint8_t *act_dev, int K,
                                   int64_t N, int fading, uint8_t *act_frames_dev);

/* A2  WPE.__call__ -> nara_wpe.wpe.wpe_v8(statistics_mode='full') (core.py:48-58).
 * psd_context (core.py:56,583; nara_wpe.wpe.get_power): the frame power is averaged
 * over the existing frames of [t - psd_context, t + psd_context]; 0 = the reference
 * default.  Y (F,T,D) -> X (F,T,D); X must not alias Y unless iterations == 0. */
int gss_wpe(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int D,
            int taps, int delay, int iterations, int psd_context, gss_cplx *X_dev);

/* Per-array WPE: WPE.__call__(Obs, stack=False) (core.py:71-79) -- one wpe_v8 per microphone
 * array -- on the pipeline's layout.  Y (F,T,A*C) holds A arrays of C channels each, array-major
 * (the morph('ACN->A*CN') order of enhance_example, core.py:428-441): channels a*C ... a*C+C-1
 * are array a, and each array is dereverberated on its own (its own inverse power, the mean
 * over ITS C channels, its own (C taps) x (C taps) system per frequency).  Y (F,T,A*C) ->
 * X (F,T,A*C): gss_wpe on the (A*F, T, C) regrouping, bit-identical up to one choice -- where
 * F*A bins make four or more rounds of single correlation waves (config 2: 3078 bins of 4
 * channels) their frames are not split over waves, which gss_wpe does at every size (the same
 * sums in another order).  A = 1 is gss_wpe.  X must not alias Y unless iterations == 0 or A > 1. */
int gss_wpe_arrays(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int A, int C,
                   int taps, int delay, int iterations, int psd_context, gss_cplx *X_dev);

/* The weights of one WPE iteration on their own: nara_wpe.wpe.get_power_inverse(Y,
 * psd_context) as wpe_v6 calls it (mean over channels of |Y|^2, optionally averaged over
 * the existing frames of [t - psd_context, t + psd_context], floored at 1e-10 * its maximum
 * over time, inverted).  Y (F,T,D) -> inverse_power (F,T).  A stage entry point for
 * checking the smoothing on its own; gss_wpe computes the same thing inside. */
int gss_wpe_inverse_power(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int D,
                          int psd_context, double *inverse_power_dev);

/* A4-A6  GSS.__call__ (core.py:154-214): initialisation from the frame activity,
 * CACGMMTrainer.fit(iterations, source_activity_mask) and the post step
 * (iterations_post: 0 = masked predict, 1 = predict, >1 = extra unmasked fit
 * iterations then predict).  Y (F,T,D), act_frames (K,T) -> gamma (F,K,T). */
int gss_cacgmm(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int D,
               const uint8_t *act_frames_dev, int K, int iterations,
               int iterations_post, double *gamma_dev);

/* What guides the mixture model, as pb_bss takes it: CACGMMTrainer.fit(y, initialization,
 * source_activity_mask=...) with any (F,K,T) initialisation and any (F,K,T) boolean mask, or
 * no mask.  Element (f, k, t) of a table sits at [f * f_stride + k * k_stride + t]. */
typedef struct {
    const double *init_dev;   /* initial affiliations, used as given (not renormalised, like
                                 pb_bss); NULL: derived from mask_dev as core.py:156-159:
                                 where(mask, 1, 1e-10) / sum over k                          */
    const uint8_t *mask_dev;  /* source_activity_mask, nonzero = active; NULL: no mask
                                 (fit(..., source_activity_mask=None), unmasked predict)     */
    int64_t init_f_stride;    /* elements between frequencies; 0 = one table for every f     */
    int64_t init_k_stride;    /* elements between classes, >= T                              */
    int64_t mask_f_stride;    /* likewise for the mask (strides of a NULL table are unread)  */
    int64_t mask_k_stride;
} gss_guidance;

/* gss_cacgmm with weights and per-frequency guidance.  The schedule is gss_cacgmm's:
 * `iterations` masked fits from the initialisation, then iterations_post as there; with
 * mask_dev == NULL every step is unmasked.  {NULL, act_frames_dev, 0, 0, 0, T} is gss_cacgmm
 * bit for bit.  GSS_ERR_INVALID: guidance NULL, both tables NULL, a non-zero f stride smaller
 * than K * k_stride, a k stride smaller than T.  The values are not validated: NaN or negative
 * weights propagate as they do upstream. */
int gss_cacgmm_guided(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int D,
                      const gss_guidance *guidance, int K, int iterations,
                      int iterations_post, double *gamma_dev);

/* gss_cacgmm_guided with ONE mixture weight per class and FRAME for all frequencies in place of
 * one per class and frequency: pb_bss's CACGMMTrainer with weight_constant_axis=-3 (Ito et al.,
 * frequency-independent source-presence priors), which the reference never calls.  Wherever an
 * E-step of gss_cacgmm_guided multiplies by pi[f, k] this one multiplies by prior[k, t], and
 * wherever an M-step forms pi[f, k] = mean_t gamma it forms prior[k, t] = (1/F) sum_f gamma[f, k, t]
 * from the clipped affiliations that go into the covariance.  The first M-step takes its prior
 * from the initialisation: the table itself when it is (K,T), its mean over f when it is (F,K,T),
 * the derived where(mask, 1, 1e-10) / sum_k table when only a mask is given.  Everything else --
 * observation, descriptor, mask rules, clip 1e-10 during the fit and none in the predict step,
 * eigenvalue floor, the iterations / iterations_post schedule -- is gss_cacgmm_guided's.  The
 * prior ties the frequencies together (class k is the same source in every bin), so the EM can
 * start from a (K,T) table that is no annotation at all; with a mask it is weak guidance (who
 * may speak, not who does).
 * gamma_dev (F,K,T); prior_dev (K,T) or NULL: the prior of the last M-step, i.e. the one the
 * predict step used (not the mean of the returned posteriors).  Always the multi-launch path, one
 * block of frequencies on one stream.  No atomics: the same call gives the same bits.
 * Errors: those of gss_cacgmm_guided.  (Entry point only: revision still 7.) */
int gss_cacgmm_shared_prior(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int D,
                            const gss_guidance *guidance, int K, int iterations,
                            int iterations_post, double *gamma_dev, double *prior_dev);

/* ---- the mixture model as an object ---------------------------------------
 * A fitted CACGMM in caller-owned device buffers: exactly what predict needs, no eigenvector
 * phases.  (Entry points only, looked up by the binding: revision still 7.)
 *
 * Scale.  The posteriors and the log-likelihood depend on (B_k^-1, ln det B_k) only through
 * -D ln(y^H B_k^-1 y) - ln det B_k, which does not change when B_k is multiplied by a positive
 * number.  pb_bss fixes that number by dividing the eigenvalues by their maximum.  The model
 * update of this library takes a Cholesky factorisation wherever it can certify that no
 * eigenvalue would be floored and then leaves B_k at the scale of D * sum(w y y^H) / sum(gamma);
 * only the classes that take the eigendecomposition (a floored eigenvalue, an all-zero frame in
 * the frequency) come out normalised.  gss_cacgmm_fit hands the model out as the EM holds it, so
 * that a later predict or fit continues from the very same bits; to compare it with a pb_bss
 * model, scale class k by c = 1 / lambda_min(precision): precision * c and log_det - D ln c
 * (pb_chime5_amd.cacgmm.CACGMM.normalized() does that on the host).  A model given to
 * gss_cacgmm_predict / gss_cacgmm_fit may have any scale, the normalised one of pb_bss
 * included. */
typedef struct {
    gss_cplx *precision_dev;  /* (F,K,D,D) row-major: B_k^-1, Hermitian, both triangles stored
                                 (a reader takes the upper one and the real part of the diagonal) */
    double   *log_det_dev;    /* (F,K): ln det B_k at the scale of precision_dev (for a normalised
                                 model: the sum of ln of the normalised, floored eigenvalues)      */
    double   *weight_dev;     /* (F,K): pi_k */
} gss_cacgmm_model;

/* CACGMMTrainer.fit.  Y (F,T,D) -> model_out.
 * init_model == NULL: fit(y, initialization=array, iterations, source_activity_mask):
 *   `iterations` >= 1 M-steps from the guidance's initialisation; schedule, mask and the clip
 *   1e-10 are the masked fit of gss_cacgmm_guided, and so are the errors of the guidance.
 * init_model != NULL: fit(y, initialization=model, iterations, source_activity_mask): every
 *   iteration is an E-step from the current model followed by an M-step, masked with
 *   guidance->mask_dev (unmasked if guidance is NULL or has no mask); guidance->init_dev is not
 *   read; iterations == 0 copies the model.  model_out may be the buffers of init_model.
 * The launches are those of gss_cacgmm_guided, in its order, plus the conversions of the model,
 * so  fit(I) + predict(mask) / fit(I) + predict() / fit(I) + fit(model, post - 1, no mask) +
 * predict()  give the posteriors of gss_cacgmm_guided(I, post) for post 0 / 1 / 2+ bit for bit --
 * except for one array (D == 4, 2 <= K <= 6), where gss_cacgmm_guided runs the whole EM in one
 * launch that keeps its model on the chip: the model calls take the multi-launch path there
 * (the one GSS_VARIANT=em_unfused selects for the closed call) and agree with the closed call to
 * rounding, not to the bit.
 * GSS_ERR_INVALID: model_out or one of its fields NULL, a field of init_model NULL,
 * iterations < 0, iterations == 0 without init_model, the stride errors of gss_cacgmm_guided.
 * D and K are limited as for gss_cacgmm. */
int gss_cacgmm_fit(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int D,
                   const gss_guidance *guidance, int K, int iterations,
                   const gss_cacgmm_model *init_model, const gss_cacgmm_model *model_out);

/* CACGMM.predict with affiliation_eps = 0, and the log-likelihood of the frames.  Y (F,T,D) of
 * any frame count (not necessarily the one the model was fitted on); guidance NULL or without a
 * mask: unmasked, only the mask fields are read.  gamma_dev (F,K,T) or NULL, loglik_dev (F,T) or
 * NULL, at least one of them.
 *   loglik[f,t] = ln sum_k pi_k m_kt exp(-D ln q_kt - ln det B_k),
 * q_kt = max(|y^H B_k^-1 y|, tiny) on the unit-normalised frame as the E-step forms it, m_kt the
 * mask (or 1), evaluated as a max-shifted log-sum-exp.  The normalising constant of the complex
 * angular central Gaussian density, ln((D-1)! / (2 pi^D)), does not depend on the data or the
 * model and is LEFT OUT.  A frame with every class masked off gives -inf.  No atomics: the same
 * call gives the same bits.
 * GSS_ERR_INVALID: model or one of its fields NULL, both outputs NULL, the stride errors of the
 * mask as gss_cacgmm_guided. */
int gss_cacgmm_predict(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int D,
                       const gss_cacgmm_model *model, int K, const gss_guidance *guidance,
                       double *gamma_dev, double *loglik_dev);

/* ---- permutation alignment of per-frequency posteriors ---------------------
 * A per-frequency CACGMM started without an annotation numbers its classes independently in
 * every bin.  The aligner finds per frequency the permutation of the classes under which the
 * rows gamma[f, k, :] of all bins look alike (pb_bss users know it as the permutation aligner;
 * the definition here is this library's own, tests/align_reference.py is its NumPy form).
 * (Entry points only, looked up by the binding: revision still 7.)
 *
 * Features: feat[f, j, :] = gamma[f, j, :] / sqrt(sum_t gamma[f, j, t]^2), all zero for a zero row
 * (cosine similarity; the mean is not removed).  The mapping starts as the identity.  A plan
 * entry (iterations, start, end) runs up to `iterations` passes over the frequencies [start, end):
 *   1. c[k, :] = sum_{f in [start, end)} feat[f, mapping[f, k], :], every row scaled to unit norm
 *      (a zero row stays zero);
 *   2. for every f of the range, all from the same c: S[k, j] = <c[k, :], feat[f, j, :]> and
 *      mapping[f, :] = the permutation p that maximises sum_k S[k, p[k]] over all K!, the
 *      lexicographically smallest among exact maxima;
 *   3. a pass that changes no mapping ends the entry.
 * Frequencies outside the range are untouched.  The library holds no plan policy: the host builds
 * the plan (pb_chime5_amd.ops.alignment_plan is the customary one).
 * The exhaustive search limits K to GSS_ALIGN_MAX_CLASSES; K = 1 gives the identity.  Values are
 * not inspected: with non-finite posteriors the mapping is unspecified but every row is a
 * permutation, every loop is bounded and every index stays in range. */
#define GSS_ALIGN_MAX_CLASSES 8
typedef struct {
    const int32_t *iterations, *start, *end;   /* HOST arrays of `entries` values, read during the call */
    int32_t entries;
} gss_align_plan;

/* gamma_dev (F,K,T) -> mapping_dev (F,K) int32, every row a permutation of 0..K-1;
 * aligned_dev (F,K,T) or NULL: aligned[f, k, :] = gamma[f, mapping[f, k], :], must not be
 * gamma_dev; activity_dev (K,T) or NULL: (1/F) sum_f aligned[f, k, t], the quantity
 * gss_cacgmm_shared_prior calls its prior.  Asynchronous on the context's stream; float64, no
 * floating-point atomics: the same call gives the same bits.
 * GSS_ERR_INVALID, before any launch: a NULL gamma_dev, mapping_dev, plan or plan array;
 * entries < 1; an entry with iterations < 1 or not 0 <= start < end <= F; F, T or K < 1;
 * aligned_dev == gamma_dev.  GSS_ERR_UNSUPPORTED: K > GSS_ALIGN_MAX_CLASSES. */
int gss_cacgmm_align(gss_ctx *ctx, const double *gamma_dev, int F, int K, int64_t T,
                     const gss_align_plan *plan, int32_t *mapping_dev, double *aligned_dev,
                     double *activity_dev);

/* The model with its classes renumbered: row (f, k) of precision (F,K,D,D), log_det (F,K) and
 * weight (F,K) of model_out is row (f, mapping[f, k]) of model, so that predict(model_out)[f, k]
 * = predict(model)[f, mapping[f, k]].  mapping_dev (F,K) int32; an entry outside [0, K) writes
 * NaN for that class and reads nothing.  Asynchronous; not in place.
 * GSS_ERR_INVALID: a NULL model, field or mapping_dev, F, K or D < 1, a buffer of model_out that
 * is one of model's.  GSS_ERR_UNSUPPORTED: K > GSS_MAX_CLASSES or D > GSS_MAX_CHANNELS. */
int gss_cacgmm_model_permute(gss_ctx *ctx, const gss_cacgmm_model *model, int F, int K, int D,
                             const int32_t *mapping_dev, const gss_cacgmm_model *model_out);

/* Frequencies whose row of the mapping the last alignment on this context left different from
 * the identity (synchronises the stream, like gss_last_wpe_zero_pivots); 0 before any. */
int gss_last_align_moved(gss_ctx *ctx, int64_t *count_host);

/* ---- cross-window class linking ---------------------------------------------
 * Two overlapping windows of a recording, separated independently, number their classes
 * independently.  On the L frames they share, the link finds the permutation of the current
 * window's classes under which its posteriors agree with the previous window's
 * (tests/link_reference.py is the NumPy form).  prev_dev (F,K,T_prev) and cur_dev (F,K,T_cur) are
 * posteriors in the device layout; frame prev_begin + t of prev is compared with frame
 * cur_begin + t of cur, t in [0, L):
 *   num[a, b] = sum_f sum_t prev[f, a, t] cur[f, b, t]
 *   S[a, b]   = num[a, b] / sqrt(sum_f sum_t prev[f, a, t]^2 * sum_f sum_t cur[f, b, t]^2),
 *               0 where a norm is zero
 *   mapping   = the permutation p that maximises sum_a S[a, p[a]] over all K!, the
 *               lexicographically smallest among exact maxima
 * so that linked[a] = cur[mapping[a]] (the aligner's convention).  mapping_dev (K,) int32,
 * scores_dev (K,K) = S.  Asynchronous on the context's stream; float64, no floating-point atomics:
 * the same call gives the same bits.  Values are not inspected (non-finite posteriors: some
 * permutation).  (Entry points only, looked up by the binding: revision still 7.)
 * GSS_ERR_INVALID, before any launch: a NULL pointer; F, K or L < 1; a negative begin or a frame
 * range that ends behind its table.  GSS_ERR_UNSUPPORTED: K > GSS_ALIGN_MAX_CLASSES. */
int gss_cacgmm_link(gss_ctx *ctx, const double *prev_dev, int64_t T_prev, int64_t prev_begin,
                    const double *cur_dev, int64_t T_cur, int64_t cur_begin, int64_t L,
                    int F, int K, int32_t *mapping_dev, double *scores_dev);

/* A table with its classes renumbered by ONE mapping for all frequencies (what a link returns):
 * out[f, a, :] = gamma[f, mapping[a], :].  gamma_dev, out_dev (F,K,T), mapping_dev (K,) int32 on
 * the device (no host round trip after gss_cacgmm_link); an entry outside [0, K) writes NaN for
 * that class and reads nothing.  Asynchronous; not in place.
 * GSS_ERR_INVALID: a NULL pointer, F, K or T < 1, out_dev == gamma_dev.
 * GSS_ERR_UNSUPPORTED: K > GSS_MAX_CLASSES. */
int gss_cacgmm_link_gather(gss_ctx *ctx, const double *gamma_dev, int F, int K, int64_t T,
                           const int32_t *mapping_dev, double *out_dev);

/* A0  mask post-processing of enhance_observation (core.py:537-554): zero the
 * context frames, pick the target class, sum the others.
 * gamma (F,K,T) -> target (F,T), distortion (F,T).  drop_context = 0 skips the
 * zeroing (bf_drop_context=False). */
int gss_masks_from_posteriors(gss_ctx *ctx, const double *gamma_dev, int F, int K,
                              int64_t T, int target_index, int drop_context,
                              int64_t start_context_frames,
                              int64_t end_context_frames,
                              double *target_mask_dev, double *distortion_mask_dev);

/* A7+A8  beamform_mvdr_souden_from_masks (beamforming_wrapper.py:108-124) with
 * eps=1e-10: masked PSD matrices, Souden MVDR, one reference channel from the
 * cross-frequency SNR argmax, optional blind analytic normalisation, apply.
 * Y (F,T,D), masks (F,T) -> Xhat (T,F).  ref_channel_dev (device int32, may be
 * NULL) receives the chosen reference channel. */
int gss_mvdr_souden(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int D,
                    const double *target_mask_dev,
                    const double *distortion_mask_dev, int ban,
                    gss_cplx *Xhat_dev, int32_t *ref_channel_dev);

/* The same with the reference channel named by the caller (pb_bss
 * get_mvdr_vector_souden(ref_channel=...), call site beamforming_wrapper.py:58-63). */
int gss_mvdr_souden_ref(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int D,
                        const double *target_mask_dev,
                        const double *distortion_mask_dev, int ban, int ref_channel,
                        gss_cplx *Xhat_dev);

/* Reference channel of the last MVDR run on this context (gss_mvdr_souden or the fused
 * pipeline); synchronises the stream.  -1: a per-channel SNR was not finite -- pb_bss
 * get_optimal_reference_channel asserts np.all(np.isfinite(SNR)) and the reference
 * aborts the utterance with an AssertionError; here Xhat is filled with NaN and the host
 * raises.  <= -2 (after gss_gev or the fused pipeline with the GEV beamformer): the noise
 * PSD matrix of frequency -2 - value is not positive definite -- scipy.linalg.eigh inside
 * pb_bss get_gev_vector raises numpy.linalg.LinAlgError there and the reference aborts the
 * utterance; Xhat is NaN and the host raises the same.  0 after a successful GEV run.
 * INT32_MIN: no beamformer has run yet. */
int gss_last_ref_channel(gss_ctx *ctx, int32_t *ref_channel_host);

/* Status words of the S targets of the last gss_enhance_observation_targets* call (same codes
 * as gss_last_ref_channel, target order; synchronises the stream).  S larger than that call's
 * number of targets is GSS_ERR_INVALID.  After any other beamformer run, after a targets call
 * with bf 'ch2' / 'sum' (no beamformer, no status) and after one that failed before its
 * beamformer, only S = 1 is accepted and gives gss_last_ref_channel's word. */
int gss_last_ref_channels(gss_ctx *ctx, int32_t *ref_channels_host, int S);

/* Number of pivots the WPE solve of the last gss_wpe / fused call on this context zeroed
 * (summed over its iterations and frequencies; synchronises the stream).  The normal
 * equations are solved by Cholesky; a non-positive pivot zeroes that row, which is the
 * minimum-norm answer of stable_solve's lstsq fallback (math/solve.py:95-114) for an
 * all-zero channel.  A count > 0 on live channels means R was rank deficient -- a segment
 * with no more frames than taps * D unknowns -- where np.linalg.solve returns a different
 * (equally arbitrary) minimiser than this library. */
int gss_last_wpe_zero_pivots(gss_ctx *ctx, int64_t *count_host);

/* Segment-wise (piecewise time-invariant) MVDR: the time span of the beamformer statistics.
 * The T frames are cut into B = ceil(T / segment_frames) segments, segment b = frames
 * [b L, min(T, (b + 1) L)); its statistics window is segments max(0, b - context_segments) ..
 * min(B - 1, b + context_segments).  Not in the reference, which has one window per call. */
typedef struct {
    int64_t segment_frames;   /* L: a positive multiple of 64 (the PSD kernel's frame tile)  */
    int32_t context_segments; /* c >= 0: segments either side in a segment's statistics     */
    double min_mass;          /* >= 0, finite: a window whose target or distortion mask sum */
                              /* is below it takes the whole-window statistics (0: never)   */
} gss_bf_segments;

/* gss_mvdr_souden with one filter per segment.  Per (segment b, frequency f): Phi_X, Phi_N are
 * the masked PSD matrices over the frames of b's statistics window (mask sum floored at 1e-10,
 * as in gss_mvdr_souden), replaced by the whole-window matrices of f -- those of
 * gss_mvdr_souden -- when min(sum of target mask, sum of distortion mask) over the window is
 * below seg->min_mass; W[b,f] is the Souden solution of that pair (eps 1e-10, same LU / lstsq
 * fallback).  ONE reference channel for the call: the SNR argmax with numerator and
 * denominator summed over all (b, f), or ref_channel >= 0 as named by the caller (-1:
 * choose).  w[b,f] = W[b,f][:, ref], with `ban` normalised against that segment's Phi_N, and
 * Xhat[t,f] = w[t / L, f]^H y[f,t].  The observation is read once for the PSD accumulation
 * and the number of launches does not depend on B or context_segments.
 * Y (F,T,D), masks (F,T) -> Xhat (T,F); ref_channel_dev (device int32, may be NULL) receives
 * the status word of gss_last_ref_channel, which works after this call (-1: non-finite SNR,
 * Xhat filled with NaN).  With min_mass = 0 an empty window gives 0 / 0 = NaN under `ban`, as
 * the reference's empty utterance does.
 * GSS_ERR_INVALID (the message names the field): seg NULL, segment_frames < 64 or not a
 * multiple of 64, context_segments < 0, min_mass negative or not finite, ref_channel outside
 * [-1, D). */
int gss_mvdr_souden_segments(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int D,
                             const double *target_mask_dev,
                             const double *distortion_mask_dev, int ban, int ref_channel,
                             const gss_bf_segments *seg, gss_cplx *Xhat_dev,
                             int32_t *ref_channel_dev);

/* Number of (segment, frequency) pairs of the last gss_mvdr_souden_segments /
 * gss_enhance_observation_segments call on this context that fell back to the whole-window
 * statistics (synchronises the stream, like gss_last_wpe_zero_pivots); 0 before any. */
int gss_last_segment_fallbacks(gss_ctx *ctx, int64_t *count_host);

/* Interferer-nulling LCMV (Souden, Benesty, Affes 2010, "A study of the LCMV and MVDR noise
 * reduction filters", eq. 51): beamform_lcmv_souden_from_masks (beamforming_wrapper.py:127-171)
 * -> pb_bss get_lcmv_vector_souden.  Who the interferer is when the masks come from posteriors. */
typedef struct {
    int32_t interferer;      /* >= 0: that class; -1: choose among `candidates`   */
    uint32_t candidates;     /* bit k: class k may be chosen; target bit ignored  */
    double min_mass;         /* >= 0, finite                                      */
} gss_bf_lcmv;

/* gss_mvdr_souden with a null on one interferer.  Per frequency, with S_m = sum_t m_t y_t y_t^H
 * and s_m = sum_t m_t for the target, interferer and noise masks m in {X, I, N}:
 *    Phi_m = S_m / max(s_m, 1e-10);  A = solve(Phi_N, Phi_I), B = solve(Phi_N, Phi_X) (one LU
 *    with partial pivoting for both, the minimum-norm lstsq answer on an exactly singular
 *    Phi_N, as in gss_mvdr_souden);  g_in = tr A,  g = g_in tr B - tr(A B),
 *    W = (g_in B - A B) / max(Re g, 1e-10);  distortion matrix Phi_D = Phi_I + Phi_N.
 * On rank-one Phi_X, Phi_I column r of W is the LCMV filter that passes the target as channel r
 * hears it and nulls the interferer.  A frequency with s_I < min_mass takes the MVDR of the
 * merged mask instead -- Phi_D = (S_I + S_N) / max(s_I + s_N, 1e-10), W = Psi / max(Re tr Psi,
 * 1e-10), Psi = solve(Phi_D, Phi_X): what gss_mvdr_souden computes for N + I -- and is counted
 * (gss_last_lcmv_fallbacks); a frequency factors one matrix, never both.  With min_mass = 0
 * nothing falls back and an empty interferer mask gives W = 0, NaN under `ban` (0 / 0), like
 * the reference function.  ONE reference channel for the call: the argmax over r of
 * sum_f w_r^H Phi_X w_r / max(sum_f w_r^H Phi_D w_r, 1e-10), or ref_channel >= 0 as named by
 * the caller (-1: choose); the floor on g and this choice are this library's (upstream is
 * believed to fix channel 0).  `ban` normalises against Phi_D.
 * Y (F,T,D), masks (F,T) -> Xhat (T,F); ref_channel_dev (device int32, may be NULL) receives the
 * status word of gss_last_ref_channel, which works after this call (-1: non-finite SNR, Xhat
 * filled with NaN).
 * GSS_ERR_INVALID (the message names the field): D < 2 (g is identically 0 on one channel),
 * D >= 30, min_mass negative or not finite, ref_channel outside [-1, D). */
int gss_lcmv_souden(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int D,
                    const double *target_mask_dev, const double *interferer_mask_dev,
                    const double *noise_mask_dev, int ban, int ref_channel, double min_mass,
                    gss_cplx *Xhat_dev, int32_t *ref_channel_dev);

/* gss_masks_from_posteriors for the LCMV: gamma (F,K,T) -> target, interferer and noise masks
 * (F,T).  The interferer is lcmv->interferer, or (-1) the class k with bit k of
 * lcmv->candidates set (k != target_index) of largest mass sum_f sum_t gamma[f,k,t] over the
 * frames the context zeroing keeps -- summed per frequency in a fixed order, then in ascending
 * f; equal masses go to the lower index; -1 (no interferer) without a candidate or when the
 * largest mass is 0.  X = gamma[target], I = gamma[interferer] (all zero for -1), N = the sum of
 * the remaining classes in ascending k; all zeroed on the context frames as in
 * gss_masks_from_posteriors.  interferer_dev (device int32, may be NULL) receives the class;
 * gss_last_lcmv_interferer works afterwards.  lcmv->min_mass is checked, not used.  K <= 19.
 * GSS_ERR_INVALID (the message names the field): lcmv NULL, interferer outside [-1, K) or equal
 * to target_index, min_mass negative or not finite. */
int gss_lcmv_masks_from_posteriors(gss_ctx *ctx, const double *gamma_dev, int F, int K,
                                   int64_t T, int target_index, const gss_bf_lcmv *lcmv,
                                   int drop_context, int64_t start_context_frames,
                                   int64_t end_context_frames, double *target_mask_dev,
                                   double *interferer_mask_dev, double *noise_mask_dev,
                                   int32_t *interferer_dev);

/* The interferer class of the last gss_lcmv_masks_from_posteriors /
 * gss_enhance_observation_lcmv call on this context, -1 when it had none (synchronises the
 * stream, like gss_last_segment_fallbacks); -1 before any. */
int gss_last_lcmv_interferer(gss_ctx *ctx, int32_t *interferer_host);

/* Number of frequencies of the last gss_lcmv_souden / gss_enhance_observation_lcmv call on this
 * context that fell back to the MVDR of the merged mask (synchronises the stream); 0 before
 * any. */
int gss_last_lcmv_fallbacks(gss_ctx *ctx, int64_t *count_host);

/* One WPE step -- correlation, solve, filter application -- with weights from the caller in
 * the place of the inverse power of the observation: R = sum_t w_t yt_t yt_t^H,
 * P = sum_t w_t yt_t y_t^H, X = Y - solve(R, P)^H yt.  Y (F,T,D), weights (F,T) -> X (F,T,D); X
 * must not alias Y.  The launches are those of one gss_wpe iteration without its power pass:
 * fed with the output of gss_wpe_inverse_power(psd_context = 0) it gives the bits of
 * gss_wpe(iterations = 1, psd_context = 0).  The weights are not inspected.  The zeroed pivots
 * are reported by gss_last_wpe_zero_pivots, as for gss_wpe.
 * GSS_ERR_INVALID: a NULL pointer, F < 1, T < 1, taps < 1, delay < 0. */
int gss_wpe_weighted(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int D, int taps,
                     int delay, const double *weights_dev, gss_cplx *X_dev);

/* WPD convolutional beamformer (weighted power minimisation distortionless response: Nakatani &
 * Kinoshita 2019, "A unified convolutional beamformer for simultaneous denoising and
 * dereverberation"; Boeddeker, Nakatani, Kinoshita, Haeb-Umbach 2020, "Jointly optimal
 * dereverberation and beamforming"; not in the reference): ONE filter over the current frame and
 * the WPE tap window, optimised under the time-varying power of the target, computed in its
 * exact factorisation into a WPE step and a weighted-power MPDR. */
typedef struct {
    int taps, delay, iterations, ban;
                           /* taps >= 1, delay >= 0: the tap window of the WPE step;            */
                           /* iterations >= 1; ban: blind analytic normalisation against Phi_a  */
    double power_floor;    /* in (0, 1], finite: the target power is floored at this fraction   */
                           /* of its maximum over the frames the gate keeps.  1e-3 in the       */
                           /* Python layer: a choice, not a measurement                         */
} gss_bf_wpd;

/* The weights of one WPD iteration on their own (a stage entry point for checking them).  With
 * the gate g (T) uint8, nonzero = 1, NULL = all ones:
 *    p_t = mask[f,t] * mean_d |Y[f,t,d]|^2      (Xhat_dev == NULL: the first iteration), or
 *    p_t = |Xhat[t,f]|^2                        (Xhat_dev != NULL: later ones; Y_dev, mask_dev
 *                                                are not read and may be NULL);
 *    p_max = max over the frames with g_t = 1 of p_t (fixed order, no atomics);
 *    a_t = g_t / max(p_t, power_floor * p_max);  a_t = 0 for every t where p_max = 0.
 * Y (F,T,D) + mask (F,T), or Xhat (T,F) -> weights (F,T).
 * GSS_ERR_INVALID (the message names the argument), before any launch: weights_dev NULL, both
 * sources NULL, F < 1, T < 1, D outside [1, 30), power_floor outside (0, 1] or not finite. */
int gss_wpd_weights(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int D,
                    const double *mask_dev, const gss_cplx *Xhat_dev, const uint8_t *gate_dev,
                    double power_floor, double *weights_dev);

/* The WPD beamformer from a target mask.  Per frequency and iteration i = 1 .. iterations:
 *    a = the weights of gss_wpd_weights (i = 1: from Y and the target mask; i > 1: from the
 *        Xhat of iteration i - 1), with wpd->power_floor and the gate;
 *    Z = gss_wpe_weighted(Y, taps, delay, a)            (the WPE solve, zero-pivot semantics);
 *    Xhat = what gss_mvdr_souden computes for the observation Z, the target mask m * g and the
 *        "distortion mask" a: Phi_X = sum m g z z^H / max(sum m g, 1e-10),
 *        Phi_a = sum a z z^H / max(sum a, 1e-10), Souden with eps 1e-10, ONE reference channel
 *        for all frequencies -- the SNR argmax, chosen anew in every iteration, or ref_channel
 *        >= 0 as named by the caller (-1: choose) --, `ban` against Phi_a.
 * Phi_X is taken from Z, not from Y: the filter C w on the stacked observation [y; yt] with
 * C = [I; -G] sees the target covariance C^H Phibar_X C, which is the covariance of z.  A frame
 * with g_t = 0 (the context frames of the fused call) enters no statistic, so the mask there does
 * not matter; the filter is still applied to it.  A frequency with p_max = 0 gives what the MVDR
 * gives for two all-zero masks: Xhat = 0, or NaN under `ban` (0 / 0).
 * Y (F,T,D), target_mask (F,T), gate (T) uint8 or NULL -> Xhat (T,F); ref_channel_dev (device
 * int32, may be NULL) receives the status word of gss_last_ref_channel, which works after this
 * call (-1: non-finite SNR, Xhat filled with NaN).  The pivots the WPE steps zeroed are counted
 * in a word of their own, gss_last_wpd_zero_pivots; gss_last_wpe_zero_pivots keeps the WPE
 * stage's count.
 * GSS_ERR_INVALID (the message names the field), before any launch: a NULL pointer (Y_dev,
 * target_mask_dev, wpd, Xhat_dev), taps < 1, delay < 0, iterations < 1, power_floor outside
 * (0, 1] or not finite, D >= 30, ref_channel outside [-1, D). */
int gss_wpd_souden(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int D,
                   const double *target_mask_dev, const uint8_t *gate_dev,
                   const gss_bf_wpd *wpd, int ref_channel, gss_cplx *Xhat_dev,
                   int32_t *ref_channel_dev);

/* Number of pivots the WPE steps of the last gss_wpd_souden / gss_enhance_observation_wpd call
 * on this context zeroed, summed over its iterations and frequencies (synchronises the stream,
 * like gss_last_wpe_zero_pivots); 0 before any. */
int gss_last_wpd_zero_pivots(gss_ctx *ctx, int64_t *count_host);

/* ---- online WPE -------------------------------------------------------------
 * Frame-recursive dereverberation with a carried state: nara_wpe's online form (a recursive
 * least-squares filter that is updated at every frame and forgets at the rate alpha), which the
 * reference never calls.  (Entry points only, looked up by the binding: revision still 7.)
 * A problem is one frequency f, or one (frequency, array) pair under per-array WPE, with C
 * channels, n = taps * C and L = taps + delay.  For each frame t, in order:
 *    buf   = [hist; y_t]                        (L+1, C): frames t-L .. t (zeros before the stream)
 *    sigma = sum |buf|^2 / ((L+1) C)
 *    w[tau C + c] = frame t - delay - tau, channel c,   tau = 0 .. taps-1
 *    x_t   = y_t - G^H w                        the OUTPUT: the filter before its update
 *    nom   = P w;  den = alpha sigma + Re(w^H nom)
 *    den > 0:  P <- (P - nom nom^H / den) / alpha,  G <- G + (nom / den) x_t^H
 *    else:     P, G unchanged -- the whole buffer is digital silence (w = 0, y_t = 0, x_t = 0),
 *              where the literal recursion divides 0 by 0
 *    hist  <- buf[1:]
 * A fresh state is P = I, G = 0, hist = 0. */
typedef struct {
    gss_cplx *inv_cov_dev;  /* (F, A, n, n) row-major; a reader takes the upper triangle and the real
                               part of the diagonal; on return both triangles are stored, the lower
                               the exact conjugate of the upper, diagonal imaginary parts 0 */
    gss_cplx *filter_dev;   /* (F, A, n, C) */
    gss_cplx *history_dev;  /* (F, A, taps + delay, C), oldest frame first */
} gss_wpe_online_state;    /* caller-owned, like gss_cacgmm_model */

/* P = I, G = 0, hist = 0 in the caller's buffers.  Errors as gss_wpe_online. */
int gss_wpe_online_init(gss_ctx *ctx, int F, int A, int C, int taps, int delay,
                        const gss_wpe_online_state *state);

/* Y (F,T,A*C) -> X (F,T,A*C), channels array-major as in gss_wpe_arrays; A = 1 is the joint WPE.
 * `state` is read, advanced by T frames and written back; NULL: a fresh state that is thrown
 * away after the call.  T = 0 is a no-op.  One persistent workgroup per problem walks the
 * frames; n <= 64 keeps the state on the chip for the whole call, larger n (or GSS_VARIANT
 * wpe_online_mem) leaves it in its buffers -- the form depends on n alone, so a recording fed in
 * blocks through one state gives the bits of the single call.  No atomics: the same call gives
 * the same bits.
 * GSS_ERR_INVALID (the message names the argument), before any launch: a NULL pointer, a NULL
 * state field, F < 1, T < 0, A < 1, C < 1, taps < 1, delay < 0 or >= 2^20, alpha outside (0, 1]
 * or not finite, X_dev == Y_dev.  GSS_ERR_UNSUPPORTED: taps * C > 512, A * C > GSS_MAX_CHANNELS. */
int gss_wpe_online(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int A, int C, int taps,
                   int delay, double alpha, const gss_wpe_online_state *state, gss_cplx *X_dev);

/* ---- online MVDR ------------------------------------------------------------
 * Souden's mask-based MVDR (optionally with blind analytic normalisation) in a causal form: the
 * two PSD matrices are exponentially forgetting running sums, the filter is recomputed at every
 * frame, and the state is carried between calls.  (Entry points only, looked up by the binding:
 * revision still 7.)  One problem per frequency f with D channels.  For each frame t, in order,
 * with y = Y[f,t,:], a = mask_x[f,t], b = mask_n[f,t] and beta = cfg->forget:
 *    Phi_X <- beta Phi_X + a y y^H,   Phi_N <- beta Phi_N + b y y^H
 *    Cholesky Phi_N = L L^H; a pivot that is not > 0 or not finite makes t a FALLBACK frame:
 *                     w = 0, Xhat[f,t] = 0, the frame is counted, the update above stays
 *    Psi = Phi_N^-1 Phi_X;  w = Psi[:, ref] / max(Re trace(Psi), 1e-10)
 *    ban:  v = Phi_N w;  w <- w sqrt(v^H v) / |w^H v|       (eps = 0 as upstream, except that
 *                     |w^H v| = 0 -- a zero filter: no target mass yet, as in the context frames
 *                     of every window -- leaves w = 0 where upstream divides 0 by 0)
 *    Xhat[f,t] = w^H y          the sums INCLUDE frame t: look-ahead L, default 0 (the entries
 *                     below; L >= 1: gss_mvdr_online_lookahead further down)
 * A fresh state is Phi_X = 0, Phi_N = loading * p_f * I, where p_f is the mean of |Y[f,t,d]|^2
 * over the frames and channels handed to the initialisation (1 when there are none, or when
 * that mean is exactly 0). */
typedef struct {
    gss_cplx *phi_x, *phi_n;   /* (F, D, D) row-major; a reader takes the upper triangle and the real
                                  part of the diagonal; on return both triangles are stored, the lower
                                  the exact conjugate of the upper, diagonal imaginary parts 0 */
    int32_t F, D;
} gss_mvdr_online_state;       /* caller-owned, like gss_wpe_online_state */

typedef struct {
    double forget;             /* beta, in (0, 1] */
    double loading;            /* of a fresh state; read only when `state` is NULL */
    int32_t ref_channel;       /* -1: chosen as by gss_mvdr_souden over the call's frames -- NOT
                                  causal: the whole-window statistics of the call pick it */
    int32_t wpe_online;        /* the last two are read by the fused entry only */
    double wpe_alpha;
} gss_bf_online;

/* Phi_X = 0, Phi_N = loading * p_f * I in the caller's buffers, p_f from Y_dev (F,T,D); Y_dev
 * NULL or T = 0: p_f = 1.  The sum for p_f has one fixed order.  GSS_ERR_INVALID before any
 * launch: a NULL state or state field, state->F / state->D other than F / D, F < 1, T < 0,
 * loading not finite or <= 0.  GSS_ERR_UNSUPPORTED: D outside [1, GSS_MAX_CHANNELS]. */
int gss_mvdr_online_init(gss_ctx *ctx, int F, int D, const gss_cplx *Y_dev, int64_t T,
                         double loading, gss_mvdr_online_state *state);

/* Y (F,T,D), masks (F,T) -> Xhat (F,T) and, when W_dev is not NULL, the filters (F,T,D).
 * `state` is read, advanced by T frames and written back; NULL: a fresh state from the workspace,
 * initialised from Y_dev with cfg->loading and thrown away.  T = 0 is a no-op.  One persistent
 * wave per frequency walks the frames with both matrices on the chip; the kernel form and every
 * order of summation depend on D alone, so a recording fed in blocks through one state gives the
 * bits of the single call, and the same call gives the same bits.  gss_last_ref_channel reports
 * the reference channel used (-1: ref_channel = -1 found no finite SNR; Xhat and W are NaN and
 * the state is untouched), gss_last_mvdr_online_fallbacks the fallback frames.
 * GSS_ERR_INVALID (the message names the argument), before any launch: a NULL pointer other than
 * state / W_dev, a NULL state field, state->F / state->D other than F / D, F < 1, T < 0, forget
 * outside (0, 1] or not finite, loading not finite or <= 0, ref_channel outside [-1, D).
 * GSS_ERR_UNSUPPORTED: D outside [1, GSS_MAX_CHANNELS]. */
int gss_mvdr_online(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int D,
                    const double *mask_x_dev, const double *mask_n_dev, int ban,
                    const gss_bf_online *cfg, gss_mvdr_online_state *state, gss_cplx *Xhat_dev,
                    gss_cplx *W_dev);

/* (frequency, frame) pairs of the last online MVDR on this context that fell back (synchronises). */
int gss_last_mvdr_online_fallbacks(gss_ctx *ctx, int64_t *count_host);

/* ---- online CACGMM ----------------------------------------------------------
 * The recursive (online) EM of the complex angular central Gaussian mixture: the class statistics
 * are running sums that forget, frame t is classified by the model of the frames before it and
 * then enters the sums, and the state is carried between calls.  (Entry points only, looked up by
 * the binding: revision still 7.)  One problem per frequency f with D channels and K classes.  The
 * state is, per class, a Hermitian S_k (D,D) and a mass n_k > 0; the model they stand for is
 * B_k = S_k / n_k, pi_k = n_k / sum_j n_j.  For each frame t, in order, with y = Y[f,t,:], m_kt
 * the mask (1 without one) and beta = cfg->forget:
 *    z       = y / max(||y||, tiny)
 *    q_k     = max(|z^H B_k^-1 z|, tiny),  l_k = ln det B_k    from a Cholesky factor of S_k; a
 *              pivot that is not > 0 or not finite makes k a FALLBACK class for this frame:
 *              B_k = I (q_k = max(||z||^2, tiny), l_k = 0), counted
 *    gamma_k = exp(lp_k - max_j lp_j) pi_k m_kt / max(sum, tiny),  lp_k = -D ln q_k - l_k
 *              (CACGMM.predict, affiliation_eps = 0; every class masked off: zeros)
 *    gamma[f,k,t] = gamma_k          the model of the frames BEFORE t: causal, zero look-ahead
 *    ||y|| == 0 exactly: the state is left alone (no decay, no update); else with
 *    g_k = clip(gamma_k, 1e-10, 1 - 1e-10):
 *    S_k <- beta S_k + g_k D z z^H / max(q_k, 10 tiny),    n_k <- beta n_k + g_k
 * There is no eigenvalue normalisation and no eigenvalue floor: the density does not depend on the
 * scale of B_k, and the decaying start term plus the clip keep every S_k of full rank.
 * K is limited to GSS_CACGMM_ONLINE_MAX_CLASSES (one wave per class in one workgroup). */
#define GSS_CACGMM_ONLINE_MAX_CLASSES 8
typedef struct {
    gss_cplx *s;               /* (F, K, D, D) row-major; a reader takes the upper triangle and the real
                                  part of the diagonal; on return both triangles are stored, the lower
                                  the exact conjugate of the upper, diagonal imaginary parts 0 */
    double *n;                 /* (F, K) */
    int32_t F, K, D;
} gss_cacgmm_online_state;     /* caller-owned, like gss_mvdr_online_state */

typedef struct {
    double forget;             /* beta, in (0, 1] */
    double prior_mass;         /* of a fresh state; read only when `state` is NULL */
} gss_em_online;

/* model == NULL: the fresh state S_k = prior_mass I, n_k = prior_mass (all classes identical: only
 * a mask tells them apart, and without one every posterior stays exactly 1 / K).  model != NULL:
 * n_k = model_mass * weight_k, S_k = n_k * precision_k^-1, inverted on the device from a Cholesky
 * factor of the precision; prior_mass is not read.  A precision without a factor is
 * GSS_ERR_INVALID AFTER the launch (this call synchronises), the message gives the count and the
 * state holds n_k I for those classes.
 * GSS_ERR_INVALID before any launch: a NULL state or state field, state->F / K / D other than
 * F / K / D, F < 1, the mass that is read not finite or <= 0, a NULL field of model.
 * GSS_ERR_UNSUPPORTED: D outside [1, GSS_MAX_CHANNELS], K outside
 * [1, GSS_CACGMM_ONLINE_MAX_CLASSES]. */
int gss_cacgmm_online_init(gss_ctx *ctx, int F, int K, int D, double prior_mass,
                           const gss_cacgmm_model *model, double model_mass,
                           gss_cacgmm_online_state *state);

/* Y (F,T,D) -> gamma (F,K,T).  guidance: only the mask fields are read; NULL or no mask: m = 1.
 * `state` is read, advanced by T frames and written back; NULL: a fresh state of cfg->prior_mass
 * from the workspace, thrown away.  T = 0 is a no-op.  One persistent workgroup per frequency
 * walks the frames, one wave per class with S_k in registers; the kernel form and every order of
 * summation depend on D and K alone, so a recording fed in blocks through one state gives the
 * bits of the single call, and the same call gives the same bits.
 * GSS_ERR_INVALID (the message names the argument), before any launch: a NULL pointer other than
 * guidance / state, a NULL state field, state->F / K / D other than F / K / D, F < 1, T < 0,
 * forget outside (0, 1] or not finite, prior_mass not finite or <= 0, the stride errors of the
 * mask as gss_cacgmm_guided.  GSS_ERR_UNSUPPORTED: D or K out of range as above. */
int gss_cacgmm_online(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int D,
                      const gss_guidance *guidance, int K, const gss_em_online *cfg,
                      gss_cacgmm_online_state *state, double *gamma_dev);

/* The model a state stands for: precision = B_k^-1 (both triangles), log_det = ln det B_k,
 * weight = pi_k.  gss_cacgmm_predict with it on a frame gives, to rounding, the posteriors
 * gss_cacgmm_online gives that frame when fed next.  A class whose S_k has no Cholesky factor
 * comes out as the identity (log_det 0) the recursion falls back to, counted where
 * gss_last_cacgmm_online_fallbacks reads.  model_out must not share buffers with the state.
 * GSS_ERR_INVALID: a NULL state, model_out or field, F / K < 1; GSS_ERR_UNSUPPORTED as above. */
int gss_cacgmm_online_model(gss_ctx *ctx, const gss_cacgmm_online_state *state,
                            const gss_cacgmm_model *model_out);

/* (frequency, frame, class) triples of the last online CACGMM on this context that fell back
 * (synchronises). */
int gss_last_cacgmm_online_fallbacks(gss_ctx *ctx, int64_t *count_host);

/* beamform_gev_from_masks (beamforming_wrapper.py:77-89,192-208): masked PSD
 * matrices, principal generalised eigenvector of (Phi_X, Phi_N) with
 * w^H Phi_N w = 1 (phase arbitrary, as upstream), optional BAN, apply.
 * Y (F,T,D), masks (F,T) -> Xhat (T,F). */
int gss_gev(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int D,
            const double *target_mask_dev, const double *distortion_mask_dev,
            int ban, gss_cplx *Xhat_dev);

/* Envelope-variance channel selection (Wolf & Nadeu 2014; not in the reference, whose
 * `multiarray` modes pick microphones by position).  For an STFT Y (F,T,D) and a non-negative
 * band table W (B,F):
 *    E[b,t,d] = sum_f W[b,f] |Y[f,t,d]|^2, floored at floor * max_t E[b,t,d];
 *    C = exp((log E - mean_t log E) / 3);   V[b,d] = mean_t (C - mean_t C)^2 (two passes),
 *    0 where max_t E[b,t,d] == 0;   score[d] = sum_b V[b,d] / max_d' V[b,d'] (a band whose
 *    maximum is 0 contributes 0).
 * Scores lie in [0, B]; a channel that is zero in every frame scores 0.  The `keep` channels of
 * highest score are kept -- equal scores in favour of the lower index, a non-finite score
 * below every finite one -- and reported in ascending channel order.  The library holds no
 * band policy: the host builds W (pb_chime5_amd.ops.mel_bank) as it builds the windows.  The
 * sums have one fixed order (no floating-point atomics): the same call gives the same bits. */
typedef struct {
    const double *bank_dev;  /* (B, F) row-major, >= 0                     */
    int32_t bands;           /* B, 1 .. 64                                  */
    int32_t keep;            /* n, 1 .. D                                   */
    double floor;            /* in [0, 1), finite                           */
} gss_channel_select;

/* Y (F,T,D) -> scores (D) and, unless NULL, the band variances V (B,D).  sel->keep is unread.
 * GSS_ERR_INVALID (the message names the field): sel or bank_dev NULL, bands outside [1, 64],
 * floor negative, >= 1 or not finite. */
int gss_channel_scores(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int D,
                       const gss_channel_select *sel, double *scores_dev,
                       double *band_var_dev);

/* Y (F,T,D) -> Ysel (F,T,n), n = sel->keep: the kept channels in ascending channel order;
 * channels_dev (device int32 (n,), may be NULL) receives their indices.  Asynchronous: n comes
 * from the caller, which channels are kept is decided on the device.  Errors as
 * gss_channel_scores, and keep outside [1, D]. */
int gss_select_channels(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int D,
                        const gss_channel_select *sel, gss_cplx *Ysel_dev,
                        int32_t *channels_dev);

/* The first n channels (ascending) the last gss_select_channels / gss_enhance_observation_select*
 * call on this context kept; synchronises the stream.  GSS_ERR_INVALID when n is smaller than 1
 * or larger than that call's count (0 before any). */
int gss_last_selected_channels(gss_ctx *ctx, int32_t *channels_host, int n);

/* Per-speaker frame activity from the posteriors (not in the reference): the power-weighted share
 * of every frame that the mixture model gives each class.  For Y (F,T,D) -- the signal the EM
 * saw, i.e. after WPE --, gamma (F,K,T) and frequency weights w (F,), NULL = all ones:
 *    p[f,t] = sum_d |Y[f,t,d]|^2;   power[t] = sum_f w[f] p[f,t];
 *    score[k,t] = sum_f w[f] gamma[f,k,t] p[f,t] / power[t],   0 where power[t] is not > 0.
 * Scores lie in [0, 1] up to rounding, are not clamped, and sum to 1 over k wherever the
 * posteriors do and the frame is not digital silence.  Y, gamma -> scores (K,T) and, unless
 * NULL, power (T).  The sums have one fixed order (no floating-point atomics): the same call gives
 * the same bits.  The library holds no policy: what the scores mean for a speaker's activity is
 * decided on the host (pb_chime5_amd.posterior_activity).
 * GSS_ERR_INVALID (the message names the argument), before any launch: Y_dev, gamma_dev or
 * scores_dev NULL, F < 1, T < 1, K outside [1, GSS_MAX_CLASSES], D outside
 * [1, GSS_MAX_CHANNELS].  The weight table is NOT inspected: negative or non-finite weights
 * propagate; the Python layer checks them (pb_chime5_amd.ops.check_freq_weights). */
int gss_posterior_activity(gss_ctx *ctx, const gss_cplx *Y_dev, const double *gamma_dev,
                           int F, int K, int64_t T, int D,
                           const double *freq_weights_dev /* (F,), NULL = ones */,
                           double *scores_dev /* (K,T) */, double *power_dev /* (T,), may be NULL */);

/* Layout helpers between the canonical device layouts and the reference's. */
int gss_layout_dtf_to_ftd(gss_ctx *ctx, const gss_cplx *src_dev, int D, int64_t T,
                          int F, gss_cplx *dst_dev);
int gss_layout_ftd_to_dtf(gss_ctx *ctx, const gss_cplx *src_dev, int F, int64_t T,
                          int D, gss_cplx *dst_dev);
/* (A, B, C) double -> (C, A, B) double, e.g. gamma (F,K,T) -> (K,T,F) with
 * A=F,B=K,C=T ... expressed as a generic 3-D permutation dst[p(i)] = src[i]:
 * perm = 0: (A,B,C)->(B,C,A);  perm = 1: (A,B,C)->(C,A,B);  perm = 2: (A,B)->(B,A)
 * (C = 1). */
int gss_layout_permute_f64(gss_ctx *ctx, const double *src_dev, int64_t A,
                           int64_t B, int64_t C, int perm, double *dst_dev);

/* ---- fused per-utterance pipeline --------------------------------------- */
typedef struct {
    int stft_size;            /* 1024 */
    int stft_shift;           /* 256  */
    int stft_fading;          /* 1    */
    int wpe;                  /* 1 = run WPE                                   */
    int wpe_taps;             /* 10   */
    int wpe_delay;            /* 2    */
    int wpe_iterations;       /* 3    */
    int bss_iterations;       /* 20   */
    int bss_iterations_post;  /* 1    */
    int bf_drop_context;      /* 1    */
    int bf;                   /* 0 = 'mvdrSouden_ban', 1 = 'ch2', 2 = 'sum',   */
                              /* 3 = 'gev_ban' (not in the reference's dispatch) */
    int postfilter;           /* 0 = None, 1 = 'mask_mul'                      */
    int wpe_psd_context;      /* 0: frames either side averaged into the WPE power */
    int wpe_arrays;           /* 0 or 1: one joint WPE over all D channels;        */
                              /* A > 1: WPE per array on D / A channels each, in   */
                              /* array-major channel order (gss_wpe_arrays); A     */
                              /* must divide D (GSS_ERR_INVALID); unread if !wpe   */
} gss_params;

/* Optional taps into the pipeline's intermediates (device pointers; any may be
 * NULL).  This is the `debug=True` contract of the reference blocks
 * (core.py:85-86,210-212,275-276,568-569).  In a gss_enhance_observation_targets* call
 * Obs_ftd, act_frames and gamma are as below; target_mask, distortion_mask, Xhat and
 * ref_channel hold S consecutive per-target blocks of the shape given below ((S,F,T), (S,F,T),
 * (S,T,F), (S,)). */
typedef struct {
    gss_cplx *Obs_ftd;        /* (F,T,D) after WPE                             */
    uint8_t *act_frames;      /* (K,T), the first T frames of the activity     */
    double *gamma;            /* (F,K,T) posteriors before context zeroing     */
    double *target_mask;      /* (F,T)                                         */
    double *distortion_mask;  /* (F,T)                                         */
    gss_cplx *Xhat;           /* (T,F)                                         */
    int32_t *ref_channel;     /* (1,)                                          */
} gss_debug_taps;

/* A0  Enhancer.enhance_observation (core.py:514-571), all intermediates kept in
 * HBM.  obs (D,N) double, act (K,N_act) uint8 in dict order with N_act >= N
 * samples (the reference slices the activity of the reference array, which may be
 * longer than the common length the arrays were cut to, and uses its first T
 * frames: core.py:177-184), target_index = position of speaker_id among the
 * activity keys; start/end_context_samples as computed by
 * start_end_context_frames (core.py:217-222).  out receives
 * gss_istft_num_samples(T,...) samples. */
int gss_enhance_observation(gss_ctx *ctx, const gss_params *params,
                            const double *obs_dev, int D, int64_t N,
                            const uint8_t *act_dev, int K, int64_t N_act,
                            int target_index,
                            int64_t start_context_samples,
                            int64_t end_context_samples,
                            double *out_dev, const gss_debug_taps *taps);

/* gss_enhance_observation guided per STFT frame instead of per sample: the tables of
 * `guidance` cover T = gss_stft_num_frames(N, ...) frames and F = stft_size / 2 + 1
 * frequencies, and replace the time-domain activity and its conversion to frames.  STFT, WPE
 * (joint or per array), beamformer, postfilter, iSTFT and the taps are those of
 * gss_enhance_observation; taps->act_frames must be NULL (there is no frame activity to
 * report).  Errors of the guidance as gss_cacgmm_guided. */
int gss_enhance_observation_guided(gss_ctx *ctx, const gss_params *params,
                                   const double *obs_dev, int D, int64_t N,
                                   const gss_guidance *guidance, int K, int target_index,
                                   int64_t start_context_samples,
                                   int64_t end_context_samples,
                                   double *out_dev, const gss_debug_taps *taps);

/* gss_enhance_observation with the segment-wise beamformer in the place of the whole-window
 * one: the masks (context frames zeroed) go through gss_mvdr_souden_segments with `ban`.
 * Everything else, the debug taps and their shapes included, is gss_enhance_observation's;
 * gss_last_ref_channel and gss_last_segment_fallbacks work afterwards.  params->bf must be 0
 * ('mvdrSouden_ban'): GSS_ERR_UNSUPPORTED otherwise (the phase of a GEV filter is arbitrary per
 * segment).  Errors of `seg` as gss_mvdr_souden_segments. */
int gss_enhance_observation_segments(gss_ctx *ctx, const gss_params *params,
                                     const double *obs_dev, int D, int64_t N,
                                     const uint8_t *act_dev, int K, int64_t N_act,
                                     int target_index,
                                     int64_t start_context_samples,
                                     int64_t end_context_samples,
                                     const gss_bf_segments *seg,
                                     double *out_dev, const gss_debug_taps *taps);

/* gss_enhance_observation with the interferer-nulling LCMV in the place of the MVDR: the
 * posteriors go through gss_lcmv_masks_from_posteriors (context frames zeroed) and the three
 * masks through gss_lcmv_souden with `ban` and lcmv->min_mass, the reference channel chosen.
 * Everything else is gss_enhance_observation's; of the taps, distortion_mask receives I + N
 * (what the postfilter and the reference's locals call the distortion).  gss_last_ref_channel,
 * gss_last_lcmv_interferer and gss_last_lcmv_fallbacks work afterwards.  params->bf must be 0
 * ('mvdrSouden_ban', i.e. ban = 1): GSS_ERR_UNSUPPORTED otherwise.  Errors of `lcmv` as
 * gss_lcmv_masks_from_posteriors, of D as gss_lcmv_souden. */
int gss_enhance_observation_lcmv(gss_ctx *ctx, const gss_params *params,
                                 const double *obs_dev, int D, int64_t N,
                                 const uint8_t *act_dev, int K, int64_t N_act,
                                 int target_index,
                                 int64_t start_context_samples,
                                 int64_t end_context_samples,
                                 const gss_bf_lcmv *lcmv,
                                 double *out_dev, const gss_debug_taps *taps);

/* gss_enhance_observation with the WPD beamformer in the place of the MVDR: STFT -> WPE as
 * configured -> frame activity -> CACGMM -> gss_masks_from_posteriors -> gss_wpd_souden ON THE
 * STFT BEFORE WPE (kept beside the WPE output, which only feeds the mixture model), with the
 * gate 0 on the context frames that bf_drop_context zeroes (NULL without it), `ban` and the
 * other settings from `wpd`, the reference channel chosen -> postfilter -> iSTFT.  The taps
 * keep their meaning: Obs_ftd is the input of the mixture model (after WPE), distortion_mask
 * as in gss_enhance_observation (the WPD does not read it).  gss_last_ref_channel and
 * gss_last_wpd_zero_pivots work afterwards; gss_last_wpe_zero_pivots is the WPE stage's count.
 * params->bf must be 0: GSS_ERR_UNSUPPORTED otherwise.  Errors of `wpd` as gss_wpd_souden. */
int gss_enhance_observation_wpd(gss_ctx *ctx, const gss_params *params,
                                const double *obs_dev, int D, int64_t N,
                                const uint8_t *act_dev, int K, int64_t N_act,
                                int target_index,
                                int64_t start_context_samples,
                                int64_t end_context_samples,
                                const gss_bf_wpd *wpd,
                                double *out_dev, const gss_debug_taps *taps);

/* gss_enhance_observation with gss_wpe_online from a fresh state in the place of the offline WPE:
 * an exponentially forgetting, time-varying dereverberation filter in front of the mixture model
 * and the beamformer.  wpe_taps, wpe_delay and wpe_arrays come from `params`; wpe_iterations is
 * not read.  Everything else, the taps included (Obs_ftd: after the online WPE), is
 * gss_enhance_observation's; gss_last_wpe_zero_pivots reads 0 afterwards (there is no solve).
 * GSS_ERR_INVALID: cfg NULL, alpha outside (0, 1] or not finite, params->wpe == 0,
 * params->wpe_psd_context != 0.  GSS_ERR_UNSUPPORTED: wpe_taps * channels per array > 512. */
typedef struct { double alpha; } gss_wpe_online_cfg;
int gss_enhance_observation_wpe_online(gss_ctx *ctx, const gss_params *params,
                                       const double *obs_dev, int D, int64_t N,
                                       const uint8_t *act_dev, int K, int64_t N_act,
                                       int target_index,
                                       int64_t start_context_samples,
                                       int64_t end_context_samples,
                                       const gss_wpe_online_cfg *cfg,
                                       double *out_dev, const gss_debug_taps *taps);

/* gss_enhance_observation with gss_mvdr_online (BAN on, a fresh state initialised from the window
 * with cfg->loading) in the place of the whole-window beamformer.  cfg->ref_channel is usually -1,
 * the window's.  cfg->wpe_online != 0: gss_wpe_online with cfg->wpe_alpha in the place of the
 * offline WPE as well, as gss_enhance_observation_wpe_online -- the two online stages in one
 * call.  params->bf must be 0.  gss_last_mvdr_online_fallbacks works afterwards.
 * GSS_ERR_INVALID: cfg NULL, the errors of gss_mvdr_online's cfg, params->bf != 0, and with
 * wpe_online those of gss_enhance_observation_wpe_online. */
int gss_enhance_observation_bf_online(gss_ctx *ctx, const gss_params *params,
                                      const double *obs_dev, int D, int64_t N,
                                      const uint8_t *act_dev, int K, int64_t N_act,
                                      int target_index,
                                      int64_t start_context_samples,
                                      int64_t end_context_samples,
                                      const gss_bf_online *cfg,
                                      double *out_dev, const gss_debug_taps *taps);

/* gss_enhance_observation with gss_cacgmm_online (a fresh state of em->prior_mass per call, the
 * mask the call's frame activity) in the place of the guided EM; bss_iterations and
 * bss_iterations_post are not read.  bf == NULL: the whole-window beamformer of params follows.
 * bf != NULL: gss_mvdr_online follows as in gss_enhance_observation_bf_online, and with
 * bf->wpe_online the online WPE precedes -- all three online stages in one call.  The masks and
 * everything downstream are unchanged.
 * GSS_ERR_INVALID: em NULL, forget outside (0, 1] or not finite, prior_mass not finite or <= 0,
 * and with bf the errors of gss_enhance_observation_bf_online.  GSS_ERR_UNSUPPORTED:
 * K > GSS_CACGMM_ONLINE_MAX_CLASSES. */
int gss_enhance_observation_gss_online(gss_ctx *ctx, const gss_params *params,
                                       const double *obs_dev, int D, int64_t N,
                                       const uint8_t *act_dev, int K, int64_t N_act,
                                       int target_index,
                                       int64_t start_context_samples,
                                       int64_t end_context_samples,
                                       const gss_em_online *em, const gss_bf_online *bf,
                                       double *out_dev, const gss_debug_taps *taps);

/* ---- sample-block stream ------------------------------------------------------
 * Samples in, samples out, in blocks of any length, with every state carried by the caller: the
 * offline path with stft_fading = 1 cut at arbitrary sample positions.  (Entry points only, looked
 * up by the binding: revision still 7.)  With W = size and H = shift (H divides W, H < W):
 *    before the first sample the history is W - H zeros (the leading fading pad);
 *    after M samples floor(M / H) frames exist, frame t covers the samples [t H - (W - H), t H + H);
 *    after M samples max(0, floor(M / H) H - (W - H)) output samples have been emitted: the
 *    algorithmic latency is W - H + (M mod H) samples;
 *    the frame activity of frame t is the OR of the activity samples its window covers, clipped to
 *    the samples that exist (gss_activity_time_to_frequency);
 *    every output sample is the sum, started from 0.0, of its frames in ascending t (gss_istft).
 * The caller ends a stream by feeding gss_stream_flush_samples() zeros (no activity) and cutting
 * the output to the M samples that went in; the frames of the flushed stream are exactly those
 * of gss_stft(fading = 1) on the whole signal.  The stream has no utterance context. */
typedef struct {
    double *x_hist;            /* (D, size): the last `size` samples per channel, oldest first */
    uint8_t *act_hist;         /* (K, size): their activity; NULL (and K = 0): an unguided stream */
    double *ola_tail;          /* (size - shift): the partial overlap-add sums the next frames complete */
    int64_t received;          /* samples fed to the analysis side (host counters, advanced by  */
    int64_t frames_out;        /* the calls) and frames taken by the synthesis side             */
    int32_t D, K, size, shift;
} gss_stream_state;            /* caller-owned, like gss_cacgmm_online_state */

typedef struct {
    double wpe_alpha;          /* the forgetting factors of the three online stages */
    double em_forget;
    double bf_forget;
    int32_t ref_channel;       /* >= 0: a stream has no window to choose one over */
} gss_stream_cfg;

/* Pure geometry, no launches.  Frames that n more samples complete after `received`; output
 * samples they finish; zeros that end a stream of `received` samples. */
int64_t gss_stream_num_frames(int64_t received, int64_t n, int size, int shift);
int64_t gss_stream_num_samples_out(int64_t received, int64_t n, int size, int shift);
int64_t gss_stream_flush_samples(int64_t received, int size, int shift);

/* Zeroes the buffers and the counters.  GSS_ERR_INVALID: a NULL state, x_hist or ola_tail,
 * act_hist NULL with K > 0 (or the reverse), size / shift other than gss_set_windows()'s.
 * GSS_ERR_UNSUPPORTED: shift == size, D outside [1, GSS_MAX_CHANNELS], K > GSS_MAX_CLASSES. */
int gss_stream_init(gss_ctx *ctx, gss_stream_state *state);

/* The analysis side.  x (D,n) float64 (in_type 0) or int16 PCM (in_type 1, times 2^-15: the
 * history is float64 either way, so a PCM stream has the bits of the float64 stream of the same
 * values), act (K,n) uint8 or NULL for an unguided stream -> the Tn = gss_stream_num_frames()
 * frames the block completes, Y (F,Tn,D) and act_frames (K,Tn); the state advanced.  The frames
 * have the bits of gss_stft(fading = 1) on the whole signal.  n = 0 is a no-op.
 * GSS_ERR_INVALID before any launch: the errors of gss_stream_init, a NULL pointer, in_type other
 * than 0 / 1, n < 0, act_dev given to an unguided state or missing for a guided one. */
int gss_stft_stream(gss_ctx *ctx, const void *x_dev, int in_type, const uint8_t *act_dev, int64_t n,
                    gss_stream_state *state, gss_cplx *Y_dev, uint8_t *act_frames_dev);

/* The synthesis side.  X (Tn,F), the next Tn frames -> the output samples they finish,
 * gss_stream_num_samples_out() of them (the leading W - H are dropped once); every frame is
 * transformed on its own, so the samples do not depend on where the blocks were cut (gss_istft
 * pairs frames 2b and 2b + 1 in one transform: equal to rounding, not to the bit).  Tn = 0 is a
 * no-op.  GSS_ERR_INVALID: the errors of gss_stream_init, a NULL pointer, Tn < 0, more frames
 * than the analysis side has produced. */
int gss_istft_stream(gss_ctx *ctx, const gss_cplx *X_dev, int64_t Tn, gss_stream_state *state,
                     double *out_dev);

/* One block through the whole front-end, every stage with the caller's state: gss_stft_stream ->
 * gss_wpe_online (params->wpe; wpe_taps, wpe_delay, wpe_arrays from params) -> gss_cacgmm_online
 * with the block's frame activity as the mask (act_dev NULL: no mask, a state made from a model)
 * -> gss_masks_from_posteriors with no frames zeroed -> gss_mvdr_online with BAN -> postfilter ->
 * gss_istft_stream.  out receives gss_stream_num_samples_out() samples; the taps cover the block's
 * Tn frames.  Of params the call reads stft_size, stft_shift, wpe, wpe_taps, wpe_delay, wpe_arrays
 * and postfilter; stft_fading must be 1 and bf 0 (GSS_ERR_UNSUPPORTED).  `wpe` is NULL exactly
 * when params->wpe == 0.  D is the stream state's, K the CACGMM state's.  n = 0 is a no-op.
 * gss_last_mvdr_online_fallbacks, gss_last_cacgmm_online_fallbacks and gss_last_ref_channel work
 * afterwards (a block that completes no frame leaves them).
 * Every argument error returns before any launch, with all four states and `out` untouched:
 * GSS_ERR_INVALID for a NULL pointer, n < 0, a state whose F / D / K differs from the stream's,
 * ref_channel outside [0, D), target_index outside [0, K), a forgetting factor outside (0, 1], a
 * WPE state with params->wpe == 0 or none with params->wpe != 0, and the errors of
 * gss_stft_stream. */
int gss_stream_block(gss_ctx *ctx, const gss_params *params, const gss_stream_cfg *cfg,
                     gss_stream_state *state, const gss_wpe_online_state *wpe,
                     gss_cacgmm_online_state *em, gss_mvdr_online_state *bf, const void *x_dev,
                     int in_type, const uint8_t *act_dev, int64_t n, int target_index,
                     double *out_dev, const gss_debug_taps *taps);

/* ---- several targets of one stream ---------------------------------------------
 * S speakers of one stream from one analysis, one online WPE and one online CACGMM: only the
 * beamformer and the synthesis differ per target.  (Entry points only: revision still 7.)
 *
 * gss_mvdr_online for S targets in one launch, one wave per (frequency, target), the masks formed
 * from the posteriors gamma (F,K,T) as gss_masks_from_posteriors with drop_context = 0 does:
 * target s has the bits of gss_mvdr_online on the masks of class targets[s].  `targets` is a host
 * array of S distinct class indices, `states` a host array of S caller-owned states, each advanced
 * in place.  postfilter = 1: Xhat times the target mask (params->postfilter = 1 of the fused
 * calls).  mask_x_dev / mask_n_dev: (S,F,T), either may be NULL (no mask table exists then);
 * Xhat (S,T,F); W (S,F,T,D) or NULL.  T = 0 is a no-op.  The reference channel is
 * cfg->ref_channel >= 0 (cfg->loading is not read: the states exist).
 * gss_last_mvdr_online_fallbacks_targets gives the fallback frames per target afterwards,
 * gss_last_mvdr_online_fallbacks their sum.
 * GSS_ERR_INVALID before any launch, every state untouched: a NULL table or pointer, S outside
 * [1, GSS_CACGMM_ONLINE_MAX_CLASSES], a target outside [0, K), the same target twice, two states
 * sharing a buffer, a state whose F / D differs from the call's, ref_channel < 0, and the errors
 * of gss_mvdr_online's cfg.  GSS_ERR_UNSUPPORTED: K outside [1, GSS_CACGMM_ONLINE_MAX_CLASSES]. */
int gss_mvdr_online_targets(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int D,
                            const double *gamma_dev, int K, const int32_t *targets, int S, int ban,
                            const gss_bf_online *cfg, const gss_mvdr_online_state *states,
                            int postfilter, double *mask_x_dev, double *mask_n_dev,
                            gss_cplx *Xhat_dev, gss_cplx *W_dev);

/* counts_host[s], s < S: the fallback frames of target s of the last gss_mvdr_online_targets /
 * gss_stream_block_targets call.  GSS_ERR_INVALID: NULL, S outside [1, that call's S]. */
int gss_last_mvdr_online_fallbacks_targets(gss_ctx *ctx, int64_t *counts_host, int S);

/* gss_istft_stream for S signals in one set of launches: X (S,Tn,F) -> out (S,m) with
 * m = gss_stream_num_samples_out(); row s has the bits of gss_istft_stream on X[s].  The
 * overlap-add tails are the caller's buffer tails_dev (S, size - shift), zero at the start of a
 * stream; the state's own ola_tail is neither read nor written, its frames_out advances once.
 * GSS_ERR_INVALID: the errors of gss_istft_stream, tails_dev NULL or the state's ola_tail, S outside
 * [1, GSS_CACGMM_ONLINE_MAX_CLASSES]. */
int gss_istft_stream_targets(gss_ctx *ctx, const gss_cplx *X_dev, int64_t Tn, int S,
                             gss_stream_state *state, double *tails_dev, double *out_dev);

/* gss_stream_block for S targets: its body up to the posteriors, then gss_mvdr_online_targets
 * (BAN, the postfilter in its epilogue, no mask launch) and gss_istft_stream_targets.  `bf` is a
 * host array of S states, tails_dev (S, size - shift) the targets' overlap-add tails, out (S,m).
 * Row s has the bits of gss_stream_block with target_index = targets[s]; the stream, WPE and
 * CACGMM states those of any such call.  Of the taps target_mask, distortion_mask and Xhat hold S
 * consecutive per-target blocks and ref_channel S words, as in gss_enhance_observation_targets.
 * Every argument error returns before any launch, with all states, the tails and `out` untouched:
 * the errors and codes of gss_stream_block, and GSS_ERR_INVALID for those of
 * gss_mvdr_online_targets' targets and states and of gss_istft_stream_targets' tails. */
int gss_stream_block_targets(gss_ctx *ctx, const gss_params *params, const gss_stream_cfg *cfg,
                             gss_stream_state *state, const gss_wpe_online_state *wpe,
                             gss_cacgmm_online_state *em, const gss_mvdr_online_state *bf,
                             double *tails_dev, const void *x_dev, int in_type,
                             const uint8_t *act_dev, int64_t n, const int32_t *targets, int S,
                             double *out_dev, const gss_debug_taps *taps);

/* ---- online MVDR with a filter look-ahead of L frames ----------------------------
 * A fixed lag: frame g is filtered with the filter of frame g + L, which has already seen what
 * follows g -- a speaker's onset above all.  (Entry points only: revision still 7.)  Frames are
 * numbered g = 0, 1, ... over the life of a delay line; w_g is the filter gss_mvdr_online solves at
 * frame g.  The recursion, the fallback rule and BAN are those of gss_mvdr_online, the running
 * sums after any sequence of calls have the bits they have without a look-ahead, and fallback
 * frames are counted when a frame ENTERS.  With G the frames that had entered at the release:
 *    Xhat[g] = w_{min(g + L, G - 1)}^H y_g       (a fallback frame at g + L: Xhat[g] = 0)
 *    the filter row g is w_{min(g + L, G - 1)};  postfilter: times the target mask of frame g
 * A call of T frames on a line that holds h frames (0 <= h <= L) releases max(0, h + T - L)
 * frames, in order, and leaves min(L, h + T) held; gss_mvdr_online_release releases the held
 * frames with the filter of the last frame that entered, empties the line and leaves the sums.
 * The line is the caller's, one per target: every wave reads and writes only its own. */
#define GSS_MVDR_ONLINE_MAX_LOOKAHEAD 64   /* a choice: one second at 16 kHz / 256 */
typedef struct {
    gss_cplx *frames;          /* (F, L, D): the held frames, oldest first */
    double *mask;              /* (F, L): their target-mask values (read by the postfilter) */
    gss_cplx *filter;          /* (F, D): the filter of the last frame that entered */
    int32_t F, D, L;
    int32_t held;              /* host counter, advanced by the calls: frames held, 0 .. L */
} gss_mvdr_online_hold;        /* caller-owned; separate from gss_mvdr_online_state */

/* Zeroes the three buffers and `held`.  GSS_ERR_INVALID: a NULL hold or buffer, F < 1, L outside
 * [1, GSS_MVDR_ONLINE_MAX_LOOKAHEAD].  GSS_ERR_UNSUPPORTED: D outside [1, GSS_MAX_CHANNELS]. */
int gss_mvdr_online_hold_init(gss_ctx *ctx, gss_mvdr_online_hold *hold);

/* gss_mvdr_online with the look-ahead hold->L.  `state` is required (a line outlives a call, so
 * there is no thrown-away state).  Xhat (F,R) and W (F,R,D) or NULL with
 * R = max(0, hold->held + T - hold->L) rows, which *frames_out receives (it may be NULL).  T = 0 is
 * a no-op.  GSS_ERR_INVALID before any launch, the state and the line untouched: the errors of
 * gss_mvdr_online, a NULL state or hold or hold buffer, hold->F / D other than F / D, hold->L
 * outside [1, GSS_MVDR_ONLINE_MAX_LOOKAHEAD], hold->held outside [0, hold->L],
 * cfg->ref_channel = -1 (the whole-window choice is per call). */
int gss_mvdr_online_lookahead(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int D,
                              const double *mask_x_dev, const double *mask_n_dev, int ban,
                              const gss_bf_online *cfg, gss_mvdr_online_state *state,
                              gss_mvdr_online_hold *hold, gss_cplx *Xhat_dev, gss_cplx *W_dev,
                              int64_t *frames_out);

/* gss_mvdr_online_targets with a look-ahead: `holds` is a host array of S lines of one L and one
 * `held`, no buffer shared.  Row s has the bits of gss_mvdr_online_lookahead on the masks of class
 * targets[s]; the postfilter multiplies by the target mask of the OUTPUT frame.  Xhat (S,R,F),
 * W (S,F,R,D) or NULL; mask_x_dev / mask_n_dev (S,F,T) or NULL: the masks of the call's T frames.
 * The errors of gss_mvdr_online_targets and of gss_mvdr_online_lookahead's hold. */
int gss_mvdr_online_lookahead_targets(gss_ctx *ctx, const gss_cplx *Y_dev, int F, int64_t T, int D,
                                      const double *gamma_dev, int K, const int32_t *targets,
                                      int S, int ban, const gss_bf_online *cfg,
                                      const gss_mvdr_online_state *states,
                                      gss_mvdr_online_hold *holds, int postfilter,
                                      double *mask_x_dev, double *mask_n_dev, gss_cplx *Xhat_dev,
                                      gss_cplx *W_dev, int64_t *frames_out);

/* The end of S lines (S = 1: the line of gss_mvdr_online_lookahead): the h = holds[0].held frames
 * with the last filter -> Xhat (S,h,F), W (S,F,h,D) or NULL; *frames_out = h.  Nothing held:
 * nothing is launched.  GSS_ERR_INVALID: the hold errors above, Xhat_dev NULL with h > 0,
 * postfilter other than 0 / 1. */
int gss_mvdr_online_release(gss_ctx *ctx, gss_mvdr_online_hold *holds, int S, int postfilter,
                            gss_cplx *Xhat_dev, gss_cplx *W_dev, int64_t *frames_out);

/* gss_stream_block_targets (S >= 1) with a look-ahead: its body up to the posteriors, then
 * gss_mvdr_online_lookahead_targets (BAN, the postfilter in its epilogue) and the synthesis of the
 * frames released -- with `release` != 0 also gss_mvdr_online_release and the synthesis of the
 * frames it releases: the last block of a stream.  out (S,m): the m samples those frames finish,
 * counted from state->frames_out, which *samples_out receives (it may be NULL; the caller sizes
 * `out` for gss_stream_num_samples_out() of the block plus, with `release`, L * shift more).  n = 0
 * with `release` only ends the lines.  The taps target_mask, distortion_mask, gamma and Obs_ftd
 * cover the block's frames, Xhat the frames released (S consecutive blocks).  The errors and
 * codes of gss_stream_block_targets and of gss_mvdr_online_lookahead_targets' holds. */
int gss_stream_block_lookahead(gss_ctx *ctx, const gss_params *params, const gss_stream_cfg *cfg,
                               gss_stream_state *state, const gss_wpe_online_state *wpe,
                               gss_cacgmm_online_state *em, const gss_mvdr_online_state *bf,
                               gss_mvdr_online_hold *holds, double *tails_dev, const void *x_dev,
                               int in_type, const uint8_t *act_dev, int64_t n,
                               const int32_t *targets, int S, int release, double *out_dev,
                               int64_t *samples_out, const gss_debug_taps *taps);

/* gss_enhance_observation plus gss_posterior_activity on the pipeline's own post-WPE observation
 * and its posteriors before context zeroing (what the taps Obs_ftd and gamma show), nothing
 * copied: scores (K,T) and, unless NULL, power (T) with T = gss_stft_num_frames(N, ...);
 * freq_weights (stft_size / 2 + 1,) or NULL for ones, not inspected.  `out` and every tap have the
 * bits of gss_enhance_observation.
 * GSS_ERR_INVALID (the message names the argument), before any launch: params, obs_dev, act_dev,
 * out_dev or scores_dev NULL, N < 1, K outside [1, GSS_MAX_CLASSES], D outside
 * [1, GSS_MAX_CHANNELS]; then the errors of gss_enhance_observation. */
int gss_enhance_observation_activity(gss_ctx *ctx, const gss_params *params,
                                     const double *obs_dev, int D, int64_t N,
                                     const uint8_t *act_dev, int K, int64_t N_act,
                                     int target_index,
                                     int64_t start_context_samples,
                                     int64_t end_context_samples,
                                     const double *freq_weights_dev,
                                     double *out_dev, double *scores_dev, double *power_dev,
                                     const gss_debug_taps *taps);

/* gss_enhance_observation on the sel->keep channels the envelope-variance measure ranks best:
 * the STFT runs on all D channels, then scores, pick and gather, then the unchanged pipeline
 * (WPE, frame activity, CACGMM, masks, beamformer, postfilter, iSTFT) on n = sel->keep
 * channels.  The limits of the pipeline apply to n (D < 30 of the MVDR / GEV, the CACGMM's
 * D >= 2), D itself is limited by GSS_MAX_CHANNELS only.  With keep == D the gather is skipped
 * and the output and every tap equal gss_enhance_observation bit for bit.  Taps: Obs_ftd is
 * (F,T,n) and ref_channel an index into the kept channels (so is gss_last_ref_channel
 * afterwards; gss_last_selected_channels maps it back); the others are unchanged.
 * GSS_ERR_INVALID for a bad `sel` as gss_select_channels; GSS_ERR_UNSUPPORTED for
 * params->wpe_arrays > 1 (a selection breaks the equal arrays of the per-array WPE) and
 * params->bf == 1 ('ch2' names a physical channel). */
int gss_enhance_observation_select(gss_ctx *ctx, const gss_params *params,
                                   const double *obs_dev, int D, int64_t N,
                                   const uint8_t *act_dev, int K, int64_t N_act,
                                   int target_index,
                                   int64_t start_context_samples,
                                   int64_t end_context_samples,
                                   const gss_channel_select *sel,
                                   double *out_dev, const gss_debug_taps *taps);

/* The same fed with 16-bit PCM, as gss_enhance_observation_pcm16. */
int gss_enhance_observation_select_pcm16(gss_ctx *ctx, const gss_params *params,
                                         const int16_t *obs_dev, int D, int64_t N,
                                         const uint8_t *act_dev, int K, int64_t N_act,
                                         int target_index,
                                         int64_t start_context_samples,
                                         int64_t end_context_samples,
                                         const gss_channel_select *sel,
                                         double *out_dev, const gss_debug_taps *taps);

/* Same pipeline fed with the 16-bit PCM samples as they sit in the WAV files: the
 * conversion of the reference's loader, float64(sample) / 2^15 (io/audioread.py:34-226 via
 * soundfile), happens inside the STFT kernel -- bit-identical, a quarter of the H2D bytes and
 * no float64 copy of the recording on the host. */
int gss_enhance_observation_pcm16(gss_ctx *ctx, const gss_params *params,
                                  const int16_t *obs_dev, int D, int64_t N,
                                  const uint8_t *act_dev, int K, int64_t N_act,
                                  int target_index,
                                  int64_t start_context_samples,
                                  int64_t end_context_samples,
                                  double *out_dev, const gss_debug_taps *taps);

/* S targets of one window from one separation: STFT, WPE and the guided CACGMM run once, then
 * the target-dependent tail (masks, PSD, beamformer, postfilter, iSTFT) for all S targets
 * together.  target_index[s] in [0, K), distinct, 1 <= S <= K (host arrays);
 * start/end_context_samples[s]: the contexts of target s (host arrays, as in
 * gss_enhance_observation).  out (S, gss_istft_num_samples(T, ...)) row-major.  Row s equals
 * gss_enhance_observation(..., target_index[s], start_context_samples[s],
 * end_context_samples[s], ...) bit for bit, and so does each per-target block of the debug
 * taps.  Bad S or indices (duplicates, out of range) give GSS_ERR_INVALID.  A target whose
 * beamformer fails gets NaN (its status word says why, gss_last_ref_channels); the others
 * finish.  gss_last_ref_channel afterwards reports target 0. */
int gss_enhance_observation_targets(gss_ctx *ctx, const gss_params *params,
                                    const double *obs_dev, int D, int64_t N,
                                    const uint8_t *act_dev, int K, int64_t N_act, int S,
                                    const int32_t *target_index,
                                    const int64_t *start_context_samples,
                                    const int64_t *end_context_samples, double *out_dev,
                                    const gss_debug_taps *taps);

/* The same fed with 16-bit PCM, as gss_enhance_observation_pcm16. */
int gss_enhance_observation_targets_pcm16(gss_ctx *ctx, const gss_params *params,
                                          const int16_t *obs_dev, int D, int64_t N,
                                          const uint8_t *act_dev, int K, int64_t N_act, int S,
                                          const int32_t *target_index,
                                          const int64_t *start_context_samples,
                                          const int64_t *end_context_samples, double *out_dev,
                                          const gss_debug_taps *taps);

/* Annotation-free separation of one window in one call: STFT, the joint offline WPE of
 * `params`, the CACGMM with a frequency-shared prior from init_dev (K,T) -- no mask,
 * params->bss_iterations iterations and one post iteration, what gss_cacgmm_shared_prior runs
 * for (iterations, 1) --, the frame power of gss_posterior_activity, then the target-dependent
 * tail of gss_enhance_observation_targets with S = K (target s = class s, no context frames,
 * the beamformer of `params`) and K iSTFTs.  obs_dev (D,N) float64; out_dev
 * (K, gss_istft_num_samples(T, ...)); prior_dev (K,T) the prior of the last M-step; power_dev (T,)
 * or NULL; gamma_dev (F,K,T) or NULL the posteriors.  taps as in the targets call (act_frames
 * must be NULL: there is no frame activity).  The name does not begin with
 * gss_enhance_observation: the call has no activity, no target index and K outputs.
 * GSS_ERR_INVALID: a NULL params, obs_dev, init_dev, out_dev or prior_dev, N < 1, and what the
 * stages reject.  GSS_ERR_UNSUPPORTED: params->wpe_arrays > 1 with WPE on (the per-array WPE).
 * The online WPE, the channel selection, the segment-wise, LCMV and WPD beamformers are options
 * of entries of their own and have no form here. */
int gss_separate_observation(gss_ctx *ctx, const gss_params *params, const double *obs_dev,
                             int D, int64_t N, const double *init_dev, int K, double *out_dev,
                             double *prior_dev, double *power_dev, double *gamma_dev,
                             const gss_debug_taps *taps);

/* Same, with host buffers: copies in, runs, copies out, synchronises. */
int gss_enhance_observation_host(gss_ctx *ctx, const gss_params *params,
                                 const double *obs_host, int D, int64_t N,
                                 const uint8_t *act_host, int K, int64_t N_act,
                                 int target_index,
                                 int64_t start_context_samples,
                                 int64_t end_context_samples,
                                 double *out_host);

/* Bytes of context workspace the last call needed (diagnostics / sizing). */
size_t gss_workspace_bytes(gss_ctx *ctx);

/* Workspace debug mode, for tests (off for a new context; it synchronises, never use it in a
 * product run).  pattern 0..255 switches it on, -1 off.  While it is on
 *  - the context's workspace is filled with the byte `pattern` at the start of every call and
 *    again whenever a fused call hands the workspace of one stage to the next,
 *  - every block gss_dev_malloc returns is filled with it,
 *  - every workspace block is followed by a guard of at least 256 bytes of it, compared with the
 *    pattern when the block is released, at the start of the next call and by the report below.
 * A kernel that reads workspace or output memory before writing it sees the pattern (0xFF: NaN as
 * a double, -1 as an integer) instead of whatever the previous call left there; one that writes
 * behind its block breaks a guard.  Results, launches and gss_workspace_bytes() of a context with
 * the mode off are those of a library without it.  Switching (in either direction) clears the
 * record of violations. */
int gss_debug_workspace(gss_ctx *ctx, int pattern);

/* Checks the guards that are still live (synchronises) and returns the number of violated guards
 * since the mode was switched on, and in buf (len bytes, may be NULL) a text naming the first:
 * block index, tag, offset and size of the block.  guard_dev (may be NULL) receives the device
 * address of live guard `guard_index` (0 = behind the first block of the last call), NULL when
 * there is none; the address lies inside the workspace allocation.  GSS_ERR_INVALID when the mode
 * is off. */
int gss_debug_workspace_report(gss_ctx *ctx, int64_t *violations, char *buf, int len,
                               int guard_index, void **guard_dev);

/* Device self-test of the f64 MFMA fragment layout the WPE kernel relies on;
 * returns 0 when the layout matches. */
int gss_selftest_mfma(gss_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* GSS_HIP_H */
