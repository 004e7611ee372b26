"""The CACGMM E-step of two builds of libgss_hip.so: the same bits?

    python tools/cmp_em_bits.py OTHER_LIBRARY          (on a GPU box)

OTHER_LIBRARY is another build of the library, the parent commit's when a change to the E-step
kernels or to the pieces they share (csrc/cacgmm_estep.h) must not move a bit.  Every case runs
once under each library, each in a process of its own (cmp_bits.py); every output is compared
byte for byte.  All cases are small (F <= 9, T <= 200 and no multiple of 64, a few iterations):
  per-frequency EM   gss_cacgmm and the guided call at D = 7 (LDS form), 24, 20, 12, 10 and 4,
                     K = 2, 3, 4, 6 and 9 (LDS form), masked and unmasked post steps, from a mask
                     only and from an initialisation array; D = 4 also under GSS_VARIANT=em_unfused
                     (the multi-launch kernels) and estep_lds; estep_wpb=1 and estep_wpb=4
  shared-prior EM    D = 24, 12, 4 and 7, register and LDS form, blind and from a mask
  model calls        cacgmm_fit / cacgmm_predict / cacgmm_log_likelihood at D = 24 and D = 5
  fused pipeline     enhance_observation, once
  digital silence    a block with one all-zero frame: the max(|q|, tiny) clamp
  log-form fall-back a predict under a hand-made model (D = 24, K = 2, precisions I and 1e12 I,
                     ln det 0 and -800): every term of the ratio form is <= 1e-288, so every
                     frame takes the branch `sum < 1e-280` (checked here in numpy first)
Exit status 1 when an array differs."""
import os
import sys
sys.path.insert(0, '.')
import numpy as np
from cmp_bits import main


def crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def scene(D, T, F, K):
    """K - 1 point sources + diffuse noise and their (K,T) activities (the last class always on)."""
    rng = np.random.default_rng([D, T, F, K])
    act = np.zeros((K, T), bool)
    act[-1] = True
    Y = 0.1 * crandn(rng, D, T, F)
    for k in range(K - 1):
        a = int(rng.integers(0, T // 2))
        b = int(rng.integers(a + T // 4, T))
        act[k, a:b] = True
        Y += crandn(rng, D, 1, F) * crandn(rng, 1, T, F) * act[k][None, :, None]
    return Y, act


class variant:
    """GSS_VARIANT for the calls inside (the library reads it per call, as in the tests); None: as it is.
    The caller's own value comes back afterwards."""

    def __init__(self, text):
        self.text = text

    def __enter__(self):
        self.before = os.environ.get('GSS_VARIANT')
        if self.text:
            os.environ['GSS_VARIANT'] = self.text

    def __exit__(self, *exc):
        if self.before is None:
            os.environ.pop('GSS_VARIANT', None)
        else:
            os.environ['GSS_VARIANT'] = self.before


def fallback_model(T, F):
    """The hand-made model of the log-form fall-back and frames for it."""
    from pb_chime5_amd.cacgmm import CACGMM
    D, K = 24, 2
    Y = crandn(np.random.default_rng(24), D, T, F)
    precision = np.zeros((F, K, D, D), complex)
    precision[:, 0] = np.eye(D)
    precision[:, 1] = 1e12 * np.eye(D)
    log_det = np.tile([0.0, -800.0], (F, 1))
    weight = np.tile([0.4, 0.6], (F, 1))
    # the ratio form in numpy: (q_min / q_k)^D pi_k exp(ln det_min - ln det_k), every frame
    yn = Y / np.linalg.norm(Y, axis=0, keepdims=True)
    q = np.abs(np.einsum('dtf,fkde,etf->fkt', yn.conj(), precision, yn))
    terms = (q.min(axis=1, keepdims=True) / q) ** D * (weight * np.exp(log_det.min(axis=1, keepdims=True) - log_det))[:, :, None]
    assert terms.max() <= 1e-288 and np.all(terms.sum(axis=1) < 1e-280), terms.max()
    return CACGMM(precision, log_det, weight), Y


def cases():
    from pb_chime5_amd import ops, synthetic
    out = {}

    # ---- per-frequency EM: em_estep_kernel (FIRST always; EM / PREDICT at D = 7 and K = 9),
    # em_estep_reg_kernel, and at D = 4 em_onchip4_kernel
    for (D, T, F, K) in ((7, 130, 5, 3), (7, 100, 3, 9), (24, 200, 9, 4), (24, 70, 3, 2), (20, 150, 4, 6),
                         (12, 199, 4, 3), (10, 90, 3, 2), (4, 200, 6, 4), (4, 130, 3, 6), (12, 100, 2, 9)):
        Y, act = scene(D, T, F, K)
        init, mask = ops.guidance_from_activity(act)
        rng = np.random.default_rng(K)
        soft = init * rng.uniform(0.5, 1.5, size=init.shape)
        out[f'gss_cacgmm {D} {K} post=1'] = ops.cacgmm_posteriors(Y, act, 3, 1)
        out[f'gss_cacgmm {D} {K} post=0'] = ops.cacgmm_posteriors(Y, act, 3, 0)      # masked predict
        out[f'guided mask only {D} {K}'] = ops.cacgmm_posteriors_guided(Y, None, mask, 3, 1)
        out[f'guided init array {D} {K}'] = ops.cacgmm_posteriors_guided(Y, soft, None, 3, 1)
        out[f'guided init + mask {D} {K}'] = ops.cacgmm_posteriors_guided(Y, soft, mask, 2, 0)
        if D == 4:
            for text in ('em_unfused', 'estep_lds', 'em_unfused,estep_lds'):
                with variant(text):
                    out[f'gss_cacgmm {D} {K} {text}'] = ops.cacgmm_posteriors(Y, act, 3, 1)
                    out[f'guided init {D} {K} {text}'] = ops.cacgmm_posteriors_guided(Y, soft, mask, 3, 0)
        if (D, K) == (24, 4):
            for wpb in (1, 4):
                with variant(f'estep_wpb={wpb}'):
                    out[f'gss_cacgmm {D} {K} estep_wpb={wpb}'] = ops.cacgmm_posteriors(Y, act, 3, 1)

    # ---- shared-prior EM: em_estep_prior_kernel (FIRST always), its register form
    for (D, T, F, K) in ((24, 130, 4, 3), (12, 100, 5, 4), (4, 199, 6, 2), (7, 90, 3, 3), (7, 70, 2, 8)):
        Y, act = scene(D, T, F, K)
        for text in (None, 'estep_lds'):
            with variant(text):
                g, p = ops.cacgmm_posteriors_blind(Y, K, 3, seed=D, return_prior=True)
                out[f'shared prior blind {D} {K} {text}'], out[f'shared prior blind {D} {K} {text} prior'] = g, p
                out[f'shared prior mask {D} {K} {text}'] = ops.cacgmm_posteriors_shared_prior(Y, None, act, 3, 1)
                out[f'shared prior mask {D} {K} {text} post=0'] = ops.cacgmm_posteriors_shared_prior(Y, None, act, 2, 0)

    # ---- the model calls: fit, refit, predict, log-likelihood (cacgmm_loglik_kernel)
    for (D, T, F, K) in ((24, 130, 3, 3), (5, 100, 4, 2), (5, 70, 2, 7)):
        Y, act = scene(D, T, F, K)
        model = ops.cacgmm_fit(Y[:, :90], None, act[:, :90], 3)
        model = ops.cacgmm_fit(Y[:, :90], None, act[:, :90], 1, model=model)
        for k, v in (('precision', model.precision), ('log_det', model.log_determinant), ('weight', model.weight)):
            out[f'fit {D} {K} {k}'] = v
        for name, m in (('masked', act), ('unmasked', None)):
            g, ll = ops.cacgmm_predict(model, Y, m, log_likelihood=True)
            out[f'predict {D} {K} {name}'], out[f'predict {D} {K} {name} loglik'] = g, ll
            out[f'log_likelihood {D} {K} {name}'] = ops.cacgmm_log_likelihood(model, Y, m)

    # ---- the fused pipeline
    u = synthetic.tiny(seed=46, num_channels=6, num_samples=19200, num_speakers=3, context=2048, noise=3e-2)
    out['enhance_observation'] = ops.enhance_observation(u.obs, u.activity_array, u.target_index, 2048, 2048,
                                                         wpe=True, wpe_taps=4, bss_iterations=5)

    # ---- one frame of digital silence: the clamp max(|q|, tiny)
    for (D, T, F, K) in ((12, 130, 3, 3), (4, 130, 3, 3), (7, 130, 3, 3)):
        Y, act = scene(D, T, F, K)
        Y = Y.copy()
        Y[:, 77] = 0.0
        out[f'silent frame {D}'] = ops.cacgmm_posteriors(Y, act, 3, 1)
        out[f'silent frame {D} shared prior'] = ops.cacgmm_posteriors_shared_prior(Y, None, act, 3, 1)

    # ---- the log-form fall-back of the ratio posterior
    model, Y = fallback_model(70, 3)
    out['log-form fall-back'] = ops.cacgmm_predict(model, Y)
    return out


main(__file__, __doc__, cases)
