"""NumPy references for the model calls (gss_cacgmm_fit / gss_cacgmm_predict), built on the
untouched oracle: scenes, the oracle's models in the public dense form, and the log-likelihood
on top of ``CACGMM._log_pdf``.  Every oracle fit is computed once per session and shared."""
import functools

import numpy as np

import gss_oracle as oracle
from test_gpu_stages import _scene

# (D, T, F, K, iterations): the oracle's model of the head of these scenes has no eigenvalue at
# the floor ...
NONFLOORED = [(6, 200, 3, 3, 5), (4, 330, 3, 3, 5), (4, 700, 2, 5, 4), (2, 130, 3, 2, 4),
              (8, 300, 2, 9, 4), (12, 333, 3, 5, 8), (20, 520, 2, 4, 4), (24, 900, 2, 5, 4)]
# ... and this one has 7
FLOORED = (24, 650, 2, 3, 4)
FLOOR = 1e-10


def head_frames(T):
    """'Fit on the head': a ragged, different frame count for predict."""
    return (2 * T // 3) // 64 * 64


@functools.lru_cache(maxsize=None)
def scene(D, T, F, K):
    """Y (D,T,F), activity (K,T) bool -- seeded as in test_gpu_guided.py.  Read-only."""
    rng = np.random.default_rng(D + T + K)
    Y, act = _scene(rng, D, T, F, K)
    Y.setflags(write=False)
    act.setflags(write=False)
    return Y, act


def to_ftd(Y):
    return np.ascontiguousarray(Y.transpose(2, 1, 0))


@functools.lru_cache(maxsize=None)
def oracle_fit(D, T, F, K, iterations, frames=None, start=0):
    """The oracle's CACGMMTrainer.fit on `frames` frames from `start` (None: all) from the GSS
    initialisation of the activity, masked."""
    Y, act = scene(D, T, F, K)
    stop = T if frames is None else start + frames
    init, mask = oracle.gss_initialization(act[:, start:stop])
    return oracle.CACGMMTrainer().fit(to_ftd(Y[:, start:stop]), init[None], iterations=iterations,
                                      source_activity_mask=mask[None])


def dense(model):
    """oracle.CACGMM -> (precision (F,K,D,D), log_det (F,K), weight (F,K))."""
    return (model._inverse_covariance(), model.log_determinant,
            np.ascontiguousarray(model.weight[..., 0]))


def floored_eigenvalues(model):
    return int(np.sum(model.covariance_eigenvalues <= FLOOR))


def mask_fkt(act, F):
    return np.repeat(np.asarray(act, bool)[None], F, axis=0)


def log_likelihood(model, Y, mask=None):
    """ln sum_k pi_k m_kt exp(-D ln q_kt - ln det B_k) per frame -> (T,F): the oracle's
    ``CACGMM._log_pdf`` on the unit-normalised frames, the weights and the mask in the log
    domain, max-shifted.  Y (D,T,F); mask (F,K,T) bool or None."""
    log_pdf, _ = model._log_pdf(oracle.normalize_observation(to_ftd(Y)))       # (F,K,T)
    w = np.broadcast_to(model.weight, log_pdf.shape).copy()
    if mask is not None:
        w = w * mask
    with np.errstate(divide='ignore'):
        terms = log_pdf + np.log(w)
    mx = np.max(terms, axis=-2, keepdims=True)
    safe = np.where(np.isfinite(mx), mx, 0.0)
    with np.errstate(divide='ignore'):
        ll = safe[..., 0, :] + np.log(np.sum(np.exp(terms - safe), axis=-2))
    return ll.T
