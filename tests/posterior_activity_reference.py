"""The posterior activity, written down in NumPy: what gss_posterior_activity computes.

For an observation Y (F,T,D) complex128 -- the signal the EM saw, i.e. after WPE --, posteriors
gamma (F,K,T) float64 and frequency weights w (F,) >= 0 (None: all ones):

    p[f,t]     = sum_d |Y[f,t,d]|^2
    power[t]   = sum_f w[f] * p[f,t]
    num[k,t]   = sum_f w[f] * gamma[f,k,t] * p[f,t]
    score[k,t] = num[k,t] / power[t]   if power[t] > 0 else 0.0

score[k,t] is the power-weighted share of frame t that the model gives class k.  It lies in
[0, 1] up to rounding, sums to 1 over k wherever the posteriors do and the frame is not digital
silence, and is not clamped.

Rounding.  Every sum is of non-negative terms, so in ANY summation order its relative error is at
most about (n - 1) 2^-53 with n = 2 F D terms (re^2 and im^2 of every bin) plus a few roundings
per term (the squares, the two products).  Two float64 implementations therefore agree to
`bar(F, D)` relative, for scores and power alike; the bar is derived, not measured.
"""
import numpy as np


def posterior_activity(Y, gamma, w=None):
    """Y (F,T,D), gamma (F,K,T), w (F,) or None -> scores (K,T), power (T,)."""
    Y = np.asarray(Y, dtype=np.complex128)
    gamma = np.asarray(gamma, dtype=np.float64)
    F, T, D = Y.shape
    assert gamma.shape[0] == F and gamma.shape[2] == T, (Y.shape, gamma.shape)
    w = np.ones(F) if w is None else np.asarray(w, dtype=np.float64)
    assert w.shape == (F,) and np.all(w >= 0), w
    p = np.sum(Y.real ** 2 + Y.imag ** 2, axis=-1)                   # (F,T)
    power = np.sum(w[:, None] * p, axis=0)                           # (T,)
    num = np.sum(w[:, None, None] * gamma * p[:, None, :], axis=0)   # (K,T)
    scores = np.zeros_like(num)
    live = power > 0
    scores[:, live] = num[:, live] / power[live]
    return scores, power


def bar(F, D):
    """The relative bar between two float64 evaluations (see the module docstring)."""
    return 4 * (2 * F * D + 8) * 2.0 ** -53


def scene(D, T, F, K, seed=None):
    """A seeded observation (F,T,D) with a spread of frame powers and normalised posteriors
    (F,K,T) with exact zeros in them."""
    rng = np.random.default_rng(1000 * D + 10 * T + F + K if seed is None else seed)
    Y = rng.standard_normal((F, T, D)) + 1j * rng.standard_normal((F, T, D))
    Y *= 10.0 ** rng.uniform(-2, 2, size=(F, T, 1))
    g = rng.uniform(size=(F, K, T)) ** 3
    if K > 1:
        g[rng.uniform(size=g.shape) < 0.2] = 0.0
        g[:, 0, :] += 1e-3                  # (no frame without mass)
    gamma = g / np.sum(g, axis=1, keepdims=True)
    return Y, gamma


def weights(F, seed=0):
    """Random non-negative weights with zeros among them (at least one weight is positive)."""
    rng = np.random.default_rng(77 + F + seed)
    w = rng.uniform(0.0, 2.0, size=F)
    w[rng.uniform(size=F) < 0.3] = 0.0
    w[rng.integers(F)] = 1.5
    return w


# ------------------------------------------------------------------ a scene with a known truth
TRUTH = dict(num_samples=32000, annotated=(4000, 28000), spoken=(4000, 16000),
             interferer=(8000, 30000), seed=11)
TRUTH_PARAMS = dict(wpe_taps=4, wpe_iterations=2, bss_iterations=10)


def truth_scene(num_channels=4):
    """Two speakers and noise; the target is ANNOTATED over TRUTH['annotated'] but its source
    is zero after TRUTH['spoken'] (a loose diariser segment).  Returns the synthetic utterance
    (its activity is the annotation) and the frames (size 1024, shift 256, fading) whose whole
    window lies inside the spoken part / inside the silent annotated part, the latter starting
    one window after the source stops so that its reverberation has died away."""
    from pb_chime5_amd import synthetic
    n = TRUTH['num_samples']
    u = synthetic.make_utterance(TRUTH['seed'], num_channels, n,
                                 [TRUTH['spoken'], TRUTH['interferer']], rir_taps=512,
                                 noise=3e-2)
    annotated = np.zeros(n, bool)
    annotated[slice(*TRUTH['annotated'])] = True
    u.activity['P01'] = annotated
    T = 1 + -(-(n + 2 * 768 - 1024) // 256)      # frames of the padded, faded STFT
    first = 256 * np.arange(T) - 768             # first sample of frame t
    spoken = (first >= TRUTH['spoken'][0]) & (first + 1024 <= TRUTH['spoken'][1])
    silent = (first >= TRUTH['spoken'][1] + 1024) & (first + 1024 <= TRUTH['annotated'][1])
    return u, spoken, silent
