"""The envelope-variance channel selection (Wolf & Nadeu 2014) in NumPy float64 (DESIGN.md
section 13): the definition of the measure and the reference of tests/test_gpu_channel_select.py
and tests/test_channel_select_api.py.  Not a test module.

For an STFT Y (F,T,D) and a non-negative band table W (B,F):

 1. band energy      E[b,t,d] = sum_f W[b,f] |Y[f,t,d]|^2
 2. floor            m[b,d] = max_t E;  E <- max(E, floor * m);  (b,d) is dead when m == 0
 3. log envelope     L = log E - mean_t log E
 4. compression      C = exp(L / 3)
 5. variance         V[b,d] = mean_t (C - mean_t C)^2 (two passes), 0 where (b,d) is dead
 6. score            score[d] = sum_b V[b,d] / max_d' V[b,d'] (a band whose maximum is 0
                     contributes 0)
"""
import numpy as np


def mel_bank(bands, stft_size, sample_rate=16000):
    """(B, F) triangular filters equally spaced on the HTK mel scale between 0 and
    sample_rate / 2, F = stft_size // 2 + 1: filter b rises linearly from edge b to edge b + 1
    and falls to edge b + 2, evaluated at the bin centre frequencies."""
    F = stft_size // 2 + 1
    top = 2595.0 * np.log10(1.0 + (sample_rate / 2.0) / 700.0)
    mel = np.linspace(0.0, top, bands + 2)
    edges = 700.0 * (10.0 ** (mel / 2595.0) - 1.0)
    freqs = np.arange(F) * (sample_rate / stft_size)
    W = np.zeros((bands, F))
    for b in range(bands):
        lo, mid, hi = edges[b], edges[b + 1], edges[b + 2]
        W[b] = np.maximum(0.0, np.minimum((freqs - lo) / (mid - lo), (hi - freqs) / (hi - mid)))
    return W


def band_energies(Y_ftd, W):
    """Y (F,T,D), W (B,F) -> E (B,T,D)."""
    power = Y_ftd.real ** 2 + Y_ftd.imag ** 2
    return np.einsum('bf,ftd->btd', np.asarray(W, np.float64), power)


def band_variances(Y_ftd, W, floor=1e-10, dtype=np.float64):
    """Y (F,T,D), W (B,F) -> V (B,D).  ``dtype=np.longdouble`` repeats steps 2 - 5 in extended
    precision (the reference's own rounding error)."""
    E = band_energies(Y_ftd, W).astype(dtype)
    m = E.max(axis=1, keepdims=True)
    dead = m[:, 0, :] == 0
    E = np.maximum(E, dtype(floor) * m)
    with np.errstate(divide='ignore', invalid='ignore'):
        logE = np.log(E)
        L = logE - logE.mean(axis=1, keepdims=True)
        C = np.exp(L / dtype(3))
        V = ((C - C.mean(axis=1, keepdims=True)) ** 2).mean(axis=1)
    return np.where(dead, dtype(0), V)


def scores_from_variances(V):
    """V (B,D) -> scores (D,)."""
    V = np.asarray(V)
    top = V.max(axis=1, keepdims=True)
    with np.errstate(divide='ignore', invalid='ignore'):
        contribution = np.where(top > 0, V / top, 0)
    return contribution.sum(axis=0)


def channel_scores(Y_ftd, W, floor=1e-10, dtype=np.float64):
    """Y (F,T,D), W (B,F) -> (scores (D,), V (B,D))."""
    V = band_variances(Y_ftd, W, floor, dtype)
    return scores_from_variances(V), V


def pick(scores, keep):
    """The ``keep`` channels of highest score in ascending channel order: equal scores go to the
    lower channel index, a non-finite score ranks below every finite one."""
    scores = np.asarray(scores, np.float64)
    finite = np.isfinite(scores)
    order = sorted(range(len(scores)),
                   key=lambda d: (not finite[d], -scores[d] if finite[d] else 0.0, d))
    return np.array(sorted(order[:keep]), dtype=int)


def boundary_gap(scores, keep):
    """Relative gap between the last kept and the first dropped score (inf when all are kept)."""
    s = np.sort(np.asarray(scores, np.float64))[::-1]
    if keep >= len(s):
        return np.inf
    return float((s[keep - 1] - s[keep]) / max(abs(s[keep - 1]), np.finfo(float).tiny))


def select(Y_ftd, W, keep, floor=1e-10):
    """-> (Y[:, :, channels], channels)."""
    channels = pick(channel_scores(Y_ftd, W, floor)[0], keep)
    return Y_ftd[:, :, channels], channels


def random_bank(rng, B, F):
    """A dense non-negative band table for scenes whose F is no STFT size: overlapping
    triangles over the F bins plus a small dense part (every weight is read)."""
    centres = np.linspace(0, F - 1, B + 2)[1:-1]
    width = max((F - 1) / (B + 1), 1.0) * 1.5
    W = np.maximum(0.0, 1.0 - np.abs(np.arange(F)[None, :] - centres[:, None]) / width)
    return W + 0.01 * rng.uniform(size=(B, F))


def scene(D, T, F):
    """The test scenes, Y (F,T,D): a sparse gated source s (T,F) seen by D channels of
    different reverberation (a one-pole recursion over frames, acc <- alpha_d acc + s[t] *
    random phase, scaled by sqrt(1 - alpha_d^2)), noise level sigma_d and gain 10^U(-2, 2);
    alpha a permutation of linspace(0.2, 0.95, D), sigma of geomspace(0.01, 0.5, D)."""
    rng = np.random.default_rng(D * 7 + T)
    gate = (rng.uniform(size=(T, 1)) < 0.35) * (rng.uniform(size=(T, F)) < 0.6)
    s = gate * (rng.standard_normal((T, F)) + 1j * rng.standard_normal((T, F)))
    alpha = rng.permutation(np.linspace(0.2, 0.95, D))
    sigma = rng.permutation(np.geomspace(0.01, 0.5, D))
    Y = np.empty((F, T, D), np.complex128)
    for d in range(D):
        phase = np.exp(2j * np.pi * rng.uniform(size=(T, F)))
        acc = np.zeros(F, np.complex128)
        x = np.empty((T, F), np.complex128)
        for t in range(T):
            acc = alpha[d] * acc + s[t] * phase[t]
            x[t] = acc
        x *= np.sqrt(1.0 - alpha[d] ** 2)
        x += sigma[d] * (rng.standard_normal((T, F)) + 1j * rng.standard_normal((T, F)))
        Y[:, :, d] = (x * 10.0 ** rng.uniform(-2, 2)).T
    return Y
