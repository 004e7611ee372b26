"""The segment-wise MVDR-Souden beamformer as a NumPy composition of the oracle's functions
(DESIGN.md section 12): the reference of tests/test_gpu_segments.py.  Not a test module."""
import numpy as np

import gss_oracle as oracle


def segment_windows(T, L, c):
    """[(segment frames [a, b), statistics window frames [lo, hi))] for the B segments."""
    B = -(-T // L)
    out = []
    for b in range(B):
        lo = max(0, b - c) * L
        hi = min(T, (min(B - 1, b + c) + 1) * L)
        out.append(((b * L, min(T, (b + 1) * L)), (lo, hi)))
    return out


def window_masses(X_mask, N_mask, L, c):
    """Masks (T,F) -> (B, F, 2): the target and distortion mask sums of every window."""
    Xm, Nm = np.asarray(X_mask, np.float64).T, np.asarray(N_mask, np.float64).T
    return np.array([[Xm[:, lo:hi].sum(-1), Nm[:, lo:hi].sum(-1)]
                     for _, (lo, hi) in segment_windows(Xm.shape[1], L, c)]).transpose(0, 2, 1)


def mass_margin(X_mask, N_mask, L, c, min_mass):
    """The smallest relative distance of a window mass from the fallback threshold."""
    if min_mass == 0:
        return np.inf
    return float(np.min(np.abs(window_masses(X_mask, N_mask, L, c) - min_mass)) / min_mass)


def mvdr_souden_segments(Y, X_mask, N_mask, ban, L, c=0, min_mass=None, ref_channel=None):
    """Y (D,T,F), masks (T,F) -> X_hat (T,F), details (ref_channel, fallbacks (B,F) bool,
    cov_x / cov_n (B,F,D,D) after the fallback, w (B,F,D))."""
    Yf = np.asarray(Y).transpose(2, 0, 1)
    Xm, Nm = np.asarray(X_mask, np.float64).T, np.asarray(N_mask, np.float64).T
    F, D, T = Yf.shape
    if min_mass is None:
        min_mass = 2 * D
    windows = segment_windows(T, L, c)
    B = len(windows)
    whole_x = oracle.get_power_spectral_density_matrix(Yf, Xm)
    whole_n = oracle.get_power_spectral_density_matrix(Yf, Nm)
    cov_x = np.empty((B, F, D, D), np.complex128)
    cov_n = np.empty((B, F, D, D), np.complex128)
    fallbacks = np.zeros((B, F), bool)
    for b, (_, (lo, hi)) in enumerate(windows):
        cov_x[b] = oracle.get_power_spectral_density_matrix(Yf[..., lo:hi], Xm[:, lo:hi])
        cov_n[b] = oracle.get_power_spectral_density_matrix(Yf[..., lo:hi], Nm[:, lo:hi])
        fall = np.minimum(Xm[:, lo:hi].sum(-1), Nm[:, lo:hi].sum(-1)) < min_mass
        cov_x[b, fall] = whole_x[fall]
        cov_n[b, fall] = whole_n[fall]
        fallbacks[b] = fall
    # one reference channel: get_optimal_reference_channel on the (B F, D, D) stacks
    w, ref = oracle.get_mvdr_vector_souden(
        cov_x.reshape(B * F, D, D), cov_n.reshape(B * F, D, D), ref_channel=ref_channel,
        eps=1e-10, return_ref_channel=True)
    if ban:
        w = oracle.blind_analytic_normalization(w, cov_n.reshape(B * F, D, D))
    w = w.reshape(B, F, D)
    X_hat = np.empty((T, F), np.complex128)
    for b, ((a, e), _) in enumerate(windows):
        X_hat[a:e] = oracle.apply_beamforming_vector(w[b], Yf[..., a:e]).T
    return X_hat, dict(ref_channel=int(ref), fallbacks=fallbacks, cov_x=cov_x, cov_n=cov_n, w=w)
