"""The interferer-nulling LCMV beamformer (Souden, Benesty, Affes 2010, eq. 51) in plain NumPy
(DESIGN.md section 15): the reference of tests/test_lcmv_api.py and tests/test_gpu_lcmv.py.
Nothing is imported from the oracle or the package.  Not a test module."""
import numpy as np

EPS = 1e-10


def psd(Yf, mask):
    """Yf (F,D,T), mask (F,T) -> Phi (F,D,D) = sum_t m y y^H / max(sum_t m, 1e-10)."""
    mask = np.asarray(mask, np.float64)
    S = np.einsum('ft,fdt,fet->fde', mask, Yf, Yf.conj())
    return S / np.maximum(mask.sum(-1), EPS)[:, None, None]


def solve(A, B):
    """solve(A, B) of one frequency; the minimum-norm lstsq answer where A is exactly singular."""
    try:
        return np.linalg.solve(A, B)
    except np.linalg.LinAlgError:
        return np.linalg.lstsq(A, B, rcond=None)[0]


def lcmv_matrix(phi_x, phi_i, phi_n, eps=EPS):
    """One frequency: W (D,D) whose column r is the filter for reference channel r, and gamma."""
    AB = solve(phi_n, np.concatenate([phi_i, phi_x], axis=1))
    D = phi_n.shape[0]
    A, B = AB[:, :D], AB[:, D:]
    g_in = np.trace(A)
    g = g_in * np.trace(B) - np.trace(A @ B)
    return (g_in * B - A @ B) / max(g.real, eps), g


def mvdr_matrix(phi_x, phi_d, eps=EPS):
    """One frequency of the Souden MVDR: Psi / max(Re tr Psi, eps), Psi = solve(Phi_D, Phi_X)."""
    psi = solve(phi_d, phi_x)
    return psi / max(np.trace(psi).real, eps)


def explicit_lcmv(d, a, phi_n, r):
    """The textbook LCMV Phi_N^-1 C (C^H Phi_N^-1 C)^-1 g, C = [d a], g = [conj(d_r), 0]."""
    C = np.stack([d, a], axis=1)
    PiC = np.linalg.solve(phi_n, C)
    return PiC @ np.linalg.solve(C.conj().T @ PiC, np.array([d[r].conj(), 0.0]))


def filters(Yf, X_mask, I_mask, N_mask, min_mass=0.0):
    """Yf (F,D,T), masks (F,T) -> W (F,D,D), Phi_X, Phi_D (F,D,D), fallbacks (F,) bool, Phi_N
    (F,D,D) (the matrix each frequency factored), gamma (F,) (NaN on the fallback)."""
    Xm, Im, Nm = (np.asarray(m, np.float64) for m in (X_mask, I_mask, N_mask))
    F, D, _ = Yf.shape
    phi_x, phi_i, phi_n = psd(Yf, Xm), psd(Yf, Im), psd(Yf, Nm)
    fall = Im.sum(-1) < min_mass
    S_d = np.einsum('ft,fdt,fet->fde', Im, Yf, Yf.conj()) + \
        np.einsum('ft,fdt,fet->fde', Nm, Yf, Yf.conj())
    merged = S_d / np.maximum(Im.sum(-1) + Nm.sum(-1), EPS)[:, None, None]
    W = np.empty((F, D, D), np.complex128)
    phi_d = phi_i + phi_n
    factored = phi_n.copy()
    gamma = np.full(F, np.nan)
    for f in range(F):
        if fall[f]:
            phi_d[f] = factored[f] = merged[f]
            W[f] = mvdr_matrix(phi_x[f], merged[f])
        else:
            W[f], g = lcmv_matrix(phi_x[f], phi_i[f], phi_n[f])
            gamma[f] = g.real
    return W, phi_x, phi_d, fall, factored, gamma


def reference_channel(W, phi_x, phi_d, eps=EPS):
    """argmax over r of sum_f w_r^H Phi_X w_r / max(sum_f w_r^H Phi_D w_r, eps); AssertionError
    on a non-finite SNR."""
    num = np.einsum('fdr,fde,fer->r', W.conj(), phi_x, W)
    den = np.einsum('fdr,fde,fer->r', W.conj(), phi_d, W)
    snr = num / np.maximum(den, eps)
    assert np.all(np.isfinite(snr)), snr
    return int(np.argmax(snr.real))


def ban(w, phi_d):
    """Blind analytic normalisation, the reference's four-operand einsum; eps = 0."""
    nominator = np.abs(np.sqrt(np.einsum('...a,...ab,...bc,...c->...', w.conj(), phi_d, phi_d, w)))
    denominator = np.abs(np.einsum('...a,...ab,...b->...', w.conj(), phi_d, w))
    with np.errstate(invalid='ignore', divide='ignore'):
        return w * (nominator / denominator)[..., None]


def lcmv_souden_from_masks(Y, X_mask, I_mask, N_mask, ban_=False, min_mass=0.0, ref_channel=None):
    """Y (D,T,F), masks (T,F) -> X_hat (T,F), details (ref_channel, fallbacks (F,) bool, w (F,D),
    phi_n (F,D,D), gamma (F,))."""
    Yf = np.asarray(Y).transpose(2, 0, 1)
    W, phi_x, phi_d, fall, phi_n, gamma = filters(
        Yf, np.asarray(X_mask).T, np.asarray(I_mask).T, np.asarray(N_mask).T, min_mass)
    if ref_channel is None:
        ref_channel = reference_channel(W, phi_x, phi_d)
    w = W[:, :, ref_channel]
    if ban_:
        w = ban(w, phi_d)
    X_hat = np.einsum('fd,fdt->tf', w.conj(), Yf)
    return X_hat, dict(ref_channel=int(ref_channel), fallbacks=fall, w=w, phi_n=phi_n,
                       gamma=gamma)


def mvdr_souden_from_masks(Y, X_mask, N_mask, ban_=False, ref_channel=None):
    """The Souden MVDR of the same conventions (what the fallback branch must equal)."""
    zero = np.zeros_like(np.asarray(X_mask, np.float64))
    return lcmv_souden_from_masks(Y, X_mask, zero, N_mask, ban_, np.inf, ref_channel)


def zero_context(masks, start, end):
    """masks (..., T, F): the Python-slice rule of the context zeroing, on a copy."""
    masks = np.array(masks, np.float64)
    masks[..., :start, :] = 0
    if end > 0:
        masks[..., -end:, :] = 0
    return masks


def class_masses(posterior, start=0, end=0, drop_context=True):
    """posterior (K,T,F) -> (K,) masses over the frames the context zeroing keeps."""
    g = zero_context(posterior, start, end) if drop_context else np.asarray(posterior, np.float64)
    return g.sum(axis=(1, 2))


def pick_interferer(posterior, target, candidates, start=0, end=0, drop_context=True):
    """The candidate class (the target is none) of largest mass, equal masses to the lower
    index; -1 without a candidate or when the largest mass is 0."""
    mass = class_masses(posterior, start, end, drop_context)
    best, found = 0.0, -1
    for k in sorted(set(candidates)):
        if k != target and mass[k] > best:
            best, found = mass[k], k
    return found


def masks_from_posteriors(posterior, target, interferer, start=0, end=0, drop_context=True):
    """posterior (K,T,F) -> X, I, N (T,F): the target's and the interferer's posteriors (zeros
    for -1) and the remaining classes added in ascending k, context frames zeroed."""
    g = zero_context(posterior, start, end) if drop_context else np.asarray(posterior, np.float64)
    K = g.shape[0]
    I = g[interferer].copy() if interferer >= 0 else np.zeros_like(g[0])
    N = np.zeros_like(g[0])
    for k in range(K):
        if k != target and k != interferer:
            N = N + g[k]
    return g[target].copy(), I, N


def crandn(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)


def scene(rng, D, T, F, noise=0.3):
    """Y (D,T,F) and soft masks X, I, N (T,F) from the true powers: target and interferer are
    point sources with random steering vectors and on / off envelopes, the diffuse noise a
    random D x D mixing of D white sources.  Also the steering vectors d, a (F,D) and the
    envelopes' activity (F,T) bool."""
    d, a = crandn(rng, F, D), crandn(rng, F, D)
    on_x, on_i = rng.random((F, T)) < 0.5, rng.random((F, T)) < 0.4
    sx, si = crandn(rng, F, T) * on_x, crandn(rng, F, T) * on_i
    n = np.einsum('fde,fte->ftd', crandn(rng, F, D, D), crandn(rng, F, T, D)) * noise
    Y = (sx[..., None] * d[:, None] + si[..., None] * a[:, None] + n).transpose(2, 1, 0)
    px, pi, pn = np.abs(sx) ** 2, np.abs(si) ** 2, np.full((F, T), noise ** 2 * D)
    tot = px + pi + pn
    return Y, (px / tot).T, (pi / tot).T, (pn / tot).T, dict(d=d, a=a, on_x=on_x, on_i=on_i)
