"""The WPD convolutional beamformer (Nakatani & Kinoshita 2019; Boeddeker et al. 2020) in plain
NumPy on top of oracle.gss_oracle: the reference of tests/test_wpd_api.py
and tests/test_gpu_wpd.py, in two forms -- the factorised definition (one WPE step with the
target-power weights, then a weighted-power MPDR on the result) and the direct solve of the stacked
(taps + 1) D system -- with the scene generator and the orthogonality invariant.  Nothing is
imported from the package.  Not a test module."""
import numpy as np

import gss_oracle as o

EPS = 1e-10
POWER_FLOOR = 1e-3

# (D, T, F, taps, delay): the smallest D; an odd D; the production tap window at 12 and 24
# channels (the 32 x 32 correlation tiles, T >= 2 (taps + 1) D at D = 24 so that the stacked
# system of the direct form is well determined); D = 29, the largest the MVDR takes; one array.
# No T is a multiple of a frame tile except 600 and 200 (64-frame chunks end inside them).
STAGE_SCENES = [(2, 70, 3, 2, 1), (5, 130, 4, 3, 2), (12, 333, 3, 10, 2), (24, 600, 2, 10, 2),
                (29, 200, 2, 2, 2), (4, 200, 3, 10, 2)]


def crandn(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)


def scene(rng, D, T, F, taps, delay, noise=0.1):
    """Y (D,T,F), the soft target mask (T,F) clipped at 1e-10 and a frame gate (T,) with nonzero
    context on both sides: a sparse target and a sparse interferer, each reverberant over
    delay + taps + 2 frames with decaying random taps, and white sensor noise."""
    s = crandn(rng, F, T) * (rng.random((F, T)) < 0.5)
    i = crandn(rng, F, T) * (rng.random((F, T)) < 0.5)
    L = delay + taps + 2
    hs = crandn(rng, F, D, L) * 0.6 ** np.arange(L)
    hi = crandn(rng, F, D, L) * 0.6 ** np.arange(L)
    Yf = noise * crandn(rng, F, D, T)
    for l in range(L):
        Yf[:, :, l:] += hs[:, :, l, None] * s[:, None, :T - l] + hi[:, :, l, None] * i[:, None, :T - l]
    ps, pi = np.abs(s) ** 2, np.abs(i) ** 2
    mask = np.clip((ps + 1e-3) / (ps + pi + 0.1), 1e-10, 1)
    gate = np.ones(T)
    gate[:7] = 0
    gate[-5:] = 0
    return np.ascontiguousarray(Yf.transpose(1, 2, 0)), np.ascontiguousarray(mask.T), gate


def weights(p, gate, floor=POWER_FLOOR):
    """p (F,T) power, gate (T,) -> a (F,T) = gate / max(p, floor * max over gated frames of p);
    all zero at a frequency whose gated maximum is 0."""
    gate = np.asarray(gate, np.float64)
    with np.errstate(invalid='ignore'):
        pmax = np.max(np.where(gate > 0, p, 0.0), axis=-1, keepdims=True)
        live = pmax > 0
        lam = np.maximum(p, floor * pmax)
        return np.where(live & (gate > 0), 1.0 / np.where(live & (lam > 0), lam, 1.0), 0.0)


def masked_power(Yf, mask_f):
    """Yf (F,D,T), mask (F,T) -> mask * mean_d |Y|^2."""
    return mask_f * np.mean(np.abs(Yf) ** 2, axis=1)


def wpe_step(Yf, a, taps, delay):
    """One WPE step with the weights a (F,T): Yf (F,D,T) -> Z (F,D,T), G [F] (taps D, D)."""
    Z = np.empty_like(Yf)
    Gs = []
    for f in range(Yf.shape[0]):
        Yt = o.build_y_tilde(Yf[f], taps, delay)
        R = (Yt * a[f]) @ Yt.conj().T
        P = (Yt * a[f]) @ Yf[f].conj().T
        G = o.stable_solve(R, P)
        Gs.append(G)
        Z[f] = Yf[f] - G.conj().T @ Yt
    return Z, Gs


def wpd_souden_from_masks(Y, X_mask, ban=False, *, taps=10, delay=2, iterations=1,
                          power_floor=POWER_FLOOR, frame_gate=None, ref_channel=None):
    """The factorised definition.  Y (D,T,F), X_mask (T,F) -> X_hat (T,F), details of the last
    iteration (a (F,T), Z (F,D,T), w (F,D), ref_channel, phi_a (F,D,D))."""
    Yf = np.asarray(Y).transpose(2, 0, 1)
    m = np.asarray(X_mask, np.float64).T
    F, D, T = Yf.shape
    assert D < 30, (D, Yf.shape)
    gate = np.ones(T) if frame_gate is None else (np.asarray(frame_gate) != 0).astype(np.float64)
    mg = m * gate
    p = masked_power(Yf, m)
    for _ in range(iterations):
        a = weights(p, gate, power_floor)
        Z, _ = wpe_step(Yf, a, taps, delay)
        phi_x = o.get_power_spectral_density_matrix(Z, mg)
        phi_a = o.get_power_spectral_density_matrix(Z, a)
        w, ref = o.get_mvdr_vector_souden(phi_x, phi_a, ref_channel=ref_channel, eps=EPS,
                                          return_ref_channel=True)
        if ban:
            w = o.blind_analytic_normalization(w, phi_a)
        out = o.apply_beamforming_vector(w, Z)
        p = np.abs(out) ** 2
    return out.T, dict(a=a, Z=Z, w=w, ref_channel=int(ref), phi_a=phi_a)


def direct(Y, X_mask, a, taps, delay, ref_channel, frame_gate=None):
    """The direct form of one iteration with given weights a (F,T) and reference channel: the
    stacked observation yb = [y; yt], Rb = sum a yb yb^H, E = [I; 0],
    C = Rb^-1 E (E^H Rb^-1 E)^-1 (= [I; -G]), S = (E^H Rb^-1 E)^-1 / max(sum a, 1e-10) (= Phi_a),
    Souden on (C^H Phib_X C, S), filter C w on yb.  No BAN.  -> X_hat (T,F)."""
    Yf = np.asarray(Y).transpose(2, 0, 1)
    m = np.asarray(X_mask, np.float64).T
    F, D, T = Yf.shape
    gate = np.ones(T) if frame_gate is None else (np.asarray(frame_gate) != 0).astype(np.float64)
    out = np.empty((F, T), np.complex128)
    for f in range(F):
        Yb = np.vstack([Yf[f], o.build_y_tilde(Yf[f], taps, delay)])
        Rb = (Yb * a[f]) @ Yb.conj().T
        mg = m[f] * gate
        phib_x = (Yb * mg) @ Yb.conj().T / max(mg.sum(), EPS)
        E = np.zeros((Yb.shape[0], D))
        E[:D] = np.eye(D)
        RiE = np.linalg.solve(Rb, E)
        S = np.linalg.inv(E.T @ RiE)
        C = RiE @ S
        phi = np.linalg.solve(S / max(a[f].sum(), EPS), C.conj().T @ phib_x @ C)
        W = phi / max(np.trace(phi).real, EPS)
        out[f] = (C @ W[:, ref_channel]).conj() @ Yb
    return out.T


def orthogonality(Y, a, X_hat, taps, delay):
    """rho = max_f ||sum_t a_t yt_t conj(xhat_t)|| / sqrt(sum a ||yt||^2 * sum a |xhat|^2): the
    output of the WPD is orthogonal to the tap window under the weights a (the normal equations
    of its WPE step, which the instantaneous filter w cannot undo); WPE with other weights
    followed by an MVDR leaves a correlation.  Y (D,T,F), a (F,T), X_hat (T,F)."""
    Yf = np.asarray(Y).transpose(2, 0, 1)
    xf = np.asarray(X_hat).T
    rho = []
    for f in range(Yf.shape[0]):
        Yt = o.build_y_tilde(Yf[f], taps, delay)
        num = np.linalg.norm((Yt * a[f]) @ xf[f].conj())
        den = np.sqrt((np.abs(Yt) ** 2 * a[f]).sum() * (np.abs(xf[f]) ** 2 * a[f]).sum())
        rho.append(num / den)
    return float(max(rho))


def context_gate(T, start, end):
    """The frame gate of a window with ``start`` / ``end`` context frames: the Python-slice rule
    of the context zeroing (masks[:start] = 0; if end > 0: masks[-end:] = 0)."""
    gate = np.ones(T)
    gate[:start] = 0
    if end > 0:
        gate[-end:] = 0
    return gate


def masks_from_posteriors(posterior, target, start=0, end=0, drop_context=True):
    """posterior (K,T,F) -> target mask, distortion mask (T,F), context frames zeroed."""
    g = np.array(posterior, np.float64)
    if drop_context:
        g *= context_gate(g.shape[1], start, end)[None, :, None]
    return g[target].copy(), np.sum(np.delete(g, target, axis=0), axis=0)
