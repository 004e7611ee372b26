"""NumPy reference of the online MVDR (gss_mvdr_online): the frame recursion as DESIGN.md section 23
writes it -- Souden's mask-based MVDR on exponentially forgetting running sums, a filter per frame,
the fallback rule of LAPACK's Cholesky --, the closed form of the two sums, and the scenes the CPU
and the GPU tests share.  Every reference run is computed once per session and shared, read-only."""
import functools

import numpy as np

TOL = 1e-10                 # relative to the largest magnitude of the compared array: X, W, Phi_X, Phi_N
STABILITY_MARGIN = 100.0    # the reference itself must move at least this much less than the bar
CLOSED_FORM_TOL = 1e-9
X_TOL = 1e-4                # |x_hat| rel err of the end-to-end tests (tests/test_gpu_pipeline.py)
EPS = 1e-10                 # the eps of the reference's wrapper around get_mvdr_vector_souden


def loading_delta(Y, loading):
    """delta_f = loading * p_f; p_f the mean of |Y[f]|^2 over frames and channels, 1 where there
    are no frames or that mean is exactly 0.  Y (F,T,D)."""
    F = Y.shape[0]
    if Y.shape[1] == 0:
        return np.full(F, float(loading))
    p = np.mean(np.abs(Y) ** 2, axis=(1, 2))
    return loading * np.where(p == 0, 1.0, p)


def fresh_state(F, D, loading, Y=None):
    delta = loading_delta(Y, loading) if Y is not None else np.full(F, float(loading))
    phi_n = np.zeros((F, D, D), np.complex128)
    phi_n[:, np.arange(D), np.arange(D)] = delta[:, None]
    return dict(phi_x=np.zeros((F, D, D), np.complex128), phi_n=phi_n)


def copy_state(state):
    return {k: v.copy() for k, v in state.items()}


def _has_cholesky(phi_n):
    """Per frequency: LAPACK's rule (a pivot <= 0 or NaN fails)."""
    try:
        np.linalg.cholesky(phi_n)
        return np.ones(len(phi_n), bool)
    except np.linalg.LinAlgError:
        pass
    ok = np.ones(len(phi_n), bool)
    for f, m in enumerate(phi_n):
        try:
            np.linalg.cholesky(m)
        except np.linalg.LinAlgError:
            ok[f] = False
    return ok


def online_mvdr(Y, mx, mn, beta, ref, ban=False, state=None, loading=None):
    """Y (F,T,D), masks (F,T) -> X (F,T), the filters W (F,T,D), the state after the T frames and
    the number of fallback frames.  ``state``: where to start, not modified; None: fresh, from Y
    with ``loading``.  The loop over the frames is the recursion, vectorised over frequencies."""
    Y = np.asarray(Y, np.complex128)
    F, T, D = Y.shape
    st = copy_state(state) if state is not None else fresh_state(F, D, loading, Y)
    phi_x, phi_n = st['phi_x'], st['phi_n']
    X = np.zeros((F, T), np.complex128)
    W = np.zeros((F, T, D), np.complex128)
    fallbacks = 0
    eye = np.eye(D)
    for t in range(T):
        y = Y[:, t]
        yy = y[:, :, None] * y.conj()[:, None, :]
        phi_x = beta * phi_x + mx[:, t, None, None] * yy
        phi_n = beta * phi_n + mn[:, t, None, None] * yy
        ok = _has_cholesky(phi_n)
        fallbacks += int(np.sum(~ok))
        if not ok.any():
            continue
        safe = np.where(ok[:, None, None], phi_n, eye)
        psi = np.linalg.solve(safe, phi_x)
        tr = np.real(np.trace(psi, axis1=-2, axis2=-1))
        w = psi[:, :, ref] / np.maximum(tr, EPS)[:, None]
        if ban:
            # oracle.blind_analytic_normalization with eps = 0; a filter that is exactly zero
            # (no target mass yet: the context frames of every window) stays zero
            v = np.einsum('fde,fe->fd', safe, w)
            nom = np.sqrt(np.real(np.einsum('fd,fd->f', v.conj(), v)))
            den = np.abs(np.einsum('fd,fd->f', w.conj(), v))
            with np.errstate(invalid='ignore', divide='ignore'):
                w = w * np.where(den == 0, 0.0, nom / den)[:, None]
        w = np.where(ok[:, None], w, 0)
        W[:, t] = w
        X[:, t] = np.einsum('fd,fd->f', w.conj(), y)
    return X, W, dict(phi_x=phi_x, phi_n=phi_n), fallbacks


def closed_form(Y, mx, mn, beta, delta):
    """Phi_X and Phi_N after the T frames of Y from a fresh state, from Y, the masks, beta and
    delta (F,) alone."""
    Y = np.asarray(Y, np.complex128)
    F, T, D = Y.shape
    g = beta ** (T - 1 - np.arange(T))
    phi_x = np.einsum('ft,ftd,fte->fde', g * mx, Y, Y.conj())
    phi_n = np.einsum('ft,ftd,fte->fde', g * mn, Y, Y.conj())
    phi_n[:, np.arange(D), np.arange(D)] += (beta ** T * np.asarray(delta))[:, None]
    return phi_x, phi_n


def rel_err(a, b):
    """max |a - b| relative to the largest magnitude of b."""
    a, b = np.asarray(a), np.asarray(b)
    scale = float(np.max(np.abs(b))) if b.size else 0.0
    return float(np.max(np.abs(a - b))) / scale if scale > 0 else float(np.max(np.abs(a), initial=0.0))


def to_ftd(Obs):
    return np.ascontiguousarray(np.asarray(Obs).transpose(2, 1, 0))


def to_dtf(Y):
    return np.ascontiguousarray(np.asarray(Y).transpose(2, 1, 0))


# ------------------------------------------------------------------ parity scenes
# (D, beta, loading, F, T); each runs with ban False and True and with ref_channel 0 and D - 1
CELLS = [
    (4, 0.99, 1e-2, 3, 150),
    (1, 0.9, 1.0, 1, 5),
    (2, 1.0, 1.0, 2, 70),           # no forgetting
    (3, 0.95, 1.0, 2, 90),          # odd D
    (7, 0.99, 1.0, 2, 100),         # the sweep's 8-lane grid
    (8, 0.99, 1.0, 2, 64),
    (9, 0.99, 1.0, 2, 64),
    (16, 0.99, 1.0, 2, 64),
    (17, 0.99, 1.0, 2, 64),
    (24, 0.995, 1.0, 2, 120),
    (29, 0.99, 1.0, 2, 80),
    (32, 0.999, 1.0, 1, 64),        # the bound
    (24, 0.995, 1.0, 2, 1),         # T = 1
    (4, 0.5, 1.0, 2, 100),
    (4, 0.9, 1.0, 2, 300),          # where a recursion that carries the inverse falls apart
]
CLOSED_FORM_CELLS = [(4, 0.99, 1e-2, 3, 150), (2, 1.0, 1.0, 2, 70)]
CHUNK_CELLS = [(4, 0.99, 1e-2, 3, 150), (24, 0.995, 1.0, 2, 120)]
CHUNKS = {150: (1, 63, 64, 22), 120: (1, 57, 56, 6)}
EVIDENCE_CELL = (4, 0.95, 1e-2, 8, 300)
EVIDENCE_BOUND = 0.8        # a condition, not a measurement
# seed of every cell whose seed 0 did not pass: a seed is kept only if the reference's own X, W and
# state move at least STABILITY_MARGIN x less than TOL when every sample and mask value moves in
# its last bit, for both values of ban and both reference channels (`python
# tests/online_mvdr_reference.py` re-derives the table).
SEEDS = {(4, 0.5, 1.0, 2, 100): 1}
EVIDENCE_SEED = 0           # the seed rule for it: the ratio of the reference is <= 0.75
# Long horizons, the same format, variants and seed rule (LONG_SEEDS: the seeds that are not 0):
#    (4, 0.99, 1e-2, 2, 6000): 0,   # moves 4.4e-14, cond(Phi_N) 5.5e+02
#    (24, 0.995, 1.0, 1, 3000): 0,   # moves 5.0e-13, cond(Phi_N) 6.7e+03
LONG_CELLS = [(4, 0.99, 1e-2, 2, 6000), (24, 0.995, 1.0, 1, 3000)]
LONG_BLOCK = 625
LONG_SEEDS = {}


def long_blocks(T):
    return (LONG_BLOCK,) * (T // LONG_BLOCK) + ((T % LONG_BLOCK,) if T % LONG_BLOCK else ())


def crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


@functools.lru_cache(maxsize=None)
def scene(cell, seed=0):
    """Two sources with random complex steering vectors, the target's drifting linearly from one
    random vector to another over the T frames; each source is complex white noise that is
    active in a random 60 % of the (f, t) points; sensor noise of standard deviation 0.1 per real
    part.  -> Y (F,T,D), mx, mn (F,T) and the target's image (F,T,D), read-only."""
    D, beta, loading, F, T = cell
    rng = np.random.default_rng([seed, D, F, T])
    a0, a1, a2 = crandn(rng, F, D), crandn(rng, F, D), crandn(rng, F, D)
    ramp = (np.arange(T) / max(T - 1, 1))[None, :, None]
    steer = a0[:, None, :] * (1 - ramp) + a1[:, None, :] * ramp           # (F,T,D)
    s1 = crandn(rng, F, T) * (rng.random((F, T)) < 0.6)
    s2 = crandn(rng, F, T) * (rng.random((F, T)) < 0.6)
    image = steer * s1[:, :, None]
    Y = image + a2[:, None, :] * s2[:, :, None] + 0.1 * crandn(rng, F, T, D)
    p1, p2 = np.abs(s1) ** 2, np.abs(s2) ** 2
    mx = (p1 + 1e-3) / (p1 + p2 + 0.05 + 1e-3)
    mn = 1 - mx
    for a in (Y, mx, mn, image):
        a.setflags(write=False)
    return Y, mx, mn, image


def last_bit(a, rng):
    a = np.asarray(a)
    if a.dtype.kind == 'c':
        return last_bit(a.real, rng) + 1j * last_bit(a.imag, rng)
    return a * (1 + (rng.integers(0, 2, a.shape) * 2 - 1) * 2.0 ** -52)


def seed_of(cell):
    return LONG_SEEDS.get(cell, 0) if cell in LONG_CELLS else SEEDS.get(cell, 0)


def variants(cell):
    """(ban, ref_channel) of a cell."""
    D = cell[0]
    return [(ban, ref) for ban in (False, True) for ref in sorted({0, D - 1})]


@functools.lru_cache(maxsize=None)
def reference(cell, ban, ref, seed=0):
    D, beta, loading, F, T = cell
    Y, mx, mn, _ = scene(cell, seed)
    X, W, st, fallbacks = online_mvdr(Y, mx, mn, beta, ref, ban, loading=loading)
    for a in (X, W, st['phi_x'], st['phi_n']):
        a.setflags(write=False)
    return X, W, st, fallbacks


def reference_movement(cell, seed=0):
    """How far the reference's X, W and state move under a last-bit change of every sample and
    mask value, relative; the largest over the cell's variants."""
    D, beta, loading, F, T = cell
    Y, mx, mn, _ = scene(cell, seed)
    rng = np.random.default_rng(12345)
    Yb, mxb, mnb = last_bit(Y, rng), last_bit(mx, rng), last_bit(mn, rng)
    worst = 0.0
    for ban, ref in variants(cell):
        X, W, st, _ = reference(cell, ban, ref, seed)
        Xb, Wb, stb, _ = online_mvdr(Yb, mxb, mnb, beta, ref, ban, loading=loading)
        worst = max(worst, rel_err(Xb, X), rel_err(Wb, W), rel_err(stb['phi_x'], st['phi_x']),
                    rel_err(stb['phi_n'], st['phi_n']))
    return worst


def choose_seed(cell, seeds=range(8)):
    for seed in seeds:
        if reference_movement(cell, seed) * STABILITY_MARGIN <= TOL:
            return seed
    raise AssertionError(f'no stable scene for {cell}')


def in_blocks(Y, mx, mn, beta, ref, ban, loading, blocks, step):
    """``step(Yb, mxb, mnb, state) -> X, W, state`` over consecutive blocks from the fresh state
    of the whole Y -> X, W, the final state."""
    state = fresh_state(Y.shape[0], Y.shape[2], loading, Y)
    Xs, Ws, t0 = [], [], 0
    for n in blocks:
        X, W, state = step(Y[:, t0:t0 + n], mx[:, t0:t0 + n], mn[:, t0:t0 + n], state)
        Xs.append(X)
        Ws.append(W)
        t0 += n
    assert t0 == Y.shape[1]
    return np.concatenate(Xs, axis=1), np.concatenate(Ws, axis=1), state


def edge_scene(cell, kind, seed=0):
    """The cell's scene with digital silence in it.  'block': 10 frames of zeros in every channel
    in the middle; 'channel': channel 1 all zero, the others live."""
    Y, mx, mn, _ = scene(cell, seed)
    Y = Y.copy()
    if kind == 'block':
        Y[:, Y.shape[1] // 2:Y.shape[1] // 2 + 10] = 0
    else:
        Y[:, :, 1] = 0
    return Y, mx, mn


def fallback_case(kind):
    """The two deterministic fallback cases -> Y, mx, mn, the state to start from, beta, and the
    number of fallback frames.  'all': Phi_N = 0 and mn = 0, every frame falls back.  'first': D = 1,
    Phi_N = 0 and mn = 0 for the first three frames only."""
    cell = (4, 0.99, 1.0, 2, 20) if kind == 'all' else (1, 0.9, 1.0, 3, 12)
    D, beta, loading, F, T = cell
    Y, mx, mn, _ = scene(cell)
    mn = mn.copy()
    if kind == 'all':
        mn[:] = 0
    else:
        mn[:, :3] = 0
    state = dict(phi_x=np.zeros((F, D, D), np.complex128), phi_n=np.zeros((F, D, D), np.complex128))
    return Y, mx, mn, state, beta, (F * T if kind == 'all' else 3 * F)


# ------------------------------------------------------------------ the evidence
def second_half_error(X, image0):
    """The energy of X - (the target's image at channel 0) over the second half of the frames,
    relative to that image's energy.  X, image0 (F,T)."""
    half = X.shape[1] // 2
    return float(np.sum(np.abs(X[:, half:] - image0[:, half:]) ** 2)
                 / np.sum(np.abs(image0[:, half:]) ** 2))


@functools.lru_cache(maxsize=None)
def evidence_window_error(seed=EVIDENCE_SEED):
    """The oracle's whole-window get_mvdr_vector_souden(ref_channel=0, eps=1e-10) on the scene."""
    import gss_oracle as oracle
    Y, mx, mn, image = scene(EVIDENCE_CELL, seed)
    Yf = Y.transpose(0, 2, 1)                                        # (F,D,T)
    cov_x = oracle.get_power_spectral_density_matrix(Yf, mx)
    cov_n = oracle.get_power_spectral_density_matrix(Yf, mn)
    w = oracle.get_mvdr_vector_souden(cov_x, cov_n, ref_channel=0, eps=1e-10)
    return second_half_error(oracle.apply_beamforming_vector(w, Yf), image[:, :, 0])


def evidence_ratio(X=None, seed=EVIDENCE_SEED):
    """error of the online form (``X`` (F,T); None: the reference's) / error of the whole window"""
    D, beta, loading, F, T = EVIDENCE_CELL
    Y, mx, mn, image = scene(EVIDENCE_CELL, seed)
    if X is None:
        X = online_mvdr(Y, mx, mn, beta, 0, False, loading=loading)[0]
    return second_half_error(X, image[:, :, 0]) / evidence_window_error(seed)


# ------------------------------------------------------------------ the pipeline
PIPE = dict(num_channels=4, num_samples=12000, wpe_taps=2, wpe_delay=2, bss_iterations=3,
            stft_size=1024, stft_shift=256, forget=0.99, loading=1e-2, wpe_alpha=0.999)
# scene seed of synthetic.tiny, kept by the rule: the chain's own |x_hat| moves at least
# STABILITY_MARGIN x less than X_TOL under a last-bit change of the samples, with the offline and
# with the online WPE
PIPE_SCENE_SEED = 0


def pipe_scene(scene_seed=None):
    from pb_chime5_amd import synthetic
    return synthetic.tiny(seed=PIPE_SCENE_SEED if scene_seed is None else scene_seed,
                          num_channels=PIPE['num_channels'], num_samples=PIPE['num_samples'])


def pipe_enhance(obs, activity, target_index, ex, wpe_online=False):
    """The oracle's stages with the reference above in the place of its beamformer (BAN on, the
    window's reference channel, a fresh state from the window), and with ``wpe_online`` the online
    WPE's reference in the place of its WPE block -> x_hat."""
    import gss_oracle as oracle
    import online_wpe_reference as wref
    p = PIPE

    def wpe_fn(Obs, taps, delay, iterations, psd_context):
        return wref.to_dtf(wref.online_wpe(wref.to_ftd(Obs), taps, delay, p['wpe_alpha'])[0])
    _, d = oracle.enhance_observation(
        obs, activity, target_index, ex, wpe_taps=p['wpe_taps'], wpe_delay=p['wpe_delay'],
        stft_size=p['stft_size'], stft_shift=p['stft_shift'], bss_iterations=p['bss_iterations'],
        return_details=True, wpe_fn=wpe_fn if wpe_online else None,
        gss_fn=oracle.gss_block_batched)
    X = online_mvdr(to_ftd(d['Obs']), d['target_mask'].T, d['distortion_mask'].T, p['forget'],
                    d['ref_channel'], True, loading=p['loading'])[0]
    return oracle.istft(X.T, p['stft_size'], p['stft_shift'], fading=True)


@functools.lru_cache(maxsize=None)
def pipe_reference(wpe_online=False, scene_seed=None):
    u = pipe_scene(scene_seed)
    return pipe_enhance(u.obs, u.activity_array, u.target_index, u.ex, wpe_online)


def abs_rel_err(a, b):
    return float(np.max(np.abs(np.abs(a) - np.abs(b))) / np.max(np.abs(b)))


def pipe_movement(wpe_online=False, scene_seed=None):
    u = pipe_scene(scene_seed)
    a = pipe_reference(wpe_online, scene_seed)
    b = pipe_enhance(last_bit(u.obs, np.random.default_rng(12345)), u.activity_array,
                     u.target_index, u.ex, wpe_online)
    return abs_rel_err(b, a)


if __name__ == '__main__':
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / 'oracle'))
    for cell in CELLS + LONG_CELLS:
        seed = choose_seed(cell)
        print(f'    {cell}: {seed},   # moves {reference_movement(cell, seed):.1e}')
    for seed in range(4):
        print(f'evidence {EVIDENCE_CELL}, seed {seed}: online / whole-window error '
              f'{evidence_ratio(seed=seed):.2f}')
    for wpe_online in (False, True):
        print(f'pipeline, wpe_online={wpe_online}: |x_hat| moves {pipe_movement(wpe_online):.1e}')
