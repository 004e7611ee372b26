"""NumPy reference of the online WPE (gss_wpe_online): the frame recursion of the issue as it is
written there -- a recursive-least-squares filter with exponential forgetting and the silence
rule --, the closed form of the weighted least-squares problem the recursion solves, and the
scenes the CPU and the GPU tests share.  Every reference run is computed once per session and
shared, read-only."""
import functools

import numpy as np

TOL = 1e-10                 # relative to the largest magnitude of the compared array: X, G, P
STABILITY_MARGIN = 100.0    # the reference itself must move at least this much less than the bar
X_TOL = 1e-4                # |x_hat| rel err of the end-to-end tests (tests/test_gpu_pipeline.py)


def fresh_state(F, A, C, taps, delay):
    n, L = taps * C, taps + delay
    P = np.zeros((F, A, n, n), np.complex128)
    P[..., np.arange(n), np.arange(n)] = 1.0
    return dict(P=P, G=np.zeros((F, A, n, C), np.complex128),
                hist=np.zeros((F, A, L, C), np.complex128))


def copy_state(state):
    return {k: v.copy() for k, v in state.items()}


def online_wpe(Y, taps, delay, alpha, arrays=1, state=None, trace=None):
    """Y (F,T,A*C), channels array-major -> X (F,T,A*C) and the state after the T frames
    (``state``: where to start, not modified; None: fresh).  One problem per (f, a); the loop
    over the frames is the recursion, everything in it is vectorised over the problems.
    ``trace``: a list that receives (w, sigma, y) of every frame, for `closed_form`."""
    Y = np.asarray(Y, np.complex128)
    F, T, D = Y.shape
    A = arrays
    C = D // A
    assert A * C == D
    n, L = taps * C, taps + delay
    st = copy_state(state) if state is not None else fresh_state(F, A, C, taps, delay)
    P, G, hist = st['P'], st['G'], st['hist']
    Yp = Y.reshape(F, T, A, C).transpose(0, 2, 1, 3)               # (F,A,T,C)
    X = np.zeros_like(Yp)
    for t in range(T):
        y = Yp[:, :, t]                                            # (F,A,C)
        buf = np.concatenate([hist, y[:, :, None]], axis=2)        # (F,A,L+1,C): frames t-L .. t
        sigma = np.sum(np.abs(buf) ** 2, axis=(2, 3)) / ((L + 1) * C)
        # w[tau * C + c] = frame t - delay - tau; frame t - j sits at buf[L - j]
        w = np.stack([buf[:, :, L - delay - tau] for tau in range(taps)], axis=2).reshape(F, A, n)
        x = y - np.einsum('fanc,fan->fac', G.conj(), w)            # a-priori error: the output
        X[:, :, t] = x
        nom = np.einsum('fanm,fam->fan', P, w)
        den = alpha * sigma + np.real(np.einsum('fan,fan->fa', w.conj(), nom))
        live = den > 0                                             # else: digital silence, skip
        k = nom / np.where(live, den, 1.0)[..., None]
        wP = np.einsum('fan,fanm->fam', w.conj(), P)
        P_new = (P - k[..., :, None] * wP[..., None, :]) / alpha
        G_new = G + k[..., :, None] * x.conj()[..., None, :]
        P = np.where(live[..., None, None], P_new, P)
        G = np.where(live[..., None, None], G_new, G)
        hist = buf[:, :, 1:]
        if trace is not None:
            trace.append((w, sigma, y))
    X = X.transpose(0, 2, 1, 3).reshape(F, T, D)
    return X, dict(P=P, G=G, hist=np.ascontiguousarray(hist))


def closed_form(Y, taps, delay, alpha, arrays=1):
    """P and G after the T frames of Y from a fresh state, as the weighted least-squares problem
    the recursion claims to solve (no frame may be digital silence):
        R = alpha^T I + sum_t alpha^(T-1-t) w_t w_t^H / sigma_t
        G = R^-1 sum_t alpha^(T-1-t) w_t y_t^H / sigma_t,      P = R^-1.
    Only w, sigma and y come from the reference's loop; P and G do not."""
    trace = []
    online_wpe(Y, taps, delay, alpha, arrays, trace=trace)
    T = len(trace)
    w0 = trace[0][0]
    n = w0.shape[-1]
    R = np.zeros(w0.shape + (n,), np.complex128)
    R[..., np.arange(n), np.arange(n)] = alpha ** T
    B = np.zeros(w0.shape + (trace[0][2].shape[-1],), np.complex128)
    for t, (w, sigma, y) in enumerate(trace):
        assert np.all(sigma > 0), 'closed form: a frame of digital silence'
        g = (alpha ** (T - 1 - t) / sigma)[..., None, None]
        R += g * w[..., :, None] * w.conj()[..., None, :]
        B += g * w[..., :, None] * y.conj()[..., None, :]
    P = np.linalg.inv(R)
    return P, np.einsum('fanm,famc->fanc', P, B)


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
# (A, C, taps, delay, alpha, F, T) of the issue, in its order.  The on-chip form serves n <= 64.
ONCHIP_MAX_N = 64
ONCHIP_CELLS = [
    (1, 4, 10, 2, 0.9999, 3, 150),
    (1, 2, 2, 1, 0.999, 2, 70),
    (1, 1, 1, 0, 1.0, 1, 5),
    (1, 3, 7, 3, 0.99, 2, 90),              # odd n
    (6, 4, 10, 2, 0.9999, 2, 100),          # per array
    (1, 6, 10, 2, 0.995, 2, 100),           # n = 60
    (1, 4, 10, 2, 0.9999, 2, 1),            # T < L
    (1, 4, 10, 2, 0.9999, 2, 7),            # T < L
    (1, 1, ONCHIP_MAX_N, 2, 0.999, 2, 80),  # the on-chip bound
]
MEMORY_CELLS = [
    (1, 1, ONCHIP_MAX_N + 1, 2, 0.999, 2, 80),      # bound + 1: the first n of the memory form
    (1, 24, 10, 2, 0.9999, 2, 40),
    (1, 12, 10, 2, 0.999, 2, 60),
    (1, 32, 16, 2, 0.9999, 1, 6),                   # n = 512
]
CELLS = ONCHIP_CELLS + MEMORY_CELLS
CHUNK_CELLS = [(1, 4, 10, 2, 0.9999, 3, 150), (1, 24, 10, 2, 0.9999, 2, 40)]
CHUNKS = {150: (1, 63, 64, 22), 40: (1, 17, 16, 6)}
CLOSED_FORM_CELLS = [(1, 4, 10, 2, 0.9999, 3, 150), (1, 2, 2, 1, 1.0, 3, 70)]
CLOSED_FORM_TOL = 1e-9
# seed of every cell whose seed 0 did not pass: a seed is kept only if the reference's own X, G and
# P move at least STABILITY_MARGIN x less than TOL when every input sample moves in its last bit
# (`python tests/online_wpe_reference.py` re-derives the table).  Seed 0 passed in every cell, so
# the table is empty.
SEEDS = {}


# Long horizons, the same format.  The third cell's last channel is scaled by 1e-7 (the
# eigenvalues of P then span fifteen decades).  Seeds by the rule above:
#    (1, 4, 10, 2, 0.999, 1, 6000): 0,   # moves 2.5e-15; P, G vs the closed form 8.7e-14, 1.1e-14
#    (1, 12, 10, 2, 0.999, 1, 1500): 0,   # moves 1.0e-14; 5.6e-14, 9.1e-15
#    (1, 4, 3, 2, 0.99, 2, 6000): 0,   # moves 8.8e-16; 7.0e-15, 2.4e-15; eigenvalues of P 4.9e-03 .. 1.1e+12
LONG_CELLS = [
    (1, 4, 10, 2, 0.999, 1, 6000),          # on-chip form, n = 40
    (1, 12, 10, 2, 0.999, 1, 1500),         # memory form, n = 120
    (1, 4, 3, 2, 0.99, 2, 6000),            # one channel at 1e-7 of the others
]
LONG_CHANNEL_GAIN = {(1, 4, 3, 2, 0.99, 2, 6000): 1e-7}
LONG_BLOCK = 625
LONG_SEEDS = {}


def crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


@functools.lru_cache(maxsize=None)
def scene(cell, seed=0):
    """White complex noise per channel through a short random 'room' (direct path, reflections at
    3, 5 and 8 frames, mixed over the channels of an array) -> Y (F,T,A*C), read-only."""
    A, C, taps, delay, alpha, F, T = cell
    rng = np.random.default_rng([seed, A, C, taps, delay, F, T])
    D = A * C
    S = crandn(rng, F, T + 8, D)
    Y = S[:, 8:].copy()
    for lag, gain in ((3, 0.5), (5, 0.3), (8, 0.2)):
        mix = gain * crandn(rng, F, D, D) / np.sqrt(2 * D)
        Y += np.einsum('ftd,fde->fte', S[:, 8 - lag:T + 8 - lag], mix)
    Y.setflags(write=False)
    return Y


def long_seed_of(cell):
    return LONG_SEEDS.get(cell, 0)


@functools.lru_cache(maxsize=None)
def long_scene(cell, seed=0):
    """The scene of a long cell: `scene`, its last channel scaled by LONG_CHANNEL_GAIN."""
    Y = scene(cell, seed)
    if cell in LONG_CHANNEL_GAIN:
        Y = Y.copy()
        Y[:, :, -1] *= LONG_CHANNEL_GAIN[cell]
        Y.setflags(write=False)
    return Y


@functools.lru_cache(maxsize=None)
def long_reference(cell, seed=0):
    A, C, taps, delay, alpha, F, T = cell
    return _freeze(*online_wpe(long_scene(cell, seed), taps, delay, alpha, A))


@functools.lru_cache(maxsize=None)
def long_closed_form(cell, seed=0):
    A, C, taps, delay, alpha, F, T = cell
    return closed_form(long_scene(cell, seed), taps, delay, alpha, A)


def long_reference_movement(cell, seed=0):
    A, C, taps, delay, alpha, F, T = cell
    X, st = long_reference(cell, seed)
    Xb, stb = online_wpe(last_bit(long_scene(cell, seed), np.random.default_rng(12345)), taps,
                         delay, alpha, A)
    return max(rel_err(Xb, X), rel_err(stb['G'], st['G']), rel_err(stb['P'], st['P']))


def long_blocks(T):
    return (LONG_BLOCK,) * (T // LONG_BLOCK) + ((T % LONG_BLOCK,) if T % LONG_BLOCK else ())


def last_bit(a, rng):
    a = np.asarray(a)
    if a.dtype.kind == 'c':
        return last_bit(a.real, rng) + 1j * last_bit(a.imag, rng)
    return a * (1 + (rng.integers(0, 2, a.shape) * 2 - 1) * 2.0 ** -52)


def _freeze(X, st):
    X.setflags(write=False)
    for v in st.values():
        v.setflags(write=False)
    return X, st


@functools.lru_cache(maxsize=None)
def reference(cell, seed=0):
    A, C, taps, delay, alpha, F, T = cell
    return _freeze(*online_wpe(scene(cell, seed), taps, delay, alpha, A))


def reference_movement(cell, seed=0):
    """How far the reference's X, G and P move under a last-bit change of the input, relative."""
    A, C, taps, delay, alpha, F, T = cell
    X, st = reference(cell, seed)
    Xb, stb = online_wpe(last_bit(scene(cell, seed), np.random.default_rng(12345)), taps, delay,
                         alpha, A)
    return max(rel_err(Xb, X), rel_err(stb['G'], st['G']), rel_err(stb['P'], st['P']))


def seed_of(cell):
    return SEEDS.get(cell, 0)


def choose_seed(cell, seeds=range(8)):
    for seed in seeds:
        if reference_movement(cell, seed) * STABILITY_MARGIN <= TOL:
            return seed
    raise AssertionError(f'no stable scene for {cell}')


def silence_scene(cell, kind, seed=0):
    """The cell's scene with digital silence in it.  'block': 2 (L+1) frames of zeros in every
    channel in the middle; 'channel': channel 1 all zero, the others live."""
    A, C, taps, delay, alpha, F, T = cell
    Y = scene(cell, seed).copy()
    if kind == 'block':
        n0, length = T // 2, 2 * (taps + delay + 1)
        assert n0 + length < T
        Y[:, n0:n0 + length] = 0
    else:
        Y[:, :, 1] = 0
    return Y


# ------------------------------------------------------------------ the dereverberation evidence
# (C, taps, delay, alpha, T) on synthetic.tiny(seed=0, 4 channels, 24000 samples), STFT 256 / 64,
# bins 10 and up: the second half of the output carries less energy than that of the input
EVIDENCE_CELLS = [(4, 10, 2, 0.9999, 300), (4, 3, 2, 0.99, 130), (2, 2, 1, 0.999, 70)]


@functools.lru_cache(maxsize=None)
def evidence_obs():
    import gss_oracle as oracle
    from pb_chime5_amd import synthetic
    u = synthetic.tiny(seed=0, num_channels=4, num_samples=24000)
    Obs = oracle.stft(u.obs, 256, 64)                  # (D,T,F)
    Y = to_ftd(Obs)[10:]
    Y.setflags(write=False)
    return Y


def evidence_ratio(cell):
    C, taps, delay, alpha, T = cell
    Y = evidence_obs()[:, :T, :C]
    X, _ = online_wpe(Y, taps, delay, alpha)
    half = T // 2
    return float(np.sum(np.abs(X[:, half:]) ** 2) / np.sum(np.abs(Y[:, half:]) ** 2))


# ------------------------------------------------------------------ the pipeline
PIPE = dict(num_channels=4, num_samples=12000, wpe_taps=2, wpe_delay=2, bss_iterations=3,
            stft_size=1024, stft_shift=256, alpha=0.999)
# scene seed of synthetic.tiny: seed 0 passed the rule (the chain's own |x_hat| moves at least
# STABILITY_MARGIN x less than X_TOL under a last-bit change of the samples, joint and per array)
PIPE_SCENE_SEED = 0


def pipe_scene(scene_seed=None):
    from pb_chime5_amd import synthetic
    return synthetic.tiny(seed=PIPE_SCENE_SEED if scene_seed is None else scene_seed,
                          num_channels=PIPE['num_channels'], num_samples=PIPE['num_samples'])


def pipe_enhance(obs, activity, target_index, ex, arrays=1):
    """The oracle's stages with the reference above in the place of its WPE block -> x_hat and
    the post-WPE Obs (D,T,F)."""
    import gss_oracle as oracle
    p = PIPE

    def wpe_fn(Obs, taps, delay, iterations, psd_context):
        return to_dtf(online_wpe(to_ftd(Obs), taps, delay, p['alpha'], arrays)[0])
    x_hat, details = oracle.enhance_observation(
        obs, activity, target_index, ex, wpe_taps=p['wpe_taps'], wpe_delay=p['wpe_delay'],
        stft_size=p['stft_size'], stft_shift=p['stft_shift'], bss_iterations=p['bss_iterations'],
        return_details=True, wpe_fn=wpe_fn, gss_fn=oracle.gss_block_batched)
    return x_hat, details['Obs']


@functools.lru_cache(maxsize=None)
def pipe_reference(arrays=1, scene_seed=None):
    u = pipe_scene(scene_seed)
    return pipe_enhance(u.obs, u.activity_array, u.target_index, u.ex, arrays)


def abs_rel_err(a, b):
    return float(np.max(np.abs(np.abs(a) - np.abs(b))) / np.max(np.abs(b)))


def pipe_movement(arrays=1, scene_seed=None):
    u = pipe_scene(scene_seed)
    a = pipe_reference(arrays, scene_seed)[0]
    b = pipe_enhance(last_bit(u.obs, np.random.default_rng(12345)), u.activity_array,
                     u.target_index, u.ex, arrays)[0]
    return abs_rel_err(b, a)


if __name__ == '__main__':
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / 'oracle'))
    for cell in CELLS:
        seed = choose_seed(cell)
        print(f'    {cell}: {seed},   # moves {reference_movement(cell, seed):.1e}')
    for cell in LONG_CELLS:
        for seed in range(8):
            moved = long_reference_movement(cell, seed)
            if moved * STABILITY_MARGIN <= TOL:
                break
        P, G = long_closed_form(cell, seed)
        st = long_reference(cell, seed)[1]
        print(f'    {cell}: {seed},   # moves {moved:.1e}; P, G vs the closed form '
              f'{rel_err(st["P"], P):.1e}, {rel_err(st["G"], G):.1e}; eigenvalues of P '
              f'{np.linalg.eigvalsh(st["P"]).min():.1e} .. {np.linalg.eigvalsh(st["P"]).max():.1e}')
    for cell in EVIDENCE_CELLS:
        print(f'    evidence {cell}: second-half energy out / in {evidence_ratio(cell):.2f}')
    for arrays in (1, 2):
        print(f'pipeline, arrays={arrays}: |x_hat| moves {pipe_movement(arrays):.1e}')
