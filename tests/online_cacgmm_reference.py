"""NumPy reference of the online CACGMM (gss_cacgmm_online): the frame recursion as DESIGN.md
section 25 writes it -- the recursive EM of the complex angular central Gaussian mixture on
exponentially forgetting running sums, float64, np.linalg.cholesky for the factor and
np.linalg.solve for the quadratic form, with the rank guard and the scale pin of section 26 (and
without them under ``plain=True``: the recursion as it was, kept to prove that the starved cell
bites) --, the closed form of the sums, and the scenes the CPU and the GPU tests share.  Every
reference run is computed once per session and shared, read-only."""
import functools

import numpy as np

import gss_oracle as oracle

TINY = oracle.TINY
TOL = 1e-10                 # relative to the largest magnitude of the compared array: gamma, S, n
STABILITY_MARGIN = 100.0    # the reference itself must move at least this much less than the bar
CLOSED_FORM_TOL = 1e-9
ROUND_TRIP_TOL = 1e-9       # from_model(to_model()) against the state
AFF_EPS = 1e-10             # the fit's affiliation_eps
X_TOL = 1e-4                # |x_hat| rel err of the end-to-end tests (tests/test_gpu_pipeline.py)
# The method's constants (csrc/cacgmm_online.hip has the same).  After the update of a live frame,
# with d = max(0, the largest diagonal entry of the updated S_k) and p = the smallest pivot of the
# Cholesky factorisation the frame's E-step made of S_k (the squared diagonal of L): the rank guard
# adds (1 - beta) RANK_EPS d phi to every diagonal entry, phi = exp(-p / (RANK_GATE d)) (0 where
# that argument is below -745, where S_k had no factor or d = 0) -- a smooth gate that is exactly
# 0 on every well-conditioned class and 1 on a class that has lost rank; and when the binary
# exponent (np.frexp's) of the largest entry then lies outside [-SCALE_BAND, SCALE_BAND], S_k is
# multiplied by the power of two that brings it to 0.
# Exponents reached with the pin off, watched after every frame: CELLS -34 .. 10, the 64-point
# stream cells 0 .. 11, the pipeline scene 0 .. 8 (test_the_band_is_never_reached_by_the_short_cells
# holds the first two inside +-40); the long cells reach -39 and, at forget 0.95, -126.
RANK_EPS = 1e-10
RANK_GATE = 1e-9
GATE_CUT = 745.0
SCALE_BAND = 64


def fresh_state(F, K, D, prior_mass):
    s = np.zeros((F, K, D, D), np.complex128)
    s[:, :, np.arange(D), np.arange(D)] = prior_mass
    return dict(s=s, n=np.full((F, K), float(prior_mass)))


def copy_state(state):
    return {k: np.array(v) for k, v in state.items()}


def _cholesky(S):
    """(F,K,D,D) -> L (identity where there is none) and ok (F,K): LAPACK's rule (a pivot <= 0 or
    NaN fails)."""
    try:
        return np.linalg.cholesky(S), np.ones(S.shape[:2], bool)
    except np.linalg.LinAlgError:
        pass
    L = np.zeros_like(S)
    ok = np.ones(S.shape[:2], bool)
    for idx in np.ndindex(*S.shape[:2]):
        try:
            L[idx] = np.linalg.cholesky(S[idx])
        except np.linalg.LinAlgError:
            ok[idx] = False
            L[idx] = np.eye(S.shape[-1])
    return L, ok


def mask_fkt(mask, F, K, T):
    """None / (K,T) / (F,K,T) -> (F,K,T) float64 of zeros and ones."""
    if mask is None:
        return np.ones((F, K, T))
    m = (np.asarray(mask) != 0).astype(np.float64)
    return np.broadcast_to(m, (F, K, T))


def frame_posterior(S, n, z, m, with_pivot=False):
    """One E-step: S (F,K,D,D), n (F,K), z (F,D) unit norm, m (F,K) -> gamma (F,K), q (F,K), ok
    (and with ``with_pivot`` the smallest pivot of every factorisation, (F,K))."""
    D = z.shape[-1]
    L, ok = _cholesky(S)
    x = np.linalg.solve(L, np.broadcast_to(z[:, None, :, None], S.shape[:3] + (1,)))[..., 0]
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(ok, n * np.sum(np.abs(x) ** 2, axis=-1), np.sum(np.abs(z) ** 2, axis=-1)[:, None])
        q = np.maximum(q, TINY)
        logdet = 2 * np.sum(np.log(np.real(np.einsum('fkdd->fkd', L))), axis=-1) - D * np.log(n)
        lp = -D * np.log(q) - np.where(ok, logdet, 0.0)
        pi = n / np.sum(n, axis=-1, keepdims=True)
        # CACGMM._predict, affiliation_eps = 0
        aff = np.exp(lp - np.amax(lp, axis=-1, keepdims=True))
        aff = aff * pi
        aff = aff * m
        aff = aff / np.maximum(np.sum(aff, axis=-1, keepdims=True), TINY)
    if with_pivot:
        return aff, q, ok, np.min(np.real(np.einsum('fkdd->fkd', L)) ** 2, axis=-1)
    return aff, q, ok


def max_diagonal(S):
    """max(0, the largest diagonal entry), NaN entries passed over (fmax)."""
    return np.fmax(np.fmax.reduce(np.real(np.einsum('...dd->...d', S)), axis=-1), 0.0)


def scale_exponents(S):
    """np.frexp's exponent of the largest diagonal entry of every S_k."""
    return np.frexp(max_diagonal(S))[1]


def guard_and_pin(S, beta, pivot, ok, band=SCALE_BAND):
    """The rank guard and the scale pin on the freshly updated S (..., D, D); ``pivot`` (...) the
    smallest pivot of the factorisation of S before the update, ``ok`` whether there was one
    -> S, the classes that were rescaled (...), the gate phi of every class (...)."""
    D = S.shape[-1]
    d = max_diagonal(S)
    with np.errstate(all='ignore'):
        x = pivot / (RANK_GATE * np.where(d > 0, d, 1.0))
        phi = np.where(ok & (d > 0) & (x < GATE_CUT), np.exp(-np.minimum(x, GATE_CUT)), 0.0)
    add = ((1 - beta) * RANK_EPS) * d * phi
    S = S.copy()
    S[..., np.arange(D), np.arange(D)] += add[..., None]
    top = d + add                                   # the largest entry after the guard, its bits
    with np.errstate(invalid='ignore'):
        e = np.frexp(top)[1]
        hit = np.isfinite(top) & (top >= TINY) & (np.abs(e) > band)
    if np.any(hit):
        S = np.where(hit[..., None, None], np.ldexp(1.0, -np.clip(e, -1000, 1000))[..., None, None] * S, S)
    return S, hit, phi


def online_cacgmm(Y, mask, beta, state, record=False, plain=False, watch=None, band=SCALE_BAND,
                  watch_every=100, pins=None, gates=None):
    """Y (F,T,D), mask None / (K,T) / (F,K,T), the state to start from (not modified) -> gamma
    (F,K,T), the state after the T frames, the number of fallback (frequency, frame, class)
    triples; with ``record`` also the clipped affiliations g and the q that entered the sums,
    both (F,K,T), and the frames that were skipped as zeros (F,T).  The loop over the frames is
    the recursion, vectorised over frequencies and classes.  ``plain``: without the rank guard
    and the scale pin.  ``watch(t, S, n)`` is called after the update of every
    ``watch_every``-th frame; ``pins``: a list that receives the (frame, frequency, class) of
    every rescaling; ``gates``: a list that receives the gate phi (F,K) of every frame (0 where
    the frame is digital silence)."""
    Y = np.asarray(Y, np.complex128)
    F, T, D = Y.shape
    st = copy_state(state)
    S, n = st['s'], st['n']
    K = n.shape[1]
    m = mask_fkt(mask, F, K, T)
    Z = oracle.normalize_observation(Y)                      # (F,D,T)
    live = np.linalg.norm(Y, axis=-1) != 0                   # (F,T)
    gamma = np.zeros((F, K, T))
    gs, qs = np.zeros((F, K, T)), np.ones((F, K, T))
    fallbacks = 0
    for t in range(T):
        z = Z[:, :, t]
        aff, q, ok, pivot = frame_posterior(S, n, z, m[:, :, t], with_pivot=True)
        gamma[:, :, t] = aff
        fallbacks += int(np.sum(~ok))
        g = np.clip(aff, AFF_EPS, 1 - AFF_EPS)
        zz = z[:, None, :, None] * z.conj()[:, None, None, :]
        upd = (g * D / np.maximum(q, 10 * TINY))[:, :, None, None] * zz
        lv = live[:, t]
        Sn = beta * S + upd
        if not plain:
            Sn, hit, phi = guard_and_pin(Sn, beta, pivot, ok, band)
            if gates is not None:
                gates.append(np.where(lv[:, None], phi, 0.0))
            if pins is not None:
                pins.extend((t, int(f), int(k)) for f, k in zip(*np.nonzero(hit & lv[:, None])))
        S = np.where(lv[:, None, None, None], Sn, S)
        n = np.where(lv[:, None], beta * n + g, n)
        gs[:, :, t], qs[:, :, t] = g, q
        if watch is not None and (t + 1) % watch_every == 0:
            watch(t + 1, S, n)
    out = gamma, dict(s=S, n=n), fallbacks
    return out + (gs, qs, live) if record else out


def closed_form(Y, g, q, beta, prior_mass):
    """S and n after the T (non-zero) frames of Y from a fresh state, from the recorded g and q
    alone: n = beta^T n0 + sum beta^(T-1-t) g_t and likewise S."""
    Y = np.asarray(Y, np.complex128)
    F, T, D = Y.shape
    Z = oracle.normalize_observation(Y)                      # (F,D,T)
    w = beta ** (T - 1 - np.arange(T))
    n = beta ** T * prior_mass + np.sum(w * g, axis=-1)
    c = w * g * D / np.maximum(q, 10 * TINY)
    S = np.einsum('fkt,fdt,fet->fkde', c, Z, Z.conj())
    S[:, :, np.arange(D), np.arange(D)] += beta ** T * prior_mass
    return S, n


def to_model(state):
    """precision = B_k^-1, log_det = ln det B_k, weight = pi_k of B_k = S_k / n_k."""
    S, n = state['s'], state['n']
    D = S.shape[-1]
    precision = n[..., None, None] * np.linalg.inv(S)
    log_det = np.linalg.slogdet(S)[1] - D * np.log(n)
    return precision, log_det, n / np.sum(n, axis=-1, keepdims=True)


def from_model(precision, weight, mass):
    n = mass * np.asarray(weight)
    return dict(s=n[..., None, None] * np.linalg.inv(precision), n=n)


def predict(Y, state, mask=None):
    """The posteriors every frame of Y gets from the FROZEN model of ``state`` -> (F,K,T)."""
    Y = np.asarray(Y, np.complex128)
    F, T, D = Y.shape
    K = state['n'].shape[1]
    m = mask_fkt(mask, F, K, T)
    Z = oracle.normalize_observation(Y)
    return np.stack([frame_posterior(state['s'], state['n'], Z[:, :, t], m[:, :, t])[0]
                     for t in range(T)], axis=-1)


def condition_numbers(state):
    return np.linalg.cond(state['s'])


def rel_err(a, b):
    """max |a - b| relative to the largest magnitude of b."""
    a, b = np.asarray(a), np.asarray(b)
    scale = float(np.max(np.abs(b))) if b.size else 0.0
    return float(np.max(np.abs(a - b))) / scale if scale > 0 else float(np.max(np.abs(a), initial=0.0))


def to_ftd(Obs):
    return np.ascontiguousarray(np.asarray(Obs).transpose(2, 1, 0))


def to_dtf(Y):
    return np.ascontiguousarray(np.asarray(Y).transpose(2, 1, 0))


def to_ktf(gamma):
    """(F,K,T) -> (K,T,F), the layout the package hands posteriors out in."""
    return np.ascontiguousarray(np.asarray(gamma).transpose(1, 2, 0))


# ------------------------------------------------------------------ parity scenes
# (D, K, beta, prior_mass, F, T), guided by the scene's activity
CELLS = [
    (4, 3, 0.99, 1.0, 3, 150),
    (1, 2, 0.9, 1.0, 1, 5),
    (2, 2, 1.0, 1.0, 2, 70),            # no forgetting
    (3, 3, 0.95, 1.0, 2, 90),           # odd D
    (8, 4, 0.99, 1.0, 2, 64),           # the sweep's 8-lane grid
    (9, 2, 0.99, 1.0, 2, 64),
    (16, 3, 0.99, 1.0, 2, 64),
    (17, 3, 0.99, 1.0, 2, 64),
    (24, 5, 0.995, 1.0, 2, 120),
    (29, 3, 0.99, 1.0, 2, 80),
    (32, 2, 0.999, 1.0, 1, 64),         # the D bound
    (4, 8, 0.9, 1.0, 2, 200),           # the K bound
    (24, 5, 0.98, 0.01, 2, 120),
    (4, 3, 0.9, 0.01, 2, 300),
    (24, 5, 0.995, 1.0, 2, 1),          # T = 1
    (4, 1, 0.99, 1.0, 2, 20),           # K = 1
]
CLOSED_FORM_CELLS = [(4, 3, 0.99, 1.0, 3, 150), (2, 2, 1.0, 1.0, 2, 70)]
CHUNK_CELLS = [(4, 3, 0.99, 1.0, 3, 150), (24, 5, 0.995, 1.0, 2, 120)]
CHUNKS = {150: (1, 63, 64, 22), 120: (1, 57, 56, 6)}
MODEL_CELL = (4, 3, 0.99, 1.0, 3, 150)      # the unguided run from a fitted model: the second half
MODEL_MASS = 50.0
# seed of every cell whose seed 0 did not pass: a seed is kept only if the reference's own gamma, S
# and n move at least STABILITY_MARGIN x less than TOL when every sample moves in its last bit
# (`python tests/online_cacgmm_reference.py` re-derives the table).
SEEDS = {(24, 5, 0.995, 1.0, 2, 120): 2, (24, 5, 0.98, 0.01, 2, 120): 2}
# the long cells under the same rule (on them the gate of the rank guard stays at 0, so these are
# the movements of the plain recursion):
#    (4, 4, 0.99, 1.0, 2, 6000): 0,   # moves 9.7e-13, cond(S) up to 2.7e+02
#    (12, 4, 0.99, 1.0, 1, 5000): 1,   # moves 2.6e-13, cond(S) up to 7.9e+02   (seed 0: 3.7e-12)
#    (24, 5, 0.99, 1.0, 1, 4000): no seed of range(8) allows TOL: 5.2e-12, 9.4e-11, 1.07e-12, 5.3e-12,
#                                 2.7e-12, 3.7e-12, 6.8e-12, 5.0e-12.  It keeps the seed that moves
#                                 least, 2, and its bar is 100 x that movement, rounded up: 1.1e-10
#    (4, 3, 0.95, 1.0, 2, 4000): 3,   # moves 1.1e-13, cond(S) up to 4.7e+02   (seeds 0 - 2 move more)
LONG_SEEDS = {(12, 4, 0.99, 1.0, 1, 5000): 1, (24, 5, 0.99, 1.0, 1, 4000): 2, (4, 3, 0.95, 1.0, 2, 4000): 3}
LONG_BARS = {(24, 5, 0.99, 1.0, 1, 4000): 1.1e-10}
LONG_BAR_CAP = 1e-8


def long_tol(cell):
    """The bar of a long cell: TOL, or 100 x the movement of its kept seed where no seed allows
    TOL (never above LONG_BAR_CAP)."""
    return LONG_BARS.get(cell, TOL)



def crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def turns(rng, T, length, p):
    """(T,) bool: on with probability p, redrawn every ``length`` frames."""
    return np.repeat(rng.random(-(-T // length)) < p, length)[:T]


@functools.lru_cache(maxsize=None)
def scene(cell, seed=0):
    """K - 1 speakers with random complex steering vectors, each on in random turns of 8 frames
    (60 %), complex white noise while on, plus a last class that is always on: sensor noise of
    standard deviation 0.3 per real part (K = 1: that class alone, on top of one speaker that
    has no class).  -> Y (F,T,D), activity (K,T) bool, read-only."""
    D, K, beta, prior_mass, F, T = cell
    rng = np.random.default_rng([seed, D, K, F, T])
    speakers = max(K - 1, 1)
    steer = crandn(rng, speakers, F, D)
    on = np.stack([turns(rng, T, 8, 0.6) for _ in range(speakers)])
    src = crandn(rng, speakers, F, T) * on[:, None, :]
    Y = np.einsum('sfd,sft->ftd', steer, src) + 0.3 * crandn(rng, F, T, D)
    activity = np.ones((K, T), bool)
    activity[:K - 1] = on[:K - 1]
    Y.setflags(write=False)
    activity.setflags(write=False)
    return Y, activity


def last_bit(a, rng):
    a = np.asarray(a)
    if a.dtype.kind == 'c':
        return last_bit(a.real, rng) + 1j * last_bit(a.imag, rng)
    return a * (1 + (rng.integers(0, 2, a.shape) * 2 - 1) * 2.0 ** -52)


def seed_of(cell):
    return SEEDS.get(cell, 0)


@functools.lru_cache(maxsize=None)
def reference(cell, seed=0):
    """gamma (F,K,T), the final state and the fallback count of the cell from its fresh state."""
    D, K, beta, prior_mass, F, T = cell
    Y, activity = scene(cell, seed)
    gamma, st, fallbacks = online_cacgmm(Y, activity, beta, fresh_state(F, K, D, prior_mass))
    for a in (gamma, st['s'], st['n']):
        a.setflags(write=False)
    return gamma, st, fallbacks


def reference_movement(cell, seed=0):
    """How far the reference's gamma, S and n move under a last-bit change of every sample,
    relative."""
    D, K, beta, prior_mass, F, T = cell
    Y, activity = scene(cell, seed)
    gamma, st, _ = reference(cell, seed)
    Yb = last_bit(Y, np.random.default_rng(12345))
    gb, stb, _ = online_cacgmm(Yb, activity, beta, fresh_state(F, K, D, prior_mass))
    return max(rel_err(gb, gamma), rel_err(stb['s'], st['s']), rel_err(stb['n'], st['n']))


def choose_seed(cell, seeds=range(8)):
    for seed in seeds:
        if reference_movement(cell, seed) * STABILITY_MARGIN <= TOL:
            return seed
    raise AssertionError(f'no stable scene for {cell}')


def in_blocks(Y, activity, state, blocks, step):
    """``step(Yb, activity_b, state) -> gamma, state`` over consecutive blocks -> gamma, the final
    state."""
    gammas, t0 = [], 0
    for nb in blocks:
        gamma, state = step(Y[:, t0:t0 + nb], activity[..., t0:t0 + nb], state)
        gammas.append(gamma)
        t0 += nb
    assert t0 == Y.shape[1]
    return np.concatenate(gammas, axis=-1), state


def edge_scene(cell, kind, seed=0):
    """The cell's scene with digital silence in it.  'block': 10 frames of zeros in every channel
    in the middle; 'channel': the last channel all zero, the others live; 'masked': every class
    masked off in frames 5 to 9."""
    Y, activity = scene(cell, seed)
    Y, activity = Y.copy(), activity.copy()
    if kind == 'block':
        Y[:, Y.shape[1] // 2:Y.shape[1] // 2 + 10] = 0
    elif kind == 'channel':
        Y[:, :, -1] = 0
    else:
        activity[:, 5:10] = False
    return Y, activity


FALLBACK_CELL = (4, 3, 0.99, 1.0, 2, 12)


def fallback_case(kind):
    """A state handed in with S_1 = 0 -> Y, activity, the state, beta and the number of fallbacks.
    'first': the cell's scene, ONE frame: class 1 has no factor and falls back.  (From the second
    frame on S_1 is a sum of fewer than D rank-one terms and its last pivots are rounding noise
    of either sign, so neither LAPACK's verdict nor any other is a property of the method; after
    D frames S_1 has full rank and the class no longer falls back at all.)
    'every': the same scene with the last channel dead: the last diagonal entry of S_1 stays
    exactly 0 (a class without a factor gets no guard), its pivot is exactly 0 in every order of
    summation, and class 1 falls back on every frame."""
    D, K, beta, prior_mass, F, T = FALLBACK_CELL
    Y, activity = scene(FALLBACK_CELL)
    if kind == 'first':
        Y, activity = Y[:, :1], activity[:, :1]
    else:
        Y = Y.copy()
        Y[:, :, -1] = 0
    state = fresh_state(F, K, D, prior_mass)
    state['s'][:, 1] = 0
    return Y, activity, state, beta, F * Y.shape[1]


# ------------------------------------------------------------------ long horizons
# the bar of a long cell is TOL where a seed of range(8) allows it (`long_tol`)
LONG_CELLS = [
    (4, 4, 0.99, 1.0, 2, 6000),         # NR = 1
    (12, 4, 0.99, 1.0, 1, 5000),        # NR = 2
    (24, 5, 0.99, 1.0, 1, 4000),        # NR = 3
    (4, 3, 0.95, 1.0, 2, 4000),         # the fast scale drift: the pin fires
]
LONG_BLOCK = 625
PIN_CELL = (4, 3, 0.95, 1.0, 2, 4000)


def long_seed_of(cell):
    return LONG_SEEDS.get(cell, 0)


@functools.lru_cache(maxsize=None)
def long_pins(cell):
    """The (frame, frequency, class) at which the reference rescales an S_k, in order."""
    D, K, beta, prior_mass, F, T = cell
    Y, activity = scene(cell, long_seed_of(cell))
    pins = []
    online_cacgmm(Y, activity, beta, fresh_state(F, K, D, prior_mass), pins=pins)
    return tuple(pins)


def long_partitions(cell):
    """'blocks': LONG_BLOCK frames each (and the rest); 'ragged': one frame, a prime, a long
    block, the rest -- for a cell whose scale pin fires, cut so that the first rescaling happens
    on the LAST frame of a block and the second one on the FIRST frame of a block (the others
    fall inside blocks)."""
    T = cell[-1]
    blocks = (LONG_BLOCK,) * (T // LONG_BLOCK) + ((T % LONG_BLOCK,) if T % LONG_BLOCK else ())
    frames = sorted({t for t, _, _ in long_pins(cell)})
    if len(frames) >= 2 and frames[0] > 2:
        cuts = [1, frames[0] + 1, frames[1]]
    else:
        cuts = [1, 998, 998 + 2 * LONG_BLOCK + 3]
    bounds = [0] + cuts + [T]
    ragged = tuple(b - a for a, b in zip(bounds[:-1], bounds[1:]))
    assert sum(ragged) == T and min(ragged) > 0
    return dict(blocks=blocks, ragged=ragged)


# ------------------------------------------------------------------ the starved class
# A class that is allowed in most frames and wins almost none of them: its effective frame count
# stays far below D, S_k loses rank, and the plain recursion loses the Cholesky factor.  The
# recipe: a 10 s scene of K - 1 speakers in half-second turns through 8-tap filters, faded STFT
# 1024 / 256, frames 3 to 627 of bins 100 and 400 replayed 12 times.
STARVED = dict(D=4, K=4, beta=0.99, prior_mass=1.0, seed=4, samples=160000, turn=8000, stft_size=1024,
               stft_shift=256, bins=(100, 400), frames=(3, 628), replays=12)
STARVED_COND = 1e12         # cond(S_k) of the guarded reference, every 100 frames, stays below
STARVED_REFEREE_TOL = 1e-6  # the float64 reference against the extended-precision referee


def turn_scene(rng, D, K, samples, turn):
    """x (D,samples) and the activity (K,samples): K - 1 speakers, white noise through a random
    8-tap filter per channel, on (60 %) in random turns, a last class that is always on, sensor
    noise at 0.1."""
    act = np.ones((K, samples), bool)
    x = 0.1 * rng.standard_normal((D, samples))
    for k in range(K - 1):
        act[k] = np.repeat(rng.random(-(-samples // turn)) < 0.6, turn)[:samples]
        src = rng.standard_normal(samples) * act[k]
        x += np.stack([np.convolve(src, h)[:samples] for h in rng.standard_normal((D, 8))])
    return x, act


@functools.lru_cache(maxsize=None)
def starved_scene():
    """-> Y (F,T,D) with F = 2, T = 7500, the frame activity (K,T) bool; read-only."""
    p = STARVED
    x, act = turn_scene(np.random.default_rng(p['seed']), p['D'], p['K'], p['samples'], p['turn'])
    Yfull = oracle.stft(x, p['stft_size'], p['stft_shift'], fading=True)          # (D,T,F)
    actf = oracle.activity_time_to_frequency(act, p['stft_size'], p['stft_shift'], True,
                                             stft_pad=True)[:, :Yfull.shape[1]]
    lo, hi = p['frames']
    Y = np.ascontiguousarray(Yfull[..., list(p['bins'])].transpose(2, 1, 0))[:, lo:hi]
    Y = np.concatenate([Y] * p['replays'], axis=1)
    activity = np.concatenate([np.asarray(actf[:, lo:hi]) != 0] * p['replays'], axis=1)
    Y.setflags(write=False)
    activity.setflags(write=False)
    return Y, activity


@functools.lru_cache(maxsize=None)
def starved_reference(plain=False):
    """gamma, the final state, the fallback count and the largest cond(S_k) seen every 100
    frames."""
    p = STARVED
    Y, activity = starved_scene()
    worst = [0.0]

    def watch(t, S, n):
        with np.errstate(all='ignore'):
            worst[0] = max(worst[0], float(np.max(np.linalg.cond(S))))
    gamma, st, fallbacks = online_cacgmm(Y, activity, p['beta'],
                                         fresh_state(Y.shape[0], p['K'], p['D'], p['prior_mass']),
                                         plain=plain, watch=watch)
    for a in (gamma, st['s'], st['n']):
        a.setflags(write=False)
    return gamma, st, fallbacks, worst[0]


@functools.lru_cache(maxsize=None)
def starved_gates():
    """The largest gate phi over frequencies and classes at every frame of the starved cell in
    the guarded reference, (T,)."""
    p = STARVED
    Y, activity = starved_scene()
    gates = []
    online_cacgmm(Y, activity, p['beta'], fresh_state(Y.shape[0], p['K'], p['D'], p['prior_mass']),
                  gates=gates)
    return np.max(np.array(gates), axis=(1, 2))


def starved_partitions():
    """'blocks': LONG_BLOCK frames each; 'ragged': one frame, then cuts in the first run of three
    frames on which the guard is well alive (phi > 0.1) -- one cut before its middle frame and one after
    it, so that a block of ONE live frame has live frames on both sides -- and the rest."""
    T = starved_scene()[0].shape[1]
    live = starved_gates() > 0.1
    run = np.nonzero(live[:-2] & live[1:-1] & live[2:])[0]
    assert len(run) and run[0] > 1
    t = int(run[0]) + 1
    bounds = [0, 1, t, t + 1, T]
    blocks = (LONG_BLOCK,) * (T // LONG_BLOCK) + ((T % LONG_BLOCK,) if T % LONG_BLOCK else ())
    return dict(blocks=blocks, ragged=tuple(b - a for a, b in zip(bounds[:-1], bounds[1:])))


@functools.lru_cache(maxsize=None)
def starved_referee():
    """gamma of the guarded recursion in 80-bit extended precision, the number of failed
    factorisations."""
    import ext_precision as xp
    p = STARVED
    Y, activity = starved_scene()
    gamma, failed = xp.online_cacgmm(Y, activity, p['beta'], p['prior_mass'], RANK_EPS, RANK_GATE,
                                     GATE_CUT, SCALE_BAND)
    gamma.setflags(write=False)
    return gamma, failed


SCALE_EXPONENTS = (-600, -200, 200, 600)


def scaled_state(state):
    """S_k multiplied by 2^e_k, e_k from SCALE_EXPONENTS, another one per class (and shifted by one
    place per frequency)."""
    F, K = state['n'].shape
    e = np.array([[SCALE_EXPONENTS[(k + f) % len(SCALE_EXPONENTS)] for k in range(K)] for f in range(F)])
    return dict(s=state['s'] * np.ldexp(1.0, e)[..., None, None], n=state['n'].copy())


# ------------------------------------------------------------------ the evidence
EVIDENCE = dict(D=4, F=8, K=3, T=600, beta=0.95, prior_mass=1.0, guided=200, scored=400, turn=25,
                noise=0.1)
EVIDENCE_BOUND = 0.8        # a condition, not a measurement
EVIDENCE_SEED = 0           # the seed rule for it: the ratio of the reference is <= 0.75


@functools.lru_cache(maxsize=None)
def evidence_scene(seed=EVIDENCE_SEED):
    """Two speakers who alternate in 25-frame turns plus an always-on noise class at 0.1.  The
    frames before 200 are stationary; from frame 200 on speaker 0's steering vector turns from a0
    to an independent a1 by a0 cos(th) + a1 sin(th), th rising linearly to pi / 2 at the end.
    -> Y (F,T,D), activity (K,T) bool."""
    e = EVIDENCE
    D, F, T = e['D'], e['F'], e['T']
    rng = np.random.default_rng([seed, 77])
    a0, a1, b = crandn(rng, F, D), crandn(rng, F, D), crandn(rng, F, D)
    th = np.clip((np.arange(T) - e['guided']) / (T - 1 - e['guided']), 0, 1) * (np.pi / 2)
    steer0 = (a0[:, None, :] * np.cos(th)[None, :, None] + a1[:, None, :] * np.sin(th)[None, :, None])
    first = (np.arange(T) // e['turn']) % 2 == 0
    activity = np.stack([first, ~first, np.ones(T, bool)])
    s0 = crandn(rng, F, T) * first
    s1 = crandn(rng, F, T) * ~first
    Y = steer0 * s0[:, :, None] + b[:, None, :] * s1[:, :, None] + e['noise'] * crandn(rng, F, T, D)
    Y.setflags(write=False)
    activity.setflags(write=False)
    return Y, activity


def evidence_error(gamma, activity):
    """mean |gamma_0 - activity_0| over the scored frames; gamma (F,K,T') covering the frames from
    ``guided`` on."""
    e = EVIDENCE
    lo = e['scored'] - e['guided']
    return float(np.mean(np.abs(gamma[:, 0, lo:] - activity[0, e['scored']:][None, :])))


@functools.lru_cache(maxsize=None)
def evidence_state(seed=EVIDENCE_SEED):
    """The reference's state after the guided, stationary frames."""
    e = EVIDENCE
    Y, activity = evidence_scene(seed)
    g = e['guided']
    return online_cacgmm(Y[:, :g], activity[:, :g], e['beta'],
                         fresh_state(e['F'], e['K'], e['D'], e['prior_mass']))[1]


def evidence_ratio(continue_fn=None, predict_fn=None, seed=EVIDENCE_SEED, beta=None):
    """error of the state continued without a mask from frame ``guided`` / error of the SAME state
    frozen there.  ``continue_fn(Y, state, beta) -> gamma`` and ``predict_fn(Y, state) -> gamma``
    (F,K,T'): None = the reference's."""
    e = EVIDENCE
    beta = e['beta'] if beta is None else beta
    Y, activity = evidence_scene(seed)
    g = e['guided']
    if beta == e['beta']:
        state = evidence_state(seed)
    else:
        state = online_cacgmm(Y[:, :g], activity[:, :g], beta,
                              fresh_state(e['F'], e['K'], e['D'], e['prior_mass']))[1]
    if continue_fn is None:
        def continue_fn(Yb, st, bt):
            return online_cacgmm(Yb, None, bt, st)[0]
    if predict_fn is None:
        predict_fn = predict
    moving = evidence_error(continue_fn(Y[:, g:], state, beta), activity)
    frozen = evidence_error(predict_fn(Y[:, g:], state), activity)
    return moving / frozen


# ------------------------------------------------------------------ the pipeline
PIPE = dict(num_channels=4, num_samples=12000, wpe_taps=2, wpe_delay=2, stft_size=1024,
            stft_shift=256, forget=0.99, prior_mass=1.0, bf_forget=0.99, bf_loading=1e-2,
            wpe_alpha=0.999)
PIPE_SCENE_SEED = 0


def pipe_scene(scene_seed=None):
    from pb_chime5_amd import synthetic
    return synthetic.tiny(seed=PIPE_SCENE_SEED if scene_seed is None else scene_seed,
                          num_channels=PIPE['num_channels'], num_samples=PIPE['num_samples'])


def pipe_enhance(obs, activity, target_index, ex, bf_online=False, wpe_online=False):
    """The oracle's stages with the reference above in the place of its mixture model (a fresh
    state, the mask the frame activity), with ``bf_online`` the online MVDR's reference in the
    place of its beamformer and with ``wpe_online`` the online WPE's in the place of its WPE
    block -> x_hat."""
    import online_mvdr_reference as mref
    import online_wpe_reference as wref
    p = PIPE

    def wpe_fn(Obs, taps, delay, iterations, psd_context):
        return wref.to_dtf(wref.online_wpe(wref.to_ftd(Obs), taps, delay, p['wpe_alpha'])[0])

    def gss_fn(Obs, acitivity_freq, iterations, iterations_post):
        Y = to_ftd(Obs)
        F, T, D = Y.shape
        act = np.asarray(acitivity_freq)[:, :T]
        gamma = online_cacgmm(Y, act, p['forget'], fresh_state(F, act.shape[0], D, p['prior_mass']))[0]
        return to_ktf(gamma)
    x_hat, d = oracle.enhance_observation(
        obs, activity, target_index, ex, wpe_taps=p['wpe_taps'], wpe_delay=p['wpe_delay'],
        stft_size=p['stft_size'], stft_shift=p['stft_shift'], return_details=True,
        wpe_fn=wpe_fn if wpe_online else None, gss_fn=gss_fn)
    if not bf_online:
        return x_hat
    X = mref.online_mvdr(to_ftd(d['Obs']), d['target_mask'].T, d['distortion_mask'].T,
                         p['bf_forget'], d['ref_channel'], True, loading=p['bf_loading'])[0]
    return oracle.istft(X.T, p['stft_size'], p['stft_shift'], fading=True)


@functools.lru_cache(maxsize=None)
def pipe_reference(bf_online=False, wpe_online=False, scene_seed=None):
    u = pipe_scene(scene_seed)
    return pipe_enhance(u.obs, u.activity_array, u.target_index, u.ex, bf_online, wpe_online)


def abs_rel_err(a, b):
    return float(np.max(np.abs(np.abs(a) - np.abs(b))) / np.max(np.abs(b)))


def pipe_movement(bf_online=False, wpe_online=False, scene_seed=None):
    u = pipe_scene(scene_seed)
    a = pipe_reference(bf_online, wpe_online, scene_seed)
    b = pipe_enhance(last_bit(u.obs, np.random.default_rng(12345)), u.activity_array,
                     u.target_index, u.ex, bf_online, wpe_online)
    return abs_rel_err(b, a)


if __name__ == '__main__':
    for cell in CELLS + LONG_CELLS:
        if cell in LONG_BARS:
            print(f'    {cell}: seeds 0 - 7 move '
                  + ', '.join(f'{reference_movement(cell, seed):.2e}' for seed in range(8)))
            continue
        seed = choose_seed(cell)
        cond = condition_numbers(reference(cell, seed)[1])
        print(f'    {cell}: {seed},   # moves {reference_movement(cell, seed):.1e}, '
              f'cond(S) up to {cond.max():.1e}')
    for beta in (EVIDENCE['beta'], 0.99):
        for seed in range(4):
            print(f'evidence beta {beta}, seed {seed}: continued / frozen error '
                  f'{evidence_ratio(seed=seed, beta=beta):.2f}')
    for bf_online, wpe_online in ((False, False), (True, False), (True, True)):
        print(f'pipeline, bf_online={bf_online}, wpe_online={wpe_online}: |x_hat| moves '
              f'{pipe_movement(bf_online, wpe_online):.1e}')
