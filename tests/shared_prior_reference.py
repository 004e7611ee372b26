"""NumPy reference of the CACGMM with a frequency-shared prior (gss_cacgmm_shared_prior), built on
the untouched oracle: a `CACGMMTrainer` whose M-step forms the mixture weight as the mean of the
affiliations over the FREQUENCY axis (pb_bss ``weight_constant_axis=-3``) instead of over time,
and the `gss_block_batched` flow around it.  Scenes, their stability under a last-bit change of
the input, and the 'bins consistent' measure of the issue live here too, so that the CPU and the
GPU tests share them.  Every reference run is computed once per session and shared."""
import functools
import sys
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
for _p in (str(_HERE.parent), str(_HERE.parent / 'oracle')):    # (run as a script: no conftest)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gss_oracle as oracle            # noqa: E402

EM_TOL = 1e-7               # tests/test_gpu_specialisations.py: max |posterior - oracle|
STABILITY_MARGIN = 100.0    # the oracle itself must move at least this much less than the bar


class SharedPriorTrainer(oracle.CACGMMTrainer):
    """weight (1, K, T): one prior per class and frame for all frequencies."""

    @staticmethod
    def _m_step(y, quadratic_form, affiliation, eigenvalue_floor):
        model = oracle.CACGMMTrainer._m_step(y, quadratic_form, affiliation, eigenvalue_floor)
        model.weight = np.mean(affiliation, axis=-3, keepdims=True)
        return model


def shared_prior_block(Obs, initialization, mask=None, iterations=20, iterations_post=1,
                       trainer=SharedPriorTrainer):
    """Obs (D,T,F); initialization (K,T) or (F,K,T); mask (K,T) / (F,K,T) bool or None ->
    posterior (K,T,F), prior (K,T) of the last M-step.  The steps of oracle.gss_block_batched:
    fit; for post >= 2 fit(model, post - 1) with no mask; predict, masked only for post 0."""
    y = np.ascontiguousarray(np.asarray(Obs).transpose(2, 1, 0))       # (F, T, D)
    init = np.asarray(initialization, np.float64)
    init = init[None] if init.ndim == 2 else init
    if mask is not None:
        mask = np.asarray(mask, bool)
        mask = mask[None] if mask.ndim == 2 else mask
    t = trainer()
    cur = t.fit(y, init, iterations=iterations, source_activity_mask=mask)
    if iterations_post != 0:
        if iterations_post != 1:
            cur = t.fit(y, cur, iterations=iterations_post - 1)
        aff = cur.predict(y)
    else:
        aff = cur.predict(y, source_activity_mask=mask)
    weight = np.asarray(cur.weight)
    prior = weight[0] if weight.shape[-1] == aff.shape[-1] else None
    return aff.transpose(1, 2, 0), prior


def per_frequency_block(Obs, initialization, iterations=20):
    """The same start through the oracle as it is (pi[f, k] constant over time) -> (K,T,F)."""
    return shared_prior_block(Obs, initialization, None, iterations, 1,
                              trainer=oracle.CACGMMTrainer)[0]


# ------------------------------------------------------------------ the method's function
def table_scene(seed, D):
    """The scene of the issue's table: two speakers through 512-tap rooms, 64000 samples ->
    Obs (D,T,F) with T = 1003, F = 129, and each speaker's true frame activity (2,T) bool."""
    from pb_chime5_amd import synthetic
    u = synthetic.make_utterance(seed, D, 64000, [(3200, 35200), (25600, 60800)], rir_taps=512,
                                 noise=1e-2, fast=True)
    Obs = oracle.stft(u.obs, 256, 64)
    T = Obs.shape[1]
    truth = np.asarray(oracle.activity_time_to_frequency(u.activity_array[:2], 256, 64, True,
                                                         stft_pad=True))[:, :T]
    return Obs, truth


TABLE_RUNS = [(s, D) for D in (4, 6) for s in (0, 1, 2)]
TABLE_K, TABLE_ITERATIONS = 3, 20


@functools.lru_cache(maxsize=None)
def table_run(seed, D):
    """One run of the issue's table through the reference: Obs, truth, the start
    `ops.blind_initialization(3, T, seed + 100)`, posterior (K,T,F) and prior (K,T)."""
    from pb_chime5_amd import ops
    Obs, truth = table_scene(seed, D)
    init = ops.blind_initialization(TABLE_K, Obs.shape[1], seed + 100)
    posterior, prior = shared_prior_block(Obs, init, None, TABLE_ITERATIONS, 1)
    for a in (Obs, truth, init, posterior, prior):
        a.setflags(write=False)
    return Obs, truth, init, posterior, prior


def _corr_rows(A, b):
    """Pearson correlation over t of every row of A (..., T) with b (T,)."""
    A = A - A.mean(axis=-1, keepdims=True)
    b = b - b.mean()
    den = np.sqrt(np.sum(A * A, axis=-1) * np.sum(b * b))
    return np.sum(A * b, axis=-1) / np.where(den > 0, den, 1.0)


def bins_consistent(posterior, assignment_from, truth):
    """Share of the frequencies in which, for every speaker, the class whose affiliation row
    correlates best (Pearson, over t) with the speaker's true frame activity is the class that
    `assignment_from` (K,T) -- the prior, or the posterior's mean over f -- gives that speaker.
    Returns (share, smallest gap between best and second-best correlation over bins and
    speakers, correlation of each speaker's assigned row of `assignment_from` with the truth)."""
    post = np.asarray(posterior).transpose(2, 0, 1)                    # (F,K,T)
    ok = np.ones(post.shape[0], bool)
    gap, corr = np.inf, []
    for s in range(truth.shape[0]):
        b = truth[s].astype(np.float64)
        c_global = _corr_rows(np.asarray(assignment_from), b)          # (K,)
        k_star = int(np.argmax(c_global))
        corr.append(float(c_global[k_star]))
        c = _corr_rows(post, b)                                        # (F,K)
        ok &= np.argmax(c, axis=1) == k_star
        srt = np.sort(c, axis=1)
        gap = min(gap, float(np.min(srt[:, -1] - srt[:, -2])))
    return float(np.mean(ok)), gap, corr


# ------------------------------------------------------------------ parity scenes
# (D, T, F, K, iterations, post) of the issue, in its order
CELLS = [(4, 327, 3, 3, 4, 1), (24, 327, 3, 5, 3, 1), (7, 135, 5, 8, 3, 0), (6, 50, 4, 2, 5, 1),
         (17, 327, 2, 19, 2, 1), (12, 200, 9, 4, 6, 2), (4, 70, 513, 3, 2, 1), (5, 130, 1, 3, 3, 1)]
FORMS = ('blind', 'random', 'weak')
# every instantiation of the register-form E-step (D x K, fit and predict), as the matrix of
# tests/test_gpu_specialisations.py names those of the per-frequency EM: F = 2, five full tiles
# and a ragged one, weakly guided
REG_CELLS = [(D, 327, 2, K, 2, 1) for D in (4, 10, 12, 20, 24) for K in (2, 3, 4, 5, 6)]
# every instantiation of the LDS-form E-step (K = 1..19; first, fit and predict launch in every
# cell: two iterations and an unmasked predict) at one unspecialised D <= 12 and one above 12,
# as EM_SWEEP_CELLS of tests/test_gpu_specialisations.py does for the per-frequency EM: F = 2,
# and every point source has D + 8 frames of its own (`em_default_frames` there).  K = 1 launches
# its three instantiations but cannot fail on values: the posterior of a single class is 1.
LDS_D, LDS_K = (7, 17), tuple(range(1, 20))


def lds_frames(D, K):
    need, T = K * (D + 8) - 1, 327
    while T <= need:
        T += 64
    return T


LDS_CELLS = [(D, lds_frames(D, K), 2, K, 2, 1) for D in LDS_D for K in LDS_K]
# the unguided (K,T) start in a handful of them: both D, K either side of the eight-class groups
LDS_BLIND_CELLS = [c for c in LDS_CELLS if (c[0], c[3]) in ((7, 2), (7, 9), (7, 19), (17, 8),
                                                            (17, 11), (17, 16))]
# the mask-only start (no initialisation: the 1 : 1e-10 table is derived on the device), with a
# (K,T) mask for every frequency and with an (F,K,T) one
MASK_ONLY_CELLS = [CELLS[0], CELLS[2], CELLS[5]]
# seed of every (cell, form) whose seed 0 did not pass: a seed is kept only if the reference's own
# posteriors and prior move at least STABILITY_MARGIN x less than EM_TOL when every input sample
# moves in its last bit (`python tests/shared_prior_reference.py` re-derives the table).  Seed 0
# passed in all 24: the reference moves by 1.4e-17 ... 8.3e-11 (the largest at D = 24, random
# start), so the table is empty.  Seed 0 passed in the 38 + 6 LDS-form cells too: the reference
# moves by 5.4e-15 ... 1.3e-11 (the largest at D = 17, K = 13, weak), exactly 0 at K = 1.
SEEDS = {}


def crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


@functools.lru_cache(maxsize=None)
def parity_scene(D, T, F, K, seed):
    """K - 1 random steering vectors with on/off runs plus 0.1 noise -> Y (D,T,F), activity (K,T)
    bool (the last class, the noise, always on).  Read-only."""
    rng = np.random.default_rng([seed, D, T, F, K])
    Y = 0.1 * crandn(rng, D, T, F)
    act = np.zeros((K, T), bool)
    act[-1] = True
    for k in range(K - 1):
        run = max(T // (2 * K), 4)
        on = np.zeros(T, bool)
        t = int(rng.integers(0, run))
        while t < T:
            length = int(rng.integers(run // 2 + 1, 2 * run))
            on[t:t + length] = True
            t += length + int(rng.integers(run // 2 + 1, 2 * run))
        act[k] = on
        Y += crandn(rng, D, 1, F) * crandn(rng, 1, T, F) * on[None, :, None]
    Y.setflags(write=False)
    act.setflags(write=False)
    return Y, act


def form_guidance(form, act, F, seed):
    """(initialization, mask) of a parity cell's form: blind = a (K,T) start and no mask, random =
    an (F,K,T) start and no mask, weak = the activity-derived start plus the activity as mask."""
    from pb_chime5_amd import ops
    K, T = act.shape
    if form == 'blind':
        return ops.blind_initialization(K, T, seed + 100), None
    if form == 'random':
        init = np.random.default_rng([seed, 7]).uniform(0.01, 1.0, size=(F, K, T))
        return init / init.sum(axis=1, keepdims=True), None
    init, mask = oracle.gss_initialization(act)
    return init, mask


def per_frequency_mask(act, F):
    """(F,K,T) bool: the activity, class 0 dropped on the first third of the frames in the upper
    half of the bins (the last class, the noise, stays on everywhere)."""
    K, T = act.shape
    mask = np.repeat(np.asarray(act, bool)[None], F, axis=0)
    mask[F // 2:, 0, :T // 3] = False
    return mask


@functools.lru_cache(maxsize=None)
def mask_only_reference(cell, per_frequency, seed=0, moved=False):
    """The reference from the start the library derives from a mask alone:
    where(mask, 1, 1e-10) / sum over k, per frequency where the mask is."""
    D, T, F, K, iterations, post = cell
    Y, act = parity_scene(D, T, F, K, seed)
    mask = per_frequency_mask(act, F) if per_frequency else np.asarray(act, bool)
    init = np.where(mask, 1.0, 1e-10)
    init = init / init.sum(axis=-2, keepdims=True)
    if moved:
        Y = last_bit(Y, np.random.default_rng(12345))
    return shared_prior_block(Y, init, mask, iterations, post) + (mask,)


def mask_only_movement(cell, per_frequency):
    a, pa, _ = mask_only_reference(cell, per_frequency)
    b, pb, _ = mask_only_reference(cell, per_frequency, moved=True)
    return max(float(np.max(np.abs(a - b))), float(np.max(np.abs(pa - pb))))


def last_bit(a, rng):
    a = np.asarray(a)
    if a.dtype.kind == 'c':
        return last_bit(a.real, rng) + 1j * last_bit(a.imag, rng)
    return a * (1 + (rng.integers(0, 2, a.shape) * 2 - 1) * 2.0 ** -52)


@functools.lru_cache(maxsize=None)
def reference(cell, form, seed):
    D, T, F, K, iterations, post = cell
    Y, act = parity_scene(D, T, F, K, seed)
    init, mask = form_guidance(form, act, F, seed)
    post_, prior = shared_prior_block(Y, init, mask, iterations, post)
    post_.setflags(write=False)
    prior.setflags(write=False)
    return post_, prior


def reference_movement(cell, form, seed):
    """How far the reference's posteriors and prior move under a last-bit change of the input."""
    D, T, F, K, iterations, post = cell
    Y, act = parity_scene(D, T, F, K, seed)
    init, mask = form_guidance(form, act, F, seed)
    a, pa = reference(cell, form, seed)
    b, pb = shared_prior_block(last_bit(Y, np.random.default_rng(12345)), init, mask, iterations,
                               post)
    if not (np.all(np.isfinite(a)) and np.all(np.isfinite(b))):
        return np.inf
    return max(float(np.max(np.abs(a - b))), float(np.max(np.abs(pa - pb))))


def seed_of(cell, form):
    return SEEDS.get((cell, form), 0)


def choose_seed(cell, form, seeds=range(8)):
    for seed in seeds:
        if reference_movement(cell, form, seed) * STABILITY_MARGIN <= EM_TOL:
            return seed
    raise AssertionError(f'no stable scene for {cell} {form}')



# ------------------------------------------------------------------ the annotation-free front door
BLIND = dict(num_channels=4, num_samples=12000, num_speakers=2, wpe_taps=2, wpe_delay=2,
             wpe_iterations=3, iterations=3, stft_size=1024, stft_shift=256)
X_TOL = 1e-4            # |x_hat| rel err of the end-to-end tests (tests/test_gpu_pipeline.py)
# scene seed of synthetic.tiny: seed 0 passed the rule (the chain's own |x_hat| moves at least
# STABILITY_MARGIN x less than X_TOL for every class under a last-bit change of the samples)
BLIND_SCENE_SEED = 0


def blind_scene(scene_seed=None):
    from pb_chime5_amd import synthetic
    return synthetic.tiny(seed=BLIND_SCENE_SEED if scene_seed is None else scene_seed,
                          num_channels=BLIND['num_channels'], num_samples=BLIND['num_samples'])


def blind_enhance(obs, ex, seed=0):
    """`Enhancer.enhance_observation_blind` composed of the oracle's stages: stft -> wpe_block ->
    the reference above from `ops.blind_initialization` -> masks with the context frames zeroed
    -> beamform_mvdr_souden_from_masks(ban) per class -> istft.  Returns x_hat (K,N), prior (K,T),
    the post-WPE Obs (D,T,F) and the posteriors (K,T,F)."""
    from pb_chime5_amd import ops
    b = BLIND
    Obs = oracle.stft(obs, b['stft_size'], b['stft_shift'], fading=True)
    Obs = oracle.wpe_block(Obs, b['wpe_taps'], b['wpe_delay'], b['wpe_iterations'], 0)
    K = b['num_speakers'] + 1
    init = ops.blind_initialization(K, Obs.shape[1], seed)
    posterior, prior = shared_prior_block(Obs, init, None, b['iterations'], 1)
    masks = posterior.copy()
    sf, ef = oracle.start_end_context_frames(ex, b['stft_size'], b['stft_shift'], True)
    masks[:, :sf, :] = 0
    if ef > 0:
        masks[:, -ef:, :] = 0
    x_hat = []
    for k in range(K):
        X = oracle.beamform_mvdr_souden_from_masks(
            Obs, masks[k], np.sum(np.delete(masks, k, axis=0), axis=0), ban=True)
        x_hat.append(oracle.istft(X, b['stft_size'], b['stft_shift'], fading=True))
    return np.stack(x_hat), prior, Obs, posterior


@functools.lru_cache(maxsize=None)
def blind_reference(scene_seed=None):
    u = blind_scene(scene_seed)
    return blind_enhance(u.obs, u.ex)


def abs_rel_err(a, b):
    return float(np.max(np.abs(np.abs(a) - np.abs(b))) / np.max(np.abs(b)))


def blind_movement(scene_seed=None):
    """Per class: how far the chain's own |x_hat| moves under a last-bit change of the samples."""
    u = blind_scene(scene_seed)
    a = blind_reference(scene_seed)[0]
    b = blind_enhance(last_bit(u.obs, np.random.default_rng(12345)), u.ex)[0]
    return [abs_rel_err(b[k], a[k]) for k in range(a.shape[0])]


if __name__ == '__main__':
    for cell in CELLS:
        for form in FORMS:
            seed = choose_seed(cell, form)
            print(f'    ({cell}, {form!r}): {seed},   # moves {reference_movement(cell, form, seed):.1e}')
    for cell in REG_CELLS:
        print(f'    ({cell}, weak): {choose_seed(cell, "weak")},   # moves '
              f'{reference_movement(cell, "weak", choose_seed(cell, "weak")):.1e}')
    for cell, form in [(c, 'weak') for c in LDS_CELLS] + [(c, 'blind') for c in LDS_BLIND_CELLS]:
        seed = choose_seed(cell, form)
        print(f'    ({cell}, {form!r}): {seed},   # moves {reference_movement(cell, form, seed):.1e}')
    for cell in MASK_ONLY_CELLS:
        for per_f in (False, True):
            print(f'    mask only {cell} per_frequency={per_f}: moves '
                  f'{mask_only_movement(cell, per_f):.1e}')
    print('blind front door, |x_hat| movement per class:', blind_movement())
