"""NumPy reference of the cross-window class link (gss_cacgmm_link) and of the recording driver
built on it (`Enhancer.enhance_recording_blind`): the scores and the exhaustive search, the window
plan, the start table, the cross-fade, a whole-recording reference on the untouched oracle's
shared-prior EM (tests/shared_prior_reference.py), and the periodic scene both test files use.
Every reference run is computed once per session and shared (read-only)."""
import functools
import itertools
import math

import numpy as np

import gss_oracle as oracle
import shared_prior_reference as spr

MIN_MARGIN = 0.1            # best minus second-best permutation total the scene tests ask for
PARITY_MIN_MARGIN = 1e-6    # ... and the parity cells
STABILITY_MARGIN = 100.0    # the reference itself must move at least this much less than the bar


# ------------------------------------------------------------------ the link
def scores(prev, cur):
    """prev, cur (F,K,L) -> S (K,K): S[a, b] = <prev[:, a], cur[:, b]> / sqrt(|prev[:, a]|^2
    |cur[:, b]|^2) over f and t, 0 where a norm is zero.  Every entry by the same expression on
    its own rows, so identical rows give identical bits."""
    prev = np.asarray(prev, np.float64)
    cur = np.asarray(cur, np.float64)
    K = prev.shape[1]
    S = np.zeros((K, K))
    for a in range(K):
        for b in range(K):
            num = np.sum(prev[:, a, :] * cur[:, b, :])
            den = np.sum(prev[:, a, :] * prev[:, a, :]) * np.sum(cur[:, b, :] * cur[:, b, :])
            S[a, b] = num / math.sqrt(den) if den > 0 else 0.0
    return S


def best_permutation(S):
    """argmax_p sum_a S[a, p[a]] over all K! permutations in lexicographic order (the first among
    exact maxima) -> (mapping (K,) int32, best total, second-best total; -inf for K = 1)."""
    K = S.shape[0]
    best, best_total, second = None, -math.inf, -math.inf
    for p in itertools.permutations(range(K)):
        total = 0.0
        for a in range(K):
            total += S[a, p[a]]
        if total > best_total:
            best, best_total, second = p, total, best_total
        elif total > second:
            second = total
    return np.array(best, np.int32), best_total, second


def link(prev, cur, prev_begin=0, cur_begin=0, L=None):
    """prev (F,K,T_prev), cur (F,K,T_cur), L frames from the two begins -> (mapping, S, margin)
    with linked[a] = cur[mapping[a]] and margin = best - second-best total (inf for K = 1)."""
    if L is None:
        L = prev.shape[2] - prev_begin
    S = scores(prev[:, :, prev_begin:prev_begin + L], cur[:, :, cur_begin:cur_begin + L])
    mapping, best, second = best_permutation(S)
    return mapping, S, best - second


def score_bound(F, L):
    """|S_device - S_reference| allowed: sums of F L non-negative terms in any order, each
    within (F L) 2^-53 relative of the exact one; a score is a ratio of three such sums and at
    most 1 -> 4 F L 2^-53 absolute covers the three sums and the sqrt and the division."""
    return 4.0 * F * L * 2.0 ** -53


# ------------------------------------------------------------------ parity cells
# (F, K, T_prev, T_cur, L, prev_begin, cur_begin, kind)
CELLS = [
    (4, 1, 20, 20, 20, 0, 0, 'plain'),              # K = 1: the identity, one score
    # one frequency, one frame: every cosine is 1, whatever the values, so no draw has a margin;
    # powers of two make every product, square, root and quotient exact -> S = 1.0 everywhere in
    # the reference and on the device, an exact tie that the tie rule decides (the identity)
    (1, 2, 1, 1, 1, 0, 0, 'one_frame'),
    (5, 3, 70, 70, 70, 0, 0, 'plain'),              # L crosses a wave
    (3, 8, 300, 300, 300, 0, 0, 'plain'),           # more frames than threads, 40320 candidates
    (513, 4, 37, 37, 37, 0, 0, 'plain'),            # more rows than the finish kernel's threads
    (7, 3, 90, 61, 40, 33, 5, 'plain'),             # begins, T_prev != T_cur
    (6, 4, 50, 50, 50, 0, 0, 'zero_row'),           # a class that is silent
    (6, 4, 50, 50, 50, 0, 0, 'tie'),                # two identical rows: an exact tie
    (33, 5, 257, 300, 256, 1, 44, 'plain'),         # every class count has a kernel of its own
    (2, 6, 64, 64, 64, 0, 0, 'plain'),
    (9, 7, 129, 129, 128, 1, 0, 'plain'),
]


def cell_id(cell):
    return '-'.join(map(str, cell))


@functools.lru_cache(maxsize=None)
def parity_input(cell, seed=0):
    """prev (F,K,T_prev) and cur (F,K,T_cur): cur's linked frames are prev's under a random
    permutation plus noise, the rest is random; columns sum to 1 over k like posteriors.  The
    'zero_row' kind silences one class of cur, the 'tie' kind makes two rows of cur equal (both
    tables).  Returns (prev, cur, the permutation hidden in cur)."""
    F, K, T_prev, T_cur, L, pb, cb, kind = cell
    rng = np.random.default_rng([seed, F, K, T_prev, T_cur, L])
    prev = rng.uniform(0.0, 1.0, size=(F, K, T_prev)) ** 3
    cur = rng.uniform(0.0, 1.0, size=(F, K, T_cur)) ** 3
    hidden = rng.permutation(K)
    if kind == 'one_frame':
        prev, cur = (2.0 ** rng.integers(-3, 1, size=a.shape) for a in (prev, cur))
        for a in (prev, cur):
            a.setflags(write=False)
        return prev, cur, hidden.astype(np.int32)
    # cur[hidden[a]] continues prev[a]
    cur[:, hidden, cb:cb + L] = prev[:, :, pb:pb + L] + 0.1 * rng.uniform(size=(F, K, L))
    prev /= prev.sum(axis=1, keepdims=True)
    cur /= cur.sum(axis=1, keepdims=True)
    if kind == 'zero_row':
        cur[:, hidden[1], :] = 0.0
    if kind == 'tie':
        cur[:, hidden[1], :] = cur[:, hidden[0], :]
    for a in (prev, cur):
        a.setflags(write=False)
    return prev, cur, hidden.astype(np.int32)


@functools.lru_cache(maxsize=None)
def parity_reference(cell, seed=0):
    F, K, T_prev, T_cur, L, pb, cb, kind = cell
    prev, cur, hidden = parity_input(cell, seed)
    mapping, S, margin = link(prev, cur, pb, cb, L)
    S.setflags(write=False)
    return mapping, S, margin


# ------------------------------------------------------------------ windows, start, cross-fade
def window_plan(N, window, hop):
    n = max(1, (N - window) // hop + 1)
    plan = [(w * hop, w * hop + window) for w in range(n)]
    plan[-1] = (plan[-1][0], N)
    return plan


def start_table(K, T, seed, w, start, previous_prior, H, L):
    from pb_chime5_amd import ops
    table = ops.blind_initialization(K, T, seed + w)
    if start == 'carry' and previous_prior is not None:
        table = np.concatenate([previous_prior[:, H:H + L], table[:, L:]], axis=1)
        table = table / table.sum(axis=0)
    return table


def stitch(pieces, offsets, total):
    """In the overlap of w and w + 1 position i of O gets (i + 0.5) / O of w + 1 and the rest of
    w; written per window as weight * piece, added.  For pieces of which at most two hold any
    position (the samples of a recording)."""
    out = np.zeros(np.shape(pieces[0])[:-1] + (total,))
    for w, (piece, o) in enumerate(zip(pieces, offsets)):
        n = piece.shape[-1]
        weight = np.ones(n)
        if w > 0:
            O = offsets[w - 1] + pieces[w - 1].shape[-1] - o
            weight[:O] = (np.arange(O) + 0.5) / O
        if w + 1 < len(pieces):
            O = o + n - offsets[w + 1]
            weight[n - O:] = 1.0 - (np.arange(O) + 0.5) / O
        out[..., o:o + n] += weight * piece
    return out


def stitch_by_blend(pieces, offsets, total):
    """The same cross-fade written window by window as (1 - r) * stitched so far + r * later on
    the overlap and a copy behind it: the expression the 1e-15 comparison of the GPU test is made
    against, and the form that also covers the frames of the STFT's padding, which three windows
    hold when window = 2 hop."""
    out = np.zeros(np.shape(pieces[0])[:-1] + (total,))
    out[..., :pieces[0].shape[-1]] = pieces[0]
    for w in range(1, len(pieces)):
        o, n = offsets[w], pieces[w].shape[-1]
        O = offsets[w - 1] + pieces[w - 1].shape[-1] - o
        r = (np.arange(O) + 0.5) / O
        out[..., o:o + O] = (1.0 - r) * out[..., o:o + O] + r * pieces[w][..., :O]
        out[..., o + O:o + n] = pieces[w][..., O:]
    return out


# ------------------------------------------------------------------ the periodic scene
SCENE = dict(num_channels=4, num_samples=160000, rir_taps=512, noise=1e-2, stft_size=256,
             stft_shift=64, window_samples=64000, hop_samples=32000, num_speakers=2,
             iterations=20)
# scene seed kept by the rule of shared_prior_reference.py: under a last-bit change of every
# sample the reference's own link scores move at least STABILITY_MARGIN x less than MIN_MARGIN
# in every window, for both starts (`python tests/link_reference.py` re-derives it)
SCENE_SEED = 0
SCENE_SEEDS = (0, 1, 2)


def _speaker_activity(N, first, length, period=2.0, repeats=5, rate=16000):
    act = np.zeros(N, bool)
    for i in range(repeats):
        a = int(round((first + period * i) * rate))
        act[min(a, N):min(a + int(round(length * rate)), N)] = True
    return act


@functools.lru_cache(maxsize=None)
def periodic_scene(seed=SCENE_SEED, moved=False):
    """synthetic.make_utterance(fast=True) with several intervals per speaker: two speakers,
    speaker 1 on [0.3 + 2 i, 1.5 + 2 i) s, speaker 2 on [1.2 + 2 i, 2.2 + 2 i) s, i = 0..4; rng
    order per speaker the source, then D rooms; then the noise; scaled by 0.1.
    -> obs (D,N), activity (2,N) bool."""
    from pb_chime5_amd import synthetic
    D, N = SCENE['num_channels'], SCENE['num_samples']
    rng = np.random.default_rng(seed)
    acts = [_speaker_activity(N, 0.3, 1.2), _speaker_activity(N, 1.2, 1.0)]
    srcs, rirs = [], []
    for act in acts:
        srcs.append(synthetic._source(rng, N) * act)
        rirs.append(np.stack([synthetic._rir(rng, SCENE['rir_taps']) for _ in range(D)]))
    obs = synthetic._reverberate_fast(np.stack(srcs), np.stack(rirs), N)
    obs = obs + rng.standard_normal(obs.shape) * SCENE['noise']
    obs = obs * 0.1
    if moved:
        obs = spr.last_bit(obs, np.random.default_rng(12345))
    acts = np.stack(acts)
    obs.setflags(write=False)
    acts.setflags(write=False)
    return obs, acts


def frame_truth(activity, num_samples=None):
    """(S,N) bool -> (S,T) bool over the STFT frames of the scene's transform."""
    size, shift = SCENE['stft_size'], SCENE['stft_shift']
    T = oracle.stft(np.zeros(activity.shape[-1]), size, shift).shape[0]
    return np.asarray(oracle.activity_time_to_frequency(activity, size, shift, True,
                                                        stft_pad=True))[:, :T]


def best_classes(prior, truth):
    """Per speaker: the class whose row of `prior` (K,T) correlates best (Pearson, over t) with
    the speaker's true frame activity, and all K correlations."""
    out = []
    for s in range(truth.shape[0]):
        c = spr._corr_rows(np.asarray(prior), truth[s].astype(np.float64))
        out.append((int(np.argmax(c)), c))
    return out


@functools.lru_cache(maxsize=None)
def recording_reference(seed=SCENE_SEED, start='fresh', moved=False):
    """The recording driver on the NumPy shared-prior EM, no WPE: per window the oracle's STFT,
    `spr.shared_prior_block` from the start table (init seed 100 + scene seed), the link against
    the previous window's linked posteriors on the shared frames without E edge frames.
    -> dict(windows, mappings (n,K), scores [S], margins, priors [linked (K,T_w)],
    prior (K,T) stitched, frames [T_w], H)."""
    obs, _ = periodic_scene(seed, moved)
    size, shift = SCENE['stft_size'], SCENE['stft_shift']
    K = SCENE['num_speakers'] + 1
    N = obs.shape[1]
    windows = window_plan(N, SCENE['window_samples'], SCENE['hop_samples'])
    H = SCENE['hop_samples'] // shift
    E = size // shift - 1
    mappings, S_all, margins, priors, frames = [], [], [], [], []
    linked_prev = None
    for w, (s, e) in enumerate(windows):
        Obs = oracle.stft(obs[:, s:e], size, shift)                     # (D,T,F)
        T_w = Obs.shape[1]
        L = (frames[-1] - H) if frames else 0
        init = start_table(K, T_w, 100 + seed, w, start, priors[-1] if priors else None, H, L)
        posterior, prior = spr.shared_prior_block(Obs, init, None, SCENE['iterations'], 1)
        gamma = posterior.transpose(2, 0, 1)                            # (F,K,T)
        if w == 0:
            mapping, S, margin = np.arange(K, dtype=np.int32), None, np.inf
        else:
            mapping, S, margin = link(linked_prev, gamma, H + E, E, L - 2 * E)
        linked_prev = gamma[:, mapping, :]
        mappings.append(mapping)
        S_all.append(S)
        margins.append(margin)
        priors.append(prior[mapping])
        frames.append(T_w)
    T = (len(windows) - 1) * H + frames[-1]
    return dict(windows=windows, mappings=np.stack(mappings), scores=S_all, margins=margins,
                priors=priors, prior=stitch_by_blend(priors, [w * H for w in range(len(windows))], T),
                frames=frames, H=H)


def reference_movement(seed, start):
    """How far the reference's link scores move under a last-bit change of the samples (inf if a
    mapping changes)."""
    a = recording_reference(seed, start)
    b = recording_reference(seed, start, moved=True)
    if not np.array_equal(a['mappings'], b['mappings']):
        return np.inf
    return max(float(np.max(np.abs(x - y))) for x, y in zip(a['scores'][1:], b['scores'][1:]))


def golden_arrays():
    """What tests/golden/link_periodic.npz holds: the reference's results on the periodic scene
    with SCENE_SEED, for the GPU tests (which do not run the NumPy EM again);
    `python tests/link_reference.py --write-golden` writes it, tests/test_link_api.py compares it
    with a fresh run."""
    _, acts = periodic_scene()
    truth = frame_truth(acts)
    out = {}
    for start in ('fresh', 'carry'):
        r = recording_reference(SCENE_SEED, start)
        out[f'{start}_mappings'] = r['mappings']
        out[f'{start}_margins'] = np.array(r['margins'][1:])
        out[f'{start}_prior'] = r['prior']
        out[f'{start}_best'] = np.array([k for k, _ in best_classes(r['prior'], truth)])
    return out


if __name__ == '__main__':
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    if '--write-golden' in sys.argv:
        path = Path(__file__).resolve().parent / 'golden' / 'link_periodic.npz'
        np.savez_compressed(path, **golden_arrays())
        print(path, path.stat().st_size, 'bytes')
        sys.exit(0)
    for cell in CELLS:
        print(cell_id(cell), 'margin %.2e' % parity_reference(cell)[2])
    for seed in SCENE_SEEDS:
        for start in ('fresh', 'carry'):
            r = recording_reference(seed, start)
            print(f'seed {seed} {start}: mappings {r["mappings"].tolist()}, margins '
                  f'{[round(float(m), 3) for m in r["margins"][1:]]}, moves '
                  f'{reference_movement(seed, start):.1e}')
