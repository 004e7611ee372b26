"""NumPy reference of a stream of several targets: the references of
tests/stream_reference.py composed with a target argument -- the two ends, the online WPE and the
online CACGMM once, then per target the masks, the online MVDR with a state of its own and the
synthesis with a tail of its own -- plus the cells, targets and seeds the CPU and the GPU tests
share.  Every reference run is computed once per session and shared, read-only."""
import functools

import numpy as np

import gss_oracle as oracle
import online_cacgmm_reference as cr
import online_mvdr_reference as mref
import online_wpe_reference as wref
import stream_reference as sr

TOL, X_TOL, ISTFT_TOL, STABILITY_MARGIN = sr.TOL, sr.X_TOL, sr.ISTFT_TOL, sr.STABILITY_MARGIN
SETTINGS = sr.SETTINGS

# (W, H, D, A, taps, delay, K, N, wpe): three cells of stream_reference and what those lack
CELLS = {
    'a': sr.CELLS['a'],                               # D = 4, K = 3: NR = 1
    'f': sr.CELLS['f'],                               # D = 24, K = 5, per-array WPE: NR = 3
    'h': sr.CELLS['h'],                               # no WPE stage
    'm': (64, 16, 12, 1, 2, 1, 3, 700, True),         # NR = 2
    'n': (64, 16, 32, 1, 2, 1, 2, 500, True),         # NR = 4, taps D = 64
    'r': (1024, 256, 24, 6, 2, 1, 5, 2048, True),     # F S = 2052 waves: more than one round, 8 frames
}
TARGETS = {'a': (0, 1, 2), 'h': (0, 1, 2), 'm': (0, 1, 2), 'n': (0, 1), 'f': (0, 1, 2, 4),
           'r': (0, 1, 2, 4)}
# The first seed of range(8) at which gamma, every target's X_hat and the final states of the
# composed reference move at least STABILITY_MARGIN x less than TOL, and |x_hat| that much less
# than X_TOL, when every sample moves in its last bit (`python tests/stream_targets_reference.py`
# re-derives the table).  The cells of stream_reference keep their seed there.
SEEDS = {
    'm': 0,   # moves 5.6e-13, |x_hat| 2.3e-13
    'n': 6,   # moves 6.4e-14, |x_hat| 1.1e-14
    'r': 0,   # moves 9.3e-15, |x_hat| 2.2e-15
}
# (Cell n, K = 2: the rule lands on a scene whose one speaker is on throughout -- the two classes
# see the same activity, the posteriors are 1/2 and the two targets coincide; its other seeds move
# 1e-11, only 10 x less than TOL.  It is there for the NR = 4 form of the kernel.  Cell r is one
# turn of 8 hops long, so each speaker is on or off for all of it whatever the seed: at seed 0
# classes 0, 1 and 4 are on and alike, class 2 is off and its row is zero.  It is there for the
# grid of F S = 2052 waves.  What tells targets apart at those two shapes is the operator test on
# random posteriors (every NR, and F = 513 with S = 4 at D = 24); cells a, f and h have scenes
# whose targets all differ.  In cell m at seed 0 speaker 0 is on throughout, so rows 0 and 2
# coincide and row 1 differs from both.)


def seed_of(name):
    return sr.seed_of(name) if name in sr.CELLS else SEEDS[name]


@functools.lru_cache(maxsize=None)
def scene(name, seed=0):
    """The recipe of `stream_reference.scene` for the cell's sizes (the shared cells: that scene
    itself) -> x (D,N) float64, activity (K,N) bool per sample, read-only."""
    if name in sr.CELLS:
        return sr.scene(name, seed)
    W, H, D, A, taps, delay, K, N, wpe = CELLS[name]
    rng = np.random.default_rng([seed, W, D, K, N])
    x = 0.3 * rng.standard_normal((D, N))
    activity = np.ones((K, N), bool)
    for k in range(K - 1):
        on = np.repeat(rng.random(-(-N // (8 * H))) < 0.6, 8 * H)[:N]
        src = rng.standard_normal(N) * on
        fir = rng.standard_normal((D, 6))
        x += np.stack([np.convolve(src, h)[:N] for h in fir])
        activity[k] = on
    x.setflags(write=False)
    activity.setflags(write=False)
    return x, activity


def partitions(name):
    """`stream_reference.partitions` for the cell's N and hop."""
    W, H, N = CELLS[name][0], CELLS[name][1], CELLS[name][7]
    head = (1, H - 1, H, H + 1, 0, W - 1, W)
    out = {'one': (N,), 'borders': head + (N - sum(head),), 'random': sr.random_cuts(N, 3)}
    if name == 'a':
        out['hops'] = (H,) * (N // H) + ((N % H,) if N % H else ())
    return out


# ------------------------------------------------------------------ the composition
def fresh_states(name, S):
    W, H, D, A, taps, delay, K, N, wpe = CELLS[name]
    F, s = W // 2 + 1, SETTINGS
    return dict(wpe=wref.fresh_state(F, A, D // A, taps, delay) if wpe else None,
                em=cr.fresh_state(F, K, D, s['gss_prior_mass']),
                bf=[mref.fresh_state(F, D, s['bf_loading']) for _ in range(S)])


def masks(gamma, target):
    """gamma (F,K,T) -> the target's row and the sum of the others in ascending k from 0.0."""
    mx = gamma[:, target]
    mn = np.zeros_like(mx)
    for k in range(gamma.shape[1]):
        if k != target:
            mn = mn + gamma[:, k]
    return mx, mn


def stages(name, Y, actf, states, targets):
    """Frames Y (D,T,F) with their activity (K,T) through the references of the three online
    stages from ``states`` (not modified), the beamformer once per target -> taps (Obs (F,T,D),
    gamma (F,K,T), the masks (S,F,T), X_hat (S,T,F), fallbacks (per target, CACGMM)) and the states
    afterwards."""
    W, H, D, A, taps, delay, K, N, wpe = CELLS[name]
    s = SETTINGS
    X = Y.transpose(2, 1, 0)
    new = dict(wpe=None, bf=[])
    if wpe:
        X, new['wpe'] = wref.online_wpe(X, taps, delay, s['wpe_alpha'], arrays=A, state=states['wpe'])
    gamma, new['em'], fb_em = cr.online_cacgmm(X, actf, s['gss_forget'], states['em'])
    mxs, mns, Xhats, fbs = [], [], [], []
    for target, state in zip(targets, states['bf']):
        mx, mn = masks(gamma, target)
        Xhat, _, after, fb = mref.online_mvdr(X, mx, mn, s['bf_forget'], s['ref_channel'], True,
                                              state=state)
        new['bf'].append(after)
        mxs.append(mx), mns.append(mn), Xhats.append(np.ascontiguousarray(Xhat.T)), fbs.append(fb)
    taps_ = dict(Obs=X, gamma=gamma, target_mask=np.stack(mxs), distortion_mask=np.stack(mns),
                 X_hat=np.stack(Xhats), fallbacks=(tuple(fbs), fb_em))
    return taps_, new


def compose_whole(name, x, activity, targets):
    """The references on the whole signal: `oracle.stft`, the stages once, `oracle.istft` per
    target -> x_hat (S,N), the taps, the final states."""
    W, H = CELLS[name][:2]
    N = x.shape[1]
    Y = oracle.stft(x, W, H, fading=True)
    actf = oracle.activity_time_to_frequency(activity, W, H, True)[:, :Y.shape[1]]
    taps, states = stages(name, Y, actf, fresh_states(name, len(targets)), targets)
    x_hat = np.stack([oracle.istft(X, W, H, fading=True)[:N] for X in taps['X_hat']])
    return x_hat, taps, states


def compose_stream(name, x, activity, targets, cuts):
    """The same in blocks of ``cuts`` samples with every state and S tails carried, flushed."""
    W, H, D = CELLS[name][:3]
    N, S = x.shape[1], len(targets)
    st = sr.RefStream(D, activity.shape[0], W, H)
    ends = [sr.RefStream(1, 0, W, H) for _ in range(S)]       # (their synthesis side only)
    states = fresh_states(name, S)
    out, all_taps = [], []
    feed = [(x[:, a:b], activity[:, a:b]) for a, b in sr.blocks_of(N, cuts)]
    feed.append((np.zeros((D, sr.flush_samples(N, W, H))), None))
    for blk, act in feed:
        Y, actf = st.stft(blk, act)
        if Y.shape[1] == 0:
            continue
        taps, states = stages(name, Y, actf, states, targets)
        out.append(np.stack([end.istft(X) for end, X in zip(ends, taps['X_hat'])]))
        all_taps.append(taps)
    axis = dict(Obs=1, gamma=2, target_mask=2, distortion_mask=2, X_hat=1)
    taps = {k: np.concatenate([t[k] for t in all_taps], axis=a) for k, a in axis.items()}
    taps['fallbacks'] = (tuple(sum(t['fallbacks'][0][s] for t in all_taps) for s in range(S)),
                         sum(t['fallbacks'][1] for t in all_taps))
    return np.concatenate(out, axis=1)[:, :N], taps, states


@functools.lru_cache(maxsize=None)
def reference(name, seed=0):
    """x_hat (S,N), the taps and the final states of the cell's scene and targets, composed on
    the whole signal."""
    x, activity = scene(name, seed)
    return sr._freeze(compose_whole(name, x, activity, TARGETS[name]))


def state_arrays(states):
    """{'wpe.P': array, ..., 'bf.phi_x': (S,F,D,D)} of the states that exist."""
    out = {f'{stage}.{k}': v for stage in ('wpe', 'em') if states[stage] is not None
           for k, v in states[stage].items()}
    for k in states['bf'][0]:
        out[f'bf.{k}'] = np.stack([st[k] for st in states['bf']])
    return out


def abs_rel_err(a, b):
    """`stream_reference.abs_rel_err`; a reference that is all zero (a target that is never
    active) measures the other side's largest magnitude."""
    scale = float(np.max(np.abs(b)))
    return float(np.max(np.abs(np.abs(a) - np.abs(b)))) / scale if scale else float(np.max(np.abs(a)))


def reference_movement(name, seed=0):
    """How far the composed reference moves under a last-bit change of every sample: (the largest
    relative movement of gamma, every target's X_hat and the final states, the movement of
    |x_hat|)."""
    x, activity = scene(name, seed)
    xh, taps, states = reference(name, seed)
    xb, tb, sb = compose_whole(name, cr.last_bit(x, np.random.default_rng(12345)), activity,
                               TARGETS[name])
    a, b = state_arrays(states), state_arrays(sb)
    moved = max([sr.rel_err(tb['gamma'], taps['gamma'])]
                + [sr.rel_err(p, q) for p, q in zip(tb['X_hat'], taps['X_hat'])]
                + [sr.rel_err(b[k], a[k]) for k in a])
    return moved, max(abs_rel_err(p, q) for p, q in zip(xb, xh))


def is_stable(name, seed):
    moved, x_moved = reference_movement(name, seed)
    return moved * STABILITY_MARGIN <= TOL and x_moved * STABILITY_MARGIN <= X_TOL


def choose_seed(name, seeds=range(8)):
    for seed in seeds:
        if is_stable(name, seed):
            return seed
    raise AssertionError(f'no stable scene for cell {name}')


def fallback_scene():
    """`online_mvdr_reference.fallback_case('first')` (D = 1, Phi_N = 0) as posteriors of three
    classes: class 1 owns the first three frames alone, so target 1 has no distortion mass there
    and falls back on them, while target 0 sees class 1 as distortion and never does.
    -> Y (F,T,D), gamma (F,K,T), the state to start from, beta, targets, the counts per target."""
    Y, mx, mn, state, beta, count = mref.fallback_case('first')
    g0 = mx.copy()
    g0[:, :3] = 0
    gamma = np.stack([g0, np.maximum(mn, 0.0) + 0.25, np.zeros_like(mx)], axis=1)
    gamma[:, 1, :3] = 0.5
    gamma[:, 2, 3:] = 0.125
    return Y, gamma, state, beta, (0, 1), (0, count)


if __name__ == '__main__':
    for name in CELLS:
        if name in sr.CELLS:
            moved, x_moved = reference_movement(name, seed_of(name))
            print(f"    # '{name}' (seed {seed_of(name)} of stream_reference): moves {moved:.1e}, "
                  f"|x_hat| {x_moved:.1e}, stable {is_stable(name, seed_of(name))}")
            continue
        seed = choose_seed(name)
        moved, x_moved = reference_movement(name, seed)
        print(f"    '{name}': {seed},   # moves {moved:.1e}, |x_hat| {x_moved:.1e}")
