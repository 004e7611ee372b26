"""NumPy reference of the online MVDR's filter look-ahead (gss_mvdr_online_lookahead), built on the
untouched tests/online_mvdr_reference.py: the one-shot formula from that reference's filters, the
block form with a list of held frames, the onset scene, and the cells the CPU and the GPU tests
share.  Every reference run is computed once per session and shared, read-only.

Frames are numbered g = 0, 1, ... over the life of a delay line, w_g is the filter the online MVDR
solves at frame g, G the frames that had entered when the line was released:
    X[g] = w_{min(g + L, G - 1)}^H y_g,    the filter row g is w_{min(g + L, G - 1)}"""
import functools

import numpy as np

import online_mvdr_reference as mr

MAX_LOOKAHEAD = 64
# (D, beta, loading, F, T, L); each runs with ban False and True and with ref_channel 0 and D - 1
CELLS = [
    (4, 0.99, 1e-2, 3, 150, 4),      # the headline small case
    (1, 0.9, 1.0, 1, 5, 1),          # D = 1
    (1, 0.9, 1.0, 1, 5, 8),          # L > T: everything comes from the release
    (9, 0.99, 1.0, 2, 64, 3),        # NR 2
    (17, 0.99, 1.0, 2, 64, 16),      # NR 3
    (24, 0.995, 1.0, 2, 120, 8),     # 24 channels
    (32, 0.999, 1.0, 1, 64, 64),     # both bounds
]
# seed of every cell whose seed 0 did not pass: a seed is kept only if the reference's own
# look-ahead X moves at least STABILITY_MARGIN x less than TOL when every sample and mask value
# moves in its last bit, for both values of ban and both reference channels (`python
# tests/online_mvdr_lookahead_reference.py` re-derives the table).
SEEDS = {}
PARTITION_CELL = CELLS[0]
PARTITIONS = [(1, 63, 64, 22), (1, 1, 1, 1, 1, 145), (3, 1, 5, 141), (1,) * 150]
CPU_PARTITION = (1, 2, 3, 4, 5, 100, 1, 184)     # of the onset scene's 300 frames

# the onset scene: the target is silent and its mask 0 for the first ONSET frames
ONSET_CELL = (4, 0.99, 1e-2, 8, 300)
ONSET = 100
ONSET_FRAMES = 16            # the error is taken over the 16 frames after the onset
ONSET_LOOKAHEAD = 4
ONSET_BOUND = 0.5            # a condition, not a measurement: error(L = 4) / error(L = 0)
ONSET_SEED = 0


def seed_of(cell):
    return SEEDS.get(cell, 0)


def lookahead_rows(T, L, G=None):
    """The filter frame of every output frame: min(g + L, G - 1)."""
    return np.minimum(np.arange(T) + L, (T if G is None else G) - 1)


def one_shot(Y, W, L):
    """X (F,T) and the filter rows (F,T,D) of a line that took the T frames of Y (F,T,D) and was
    released, from the filters W (F,T,D) of `mr.online_mvdr`."""
    rows = lookahead_rows(Y.shape[1], L)
    Wl = W[:, rows]
    return np.einsum('ftd,ftd->ft', Wl.conj(), Y), Wl


def lookahead_mvdr(Y, mx, mn, beta, ref, ban, L, state=None, loading=None):
    """`mr.online_mvdr` with the look-ahead L, one call and its release -> X, the filter rows, the
    state after the T frames and the fallback count (that of L = 0)."""
    _, W, st, fallbacks = mr.online_mvdr(Y, mx, mn, beta, ref, ban, state=state, loading=loading)
    X, Wl = one_shot(np.asarray(Y, np.complex128), W, L)
    return X, Wl, st, fallbacks


class Line:
    """The block form: a list of held frames and the last filter.  `step` takes the next frames
    and returns what they release, `release` the rest."""

    def __init__(self, L):
        self.L, self.held, self.last = L, [], None

    def step(self, Y, mx, mn, beta, ref, ban, state):
        """Y (F,T,D) -> X (F,R), the filter rows (F,R,D), the state after the T frames."""
        _, W, state, _ = mr.online_mvdr(Y, mx, mn, beta, ref, ban, state=state)
        F, T, D = Y.shape
        X, rows = [], []
        for t in range(T):
            self.held.append(np.asarray(Y[:, t], np.complex128))
            self.last = W[:, t]
            if len(self.held) > self.L:
                y = self.held.pop(0)
                X.append(np.einsum('fd,fd->f', self.last.conj(), y))
                rows.append(self.last)
        X = np.stack(X, axis=1) if X else np.zeros((F, 0), np.complex128)
        rows = np.stack(rows, axis=1) if rows else np.zeros((F, 0, D), np.complex128)
        return X, rows, state

    def release(self):
        if not self.held:
            return None
        X = np.stack([np.einsum('fd,fd->f', self.last.conj(), y) for y in self.held], axis=1)
        self.held = []
        return X


def in_blocks(Y, mx, mn, beta, ref, ban, loading, L, blocks):
    """The scene through one `Line` in consecutive blocks, then the release -> X (F,T), the list
    of frames every call released."""
    state = mr.fresh_state(Y.shape[0], Y.shape[2], loading, Y)
    line, Xs, counts, t0 = Line(L), [], [], 0
    for n in blocks:
        X, _, state = line.step(Y[:, t0:t0 + n], mx[:, t0:t0 + n], mn[:, t0:t0 + n], beta, ref, ban,
                                state)
        Xs.append(X)
        counts.append(X.shape[1])
        t0 += n
    assert t0 == Y.shape[1]
    tail = line.release()
    if tail is not None:
        Xs.append(tail)
    return np.concatenate(Xs, axis=1), counts


def released(blocks, L):
    """Frames every call of a line releases: max(0, h + T - L) with h = min(L, frames so far)."""
    out, h = [], 0
    for n in blocks:
        out.append(max(0, h + n - L))
        h = min(L, h + n)
    return out


def variants(cell):
    return mr.variants(cell[:5])


@functools.lru_cache(maxsize=None)
def reference(cell, ban, ref, seed=0):
    """X (F,T), the filter rows (F,T,D), the final state and the fallback count of the cell."""
    D, beta, loading, F, T, L = cell
    Y, mx, mn, _ = mr.scene(cell[:5], seed)
    X, Wl, st, fallbacks = lookahead_mvdr(Y, mx, mn, beta, ref, ban, L, loading=loading)
    for a in (X, Wl, st['phi_x'], st['phi_n']):
        a.setflags(write=False)
    return X, Wl, st, fallbacks


def reference_movement(cell, seed=0):
    """How far the reference's look-ahead X moves under a last-bit change of every sample and mask
    value, relative; the largest over the cell's variants."""
    D, beta, loading, F, T, L = cell
    Y, mx, mn, _ = mr.scene(cell[:5], seed)
    rng = np.random.default_rng(12345)
    Yb, mxb, mnb = mr.last_bit(Y, rng), mr.last_bit(mx, rng), mr.last_bit(mn, rng)
    worst = 0.0
    for ban, ref in variants(cell):
        X = reference(cell, ban, ref, seed)[0]
        Xb = lookahead_mvdr(Yb, mxb, mnb, beta, ref, ban, L, loading=loading)[0]
        worst = max(worst, mr.rel_err(Xb, X))
    return worst


def choose_seed(cell, seeds=range(8)):
    for seed in seeds:
        if reference_movement(cell, seed) * mr.STABILITY_MARGIN <= mr.TOL:
            return seed
    raise AssertionError(f'no stable scene for {cell}')


# ------------------------------------------------------------------ the onset scene
@functools.lru_cache(maxsize=None)
def onset_scene(seed=ONSET_SEED, beta=None):
    """`mr.scene(ONSET_CELL)` with the target silent and its mask 0 for the first ONSET frames; the
    interferer and the noise as there.  -> Y (F,T,D), mx, mn (F,T), the target's image (F,T,D)."""
    Y, mx, mn, image = mr.scene(ONSET_CELL, seed)
    Y, mx, mn, image = Y.copy(), mx.copy(), mn.copy(), image.copy()
    Y[:, :ONSET] -= image[:, :ONSET]
    image[:, :ONSET] = 0
    mx[:, :ONSET] = 0
    mn[:, :ONSET] = 1
    for a in (Y, mx, mn, image):
        a.setflags(write=False)
    return Y, mx, mn, image


def onset_error(X, image0):
    """The energy of X - (the target's image at channel 0) over the ONSET_FRAMES frames after the
    onset, relative to that image's energy.  X, image0 (F,T)."""
    sl = slice(ONSET, ONSET + ONSET_FRAMES)
    return float(np.sum(np.abs(X[:, sl] - image0[:, sl]) ** 2) / np.sum(np.abs(image0[:, sl]) ** 2))


def onset_errors(L=ONSET_LOOKAHEAD, seed=ONSET_SEED, beta=None, X=None):
    """(error at L = 0, error at L) of the reference on the onset scene (``X``: the look-ahead
    output to judge in the reference's place); ban False, ref 0."""
    D, beta0, loading, F, T = ONSET_CELL
    beta = beta0 if beta is None else beta
    Y, mx, mn, image = onset_scene(seed)
    X0, W, _, _ = mr.online_mvdr(Y, mx, mn, beta, 0, False, loading=loading)
    if X is None:
        X = one_shot(Y, W, L)[0]
    return onset_error(X0, image[:, :, 0]), onset_error(X, image[:, :, 0])


def onset_ratio(L=ONSET_LOOKAHEAD, seed=ONSET_SEED, beta=None, X=None):
    e0, eL = onset_errors(L, seed, beta, X)
    return eL / e0


if __name__ == '__main__':
    for cell in CELLS:
        seed = choose_seed(cell)
        print(f'    {cell}: {seed},   # moves {reference_movement(cell, seed):.1e}')
    for beta in (0.99, 0.95):
        for seed in range(6):
            e0, eL = onset_errors(seed=seed, beta=beta)
            print(f'onset, forget {beta}, seed {seed}: error {e0:.3f} at L = 0, {eL:.3f} at '
                  f'L = {ONSET_LOOKAHEAD}, ratio {eL / e0:.3f}')
