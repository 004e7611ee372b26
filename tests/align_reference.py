"""NumPy reference of the permutation alignment (gss_cacgmm_align, include/gss_hip.h) and the
scenes the CPU and the GPU tests share.

The definition, for posteriors gamma (F,K,T):

* features  ``feat[f,j,:] = gamma[f,j,:] / sqrt(sum_t gamma[f,j,t]^2)``, all zero for a zero row;
* the mapping (F,K) starts as the identity; a plan entry ``(iterations, start, end)`` runs up to
  ``iterations`` passes over ``[start, end)``; a pass forms ``c[k,:] = sum_f feat[f, mapping[f,k], :]``
  over the range, scales every row to unit norm (a zero row stays zero), and gives every f of the
  range, all from the same c, the permutation p that maximises ``sum_k <c[k,:], feat[f,p[k],:]>``
  over all K! permutations, the lexicographically smallest among exact maxima; a pass that changes
  no mapping ends the entry;
* ``aligned[f,k,:] = gamma[f, mapping[f,k], :]`` and ``activity[k,t] = mean_f aligned[f,k,t]``.

`align` also returns the MARGIN: the smallest gap between the best and the second-best total over
all passes and frequencies.  A parity scene is kept only if its margin is at least `MIN_MARGIN`
(four orders above what two float64 summation orders of unit-norm rows can differ by), so that
the GPU's mapping can be asked to EQUAL the reference's; otherwise the next seed of range(8) is
taken.  Every reference run is computed once per session and shared."""
import functools
import itertools

import numpy as np

import gss_oracle as oracle
import shared_prior_reference as spr

MIN_MARGIN = 1e-9
ACTIVITY_TOL = 1e-10        # the bar of the project's other fixed-order float64 reductions
POSTERIOR_TOL = 1e-7        # tests/test_gpu_cacgmm_model.py: max |posterior - reference|


@functools.lru_cache(maxsize=None)
def permutations(K):
    """All K! permutations in lexicographic order, (K!, K) int."""
    return np.array(list(itertools.permutations(range(K))), dtype=np.int64).reshape(-1, K)


def features(gamma):
    gamma = np.asarray(gamma, np.float64)
    n = np.sqrt(np.sum(gamma * gamma, axis=-1, keepdims=True))
    return np.where(n > 0, gamma / np.where(n > 0, n, 1.0), 0.0)


def align(gamma, plan):
    """gamma (F,K,T), plan [(iterations, start, end), ...] -> mapping (F,K) int32, margin, number
    of passes that ran."""
    gamma = np.asarray(gamma, np.float64)
    F, K, T = gamma.shape
    feat = features(gamma)
    perms = permutations(K)
    mapping = np.tile(np.arange(K, dtype=np.int32), (F, 1))
    margin, passes = np.inf, 0
    ks = np.arange(K)
    for iterations, start, end in plan:
        assert iterations >= 1 and 0 <= start < end <= F, (iterations, start, end, F)
        for _ in range(iterations):
            passes += 1
            rows = np.arange(start, end)
            c = np.sum(feat[rows[:, None], mapping[start:end]], axis=0)          # (K,T)
            n = np.sqrt(np.sum(c * c, axis=-1, keepdims=True))
            c = np.where(n > 0, c / np.where(n > 0, n, 1.0), 0.0)
            S = np.einsum('kt,fjt->fkj', c, feat[start:end])                     # (n,K,K)
            totals = np.sum(S[:, ks[None, :], perms], axis=-1)                   # (n,K!)
            best = np.argmax(totals, axis=1)                                     # the first maximum
            if perms.shape[0] > 1:
                srt = np.sort(totals, axis=1)
                margin = min(margin, float(np.min(srt[:, -1] - srt[:, -2])))
            new = perms[best].astype(np.int32)
            changed = not np.array_equal(new, mapping[start:end])
            mapping[start:end] = new
            if not changed:
                break
    return mapping, margin, passes


def gather(gamma, mapping):
    """aligned[f,k,:] = gamma[f, mapping[f,k], :]"""
    gamma = np.asarray(gamma)
    return gamma[np.arange(gamma.shape[0])[:, None], mapping]


def activity(aligned):
    return np.mean(aligned, axis=0)


def moved(mapping):
    """Frequencies whose row is not the identity (gss_last_align_moved)."""
    return int(np.sum(np.any(mapping != np.arange(mapping.shape[1]), axis=1)))


def align_ktf(posterior, plan):
    """posterior (K,T,F) -> aligned (K,T,F), mapping (F,K), activity (K,T), margin."""
    gamma = np.ascontiguousarray(np.asarray(posterior).transpose(2, 0, 1))
    mapping, margin, _ = align(gamma, plan)
    aligned = gather(gamma, mapping)
    return aligned.transpose(1, 2, 0), mapping, activity(aligned), margin


def is_permutation_rows(mapping):
    K = mapping.shape[1]
    return bool(np.array_equal(np.sort(mapping, axis=1), np.broadcast_to(np.arange(K), mapping.shape)))


def global_permutation(mapping_a, mapping_b):
    """The one permutation q with mapping_a[f, k] == mapping_b[f, q[k]] for every f, or None."""
    K = mapping_a.shape[1]
    for q in permutations(K):
        if np.array_equal(mapping_a, mapping_b[:, q]):
            return q
    return None


# ------------------------------------------------------------------ parity scenes
# (D, T, F, K): the issue's eight, then the column sum's slices (F = 513), T < 64 and K = 1
CELLS = [(4, 70, 5, 2), (4, 327, 9, 3), (6, 135, 16, 5), (7, 200, 33, 4), (8, 135, 12, 8),
         (4, 64, 1, 3), (5, 65, 2, 6), (6, 130, 40, 7),
         (4, 70, 513, 3), (4, 37, 6, 3), (4, 90, 7, 1)]
# seed of every cell whose seed 0 does not pass the margin rule for both plans
# (`python tests/align_reference.py` re-derives the table).  Seed 0 passed in all eleven: the
# margins are 2.5e-6 (K = 8) ... 1.6 (F = 1), so the table is empty.
SEEDS = {}


def plans(F):
    """The two plans of a parity cell."""
    from pb_chime5_amd import ops
    return ([(4, 0, F)],
            ops.alignment_plan(F, segment_start=F // 3, segment_width=max(F // 3, 1),
                               segment_shift=max(F // 8, 1), main_iterations=6, sub_iterations=2))


@functools.lru_cache(maxsize=None)
def parity_input(cell, seed):
    """gamma (F,K,T) of a cell: per-frequency oracle EM, 5 iterations, from a random (F,K,T) start
    on `spr.parity_scene` -- classes numbered independently in every bin.  Read-only."""
    D, T, F, K = cell
    Y, _ = spr.parity_scene(D, T, F, K, seed)
    start = np.random.default_rng([seed, 7]).uniform(0.01, 1.0, size=(F, K, T))
    start = start / start.sum(axis=1, keepdims=True)
    posterior, _ = spr.shared_prior_block(Y, start, None, 5, 1, trainer=oracle.CACGMMTrainer)
    gamma = np.ascontiguousarray(posterior.transpose(2, 0, 1))
    gamma.setflags(write=False)
    return gamma


@functools.lru_cache(maxsize=None)
def parity_reference(cell, seed, plan_index):
    gamma = parity_input(cell, seed)
    mapping, margin, passes = align(gamma, plans(cell[2])[plan_index])
    mapping.setflags(write=False)
    return mapping, margin, passes


def cell_margin(cell, seed):
    return min(parity_reference(cell, seed, i)[1] for i in range(2))


def seed_of(cell):
    return SEEDS.get(cell, 0)


def choose_seed(cell, seeds=range(8)):
    for seed in seeds:
        if cell_margin(cell, seed) >= MIN_MARGIN:
            return seed
    raise AssertionError(f'no scene with a margin of {MIN_MARGIN} for {cell}')


# ------------------------------------------------------------------ the method's scenes
TABLE_RUNS = [(0, 4), (1, 4), (0, 6)]       # (seed, D) of spr.table_scene
TABLE_PLAN_F = 129


def table_starts(seed, D):
    """The two starts of the method test for a table scene: a random (K,T,F) start (classes
    numbered independently per bin) and the common (K,T) blind start."""
    from pb_chime5_amd import ops
    Obs, truth = spr.table_scene(seed, D)
    _, T, F = Obs.shape
    rng = np.random.default_rng([seed, D, 11])
    rand = rng.uniform(0.01, 1.0, size=(spr.TABLE_K, T, F))
    rand = rand / rand.sum(axis=0, keepdims=True)
    return Obs, truth, {'random': rand,
                        'blind': ops.blind_initialization(spr.TABLE_K, T, seed + 100)}


def scramble(posterior, seed):
    """posterior (K,T,F) with a random permutation of the classes in every bin, and the (F,K)
    mapping that was applied: scrambled[k,:,f] = posterior[perm[f,k],:,f]."""
    K, T, F = posterior.shape
    rng = np.random.default_rng([seed, 23])
    perm = np.stack([rng.permutation(K) for _ in range(F)]).astype(np.int32)
    out = np.asarray(posterior)[perm.T[:, None, :], np.arange(T)[None, :, None],
                                np.arange(F)[None, None, :]]
    return np.ascontiguousarray(out), perm


if __name__ == '__main__':
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    for cell in CELLS:
        seed = choose_seed(cell)
        print(f'    {cell}: {seed},   # margin {cell_margin(cell, seed):.1e}, passes '
              f'{[parity_reference(cell, seed, i)[2] for i in range(2)]}, moved '
              f'{[moved(parity_reference(cell, seed, i)[0]) for i in range(2)]}')
