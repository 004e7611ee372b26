"""Random guided-EM inputs against the oracle, refereed in extended precision: 1 - 32 channels,
1 - 19 classes, 8 - 300 frames, classes that are active for a handful of frames or never, 1 - 5
iterations, 0 - 2 post iterations.  Where GPU and oracle differ by more than 1e-8 the frequency
that differs most is re-run by the 80-bit guided EM of tests/ext_precision.py (own Jacobi
eigensolver, same formulas): any two float64 implementations drift apart on classes with fewer
frames than channels (the 1e-10 eigenvalue floor cuts through a continuum of eigenvalues and every
iteration multiplies a rounding difference by 10 - 100), so the GPU is held to the ORACLE'S OWN
distance from the referee -- or, where that one sample of float64 noise happens to be small, to
what the oracle's output moves by when its input changes in the last bit (ext_precision.
em_yardstick): GPU - referee <= 5 x yardstick + 1e-9.  (Until round 5 the
yardstick was 30 x the distance between the oracle and a brute-force float64 EM that shares
LAPACK's eigh with it -- a ratio between two float64 programs, with one case at 35.7 explained by
hand two rounds running.)  The last line is a machine-written tally.
    python tools/fuzz_em.py [SEED] [CASES]
GSS_FUZZ_ZEROS=1: every case with a block of frames that are zero in every channel.
GSS_FUZZ_GUIDED=1: every case with weighted and per-frequency guidance (gss_cacgmm_guided): an
(F,K,T) initialisation of random weights on the activity, for every frequency or one table for all,
a mask with per-frequency holes, or no mask at all.  The referee takes a (K,T) activity only, so
these cases are held to the oracle's last-bit movement alone (4 draws): GPU - oracle <= 5 x
movement + 1e-9."""
import os
import sys
import warnings
from pathlib import Path

import numpy as np

R = Path(__file__).resolve().parents[1]
for p in (str(R), str(R / 'oracle'), str(R / 'tests')):
    sys.path.insert(0, p)


def oracle_guided(oracle, obs, init, mask, it, post):
    """obs (D,T,F), init (F,K,T), mask (F,K,T) bool or None -> (K,T,F): gss_block_batched's steps."""
    trainer = oracle.CACGMMTrainer()
    y = np.ascontiguousarray(obs.transpose(2, 1, 0))
    cur = trainer.fit(y, init, iterations=it, source_activity_mask=mask)
    if post == 0:
        return cur.predict(y, source_activity_mask=mask).transpose(1, 2, 0)
    if post != 1:
        cur = trainer.fit(y, cur, iterations=post - 1)
    return cur.predict(y).transpose(1, 2, 0)


def draw_guidance(rng, act, F):
    """Weighted, per-frequency guidance on the activity `act` (K,T): init (F,K,T), mask (F,K,T)
    bool or None."""
    K, T = act.shape
    mask = np.repeat(act[None], F, axis=0)
    if rng.integers(0, 2):
        for f in range(F):                                       # holes that differ by frequency
            a = int(rng.integers(0, T))
            mask[f, int(rng.integers(0, K)), a:a + int(rng.integers(1, T))] = False
    w = rng.uniform(0.05, 1.0, size=(F if rng.integers(0, 2) else 1, K, T))
    init = np.repeat(w, F // w.shape[0], axis=0) * np.where(mask, 1.0, 1e-10)
    init /= init.sum(axis=1, keepdims=True)
    return init, (mask if rng.integers(0, 4) else None)


def main():
    import gss_oracle as oracle
    from pb_chime5_amd import ops
    import ext_precision
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    cases = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    rng = np.random.default_rng(seed)
    warnings.simplefilter('ignore')
    bad = 0
    refereed = closer = 0
    worst_ratio = 0.0
    for case in range(cases):
        D = int(rng.integers(1, 33)); K = int(rng.integers(1, 20))
        T = int(rng.integers(8, 300)); F = int(rng.integers(1, 4))
        # GSS_FUZZ_D / GSS_FUZZ_KMAX / GSS_FUZZ_TMAX aim the sweep at one kernel family (the
        # draws above are still consumed): e.g. D = 4, K <= 6, up to 1200 frames = the one-launch
        # kernel of the one-array regime over several 256-frame chunks
        if os.environ.get('GSS_FUZZ_D'):
            D = int(os.environ['GSS_FUZZ_D'])
        if os.environ.get('GSS_FUZZ_KMAX'):
            K = 1 + K % int(os.environ['GSS_FUZZ_KMAX'])
        if os.environ.get('GSS_FUZZ_TMAX'):
            T = 8 + (T * 7919) % int(os.environ['GSS_FUZZ_TMAX'])
        it = int(rng.integers(1, 6)); post = int(rng.integers(0, 3))
        act = np.zeros((K, T), bool)
        act[-1] = True                                           # garbage class
        for k in range(K - 1):
            mode = int(rng.integers(0, 5))
            if mode == 0:
                continue                                         # never active
            a = int(rng.integers(0, T)); b = a + int(rng.integers(1, 6 if mode == 1 else T))
            act[k, a:b] = True
        if rng.integers(0, 6) == 0:
            act[-1] = rng.uniform(size=T) < 0.5                  # frames nobody claims
        steer = rng.standard_normal((F, K, D)) + 1j * rng.standard_normal((F, K, D))
        src = (rng.standard_normal((F, K, T)) + 1j * rng.standard_normal((F, K, T))) * act[None]
        obs = np.einsum('fkd,fkt->dtf', steer, src)
        obs = obs + 10.0 ** rng.uniform(-2, 0) * (rng.standard_normal(obs.shape) + 1j * rng.standard_normal(obs.shape))
        if os.environ.get('GSS_FUZZ_ZEROS'):
            # digital silence: frames that are zero in every channel (their quadratic forms sit
            # on the clamp max(|q|, tiny), where the eigenvalue normalisation of pb_bss shows --
            # EXPERIMENTS round 6, item 12); a generator of its own: the stream above is the same
            # with and without
            zr = np.random.default_rng([seed, case, 12])
            nz = int(zr.integers(1, max(2, T // 3)))
            a = int(zr.integers(0, T))
            zt = np.zeros(T, bool)
            zt[a:a + nz] = True                                  # a block ...
            zt[zr.integers(0, T, size=int(zr.integers(0, 4)))] = True    # ... and stray frames
            if zr.integers(0, 3) == 0:
                obs[:, zt, int(zr.integers(0, F))] = 0.0         # one frequency only
            else:
                obs[:, zt, :] = 0.0
        tag = dict(case=case, D=D, K=K, T=T, F=F, it=it, post=post, active=act.sum(axis=1).tolist())
        # GSS_FUZZ_ONLY=case: replay one case of the stream (the draws of the others are consumed)
        if os.environ.get('GSS_FUZZ_ONLY') and case != int(os.environ['GSS_FUZZ_ONLY']):
            continue
        res = {}
        sides = (('oracle', lambda: oracle.gss_block_batched(obs, act, iterations=it, iterations_post=post)),
                 ('gpu', lambda: ops.cacgmm_posteriors(obs, act, it, post)))
        guided = bool(os.environ.get('GSS_FUZZ_GUIDED'))
        if guided:
            # (a generator of its own: the stream above is the same with and without)
            init, mask = draw_guidance(np.random.default_rng([seed, case, 13]), act, F)
            tag['guided'] = dict(mask=mask is not None,
                                 per_f=bool(F > 1 and not np.array_equal(init[0], init[-1])))
            sides = (('oracle', lambda: oracle_guided(oracle, obs, init, mask, it, post)),
                     ('gpu', lambda: ops.cacgmm_posteriors_guided(
                         obs, init.transpose(1, 2, 0),
                         None if mask is None else mask.transpose(1, 2, 0), it, post)))
        for side, fn in sides:
            try:
                res[side] = fn()
            except (AssertionError, NotImplementedError, np.linalg.LinAlgError) as e:
                res[side] = type(e).__name__ + ': ' + str(e)[:80]
        o, g = res['oracle'], res['gpu']
        if isinstance(o, str) or isinstance(g, str):
            if isinstance(o, str) != isinstance(g, str):
                print('only one side raises:', 'oracle', o if isinstance(o, str) else '-', '| gpu',
                      g if isinstance(g, str) else '-', tag)
                bad += 1
            continue
        if np.isnan(o).any() or np.isnan(g).any():
            if not np.array_equal(np.isnan(o), np.isnan(g)):
                print('NaN pattern differs', int(np.isnan(o).sum()), int(np.isnan(g).sum()), tag)
                bad += 1
            continue
        d_go = np.max(np.abs(g - o))
        if d_go < 1e-8:
            continue
        f = int(np.argmax(np.max(np.abs(g - o), axis=(0, 1))))
        if guided:
            eps, pr, yard = np.finfo(np.float64).eps, np.random.default_rng(20260929), 0.0
            of = obs[..., f:f + 1]
            for _ in range(4):
                pert = of.real * (1 + eps * pr.choice([-1.0, 1.0], size=of.shape)) \
                    + 1j * of.imag * (1 + eps * pr.choice([-1.0, 1.0], size=of.shape))
                moved = oracle_guided(oracle, pert, init[f:f + 1],
                                      None if mask is None else mask[f:f + 1], it, post)
                yard = max(yard, float(np.max(np.abs(moved[..., 0] - o[..., f]))))
            refereed += 1
            worst_ratio = max(worst_ratio, d_go / max(yard, 1e-9))
            if not d_go <= 5 * yard + 1e-9:
                print('EM (guided): GPU-oracle', d_go, 'oracle last-bit movement', yard, 'frequency', f, tag)
                bad += 1
            continue
        r = ext_precision.guided_em(np.ascontiguousarray(obs[..., f].T), act, it, post)
        d_or = np.max(np.abs(o[..., f] - r))
        d_gr = np.max(np.abs(g[..., f] - r))
        # the yardstick: oracle - referee, or what the oracle's own output moves by when its
        # input changes in the last bit (ONE float64 run is one sample of the formulation's noise)
        yard = ext_precision.em_yardstick(np.ascontiguousarray(obs[..., f:f + 1]), act, it, post,
                                          o[..., f], r)
        refereed += 1
        worst_ratio = max(worst_ratio, d_gr / max(yard, 1e-9))
        closer += d_gr <= d_or
        if os.environ.get('GSS_FUZZ_DUMP'):
            # inputs and all three results of the replayed case, for a look at it on the CPU
            np.savez(os.environ['GSS_FUZZ_DUMP'], obs=obs, act=act, it=it, post=post, f=f, gpu=g,
                     oracle=o, referee=r)
        if os.environ.get('GSS_FUZZ_ONLY'):
            print('replay: GPU-oracle', np.max(np.abs(g[..., f] - o[..., f])), 'oracle-referee', d_or,
                  'GPU-referee', d_gr, 'yardstick', yard, tag)
        if not d_gr <= 5 * yard + 1e-9:
            print('EM: GPU-referee', d_gr, 'oracle-referee', d_or, 'yardstick', yard, 'frequency', f, tag)
            bad += 1
    print('em fuzz: seed', seed, 'cases', cases, 'failures', bad, 'refereed', refereed,
          'GPU closer to the referee than the oracle in', closer,
          'worst (GPU - referee) / yardstick', worst_ratio)


if __name__ == '__main__':
    main()
