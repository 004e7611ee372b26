"""What the fused annotation-free window call saves, and what a link costs.

Per window, from host samples to host signals, on one synthetic window at the headline shape
(24 ch, T = 941, K = 5) and the one-array shape (4 ch, T = 2169, K = 5), F = 513, WPE 10 taps x 3
iterations, 20 EM iterations:

    stage    Enhancer.enhance_observation_blind(fused=False): the stage operators, a host round
             trip after the STFT, after WPE and after the EM, K beamformer calls, K iSTFTs (the
             path the parent commit has: the baseline)
    fused    Enhancer.enhance_observation_blind(fused=True): gss_separate_observation, one call
    resident the same library call alone, inputs and outputs in HBM (ops.ResidentSeparation)

and gss_cacgmm_link alone on two (F,K,T) tables in HBM over L = T // 2 shared frames.

bench.py's protocol: a warm-up, then the forms ALTERNATE inside one process; every round times
`steps` calls of each between two device synchronisations.  One JSON line per shape: per form
the median ms and the spread (min, max) of its rounds, the ratio of the medians, and whether the
fused form is faster by more than the spread (the larger of the two forms' max - min).

    python tools/recording_cost.py [--steps 2] [--rounds 5] [--warmup 1]
                                   [--shape all|headline|one_array] [--out FILE]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

R = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(R))

F = 513
SHAPES = [('headline (24 ch, T = 941, K = 5)', 24, 240000, 5),
          ('one array (4 ch, T = 2169, K = 5)', 4, 554490, 5)]


def window(D, N, K):
    """K - 1 speakers with staggered activity through 512-tap rooms -> obs (D,N)."""
    from pb_chime5_amd import synthetic
    step = N // (K + 1)
    intervals = [(k * step, min(N, (k + 3) * step)) for k in range(K - 1)]
    return synthetic.make_utterance(D + K, D, N, intervals, rir_taps=512, noise=1e-2,
                                    fast=True).obs


def spread(values):
    return dict(median=round(float(np.median(values)), 4), min=round(min(values), 4),
                max=round(max(values), 4))


def rounds_of(ctx, calls, args, steps):
    for fn in calls.values():
        for _ in range(args.warmup):
            fn()
    ms = {v: [] for v in calls}
    for _ in range(args.rounds):
        for v, fn in calls.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            ctx.synchronize()
            ms[v].append(1e3 * (time.perf_counter() - t0) / steps)
    return ms


def measure(ctx, args, name, D, N, K):
    from pb_chime5_amd import core, ops
    obs = window(D, N, K)
    enh = core.get_enhancer(bss_iterations=20)
    T = ops.stft_frames(N, 1024, 256, True)
    params = enh._blind_params()
    ops._prepare_windows(ctx, 1024, 256, None)
    win = ops.ResidentSeparation(ctx, obs, ops.blind_initialization(K, T, 0), params)
    calls = {'stage': lambda: enh.enhance_observation_blind(obs, K - 1),
             'fused': lambda: enh.enhance_observation_blind(obs, K - 1, fused=True),
             'resident': win.enqueue}
    ms = rounds_of(ctx, calls, args, args.steps)
    # the link alone: the window's own posteriors against themselves, half the frames shared
    L = T // 2
    mapping_d, scores_d = ctx.empty(64), ctx.empty(8 * K * K)
    link = {'link': lambda: ops.link_posteriors_device(
        ctx, win.gamma_d, T, T - L, win.gamma_d, T, 0, L, F, K, mapping_d, scores_d)}
    link_ms = rounds_of(ctx, link, args, 20 * args.steps)
    ctx.profile_reset()
    ctx.profile_enable(True)
    link['link']()
    kernels = ctx.profile_report()
    ctx.profile_enable(False)
    ctx.profile_reset()
    med = {v: float(np.median(x)) for v, x in ms.items()}
    noise = max(max(ms[v]) - min(ms[v]) for v in ('stage', 'fused'))
    line = dict(case=name, D=D, N=N, T=T, K=K, F=F, steps=args.steps, rounds=args.rounds,
                warmup=args.warmup, ms={v: spread(x) for v, x in ms.items()},
                fused_over_stage=round(med['fused'] / med['stage'], 4),
                saved_ms=round(med['stage'] - med['fused'], 4), spread_ms=round(noise, 4),
                fused_is_faster_by_more_than_the_spread=bool(med['stage'] - med['fused'] > noise),
                link=dict(shared_frames=L, ms=spread(link_ms['link']),
                          kernels_of_one_call_ms={k: dict(calls=v['calls'], ms=round(v['ms'], 4))
                                                  for k, v in kernels.items()}))
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--shape', choices=('all', 'headline', 'one_array'), default='all')
    ap.add_argument('--out', default=str(R / 'profiles' / 'recording_cost.jsonl'))
    args = ap.parse_args()
    from pb_chime5_amd._capi import default_context
    ctx = default_context(0)
    lines = [measure(ctx, args, name, D, N, K) for name, D, N, K in SHAPES
             if args.shape == 'all' or (args.shape == 'one_array') == (D == 4)]
    with open(args.out, 'w') as fd:
        for line in lines:
            fd.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
