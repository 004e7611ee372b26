"""What S speakers of one stream cost, from host samples to host samples, at the shapes of
tools/stream_cost.py (F = 513, 16 kHz; one_array (D, K) = (4, 4), joint24 (24, 5) with the online
WPE per array) for blocks of 256 samples (one hop) and 160 000 samples, S = 2 and S = K - 1.
Contenders, ALTERNATING inside one process after a warm-up:

    singles   S single-target `StreamingEnhancer`s fed the block one after another
    targets   one `StreamingEnhancer(targets=...)`, one gss_stream_block_targets call per block

Every stream keeps running from block to block (its states carried), cycling through one 10 s
scene.  One JSON line per (shape, block, S): per contender the median ms per block and the spread
(min, max) of the rounds, their ratio, and the per-kernel event times of one profiled block of
each contender (runs of their own after the timed rounds; `singles`: of ONE of the S streams) --
against the expectation of DESIGN.md section 27.  Lines are written as they are measured.

    python tools/stream_targets_cost.py [--steps 3] [--hop-steps 200] [--rounds 7] [--warmup 1] [--shape all|NAME] [--out FILE]"""
import argparse
import json
import time

import numpy as np

from stream_cost import DELAY, N, R, RATE, SHAPES, SHIFT, SIZE, TAPS, scene

BLOCKS = (256, 160000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--hop-steps', type=int, default=200,
                    help='steps of a timed window of one-hop blocks: long enough to time')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--shape', default='all')
    ap.add_argument('--out', default=str(R / 'profiles' / 'stream_targets_cost.jsonl'))
    args = ap.parse_args()
    from pb_chime5_amd._capi import default_context
    ctx = default_context(0)
    with open(args.out, 'a' if args.shape != 'all' else 'w') as fd:
        for name, D, K, A in SHAPES:
            if args.shape not in ('all', name):
                continue
            x, act = scene(np.random.default_rng(D), D, K)
            for block in BLOCKS:
                for S in sorted({2, K - 1}):
                    fd.write(json.dumps(measure(ctx, args, name, D, K, A, block, S, x, act)) + '\n')
                    fd.flush()


def profile_of(ctx, fn):
    ctx.profile_reset()
    ctx.profile_enable(True)
    fn()
    report = ctx.profile_report()
    ctx.profile_enable(False)
    ctx.profile_reset()
    return {k: dict(calls=v['calls'], ms=round(v['ms'], 4)) for k, v in report.items()}


def measure(ctx, args, name, D, K, A, block, S, x, act):
    from pb_chime5_amd.streaming import StreamingEnhancer
    kw = dict(stft_size=SIZE, stft_shift=SHIFT, wpe_taps=TAPS, wpe_delay=DELAY, wpe_arrays=A, ctx=ctx)
    singles = [StreamingEnhancer(D, K, target=s, **kw) for s in range(S)]
    targets = StreamingEnhancer(D, K, targets=range(S), **kw)
    at = {'singles': 0, 'targets': 0}

    def cut(v):
        a = at[v]
        at[v] = (a + block) % N if a + 2 * block <= N else 0
        return x[:, a:a + block], act[:, a:a + block]

    def run_singles():
        blk, activity = cut('singles')
        return np.stack([enh.process(blk, activity) for enh in singles])

    def run_targets():
        return targets.process(*cut('targets'))
    calls = {'singles': run_singles, 'targets': run_targets}
    steps = args.steps if block > SHIFT else args.hop_steps
    for fn in calls.values():
        for _ in range(args.warmup):
            fn()
    ms = {v: [] for v in calls}
    for _ in range(args.rounds):
        for v, fn in calls.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                out = fn()
            ms[v].append(1e3 * (time.perf_counter() - t0) / steps)
            assert out.shape[0] == S and np.all(np.isfinite(out)), v
    med = {v: float(np.median(t)) for v, t in ms.items()}
    one = singles[0]
    kernels = {'targets': profile_of(ctx, run_targets),
               'one_single': profile_of(ctx, lambda: one.process(*cut('singles')))}
    duration = 1e3 * block / RATE
    line = dict(case=name, D=D, K=K, wpe_arrays=A, F=SIZE // 2 + 1, block=block, S=S,
                frames=block // SHIFT, block_ms=duration, steps=steps, rounds=args.rounds,
                warmup=args.warmup, fallbacks=dict(targets.fallbacks),
                ms={v: dict(median=round(med[v], 4), min=round(min(t), 4), max=round(max(t), 4))
                    for v, t in ms.items()},
                times_real_time={v: round(duration / med[v], 1) for v in med},
                singles_over_targets=round(med['singles'] / med['targets'], 2),
                targets_over_one_single=round(med['targets'] / (med['singles'] / S), 2),
                kernels_of_one_block_ms=kernels)
    print(json.dumps(line), flush=True)
    return line


if __name__ == '__main__':
    main()
