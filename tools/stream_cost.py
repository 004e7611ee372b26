"""What a block of a sample-block stream costs, from host samples to host samples, at F = 513
(stft 1024 / 256) and 16 kHz:

    one_array   (D, K) = (4, 4)    joint online WPE, 10 taps
    joint24     (24, 5)            online WPE per array over 6 arrays, 10 taps

for blocks of 256 (one hop), 4096, 16 000 and 160 000 samples.  Contenders, ALTERNATING inside one
process after a warm-up: `fused` -- `StreamingEnhancer.process`, one gss_stream_block call per
block; `stages` -- the same blocks with ``fused=False``, through the stage operators with explicit
states; and, for the 160 000-sample block, `whole` -- one gss_enhance_observation_gss_online call
(online WPE, online CACGMM, online MVDR from fresh states) on those samples.  Every stream keeps
running from block to block (its states carried), cycling through one 10 s scene.  One JSON line
per (shape, block): per contender the median ms per block and the spread (min, max) of the rounds,
the block's own duration, how many times faster than real time the median is, and the per-kernel
event times of one profiled fused block (a run of its own after the timed rounds) -- against the
expectation of DESIGN.md section 26.  Lines are written as they are measured.

With ``--lookahead L`` a fourth contender `lookahead` joins: the fused stream with
``lookahead=L`` (one gss_stream_block_lookahead call per block), and the line gains its ratio to
`fused`; ``--blocks`` picks the block sizes.

    python tools/stream_cost.py [--steps 5] [--rounds 7] [--warmup 1] [--shape all|NAME] [--out FILE]
                                [--lookahead L] [--blocks N [N ...]]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

R = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(R))

RATE, SIZE, SHIFT, TAPS, DELAY, N = 16000, 1024, 256, 10, 2, 160000
SHAPES = [('one_array', 4, 4, 1), ('joint24', 24, 5, 6)]
BLOCKS = (256, 4096, 16000, 160000)


def scene(rng, D, K):
    """x (D,N) float64 and the activity (K,N) bool: K - 1 speakers, white noise through a random
    8-tap filter per channel, on in random turns of 0.5 s, a last class that is always on, sensor
    noise."""
    act = np.ones((K, N), bool)
    x = 0.1 * rng.standard_normal((D, N))
    for k in range(K - 1):
        act[k] = np.repeat(rng.random(-(-N // 8000)) < 0.6, 8000)[:N]
        src = rng.standard_normal(N) * act[k]
        x += np.stack([np.convolve(src, h)[:N] for h in rng.standard_normal((D, 8))])
    return x, act


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--shape', default='all')
    ap.add_argument('--out', default=str(R / 'profiles' / 'stream_cost.jsonl'))
    ap.add_argument('--lookahead', type=int, default=0)
    ap.add_argument('--blocks', type=int, nargs='+', default=list(BLOCKS))
    args = ap.parse_args()
    from pb_chime5_amd._capi import default_context
    ctx = default_context(0)
    with open(args.out, 'a' if args.shape != 'all' else 'w') as fd:
        for name, D, K, A in SHAPES:
            if args.shape not in ('all', name):
                continue
            x, act = scene(np.random.default_rng(D), D, K)
            for block in args.blocks:
                fd.write(json.dumps(measure(ctx, args, name, D, K, A, block, x, act)) + '\n')
                fd.flush()


def measure(ctx, args, name, D, K, A, block, x, act):
    from pb_chime5_amd import ops
    from pb_chime5_amd.streaming import StreamingEnhancer
    kw = dict(stft_size=SIZE, stft_shift=SHIFT, wpe_taps=TAPS, wpe_delay=DELAY, wpe_arrays=A, ctx=ctx)
    streams = {'fused': StreamingEnhancer(D, K, fused=True, **kw),
               'stages': StreamingEnhancer(D, K, fused=False, **kw)}
    if args.lookahead:
        streams['lookahead'] = StreamingEnhancer(D, K, fused=True, lookahead=args.lookahead, **kw)
    at = {v: 0 for v in streams}

    def step(v):
        a = at[v]
        at[v] = (a + block) % N if a + 2 * block <= N else 0
        return streams[v].process(x[:, a:a + block], act[:, a:a + block])
    calls = {v: (lambda v=v: step(v)) for v in streams}
    if block == N:
        calls['whole'] = lambda: ops.enhance_observation_gss_online(
            x, act, 0, 0, 0, bf_online=True, ref_channel=0, wpe_online=True, wpe_arrays=A, ctx=ctx,
            stft_size=SIZE, stft_shift=SHIFT, wpe_taps=TAPS, wpe_delay=DELAY)
    for fn in calls.values():
        for _ in range(args.warmup):
            fn()
    ms = {v: [] for v in calls}
    for _ in range(args.rounds):
        for v, fn in calls.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                out = fn()
            ms[v].append(1e3 * (time.perf_counter() - t0) / args.steps)
            assert np.all(np.isfinite(out)), v
    med = {v: float(np.median(t)) for v, t in ms.items()}
    ctx.profile_reset()
    ctx.profile_enable(True)
    calls['fused']()
    report = ctx.profile_report()
    ctx.profile_enable(False)
    ctx.profile_reset()
    duration = 1e3 * block / RATE
    line = dict(case=name, D=D, K=K, wpe_arrays=A, F=SIZE // 2 + 1, block=block,
                frames=block // SHIFT, block_ms=duration, steps=args.steps, rounds=args.rounds,
                warmup=args.warmup, fallbacks=dict(streams['fused'].fallbacks),
                ms={v: dict(median=round(med[v], 4), min=round(min(t), 4), max=round(max(t), 4))
                    for v, t in ms.items()},
                times_real_time={v: round(duration / med[v], 1) for v in med},
                faster_than_its_duration={v: bool(med[v] < duration) for v in med},
                stages_over_fused=round(med['stages'] / med['fused'], 2),
                kernels_of_one_fused_block_ms={k: dict(calls=v['calls'], ms=round(v['ms'], 4))
                                               for k, v in report.items()})
    if 'lookahead' in med:
        line['lookahead'] = args.lookahead
        line['lookahead_over_fused'] = round(med['lookahead'] / med['fused'], 3)
    if 'whole' in med:
        line['fused_over_whole'] = round(med['fused'] / med['whole'], 3)
    print(json.dumps(line), flush=True)
    return line


if __name__ == '__main__':
    main()
