"""What the WPD beamformer costs: bf='wpdSouden_ban' (1 and 2 iterations) against
'mvdrSouden_ban' on the config-2 scene (24 channels, 15 s, 4 speakers + Noise; F = 513, T = 941,
K = 5) and on one array of it (4 channels), resident in HBM.  A warm-up, then `steps` fused calls
with HIP events around every launch (gss_profile_report): milliseconds per utterance, summed over
the kernels, and per kernel name.  No target is attached to the figures.

One JSON line, also written to profiles/wpd_cost.jsonl.

    python tools/wpd_cost.py [--steps 5] [--warmup 2]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

R = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(R))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=str(R / 'profiles' / 'wpd_cost.jsonl'))
    args = ap.parse_args()
    from pb_chime5_amd import ops, synthetic
    from pb_chime5_amd._capi import default_context
    ctx = default_context(0)
    params = ops.make_params(wpe=True, wpe_taps=10, wpe_delay=2, wpe_iterations=3,
                             bss_iterations=20, bss_iterations_post=1)
    ops._prepare_windows(ctx, params.stft_size, params.stft_shift)
    result = {}
    for D in (24, 4):
        utt = synthetic.config2(seed=2, num_channels=D, seconds=15.0, num_speakers=4)
        c0 = utt.ex['start_orig']['original']
        c1 = utt.ex['end']['original'] - utt.ex['end_orig']['original']
        res = ops.ResidentUtterance(ctx, utt.obs, utt.activity_array, params)
        for name, iterations in (('mvdrSouden_ban', 0), ('wpdSouden_ban', 1),
                                 ('wpdSouden_ban, 2 iterations', 2)):
            wpd = ops.check_bf_wpd(10, 2, iterations, ops.WPD_POWER_FLOOR, True, D) \
                if iterations else None
            for _ in range(args.warmup):
                res.enqueue(utt.target_index, c0, c1, wpd=wpd)
            ctx.synchronize()
            ctx.profile_filter(None)
            ctx.profile_enable(True)
            ctx.profile_reset()
            for _ in range(args.steps):
                res.enqueue(utt.target_index, c0, c1, wpd=wpd)
            ctx.synchronize()
            prof = ctx.profile_report()
            ctx.profile_enable(False)
            x_hat = res.result()
            result[f'D={D} {name}'] = dict(
                ms_per_utterance=round(sum(v['ms'] for v in prof.values()) / args.steps, 3),
                kernels_ms={k: round(v['ms'] / args.steps, 4) for k, v in sorted(prof.items())},
                launches={k: v['calls'] // args.steps for k, v in sorted(prof.items())},
                frames=res.T, finite=bool(np.all(np.isfinite(x_hat))),
                wpd_zero_pivots=ctx.last_wpd_zero_pivots() if iterations else None)
            print(f'D={D} {name}: {result[f"D={D} {name}"]["ms_per_utterance"]} ms', flush=True)
    line = json.dumps(dict(tool='wpd_cost', steps=args.steps, **result))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, 'a') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
