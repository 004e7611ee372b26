"""What the posterior activity costs at the headline workload: the config-2 scene (24 channels,
15 s, 4 speakers + Noise; F = 513, T = 941, K = 5) resident in HBM.

    stage    gss_posterior_activity on the utterance's own post-WPE observation and posteriors
             (the debug taps of one call), `steps` calls profiled: ms per call of pact_sums and
             pact_scores (gss_profile_report) and their algorithmic bytes 16 F T D + 8 F K T over
             that time
    fused    gss_enhance_observation_activity against gss_enhance_observation with bench.py's
             protocol -- a warm-up, then `steps` utterances enqueued back to back that end in ONE
             synchronisation --, the two ALTERNATING inside one process over `rounds` rounds

One JSON line, also written to profiles/posterior_activity_cost.jsonl.

    python tools/posterior_activity_cost.py [--steps 10] [--rounds 5] [--warmup 3]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

R = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(R))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=str(R / 'profiles' / 'posterior_activity_cost.jsonl'))
    args = ap.parse_args()
    from pb_chime5_amd import ops, synthetic
    from pb_chime5_amd._capi import c_void_p, default_context
    ctx = default_context(0)
    utt = synthetic.config2(seed=2, num_channels=24, seconds=15.0, num_speakers=4)
    params = ops.make_params(wpe=True, wpe_taps=10, wpe_delay=2, wpe_iterations=3,
                             bss_iterations=20, bss_iterations_post=1)
    ops._prepare_windows(ctx, params.stft_size, params.stft_shift)
    res = ops.ResidentUtterance(ctx, utt.obs, utt.activity_array, params)
    c0 = utt.ex['start_orig']['original']
    c1 = utt.ex['end']['original'] - utt.ex['end_orig']['original']
    F, T, D, K = params.stft_size // 2 + 1, res.T, res.D, res.K
    s_d, p_d = ctx.empty(8 * K * T), ctx.empty(8 * T)

    # the stage on the taps of one call
    bufs, taps = ops._debug_taps(res)
    res.enqueue(utt.target_index, c0, c1, taps)
    ctx.synchronize()

    def stage():
        ctx._check(ctx.lib.gss_posterior_activity(
            ctx.handle, c_void_p(bufs['Obs_ftd'].ptr), c_void_p(bufs['gamma'].ptr), F, K, T, D,
            None, c_void_p(s_d.ptr), c_void_p(p_d.ptr)), 'gss_posterior_activity')
    for _ in range(args.warmup):
        stage()
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(args.steps):
        stage()
    report = ctx.profile_report()
    ctx.profile_enable(False)
    ctx.profile_reset()
    stage_scores = ctx.to_host(s_d, (K, T), np.float64)
    per_call = {k: report[k]['ms'] / report[k]['calls'] for k in ('pact_sums', 'pact_scores')}
    both = sum(per_call.values())
    nbytes = 16 * F * T * D + 8 * F * K * T

    variants = {
        'plain': lambda: res.enqueue(utt.target_index, c0, c1),
        'activity': lambda: res.enqueue(utt.target_index, c0, c1, activity=(None, s_d, p_d)),
    }
    outputs = {}
    for v, fn in variants.items():
        for _ in range(args.warmup):
            fn()
        ctx.synchronize()
        outputs[v] = res.result()
    assert np.array_equal(outputs['plain'], outputs['activity'])
    assert np.array_equal(ctx.to_host(s_d, (K, T), np.float64), stage_scores)
    ms = {v: [] for v in variants}
    for _ in range(args.rounds):
        for v, fn in variants.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            ctx.synchronize()
            ms[v].append(1e3 * (time.perf_counter() - t0) / args.steps)
    med = {v: float(np.median(x)) for v, x in ms.items()}
    line = dict(case='config 2 (24 ch, 15 s)', F=F, T=T, D=D, K=K, steps=args.steps,
                rounds=args.rounds, warmup=args.warmup,
                stage_ms_per_call={k: round(v, 5) for k, v in per_call.items()},
                stage_bytes=nbytes, stage_tb_per_s=round(nbytes / both * 1e-9, 3),
                pact_sums_tb_per_s=round(nbytes / per_call['pact_sums'] * 1e-9, 3),
                ms={v: dict(median=round(med[v], 3), min=round(min(x), 3), max=round(max(x), 3))
                    for v, x in ms.items()},
                activity_minus_plain_ms=round(med['activity'] - med['plain'], 4),
                activity_over_plain=round(med['activity'] / med['plain'], 5),
                workspace_bytes=ctx.workspace_bytes())
    print(json.dumps(line), flush=True)
    with open(args.out, 'w') as fd:
        fd.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
