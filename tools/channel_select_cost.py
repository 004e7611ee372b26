"""What the envelope-variance channel selection costs and saves at the headline workload: the
config-2 scene (24 channels, 15 s, 4 speakers + Noise; F = 513, T = 941) resident in HBM, timed
with bench.py's protocol -- a warm-up, then `steps` utterances enqueued back to back that end
in ONE synchronisation -- for

    plain24      gss_enhance_observation (no selection, the headline itself)
    select24     gss_enhance_observation_select, keep = 24 (scores + pick, no gather)
    select20     ... keep = 20 (the usual 80 %)
    select16     ... keep = 16
    select12     ... keep = 12

The variants ALTERNATE inside one process; one JSON line in profiles/channel_select_cost.jsonl:
per variant the median ms per step over the rounds and their spread (min, max), the ratio of
the medians to plain24, the per-kernel split of one profiled step of select20 and plain24
(gss_profile_report, ms), and chsel_bands as a share of the HBM roof with the byte count
16 F T D + 8 B T D.

    python tools/channel_select_cost.py [--steps 10] [--rounds 5] [--warmup 3]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

R = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(R))

KEEPS = (24, 20, 16, 12)
HBM_PEAK_TBS = 8.0          # MI355X HBM3E, vendor figure


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=str(R / 'profiles' / 'channel_select_cost.jsonl'))
    args = ap.parse_args()
    from pb_chime5_amd import ops, synthetic
    from pb_chime5_amd._capi import default_context
    ctx = default_context(0)
    utt = synthetic.config2(seed=2, num_channels=24, seconds=15.0, num_speakers=4)
    params = ops.make_params(wpe=True, wpe_taps=10, wpe_delay=2, wpe_iterations=3,
                             bss_iterations=20, bss_iterations_post=1)
    ops._prepare_windows(ctx, params.stft_size, params.stft_shift)
    res = ops.ResidentUtterance(ctx, utt.obs, utt.activity_array, params)
    c0 = utt.ex['start_orig']['original']
    c1 = utt.ex['end']['original'] - utt.ex['end_orig']['original']
    F, T, D = params.stft_size // 2 + 1, res.T, res.D
    selects = {n: ops.ChannelSelect(n, F) for n in KEEPS}
    B = selects[24].bands

    variants = {'plain24': lambda: res.enqueue(utt.target_index, c0, c1)}
    for n in KEEPS:
        variants[f'select{n}'] = (lambda sel: lambda: res.enqueue(
            utt.target_index, c0, c1, channel_select=sel))(selects[n])

    kernels, outputs, kept = {}, {}, {}
    for v, fn in variants.items():
        for _ in range(args.warmup):
            fn()
        ctx.synchronize()
        outputs[v] = res.result()
        assert np.all(np.isfinite(outputs[v]))
        if v != 'plain24':
            kept[v] = ctx.last_selected_channels(int(v[6:]))
        ctx.profile_enable(True)
        ctx.profile_reset()
        fn()
        kernels[v] = {k: round(p['ms'], 4) for k, p in ctx.profile_report().items()}
        ctx.profile_enable(False)
    assert np.array_equal(outputs['plain24'], outputs['select24'])

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

    def stage(prof):
        names = ('chsel_bands', 'chsel_scores', 'chsel_pick', 'chsel_gather', 'wpe_power', 'stft',
                 'wpe_corr')
        return {k: prof.get(k) for k in names if k in prof}
    bands_ms = kernels['select20']['chsel_bands']
    bands_bytes = 16 * F * T * D + 8 * B * T * D
    line = dict(case='config 2 (24 ch, 15 s)', F=F, T=T, D=D, bands=B, steps=args.steps,
                rounds=args.rounds, warmup=args.warmup,
                ms={v: dict(median=round(med[v], 3), min=round(min(x), 3), max=round(max(x), 3))
                    for v, x in ms.items()},
                spread_of_plain24=round((max(ms['plain24']) - min(ms['plain24'])) / med['plain24'], 5),
                over_plain24={v: round(med[v] / med['plain24'], 4) for v in med if v != 'plain24'},
                quadratic_expectation={f'select{n}': round((n / D) ** 2, 4) for n in KEEPS},
                kept_channels=kept,
                selection_kernels_ms={v: stage(kernels[v]) for v in ('plain24', 'select24', 'select20')},
                chsel_bands=dict(ms=bands_ms, bytes=bands_bytes,
                                 tb_per_s=round(bands_bytes / bands_ms * 1e-9, 3),
                                 share_of_hbm_peak=round(bands_bytes / bands_ms * 1e-9 / HBM_PEAK_TBS, 3)),
                kernels_ms={v: kernels[v] for v in ('plain24', 'select20')},
                workspace_bytes=ctx.workspace_bytes())
    print(json.dumps(line), flush=True)
    with open(args.out, 'w') as fd:
        fd.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
