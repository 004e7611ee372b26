"""What S targets of one window cost as ONE gss_enhance_observation_targets call against S
gss_enhance_observation calls (the same outputs, bit for bit), inputs resident in HBM and timed
with bench.py's protocol (warm-up steps, then `steps` enqueued back to back between two
synchronisations):

    config 2     24 ch, 15 s, T = 941, K = 5, MVDR + BAN          S = 1 ... 4
    one array    4 ch, dev-shaped item, T = 2169, K = 5            S = 1 ... 3
    config 5     12 ch, 120 s, T = 7503, 40 EM iterations, GEV    S = 1, 2

One JSON line per case and S in profiles/targets_cost.jsonl: ms per step of the targets call
and of the S single calls, ms per extra target, and the per-kernel times of the targets call
(the library's own event profiler, a second run) -- printed as a table of the tail.

    python tools/targets_cost.py [--steps 10] [--warmup 2] [--case N]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

R = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(R))

import bench  # noqa: E402  (time_resident, profile_kernels, other_workload)

# kernels that run once per window whatever S is (the rest is the target-dependent tail)
FRONT = ('stft', 'wpe_', 'em_', 'activity')


def cases(ops, synthetic):
    u2 = synthetic.config2()
    u1, p1, _ = bench.other_workload('1a', synthetic, ops)
    u5, p5, _ = bench.other_workload('5', synthetic, ops)
    return [('config 2 (24 ch, 15 s, K = 5)', u2, ops.make_params(), [1, 2, 3, 4]),
            ('one array (4 ch, 34.7 s, K = 5)', u1, p1, [1, 2, 3]),
            ('config 5 (12 ch, 120 s, GEV, 40 EM iterations)', u5, p5, [1, 2])]


class ResidentTargets:
    """A targets call on an ops.ResidentUtterance: inputs and outputs stay on the device."""

    def __init__(self, ctx, ops, utt, params, targets, c0, c1):
        self.ctx = ctx
        self.res = ops.ResidentUtterance(ctx, utt.obs, utt.activity_array, params)
        self.S = S = len(targets)
        self.args = (targets, [c0] * S, [c1] * S)
        self.out_d = ctx.empty(8 * S * self.res.n_out)

    def enqueue(self):
        self.res.enqueue_targets(*self.args, self.out_d)

    def result(self):
        return self.ctx.to_host(self.out_d, (self.S, self.res.n_out), np.float64)


def timed(ctx, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    ctx.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def kernel_ms(ctx, fn, steps):
    ctx.profile_filter(None)
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(steps):
        fn()
    ctx.synchronize()
    prof = ctx.profile_report()
    ctx.profile_enable(False)
    return {k: v['ms'] / steps for k, v in sorted(prof.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--case', type=int, default=None)
    ap.add_argument('--out', default=str(R / 'profiles' / 'targets_cost.jsonl'))
    args = ap.parse_args()
    from pb_chime5_amd import ops, synthetic
    from pb_chime5_amd._capi import default_context
    ctx = default_context(0)
    lines = []
    for i, (name, u, params, S_list) in enumerate(cases(ops, synthetic)):
        if args.case is not None and i != args.case:
            continue
        ops._prepare_windows(ctx, params.stft_size, params.stft_shift)
        c0 = u.ex['start_orig']['original']
        c1 = u.ex['end']['original'] - u.ex['end_orig']['original']
        single = ops.ResidentUtterance(ctx, u.obs, u.activity_array, params)
        one_ms = timed(ctx, lambda: single.enqueue(0, c0, c1), args.steps, args.warmup)
        for S in S_list:
            targets = list(range(S))
            multi = ResidentTargets(ctx, ops, u, params, targets, c0, c1)

            def singles():
                for t in targets:
                    single.enqueue(t, c0, c1)
            singles_ms = timed(ctx, singles, args.steps, args.warmup)
            targets_ms = timed(ctx, multi.enqueue, args.steps, args.warmup)
            x = multi.result()
            assert np.all(np.isfinite(x))
            kern = kernel_ms(ctx, multi.enqueue, args.steps)
            tail = {k: v for k, v in kern.items() if not k.startswith(FRONT)}
            line = dict(case=name, S=S, T=single.T, D=single.D, K=single.K,
                        ms_one_target_call=round(one_ms, 4),
                        ms_targets_call=round(targets_ms, 4),
                        ms_single_calls=round(singles_ms, 4),
                        ratio_to_one_target_call=round(targets_ms / one_ms, 4),
                        ms_per_extra_target=round((targets_ms - one_ms) / max(S - 1, 1), 4)
                        if S > 1 else None,
                        speedup_vs_single_calls=round(singles_ms / targets_ms, 3),
                        tail_kernels_ms={k: round(v, 4) for k, v in tail.items()},
                        tail_ms=round(sum(tail.values()), 4),
                        steps=args.steps, warmup=args.warmup)
            print(json.dumps(line), flush=True)
            lines.append(line)
    with open(args.out, 'w') as fd:
        for line in lines:
            fd.write(json.dumps(line) + '\n')
    names = sorted({k for line in lines for k in line['tail_kernels_ms']})
    print('\nper-kernel time of the target-dependent tail (ms per call)')
    print('%-24s' % 'kernel' + ''.join('%12s' % f"c{i}S{l['S']}" for i, l in
                                       enumerate(lines)))
    for k in names:
        print('%-24s' % k + ''.join('%12.4f' % l['tail_kernels_ms'].get(k, 0.0) for l in lines))


if __name__ == '__main__':
    main()
