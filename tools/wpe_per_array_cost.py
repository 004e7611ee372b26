"""What per-array WPE (gss_params.wpe_arrays) costs against the joint WPE of the reference's
multiarray pipeline: the fused pipeline with its inputs resident in HBM, timed with bench.py's
own protocol (time_resident), at

    config 2            24 ch = 6 arrays x 4, 15 s               (the headline scene)
    config 2 outer      12 ch = 6 arrays x 2 ('outer_array_mics')
    config 5            12 ch = 6 arrays x 2, T = 7503, GEV, 40 EM iterations
    one array           4 ch, dev-shaped item (A = 1: per-array is the joint path)

One JSON line per case and mode: ms per step, ms of the WPE stage (its kernels, timed by the
library's per-kernel events in a second run), utterance-s/s.  ``--geometry`` adds the
per-array cases under each correlation geometry of one array (GSS_VARIANT corr_ksplit=1:
single waves, 2 / 4: frames split over 2 / 4 waves) -- how the default was chosen.

    python tools/wpe_per_array_cost.py [--steps 10] [--warmup 2] [--geometry]"""
import argparse
import json
import os
import sys
from pathlib import Path

R = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(R))

import bench  # noqa: E402  (time_resident, profile_kernels, other_workload)


def cases(ops, synthetic):
    u2 = synthetic.config2()
    p2 = ops.make_params()
    u2o = synthetic.config2(num_channels=12)
    u5, p5, _ = bench.other_workload('5', synthetic, ops)
    u1, p1, _ = bench.other_workload('1a', synthetic, ops)
    return [('config 2 (6 x 4 ch, 15 s)', u2, p2, 6, 15.0),
            ('config 2 outer mics (6 x 2 ch, 15 s)', u2o, p2, 6, 15.0),
            ('config 5 (6 x 2 ch, 120 s, GEV, 40 EM iterations)', u5, p5, 6, 120.0),
            ('one array (1 x 4 ch, 34.7 s)', u1, p1, 1, u1.obs.shape[1] / 16000.0)]


def with_arrays(ops, params, A):
    p = ops.GssParams.from_buffer_copy(params)
    p.wpe_arrays = A
    return p


def measure(ctx, ops, u, params, steps, warmup, kernel_times=True):
    ms, res = bench.time_resident(ctx, ops, u, params, steps, warmup)
    prof = bench.profile_kernels(ctx, res, u, steps) if kernel_times else {}
    wpe = {k: v['ms'] / steps for k, v in prof.items() if k.startswith('wpe_')}
    return ms, sum(wpe.values()), wpe, res.result()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--geometry', action='store_true')
    ap.add_argument('--case', type=int, default=None, help='only this case (0 ... 3)')
    ap.add_argument('--mode', choices=('joint', 'per_array'), default=None, help='only this mode')
    ap.add_argument('--no-kernel-times', action='store_true',
                    help='skip the per-kernel timing run (e.g. under rocprofv3)')
    args = ap.parse_args()
    from pb_chime5_amd import ops, synthetic
    from pb_chime5_amd._capi import default_context
    ctx = default_context(0)
    for i, (name, u, params, A, seconds) in enumerate(cases(ops, synthetic)):
        if args.case is not None and i != args.case:
            continue
        modes = [('joint', 0, None), ('per_array', A, None)]
        if args.mode:
            modes = [m for m in modes if m[0] == args.mode]
        if args.geometry and A > 1:
            modes += [(f'per_array corr_ksplit={k}', A, f'corr_ksplit={k}') for k in (1, 2, 4)]
        base = None
        for mode, arrays, variant in modes:
            if variant:
                os.environ['GSS_VARIANT'] = variant
            try:
                ms, wpe_ms, wpe, x = measure(ctx, ops, u, with_arrays(ops, params, arrays),
                                             args.steps, args.warmup, not args.no_kernel_times)
            finally:
                os.environ.pop('GSS_VARIANT', None)
            if base is None:
                base = x
            line = dict(case=name, mode=mode, channels=int(u.obs.shape[0]), arrays=A,
                        frames=int(ops.stft_frames(u.obs.shape[1], 1024, 256, True)),
                        ms_per_step=round(ms, 3), wpe_stage_ms=round(wpe_ms, 3),
                        utterance_s_per_s=round(seconds / (ms * 1e-3), 1),
                        wpe_kernels_ms={k: round(v, 3) for k, v in sorted(wpe.items())})
            if A == 1 and mode == 'per_array' and base is not x:
                line['bit_identical_to_joint'] = bool((x == base).all())
            print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
