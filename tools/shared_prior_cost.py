"""What the frequency-shared prior costs the EM: gss_cacgmm_guided against gss_cacgmm_shared_prior
on the same observation and the same guidance, everything resident in HBM, at the headline shape
(24 ch, T = 941, K = 5) and the one-array shape (4 ch, T = 2169, K = 5), F = 513, 20 + 1
iterations, from two starts:

    annotated    the activity's own initialisation and the activity as mask (f strides 0): the
                 guided call as the pipeline makes it, the shared prior as weak guidance
    blind        `ops.blind_initialization` and no mask: what the shared prior is for.  The
                 per-frequency model is not meant to start there (its classes starve and their
                 covariances take the eigendecomposition), so this ratio compares two different
                 computations and is reported for completeness

The two calls ALTERNATE inside one process after a warm-up; every round times `steps` calls of
each between two synchronisations.  One JSON line per (shape, start): per call the median ms and
the spread (min, max) of its rounds, the ratio of the medians, and the per-kernel event times of
one profiled call of each (runs of their own after the timed rounds).

With one array the guided call is the one-launch kernel; run the tool once more with
GSS_VARIANT=em_unfused for the like-for-like multi-launch baseline (the line says which it was).

    python tools/shared_prior_cost.py [--steps 5] [--rounds 7] [--warmup 2] [--shape all|headline|one_array]
                                       [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

R = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(R))

from tools.guided_cost import F, ITERATIONS, POST, SHAPES, scene      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--shape', choices=('all', 'headline', 'one_array'), default='all')
    ap.add_argument('--out', default=str(R / 'profiles' / 'shared_prior_cost.jsonl'))
    args = ap.parse_args()
    from pb_chime5_amd import ops
    from pb_chime5_amd._capi import GssGuidance, default_context
    ctx = default_context(0)
    variant = os.environ.get('GSS_VARIANT', '')
    lines = []
    for name, D, T, K in SHAPES:
        if args.shape != 'all' and (args.shape == 'one_array') != (D == 4):
            continue
        Y, act = scene(np.random.default_rng(D + T), D, T, K)
        Y_d = ctx.to_device(Y)
        gamma, prior = ctx.empty(8 * F * K * T), ctx.empty(8 * K * T)
        init_kt = np.where(act, 1.0, 1e-10)
        init_kt /= init_kt.sum(axis=0, keepdims=True)
        bufs = dict(blind=ctx.to_device(ops.blind_initialization(K, T, 0)),
                    init=ctx.to_device(init_kt), act=ctx.to_device(act.astype(np.uint8)))
        starts = {
            'annotated': GssGuidance(init_dev=bufs['init'].ptr, mask_dev=bufs['act'].ptr,
                                     init_f_stride=0, init_k_stride=T, mask_f_stride=0,
                                     mask_k_stride=T),
            'blind': GssGuidance(init_dev=bufs['blind'].ptr, init_f_stride=0, init_k_stride=T)}
        for start, g in starts.items():
            lines.append(measure(ctx, args, name, start, variant, D, T, K, Y_d, g, gamma, prior))
    with open(args.out, 'a' if variant else 'w') as fd:
        for line in lines:
            fd.write(json.dumps(line) + '\n')


def measure(ctx, args, name, start, variant, D, T, K, Y_d, g, gamma, prior):
    from pb_chime5_amd._capi import c_void_p
    lib, h = ctx.lib, ctx.handle
    calls = {
        'guided': lambda: ctx._check(lib.gss_cacgmm_guided(
            h, c_void_p(Y_d.ptr), F, T, D, ctypes.byref(g), K, ITERATIONS, POST,
            c_void_p(gamma.ptr)), 'gss_cacgmm_guided'),
        'shared_prior': lambda: ctx._check(lib.gss_cacgmm_shared_prior(
            h, c_void_p(Y_d.ptr), F, T, D, ctypes.byref(g), K, ITERATIONS, POST,
            c_void_p(gamma.ptr), c_void_p(prior.ptr)), 'gss_cacgmm_shared_prior')}
    for fn in calls.values():
        for _ in range(args.warmup):
            fn()
    ms = {v: [] for v in calls}
    for _ in range(args.rounds):
        for v, fn in calls.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            ctx.synchronize()
            ms[v].append(1e3 * (time.perf_counter() - t0) / args.steps)
    med = {v: float(np.median(x)) for v, x in ms.items()}
    reports = {}
    for v, fn in calls.items():
        ctx.profile_reset()
        ctx.profile_enable(True)
        fn()
        reports[v] = ctx.profile_report()
        ctx.profile_enable(False)
        ctx.profile_reset()
    line = dict(case=name, start=start, D=D, T=T, K=K, F=F, iterations=ITERATIONS,
                iterations_post=POST,
                variant=variant, steps=args.steps, rounds=args.rounds, warmup=args.warmup,
                ms={v: dict(median=round(med[v], 4), min=round(min(x), 4), max=round(max(x), 4))
                    for v, x in ms.items()},
                shared_prior_over_guided=round(med['shared_prior'] / med['guided'], 4),
                kernels_of_one_call_ms={
                    c: {k: dict(calls=v['calls'], ms=round(v['ms'], 4)) for k, v in r.items()}
                    for c, r in reports.items()})
    print(json.dumps(line), flush=True)
    return line

if __name__ == '__main__':
    main()
