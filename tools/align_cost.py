"""What the permutation alignment costs next to the EM it follows: gss_cacgmm_align with the
default plan (`ops.alignment_plan(513)`: 20 + 5 x 2 passes at most) against gss_cacgmm_guided
(20 + 1 iterations from the blind start, no mask) on the same observation, everything resident
in HBM, at the headline shape (24 ch, T = 941, K = 5) and the one-array shape (4 ch, T = 2169,
K = 5), F = 513, from two inputs:

    scrambled    the shared-prior posteriors of the scene (classes aligned by construction) with
                 a random permutation of the classes in every bin: every pass has work to do
                 until the mapping settles
    aligned      the same posteriors as they are: the first pass of every entry changes nothing
                 and the rest of the entry returns at once on the device-side word

The alignment writes all three outputs (mapping, aligned posteriors, activity).  The two calls
ALTERNATE inside one process after a warm-up; every round times `steps` calls of each between two
synchronisations.  One JSON line per (shape, input): per call the median ms and the spread (min,
max) of its rounds, the ratio of the medians, the rows the alignment moved, and the per-kernel
event times of one profiled call of each (runs of their own after the timed rounds).

    python tools/align_cost.py [--steps 5] [--rounds 7] [--warmup 2] [--shape all|headline|one_array]
                               [--out FILE]"""
import argparse
import ctypes
import json
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
    ap.add_argument('--out', default=str(R / 'profiles' / 'align_cost.jsonl'))
    args = ap.parse_args()
    from pb_chime5_amd import ops
    from pb_chime5_amd._capi import GssGuidance, c_void_p, default_context
    ctx = default_context(0)
    lines = []
    for name, D, T, K in SHAPES:
        if args.shape != 'all' and (args.shape == 'one_array') != (D == 4):
            continue
        Y, _ = scene(np.random.default_rng(D + T), D, T, K)
        Y_d = ctx.to_device(Y)
        blind = ctx.to_device(ops.blind_initialization(K, T, 0))
        g = GssGuidance(init_dev=blind.ptr, init_f_stride=0, init_k_stride=T)
        gamma = ctx.empty(8 * F * K * T)
        ctx._check(ctx.lib.gss_cacgmm_shared_prior(
            ctx.handle, c_void_p(Y_d.ptr), F, T, D, ctypes.byref(g), K, ITERATIONS, POST,
            c_void_p(gamma.ptr), None), 'gss_cacgmm_shared_prior')
        aligned = ctx.to_host(gamma, (F, K, T), np.float64)
        rng = np.random.default_rng(K + T)
        perm = np.stack([rng.permutation(K) for _ in range(F)])
        inputs = {'scrambled': aligned[np.arange(F)[:, None], perm], 'aligned': aligned}
        for label, table in inputs.items():
            lines.append(measure(ctx, args, name, label, D, T, K, Y_d, g, gamma,
                                 ctx.to_device(table)))
    with open(args.out, 'w') as fd:
        for line in lines:
            fd.write(json.dumps(line) + '\n')


def measure(ctx, args, name, label, D, T, K, Y_d, g, gamma, table_d):
    from pb_chime5_amd import ops
    from pb_chime5_amd._capi import c_void_p
    lib, h = ctx.lib, ctx.handle
    plan = ops.alignment_plan(F)
    dplan = ops.DeviceAlignPlan(plan)
    mapping, out, activity = ctx.empty(4 * F * K), ctx.empty(8 * F * K * T), ctx.empty(8 * K * T)
    calls = {
        'guided': lambda: ctx._check(lib.gss_cacgmm_guided(
            h, c_void_p(Y_d.ptr), F, T, D, ctypes.byref(g), K, ITERATIONS, POST,
            c_void_p(gamma.ptr)), 'gss_cacgmm_guided'),
        'align': lambda: ctx._check(lib.gss_cacgmm_align(
            h, c_void_p(table_d.ptr), F, K, T, ctypes.byref(dplan.struct), c_void_p(mapping.ptr),
            c_void_p(out.ptr), c_void_p(activity.ptr)), 'gss_cacgmm_align')}
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
    moved = ctx.last_align_moved()
    reports = {}
    for v, fn in calls.items():
        ctx.profile_reset()
        ctx.profile_enable(True)
        fn()
        reports[v] = ctx.profile_report()
        ctx.profile_enable(False)
        ctx.profile_reset()
    line = dict(case=name, input=label, D=D, T=T, K=K, F=F, iterations=ITERATIONS,
                iterations_post=POST, plan=plan, passes_at_most=sum(e[0] for e in plan),
                rows_moved=moved, steps=args.steps, rounds=args.rounds, warmup=args.warmup,
                ms={v: dict(median=round(med[v], 4), min=round(min(x), 4), max=round(max(x), 4))
                    for v, x in ms.items()},
                align_over_guided=round(med['align'] / med['guided'], 4),
                kernels_of_one_call_ms={
                    c: {k: dict(calls=v['calls'], ms=round(v['ms'], 4)) for k, v in r.items()}
                    for c, r in reports.items()})
    print(json.dumps(line), flush=True)
    return line


if __name__ == '__main__':
    main()
