"""What the online CACGMM costs next to the iterated one: gss_cacgmm_online (fresh state, forget =
0.99, prior_mass = 1, masked by the activity) against gss_cacgmm_guided (20 iterations, post 1)
on the same observation and activity, everything resident in HBM, F = 513, at

    one_array   (D, K, T) = (4, 4, 2169)
    joint24     (24, 5, 941)
    joint12     (12, 4, 7503)      a 120 s window

The two calls ALTERNATE inside one process after a warm-up; every round times `steps` calls of each
between two synchronisations.  One JSON line per shape: per call the median ms and the spread
(min, max) of its rounds, the ratio of the medians, the per-kernel event times of one profiled
call of each (runs of their own after the timed rounds), and microseconds per frame of the serial
kernel -- against the expectation of DESIGN.md section 25 (a dependent chain of D pivots per
frame, as the online MVDR's, with K waves side by side).  Lines are written as they are measured.

    python tools/cacgmm_online_cost.py [--steps 5] [--rounds 7] [--warmup 1] [--shape all|NAME] [--out FILE]"""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np

R = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(R))

F, FORGET, PRIOR_MASS, ITERATIONS = 513, 0.99, 1.0, 20
SHAPES = [('one_array', 4, 4, 2169), ('joint24', 24, 5, 941), ('joint12', 12, 4, 7503)]


def scene(rng, T, D, K):
    """Y (F,T,D) complex128 and the activity (K,T) uint8: K - 1 speakers in random turns of 50
    frames, a last class that is always on, sensor noise."""
    def crandn(*shape):
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    act = np.ones((K, T), np.uint8)
    act[:K - 1] = np.repeat(rng.random((K - 1, -(-T // 50))) < 0.6, 50, axis=1)[:, :T]
    Y = 0.1 * crandn(F, T, D)
    for k in range(K - 1):
        Y += crandn(F, 1, D) * (crandn(F, T) * act[k])[:, :, None]
    return np.ascontiguousarray(Y), np.ascontiguousarray(act)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--shape', default='all')
    ap.add_argument('--out', default=str(R / 'profiles' / 'cacgmm_online_cost.jsonl'))
    args = ap.parse_args()
    from pb_chime5_amd._capi import default_context
    ctx = default_context(0)
    with open(args.out, 'a' if args.shape != 'all' else 'w') as fd:
        for name, D, K, T in SHAPES:
            if args.shape not in ('all', name):
                continue
            Y, act = scene(np.random.default_rng(D + T), T, D, K)
            bufs = [ctx.to_device(a) for a in (Y, act)] + [ctx.empty(8 * F * K * T)]
            line = measure(ctx, args, name, D, K, T, *bufs)
            fd.write(json.dumps(line) + '\n')
            fd.flush()
            del bufs


def measure(ctx, args, name, D, K, T, Y_d, act_d, G_d):
    from pb_chime5_amd._capi import GssEmOnline, GssGuidance, c_void_p
    lib, h = ctx.lib, ctx.handle
    Y, G = c_void_p(Y_d.ptr), c_void_p(G_d.ptr)
    cfg = GssEmOnline(forget=FORGET, prior_mass=PRIOR_MASS)
    guide = GssGuidance(init_dev=None, mask_dev=act_d.ptr, init_f_stride=0, init_k_stride=0,
                        mask_f_stride=0, mask_k_stride=T)
    calls = {
        'online': lambda: ctx._check(lib.gss_cacgmm_online(
            h, Y, F, T, D, ctypes.byref(guide), K, ctypes.byref(cfg), None, G), 'gss_cacgmm_online'),
        'iterated': lambda: ctx._check(lib.gss_cacgmm_guided(
            h, Y, F, T, D, ctypes.byref(guide), K, ITERATIONS, 1, G), 'gss_cacgmm_guided')}
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
    calls['online']()
    serial = reports['online'].get('cacgmm_online', {}).get('ms')
    line = dict(case=name, D=D, K=K, T=T, F=F, forget=FORGET, prior_mass=PRIOR_MASS,
                iterations=ITERATIONS, steps=args.steps, rounds=args.rounds, warmup=args.warmup,
                fallbacks=ctx.last_cacgmm_online_fallbacks(),
                ms={v: dict(median=round(med[v], 4), min=round(min(x), 4), max=round(max(x), 4))
                    for v, x in ms.items()},
                online_over_iterated=round(med['online'] / med['iterated'], 2),
                kernels_of_one_call_ms={
                    c: {k: dict(calls=v['calls'], ms=round(v['ms'], 4)) for k, v in r.items()}
                    for c, r in reports.items()})
    if serial:
        line['serial_kernel_us_per_frame'] = round(1e3 * serial / T, 4)
    print(json.dumps(line), flush=True)
    return line


if __name__ == '__main__':
    main()
