"""What the online WPE costs next to the offline one: gss_wpe_online (fresh state, alpha = 0.9999)
against gss_wpe / gss_wpe_arrays (3 iterations) on the same observation, everything resident in
HBM, taps = 10, delay = 2, F = 513, at

    per_array   (A, C, T) = (6, 4, 941)     n = 40: on-chip form, 3078 problems
    one_array   (1, 4, 2169)                n = 40: on-chip form, 513 problems
    joint24     (1, 24, 941)                n = 240: memory form
    joint12     (1, 12, 7503)               n = 120: memory form, a 120 s window

The two calls ALTERNATE inside one process after a warm-up; every round times `steps` calls of
each between two synchronisations.  One JSON line per shape: per call the median ms and the spread
(min, max) of its rounds, the ratio of the medians, the per-kernel event times of one profiled
call of each (runs of their own after the timed rounds), microseconds per frame of the serial
kernel, and for the memory form the bytes per second it moved -- against the two-crossing model
of DESIGN.md section 19 (one triangle of P read and written per frame) and against what the
kernel does move (the full matrix, read and written).  Lines are written as they are measured.

    python tools/wpe_online_cost.py [--steps 5] [--rounds 7] [--warmup 1] [--shape all|NAME] [--out FILE]"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

R = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(R))

F, TAPS, DELAY, ITERATIONS, ALPHA = 513, 10, 2, 3, 0.9999
SHAPES = [('per_array', 6, 4, 941), ('one_array', 1, 4, 2169), ('joint24', 1, 24, 941),
          ('joint12', 1, 12, 7503)]
ONCHIP_MAX_N = 64


def scene(rng, T, D):
    """(F,T,D) complex128: white noise plus two reflections."""
    S = (rng.standard_normal((F, T + 5, D)) + 1j * rng.standard_normal((F, T + 5, D)))
    return np.ascontiguousarray(S[:, 5:] + 0.5 * S[:, 2:-3] + 0.3 * S[:, :-5])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--shape', default='all')
    ap.add_argument('--out', default=str(R / 'profiles' / 'wpe_online_cost.jsonl'))
    args = ap.parse_args()
    from pb_chime5_amd._capi import default_context
    ctx = default_context(0)
    variant = os.environ.get('GSS_VARIANT', '')
    with open(args.out, 'a' if variant or args.shape != 'all' else 'w') as fd:
        for name, A, C, T in SHAPES:
            if args.shape not in ('all', name):
                continue
            Y_d = ctx.to_device(scene(np.random.default_rng(A * C + T), T, A * C))
            X_d = ctx.empty(16 * F * T * A * C)
            line = measure(ctx, args, name, variant, A, C, T, Y_d, X_d)
            fd.write(json.dumps(line) + '\n')
            fd.flush()
            del Y_d, X_d


def measure(ctx, args, name, variant, A, C, T, Y_d, X_d):
    from pb_chime5_amd._capi import c_void_p
    lib, h = ctx.lib, ctx.handle
    Y, X = c_void_p(Y_d.ptr), c_void_p(X_d.ptr)
    if A > 1:
        def offline():
            ctx._check(lib.gss_wpe_arrays(h, Y, F, T, A, C, TAPS, DELAY, ITERATIONS, 0, X),
                       'gss_wpe_arrays')
    else:
        def offline():
            ctx._check(lib.gss_wpe(h, Y, F, T, C, TAPS, DELAY, ITERATIONS, 0, X), 'gss_wpe')
    calls = {
        'online': lambda: ctx._check(lib.gss_wpe_online(h, Y, F, T, A, C, TAPS, DELAY, ALPHA, None,
                                                        X), 'gss_wpe_online'),
        'offline': offline}
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
    n = TAPS * C
    memory_form = n > ONCHIP_MAX_N or 'wpe_online_mem' in variant
    serial = reports['online'].get('wpe_online_mem' if memory_form else 'wpe_online_onchip',
                                   {}).get('ms')
    line = dict(case=name, A=A, C=C, T=T, F=F, n=n, taps=TAPS, delay=DELAY, alpha=ALPHA,
                offline_iterations=ITERATIONS, form='memory' if memory_form else 'on-chip',
                variant=variant, steps=args.steps, rounds=args.rounds, warmup=args.warmup,
                ms={v: dict(median=round(med[v], 4), min=round(min(x), 4), max=round(max(x), 4))
                    for v, x in ms.items()},
                online_over_offline=round(med['online'] / med['offline'], 4),
                kernels_of_one_call_ms={
                    c: {k: dict(calls=v['calls'], ms=round(v['ms'], 4)) for k, v in r.items()}
                    for c, r in reports.items()})
    if serial:
        line['serial_kernel_us_per_frame'] = round(1e3 * serial / T, 4)
        if memory_form:
            problems = F * A
            model = 2.0 * 16 * problems * (n * (n + 1) // 2) * T      # one triangle, read + written
            moved = 2.0 * 16 * problems * (n * n + n * C) * T         # full P and G, read + written
            line['traffic'] = dict(
                model_two_crossings_of_the_triangle_gb=round(model / 1e9, 3),
                moved_full_matrix_gb=round(moved / 1e9, 3),
                model_tb_per_s=round(model / (serial * 1e-3) / 1e12, 4),
                moved_tb_per_s=round(moved / (serial * 1e-3) / 1e12, 4))
    print(json.dumps(line), flush=True)
    return line


if __name__ == '__main__':
    main()
