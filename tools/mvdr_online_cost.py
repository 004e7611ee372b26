"""What the online MVDR costs next to the whole-window and the segment-wise one: gss_mvdr_online
(fresh state, forget = 0.99, loading = 1e-2, BAN, reference channel 0) against gss_mvdr_souden_ref
and gss_mvdr_souden_segments (256-frame segments) on the same observation and masks, everything
resident in HBM, F = 513, at

    one_array   (D, T) = (4, 2169)
    joint24     (24, 941)
    joint12     (12, 7503)      a 120 s window

The three calls ALTERNATE inside one process after a warm-up; every round times `steps` calls of
each between two synchronisations.  One JSON line per shape: per call the median ms and the spread
(min, max) of its rounds, the ratios of the medians, the per-kernel event times of one profiled
call of each (runs of their own after the timed rounds), and microseconds per frame of the serial
kernel -- against the expectation of DESIGN.md section 23 (about D^3 complex multiply-adds per
frame and frequency, and a dependent chain of D pivots per frame).  Lines are written as they are
measured.

With ``--lookahead L [L ...]`` the contenders are instead the existing kernel twice (gss_mvdr_online
with a carried state, L = 0 against L = 0: the spread) and gss_mvdr_online_lookahead at every L
given, each with a carried state and delay line, so every call releases T frames -- the yardstick
is the existing kernel.

    python tools/mvdr_online_cost.py [--steps 5] [--rounds 7] [--warmup 1] [--shape all|NAME] [--out FILE]
                                     [--lookahead L [L ...]]"""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np

R = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(R))

F, FORGET, LOADING, SEGMENT_FRAMES = 513, 0.99, 1e-2, 256
SHAPES = [('one_array', 4, 2169), ('joint24', 24, 941), ('joint12', 12, 7503)]


def scene(rng, T, D):
    """Y (F,T,D) complex128 and two masks (F,T) that add up to 1: two sources and sensor noise."""
    def crandn(*shape):
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    s1, s2 = crandn(F, T), crandn(F, T)
    Y = (crandn(F, 1, D) * s1[:, :, None] + crandn(F, 1, D) * s2[:, :, None]
         + 0.1 * crandn(F, T, D))
    p1, p2 = np.abs(s1) ** 2, np.abs(s2) ** 2
    mx = (p1 + 1e-3) / (p1 + p2 + 0.05 + 1e-3)
    return np.ascontiguousarray(Y), np.ascontiguousarray(mx), np.ascontiguousarray(1 - mx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--shape', default='all')
    ap.add_argument('--out', default=str(R / 'profiles' / 'mvdr_online_cost.jsonl'))
    ap.add_argument('--lookahead', type=int, nargs='+', default=[])
    args = ap.parse_args()
    from pb_chime5_amd._capi import default_context
    ctx = default_context(0)
    with open(args.out, 'a' if args.shape != 'all' else 'w') as fd:
        for name, D, T in SHAPES:
            if args.shape not in ('all', name):
                continue
            Y, mx, mn = scene(np.random.default_rng(D + T), T, D)
            bufs = [ctx.to_device(a) for a in (Y, mx, mn)] + [ctx.empty(16 * F * T)]
            line = (measure_lookahead if args.lookahead else measure)(ctx, args, name, D, T, *bufs)
            fd.write(json.dumps(line) + '\n')
            fd.flush()
            del bufs


def measure(ctx, args, name, D, T, Y_d, mx_d, mn_d, X_d):
    from pb_chime5_amd._capi import GssBfOnline, GssBfSegments, c_void_p
    lib, h = ctx.lib, ctx.handle
    Y, mx, mn, X = (c_void_p(b.ptr) for b in (Y_d, mx_d, mn_d, X_d))
    cfg = GssBfOnline(forget=FORGET, loading=LOADING, ref_channel=0)
    seg = GssBfSegments(segment_frames=SEGMENT_FRAMES, context_segments=0, min_mass=2.0 * D)
    calls = {
        'online': lambda: ctx._check(lib.gss_mvdr_online(
            h, Y, F, T, D, mx, mn, 1, ctypes.byref(cfg), None, X, None), 'gss_mvdr_online'),
        'window': lambda: ctx._check(lib.gss_mvdr_souden_ref(
            h, Y, F, T, D, mx, mn, 1, 0, X), 'gss_mvdr_souden_ref'),
        'segments': lambda: ctx._check(lib.gss_mvdr_souden_segments(
            h, Y, F, T, D, mx, mn, 1, 0, ctypes.byref(seg), X, None), 'gss_mvdr_souden_segments')}
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
    serial = reports['online'].get('mvdr_online', {}).get('ms')
    line = dict(case=name, D=D, T=T, F=F, forget=FORGET, loading=LOADING,
                segment_frames=SEGMENT_FRAMES, steps=args.steps, rounds=args.rounds,
                warmup=args.warmup, fallbacks=ctx.last_mvdr_online_fallbacks(),
                ms={v: dict(median=round(med[v], 4), min=round(min(x), 4), max=round(max(x), 4))
                    for v, x in ms.items()},
                online_over_window=round(med['online'] / med['window'], 2),
                online_over_segments=round(med['online'] / med['segments'], 2),
                kernels_of_one_call_ms={
                    c: {k: dict(calls=v['calls'], ms=round(v['ms'], 4)) for k, v in r.items()}
                    for c, r in reports.items()})
    if serial:
        line['serial_kernel_us_per_frame'] = round(1e3 * serial / T, 4)
        # D^3 complex multiply-adds = 8 D^3 real flops per frame and frequency
        line['serial_kernel_gflops_of_d_cubed'] = round(8.0 * D ** 3 * F * T / (serial * 1e-3) / 1e9, 2)
    print(json.dumps(line), flush=True)
    return line


def measure_lookahead(ctx, args, name, D, T, Y_d, mx_d, mn_d, X_d):
    from pb_chime5_amd import ops
    from pb_chime5_amd._capi import GssBfOnline, c_void_p
    lib, h = ctx.lib, ctx.handle
    Y, mx, mn, X = (c_void_p(b.ptr) for b in (Y_d, mx_d, mn_d, X_d))
    cfg = GssBfOnline(forget=FORGET, loading=LOADING, ref_channel=0)

    def existing():
        state = ops.OnlineMVDRState.fresh(F, D, LOADING, ctx=ctx)
        return lambda: ctx._check(lib.gss_mvdr_online(
            h, Y, F, T, D, mx, mn, 1, ctypes.byref(cfg), ctypes.byref(state.struct()), X, None),
            'gss_mvdr_online')

    def lookahead(L):
        state = ops.OnlineMVDRState.fresh(F, D, LOADING, ctx=ctx)
        hold = ops.OnlineMVDRHold.fresh(F, D, L, ctx=ctx)
        line = hold.struct()          # the one struct of the loop: the library advances `held`

        def call(hold=hold):          # (the closure keeps the line's buffers alive)
            ctx._check(lib.gss_mvdr_online_lookahead(
                h, Y, F, T, D, mx, mn, 1, ctypes.byref(cfg), ctypes.byref(state.struct()),
                ctypes.byref(line), X, None, None), 'gss_mvdr_online_lookahead')
        return call
    calls = {'L0': existing(), 'L0_again': existing()}
    calls.update({f'L{L}': lookahead(L) for L in args.lookahead})
    for fn in calls.values():
        for _ in range(max(args.warmup, 1)):
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
    line = dict(case=name, D=D, T=T, F=F, forget=FORGET, lookahead=args.lookahead, steps=args.steps,
                rounds=args.rounds, warmup=max(args.warmup, 1),
                ms={v: dict(median=round(med[v], 4), min=round(min(x), 4), max=round(max(x), 4))
                    for v, x in ms.items()},
                over_L0={v: round(med[v] / med['L0'], 4) for v in med},
                kernels_of_one_call_ms={
                    c: {k: dict(calls=v['calls'], ms=round(v['ms'], 4)) for k, v in r.items()}
                    for c, r in reports.items()})
    print(json.dumps(line), flush=True)
    return line


if __name__ == '__main__':
    main()
