"""What the segment-wise MVDR costs: gss_mvdr_souden (one filter per window, the baseline)
against gss_mvdr_souden_segments on the same observation and masks, everything resident in HBM,

    whole        gss_mvdr_souden
    L256_c0      gss_mvdr_souden_segments, segment_frames 256, context_segments 0
    L256_c1      ... 256, 1
    L64_c2       ... 64, 2

at the headline shape (F = 513, T = 941, D = 24) and at config 5 (F = 513, T = 7503, D = 12),
`ban` on, min_mass = 2 D.  The variants ALTERNATE inside one process after a warm-up; every
round times `steps` calls of each between two synchronisations.  One JSON line per shape in
profiles/segments_cost.jsonl: per variant the median ms per call and the spread (min, max) of
its rounds, the ratios of the medians to `whole`, the per-kernel split of one profiled call
(gss_profile_report, ms) and the share of (segment, frequency) pairs that fell back.

    python tools/segments_cost.py [--steps 5] [--rounds 7] [--warmup 2]"""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np

R = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(R))

SHAPES = [('headline (24 ch, T = 941)', 24, 941), ('config 5 (12 ch, T = 7503)', 12, 7503)]
SEGMENTS = [('L256_c0', 256, 0), ('L256_c1', 256, 1), ('L64_c2', 64, 2)]
F = 513


def scene(rng, D, T):
    """Two point sources on their activity + diffuse noise (F,T,D), and a target mask (F,T):
    uniform weights on the first source's activity."""
    act = np.zeros((2, T), bool)
    Y = 0.1 * (rng.standard_normal((F, T, D)) + 1j * rng.standard_normal((F, T, D)))
    for k in range(2):
        a = int(rng.integers(0, T // 2))
        act[k, a:int(rng.integers(a + T // 4, T))] = True
        steer = rng.standard_normal((F, 1, D)) + 1j * rng.standard_normal((F, 1, D))
        src = rng.standard_normal((F, T, 1)) + 1j * rng.standard_normal((F, T, 1))
        Y += steer * src * act[k][None, :, None]
    return Y, rng.uniform(size=(F, T)) * act[0][None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=str(R / 'profiles' / 'segments_cost.jsonl'))
    args = ap.parse_args()
    from pb_chime5_amd._capi import GssBfSegments, c_void_p, default_context
    ctx = default_context(0)
    lib, h = ctx.lib, ctx.handle
    lines = []
    for name, D, T in SHAPES:
        rng = np.random.default_rng(D + T)
        Y, xm = scene(rng, D, T)
        Y_d, mx_d, mn_d = ctx.to_device(Y), ctx.to_device(xm), ctx.to_device(1 - xm)
        X_d = ctx.empty(16 * F * T)

        def segments(L, c):
            seg = GssBfSegments(L, c, 2.0 * D)
            return lambda: ctx._check(lib.gss_mvdr_souden_segments(
                h, c_void_p(Y_d.ptr), F, T, D, c_void_p(mx_d.ptr), c_void_p(mn_d.ptr), 1, -1,
                ctypes.byref(seg), c_void_p(X_d.ptr), None), 'gss_mvdr_souden_segments')
        variants = {'whole': lambda: ctx._check(lib.gss_mvdr_souden(
            h, c_void_p(Y_d.ptr), F, T, D, c_void_p(mx_d.ptr), c_void_p(mn_d.ptr), 1,
            c_void_p(X_d.ptr), None), 'gss_mvdr_souden')}
        variants.update({v: segments(L, c) for v, L, c in SEGMENTS})
        kernels, fallback_share = {}, {}
        for v, fn in variants.items():
            for _ in range(args.warmup):
                fn()
            ctx.profile_enable(True)
            ctx.profile_reset()
            fn()
            kernels[v] = {k: round(p['ms'], 4) for k, p in ctx.profile_report().items()}
            ctx.profile_enable(False)
            if v != 'whole':
                L = dict((s[0], s[1]) for s in SEGMENTS)[v]
                fallback_share[v] = round(ctx.last_segment_fallbacks() / (F * -(-T // L)), 4)
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
        line = dict(case=name, D=D, T=T, F=F, ban=1, min_mass=2 * D, steps=args.steps,
                    rounds=args.rounds, warmup=args.warmup,
                    ms={v: dict(median=round(med[v], 4), min=round(min(x), 4), max=round(max(x), 4))
                        for v, x in ms.items()},
                    spread_of_whole=round((max(ms['whole']) - min(ms['whole'])) / med['whole'], 5),
                    over_whole={v: round(med[v] / med['whole'], 4) for v in med if v != 'whole'},
                    kernels_ms=kernels, fallback_share=fallback_share,
                    workspace_bytes=ctx.workspace_bytes())
        print(json.dumps(line), flush=True)
        lines.append(line)
    with open(args.out, 'w') as fd:
        for line in lines:
            fd.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
