"""What weighted / per-frequency guidance costs the EM: gss_cacgmm against gss_cacgmm_guided on
the same observation, everything resident in HBM,

    binary       gss_cacgmm, the (K,T) frame activity
    broadcast    gss_cacgmm_guided, one (K,T) initialisation + one (K,T) mask for every frequency
                 (f strides 0): the same bytes read, plus the initialisation once
    per_f        gss_cacgmm_guided, (F,K,T) initialisation and (F,K,T) mask: F K T mask bytes per
                 E-step beside the 16 F T D of the normalised observation (K / (16 D)), and
                 8 F K T once

at the headline shape (24 ch, T = 941, K = 5, 20 + 1 iterations) and the one-array shape (4 ch,
T = 2169, K = 5), F = 513.  The variants ALTERNATE inside one process after a warm-up; every
round times `steps` calls of each between two synchronisations.  One JSON line per shape in
profiles/guided_cost.jsonl: per variant the median ms per call and the spread (min, max) of its
rounds, and the ratios of the medians to `binary`.

    python tools/guided_cost.py [--steps 5] [--rounds 7] [--warmup 2]"""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np

R = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(R))

SHAPES = [('headline (24 ch, T = 941, K = 5)', 24, 941, 5), ('one array (4 ch, T = 2169, K = 5)', 4, 2169, 5)]
F, ITERATIONS, POST = 513, 20, 1


def scene(rng, D, T, K):
    """K - 1 point sources on their activity + diffuse noise, (F,T,D) complex128 and (K,T) bool."""
    act = np.zeros((K, T), bool)
    act[-1] = True
    Y = 0.1 * (rng.standard_normal((F, T, D)) + 1j * rng.standard_normal((F, T, D)))
    for k in range(K - 1):
        a = int(rng.integers(0, T // 2))
        act[k, a:int(rng.integers(a + T // 4, T))] = True
        steer = rng.standard_normal((F, 1, D)) + 1j * rng.standard_normal((F, 1, D))
        src = rng.standard_normal((F, T, 1)) + 1j * rng.standard_normal((F, T, 1))
        Y += steer * src * act[k][None, :, None]
    return Y, act


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=str(R / 'profiles' / 'guided_cost.jsonl'))
    args = ap.parse_args()
    from pb_chime5_amd._capi import GssGuidance, c_void_p, default_context
    ctx = default_context(0)
    lib, h = ctx.lib, ctx.handle
    lines = []
    for name, D, T, K in SHAPES:
        rng = np.random.default_rng(D + T)
        Y, act = scene(rng, D, T, K)
        Y_d = ctx.to_device(Y)
        act8 = act.astype(np.uint8)
        init_kt = np.where(act, 1.0, 1e-10)
        init_kt /= init_kt.sum(axis=0, keepdims=True)
        # per frequency: the activity with weights of its own in every bin
        init_f = rng.uniform(0.05, 1.0, size=(F, K, T)) * np.where(act, 1.0, 1e-10)[None]
        init_f /= init_f.sum(axis=1, keepdims=True)
        bufs = dict(act=ctx.to_device(act8), init_kt=ctx.to_device(init_kt),
                    mask_f=ctx.to_device(np.repeat(act8[None], F, axis=0)),
                    init_f=ctx.to_device(init_f), gamma=ctx.empty(8 * F * K * T))
        g_b = GssGuidance(init_dev=bufs['init_kt'].ptr, mask_dev=bufs['act'].ptr,
                          init_f_stride=0, init_k_stride=T, mask_f_stride=0, mask_k_stride=T)
        g_f = GssGuidance(init_dev=bufs['init_f'].ptr, mask_dev=bufs['mask_f'].ptr,
                          init_f_stride=K * T, init_k_stride=T, mask_f_stride=K * T, mask_k_stride=T)

        def guided(g):
            return lambda: ctx._check(lib.gss_cacgmm_guided(
                h, c_void_p(Y_d.ptr), F, T, D, ctypes.byref(g), K, ITERATIONS, POST,
                c_void_p(bufs['gamma'].ptr)), 'gss_cacgmm_guided')
        variants = {
            'binary': lambda: ctx._check(lib.gss_cacgmm(
                h, c_void_p(Y_d.ptr), F, T, D, c_void_p(bufs['act'].ptr), K, ITERATIONS, POST,
                c_void_p(bufs['gamma'].ptr)), 'gss_cacgmm'),
            'broadcast': guided(g_b), 'per_f': guided(g_f)}
        out = {}
        for v, fn in variants.items():
            for _ in range(args.warmup):
                fn()
            out[v] = ctx.to_host(bufs['gamma'], (F, K, T), np.float64)
        # the broadcast tables are the activity's own initialisation: the unweighted posteriors
        same = float(np.max(np.abs(out['broadcast'] - out['binary'])))
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
        line = dict(case=name, D=D, T=T, K=K, F=F, iterations=ITERATIONS, iterations_post=POST,
                    steps=args.steps, rounds=args.rounds, warmup=args.warmup,
                    ms={v: dict(median=round(med[v], 4), min=round(min(x), 4), max=round(max(x), 4))
                        for v, x in ms.items()},
                    spread_of_binary=round((max(ms['binary']) - min(ms['binary'])) / med['binary'], 5),
                    broadcast_over_binary=round(med['broadcast'] / med['binary'], 5),
                    per_f_over_binary=round(med['per_f'] / med['binary'], 5),
                    mask_bytes_over_observation_bytes=round(K / (16 * D), 5),
                    broadcast_minus_binary_max_abs=same)
        print(json.dumps(line), flush=True)
        lines.append(line)
    with open(args.out, 'w') as fd:
        for line in lines:
            fd.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
