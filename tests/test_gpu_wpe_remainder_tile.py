"""WPE at 17 - 28 channels: the second, partly empty channel tile of the filter application and of
the correlation's P tiles runs as groups of four channels on v_mfma_f64_4x4x4_4b_f64 (wpe.hip,
`wpe_apply_rg_kernel`, remainder groups of `corr_chunk`); GSS_VARIANT remainder_full_tile is the
full 16-column tile as before.

Every case: `gss_wpe` (ops.wpe_dtf) on F = 3 frequencies of the scene generator of
tests/test_gpu_specialisations.py against the CPU oracle with that file's bound (WPE_TOL), no
zeroed pivot, once on the default path and once under the key; the two GPU results agree within
the bound test_kernel_variants_agree (tests/test_gpu_pipeline.py) puts on the WPE output.

Channel counts 17 ... 29 give remainders 1, 2, 4, 6, 8, 12 (one, two and three groups, whole and
partly filled) and 13, which keeps the full tile.  T = 70 is a partial 16-frame row tile, a
partial 64-frame chunk and less than one workgroup's 128 frames of the filter application.  At two
taps the correlation runs one wave per 16 x 16 sub-tile, so those channel counts meet the new P
tiles only under corr_ts=2 (the edge cases at D = 17 and 28); the workload's filter (10 taps,
delay 2) meets them by default, T = 409 with a last chunk of 25 frames in two groups of 16.
"""
import functools

import numpy as np
import pytest

import test_gpu_specialisations as spec
from test_gpu_specialisations import oracle

gpu = pytest.mark.gpu

F = 3
ITERATIONS = 2
VARIANT_TOL = 1e-5       # test_kernel_variants_agree: rel_err of the WPE output
KEY = 'remainder_full_tile'

SMALL = [(D, 2, 1, T) for D in (17, 18, 20, 22, 24, 28, 29) for T in (150, 70)]
WORKLOAD = [(D, 10, 2, T) for D in (20, 24) for T in (400, 409)]


@functools.lru_cache(maxsize=None)
def scene(D, taps, delay, T):
    """(Y, oracle X) of a case: computed once, shared, read-only."""
    saved = spec.WPE_F
    spec.WPE_F = F           # (the generator draws its module's number of frequencies)
    try:
        (Y,) = spec.wpe_inputs(D, taps, delay, T, 0)
    finally:
        spec.WPE_F = saved
    assert Y.shape == (D, T, F)
    want = oracle.wpe_block(Y, taps, delay, ITERATIONS)
    Y.setflags(write=False)
    want.setflags(write=False)
    return Y, want


def run(gpu_ctx, monkeypatch, D, taps, delay, T, texts):
    """The case under every variant text: each against the oracle, each against the first."""
    from pb_chime5_amd import ops
    Y, want = scene(D, taps, delay, T)
    results, bad = [], []
    try:
        for text in texts:
            spec._variant(monkeypatch, text)
            got = ops.wpe_dtf(Y, taps, delay, ITERATIONS, ctx=gpu_ctx)
            zeroed = gpu_ctx.last_wpe_zero_pivots()
            err = float(np.max(np.abs(got - want)) / np.max(np.abs(Y)))
            results.append(got)
            between = spec.rel_err(got, results[0])
            print(f'wpe D={D} taps={taps} delay={delay} T={T} [{text or "default"}]: oracle {err:.2e}, '
                  f'to the first {between:.2e}, zeroed pivots {zeroed}')
            if not err < spec.WPE_TOL or zeroed != 0 or not between < VARIANT_TOL:
                bad.append((text, err, between, zeroed))
    finally:
        spec._variant(monkeypatch, '')
    assert not bad, bad


@gpu
@pytest.mark.parametrize('D,taps,delay,T', SMALL)
def test_channel_counts(gpu_ctx, monkeypatch, D, taps, delay, T):
    run(gpu_ctx, monkeypatch, D, taps, delay, T, ['', KEY])


@gpu
@pytest.mark.parametrize('D,T', [(17, 70), (28, 150)])
def test_channel_counts_on_32x32_correlation_tiles(gpu_ctx, monkeypatch, D, T):
    """One and three remainder groups in the P tiles of the persistent correlation kernel."""
    run(gpu_ctx, monkeypatch, D, 2, 1, T, ['corr_ts=2', f'corr_ts=2,{KEY}'])


@gpu
@pytest.mark.parametrize('D,taps,delay,T', WORKLOAD)
def test_workload_filter(gpu_ctx, monkeypatch, D, taps, delay, T):
    run(gpu_ctx, monkeypatch, D, taps, delay, T, ['', KEY])


@gpu
@pytest.mark.parametrize('text', ['corr_blocked', 'corr_nw=2'])
def test_other_correlation_forms(gpu_ctx, monkeypatch, text):
    """24 channels with chunk-wise sums (which keep the full P tile) and two-wave workgroups."""
    run(gpu_ctx, monkeypatch, 24, 10, 2, 409, ['', KEY, text, f'{text},{KEY}'])
