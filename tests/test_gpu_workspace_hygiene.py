"""No kernel reads workspace or output memory before it writes it, and none writes behind its
block ("Workspace hygiene").

Every intermediate of a call lives in one bump arena per context that is never cleared, and the
fused entries hand the arena of one stage to the next; outputs and states come from a bare
hipMalloc.  The library's workspace debug mode (`Context.debug_workspace(pattern)`) fills all of
that with one byte before use and puts a guard of that byte behind every arena block.  A cell
below runs an entry twice on the same seeded input, once in 0x00 and once in 0xFF (NaN as a
double, -1 as an integer), with inputs, outputs and states allocated after the mode is on, and
asserts

 1. no guard was overwritten (`hygiene` prints the report's text),
 2. every output of the two runs is equal to the bit,
 3. the 0xFF run is within the bar the project already has for that stage of its CPU oracle or
    reference.

Scenes, oracle runners and bars are those of the modules that own them (imported, not copied);
where the owning test states its bar as a literal, the constant below names the test it is from.
The fused entries run on one short two-array utterance.  The plain call is held to the oracle;
the entries that differ from it in one stage are held, bit for bit, to the identities their own
tests document (pcm16 and host twins, targets rows, the guided call fed the frame activity, the
activity call) and, where a stage of their own follows, to that stage's NumPy reference on the
call's own taps.
"""
import ctypes
import functools

import numpy as np
import pytest

import cacgmm_model_reference as cm_ref
import channel_select_reference as cs_ref
import gss_oracle as oracle
import lcmv_reference as lr
import online_wpe_reference as wr
import posterior_activity_reference as pa_ref
import segments_reference as sr
import shared_prior_reference as spr
import wpd_reference as wpd_ref
from conftest import rel_err
from test_gpu_cacgmm_model import BAR_LOG_DET, BAR_PRECISION, BAR_WEIGHT, _rel_fro
from test_gpu_channel_select import BAR as CHSEL_BAR
from test_gpu_channel_select import _case as chsel_case
from test_gpu_guided import _oracle_guided, _per_frequency_guidance, _scene_of
from test_gpu_lcmv import _stage_scene as lcmv_scene
from test_gpu_pipeline import TOL_STFT_MAG
from test_gpu_posterior_activity import _case as pact_case
from test_gpu_posterior_activity import _within as pact_within
from test_gpu_segments import MIN_MASS as SEG_MIN_MASS
from test_gpu_segments import _stage_scene as seg_scene
from test_gpu_specialisations import (BF_TOL, EM_ITERATIONS, EM_TOL, GEV_TOL, WPE_TOL, _variant,
                                      cell, wpe_iterations)
from test_gpu_stages import _reverberant, _scene
from test_gpu_wpd import STAGE_BAR as WPD_BAR
from test_gpu_wpd import _reference as wpd_reference
from test_gpu_wpd import _scene as wpd_scene
from test_gpu_wpe_per_array import _oracle_per_array

pytestmark = pytest.mark.gpu

PATTERNS = (0x00, 0xFF)
# Bars their owning tests state as literals inside the test bodies.  They are re-typed here, each
# beside the name of the test it is from, because there is no constant to import and giving them
# names in the owning modules would mean editing tests that this module only reads; whoever
# changes one of those bars changes its copy here.
STFT_TOL = 1e-13            # test_gpu_stages.test_stft_matches_oracle
ISTFT_TOL = 1e-12           # test_gpu_stages.test_istft_matches_oracle
WPE_PSD_TOL = 1e-8          # test_gpu_stages.test_wpe_psd_context_matches_oracle, / max |Y|
WPE_ARRAYS_TOL = 1e-7       # test_gpu_wpe_per_array.test_stage_is_wpe_v8_per_array_bit_for_bit
LOGLIK_TOL = 1e-7           # test_gpu_cacgmm_model.test_log_likelihood
X_TOL = wr.X_TOL            # x_hat of the end-to-end tests (test_gpu_pipeline.test_tiny_with_wpe_vs_oracle)
ONLINE_OBS_TOL = 1e-9       # test_gpu_wpe_online.test_pipeline: the fused call's Obs tap


@pytest.fixture(scope='module')
def hctx():
    """The module's own context: the session's `gpu_ctx` is never put into the debug mode."""
    from pb_chime5_amd._capi import Context
    ctx = Context(0)
    yield ctx
    ctx.close()


def _bits(value):
    if isinstance(value, np.ndarray):
        return value.dtype.str, value.shape, np.ascontiguousarray(value).tobytes()
    return value


def same_bits(a, b):
    """The names of the outputs of two runs that differ in a bit (NaN payloads included)."""
    assert sorted(a) == sorted(b)
    return [name for name in sorted(a) if _bits(a[name]) != _bits(b[name])]


def poisoned(ctx, pattern, call):
    """call(ctx) -> {name: array | int} with the mode on in `pattern`; the guard report after it."""
    ctx.debug_workspace(pattern)
    try:
        out = call(ctx)
        count, text, _ = ctx.debug_workspace_report()
    finally:
        ctx.debug_workspace(None)
    return out, count, text


def hygiene(ctx, call, what):
    """Criteria 1 and 2 of the module docstring; returns the outputs of the 0xFF run."""
    outs = {}
    for pattern in PATTERNS:
        out, count, text = poisoned(ctx, pattern, call)
        print(f'{what} [0x{pattern:02X}]: {count} guard violations {text}')
        assert count == 0, f'{what} [0x{pattern:02X}]: {text}'
        outs[pattern] = out
    differ = same_bits(outs[0x00], outs[0xFF])
    assert not differ, f'{what}: {differ} depend on what the workspace held'
    return outs[0xFF]


def crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# ================================================================== the instrument tests itself
def test_poison_reaches_a_fresh_block_and_switches_off(hctx):
    plain = hctx.workspace_bytes()
    hctx.debug_workspace(0xFF)
    try:
        got = hctx.to_host(hctx.empty(4096), (4096,), np.uint8)
    finally:
        hctx.debug_workspace(None)
    assert np.all(got == 0xFF)
    assert hctx.workspace_bytes() == plain
    with pytest.raises(ValueError, match='debug mode is off'):
        hctx.debug_workspace_report()
    with pytest.raises(ValueError, match='pattern=256'):
        hctx.debug_workspace(256)


def _mvdr_call(D):
    (Y, xm, nm), _ = cell(('mvdr', D))

    def call(ctx):
        from pb_chime5_amd import ops
        out = {}
        for ban in (False, True):
            got, ref = ops.mvdr_souden_from_masks(Y, xm, nm, ban=ban, return_ref_channel=True, ctx=ctx)
            out.update({f'ban={ban}': got, f'ref ban={ban}': ref})
        return out
    return call


def test_an_overwritten_guard_is_reported_with_its_block(hctx):
    """One byte of a live guard is overwritten through gss_memset (the address lies inside the
    arena's own allocation): exactly one violation, naming that block."""
    from pb_chime5_amd._capi import c_void_p
    (Y, xm, nm), _ = cell(('mvdr', 7))
    hctx.debug_workspace(0xFF)
    try:
        from pb_chime5_amd import ops
        ops.mvdr_souden_from_masks(Y, xm, nm, ctx=hctx)
        count, text, addr = hctx.debug_workspace_report(guard_index=1)
        assert (count, text) == (0, '') and addr
        assert hctx.debug_workspace_report(guard_index=10 ** 6)[2] is None
        hctx._check(hctx.lib.gss_memset(hctx.handle, c_void_p(addr + 3), 0x5A, 1), 'gss_memset')
        count, text, _ = hctx.debug_workspace_report()
        again = hctx.debug_workspace_report()
    finally:
        hctx.debug_workspace(None)
    print(text)
    assert count == 1 and again[:2] == (1, text)
    assert 'block 1 ' in text and 'byte 3 ' in text and '0x5a' in text and '0xff' in text


def _download(ctx, addr, nbytes):
    from pb_chime5_amd._capi import c_void_p
    out = np.empty(nbytes, np.uint8)
    ctx._check(ctx.lib.gss_memcpy_d2h(ctx.handle, out.ctypes.data_as(c_void_p), c_void_p(addr), nbytes),
               'gss_memcpy_d2h')
    return out


def test_the_arena_holds_the_pattern_after_a_fused_call(hctx):
    """Poison and re-poison, looked at directly: after a fused call every live guard holds the
    pattern, and so do the 4 KiB behind the last one -- bytes that the WPE and the EM worked in
    before `arena_release` handed them on (they lie inside the arena: the headroom of the mode
    alone is 1 MiB)."""
    hctx.debug_workspace(0xFF)
    try:
        _fused_call('plain')(hctx)
        guards = []
        while hctx.debug_workspace_report(guard_index=len(guards))[2]:
            guards.append(hctx.debug_workspace_report(guard_index=len(guards))[2])
        held = [_download(hctx, addr, 256) for addr in guards]
        behind = _download(hctx, guards[-1] + 512, 4096)
    finally:
        hctx.debug_workspace(None)
    assert len(guards) >= 8 and guards == sorted(guards)
    assert all(np.all(h == 0xFF) for h in held)
    assert np.all(behind == 0xFF)


def test_mode_off_gives_the_bits_of_either_pattern(hctx):
    """One stage cell and one fused cell: off, 0x00 and 0xFF agree to the bit, and the mode leaves
    `workspace_bytes()` as the plain run set it."""
    for what, call in (('mvdr D=7', _mvdr_call(7)), ('fused plain', _fused_call('plain'))):
        off = call(hctx)
        plain_bytes = hctx.workspace_bytes()
        on = hygiene(hctx, call, what)
        assert not same_bits(off, on), what
        assert hctx.workspace_bytes() == plain_bytes
        assert not same_bits(off, call(hctx)), what


# ================================================================== STFT / iSTFT
@pytest.mark.parametrize('fading', [True, False])
@pytest.mark.parametrize('size,shift,N,T', [(64, 16, 1237, 131), (1024, 256, 4097, 37)])
def test_stft_and_istft(hctx, size, shift, N, T, fading):
    """D = 5 (the kernel transforms channels in pairs: one is left over), an odd sample count;
    the iSTFT's overlap-add into a poisoned output."""
    rng = np.random.default_rng(size + N)
    x = rng.standard_normal((5, N))
    X = crandn(rng, 2, T, size // 2 + 1)

    def call(ctx):
        from pb_chime5_amd import ops
        return {'stft': ops.stft(x, size, shift, fading=fading, ctx=ctx),
                'istft': ops.istft(X, size, shift, fading=fading, ctx=ctx)}
    got = hygiene(hctx, call, f'stft {size}/{shift} fading={fading}')
    assert rel_err(got['stft'], oracle.stft(x, size, shift, fading=fading)) < STFT_TOL
    assert rel_err(got['istft'], oracle.istft(X, size, shift, fading=fading)) < ISTFT_TOL


# ================================================================== WPE
def _wpe_call(key, psd_context=0, iterations=None):
    (Y,), _ = cell(key)
    iterations = wpe_iterations(key) if iterations is None else iterations

    def call(ctx):
        from pb_chime5_amd import ops
        X = ops.wpe_dtf(Y, key[2], key[3], iterations, psd_context, ctx=ctx)
        return {'X': X, 'zero_pivots': ctx.last_wpe_zero_pivots()}
    return call


# (D, taps, delay, GSS_VARIANT): one wave per sub-tile; the 32 x 32 tiling on the persistent
# kernel, plain and with block-wise sums; on the register-staged kernel; a short filter with odd
# n; n = 1; three frame phases of the packed filter application
WPE_CELLS = [(4, 10, 2, ''), (24, 10, 2, ''), (24, 10, 2, 'corr_blocked'), (32, 10, 20, ''),
             (7, 3, 1, ''), (1, 1, 1, ''), (12, 10, 2, 'apply_ph=3')]


@pytest.mark.parametrize('D,taps,delay,variant', WPE_CELLS)
def test_wpe(hctx, monkeypatch, D, taps, delay, variant):
    key = ('wpe', D, taps, delay)
    (Y,), want = cell(key)
    try:
        _variant(monkeypatch, variant)
        got = hygiene(hctx, _wpe_call(key), f'wpe {key[1:]} [{variant}]')
    finally:
        _variant(monkeypatch, '')
    err = float(np.max(np.abs(got['X'] - want['X'])) / np.max(np.abs(Y)))
    print(f'wpe {key[1:]} [{variant}]: {err:.2e}')
    assert err < WPE_TOL and got['zero_pivots'] == 0


def test_wpe_psd_context_and_no_iterations(hctx):
    key = ('wpe', 4, 10, 2)
    (Y,), _ = cell(key)
    got = hygiene(hctx, _wpe_call(key, psd_context=3), 'wpe psd_context=3')
    want = oracle.wpe_block(Y, 10, 2, wpe_iterations(key), 3)
    err = float(np.max(np.abs(got['X'] - want)) / np.max(np.abs(Y)))
    print(f'wpe psd_context=3: {err:.2e}')
    assert err < WPE_PSD_TOL and got['zero_pivots'] == 0
    # no iteration: the input, copied into the poisoned output
    got = hygiene(hctx, _wpe_call(key, iterations=0), 'wpe iterations=0')
    assert np.array_equal(got['X'], Y) and got['zero_pivots'] == 0


def test_wpe_per_array(hctx):
    """Two arrays of four channels: regrouped into the workspace, solved as 2 F bins, scattered."""
    A, C, T, F, taps, delay, iters = 2, 4, 327, 3, 5, 2, 3
    Y = _reverberant(np.random.default_rng(100 * A + 10 * C), A * C, T, F)

    def call(ctx):
        from pb_chime5_amd import ops
        X = ops.wpe_arrays_dtf(Y, A, taps, delay, iters, 0, ctx=ctx)
        return {'X': X, 'zero_pivots': ctx.last_wpe_zero_pivots()}
    got = hygiene(hctx, call, 'per-array wpe')
    want = _oracle_per_array(oracle.wpe_block, A)(Y, taps, delay, iters, 0)
    print(f'per-array wpe: {rel_err(got["X"], want):.2e}')
    assert rel_err(got['X'], want) < WPE_ARRAYS_TOL and got['zero_pivots'] == 0


# ------------------------------------------------------------------ online WPE
ONLINE_CELLS = [wr.ONCHIP_CELLS[0], wr.ONCHIP_CELLS[4], wr.MEMORY_CELLS[2]]


@pytest.mark.parametrize('form', ['default', 'mem'])
@pytest.mark.parametrize('cell_', ONLINE_CELLS, ids=str)
def test_wpe_online(hctx, monkeypatch, cell_, form):
    """The LDS form and the memory form (where n selects it and forced): from a state the library
    initialises in a poisoned block and hands back, from a throw-away state in the arena, and in
    two chunks through one state."""
    A, C, taps, delay, alpha, F, T = cell_
    Y = wr.scene(cell_, wr.seed_of(cell_))
    cut = min(64, T // 2)

    def run(ctx, Yp, state):
        from pb_chime5_amd import ops
        return wr.to_ftd(ops.wpe_online_dtf(wr.to_dtf(Yp), taps, delay, alpha, arrays=A,
                                            state=state, ctx=ctx))

    def call(ctx):
        from pb_chime5_amd import ops
        out = {}
        state = ops.OnlineWPEState.fresh(F, A, C, taps, delay, ctx=ctx)
        out['X'] = run(ctx, Y, state)
        out.update({f'state {k}': v for k, v in state.to_host().items()})
        out['X thrown away'] = run(ctx, Y, None)
        state = ops.OnlineWPEState.fresh(F, A, C, taps, delay, ctx=ctx)
        out['X chunks'] = np.concatenate([run(ctx, Y[:, :cut], state), run(ctx, Y[:, cut:], state)],
                                         axis=1)
        out.update({f'chunks {k}': v for k, v in state.to_host().items()})
        return out
    try:
        _variant(monkeypatch, 'wpe_online_mem' if form == 'mem' else '')
        got = hygiene(hctx, call, f'online wpe {cell_} {form}')
    finally:
        _variant(monkeypatch, '')
    Xr, st = wr.reference(cell_, wr.seed_of(cell_))
    errs = dict(X=rel_err(got['X'], Xr), G=rel_err(got['state filter'], st['G']),
                P=rel_err(got['state inv_cov'], st['P']))
    print(f'online wpe {cell_} {form}: {errs}')
    assert max(errs.values()) < wr.TOL, errs
    assert np.array_equal(got['state history'], st['hist'])
    # (documented identities of the stage: a throw-away state and blocks give the single call's bits)
    assert np.array_equal(got['X thrown away'], got['X'])
    assert np.array_equal(got['X chunks'], got['X'])
    for k in ('inv_cov', 'filter', 'history'):
        assert np.array_equal(got[f'chunks {k}'], got[f'state {k}']), k


# ================================================================== CACGMM
def _em_call(D, K, posts=(0, 1)):
    (Y, act), _ = cell(('em', D, K))

    def call(ctx):
        from pb_chime5_amd import ops
        return {f'post={p}': ops.cacgmm_posteriors(Y, act, EM_ITERATIONS, p, ctx=ctx) for p in posts}
    return call


# (D, K, GSS_VARIANT): the one-launch kernel; the same shape as separate launches; the register
# E-step; the eigendecomposition forced; the LDS form at an unspecialised D below and above 12;
# 28 channels
EM_CELLS = [(4, 3, ''), (4, 3, 'em_unfused'), (12, 3, ''), (12, 3, 'force_eigh'), (24, 6, ''),
            (7, 5, ''), (17, 9, ''), (28, 2, '')]


@pytest.mark.parametrize('D,K,variant', EM_CELLS)
def test_cacgmm(hctx, monkeypatch, D, K, variant):
    _, want = cell(('em', D, K))
    try:
        _variant(monkeypatch, variant)
        got = hygiene(hctx, _em_call(D, K), f'em D={D} K={K} [{variant}]')
    finally:
        _variant(monkeypatch, '')
    for name, w in want.items():
        err = float(np.max(np.abs(got[name] - w)))
        print(f'em D={D} K={K} [{variant}] {name}: {err:.2e}')
        assert err < EM_TOL


@pytest.mark.parametrize('streams', [1, 2])
def test_cacgmm_over_blocks_of_frequencies(hctx, monkeypatch, streams):
    """Blocks of eight frequencies with a ragged last one, one and two in flight: with two the
    second stream works in the arena beside the first."""
    D, T, F, K, iters, post = 7, 150, 33, 3, 3, 2      # of test_gpu_stages' test of the same name
    Y, act = _scene(np.random.default_rng(D + T + F), D, T, F, K)
    mb = max(int(np.ceil((16 * D + 8 * K) * T / 2 ** 20 * 8 * streams)), 1)

    def call(ctx):
        from pb_chime5_amd import ops
        return {'posterior': ops.cacgmm_posteriors(Y, act, iters, post, ctx=ctx)}
    try:
        _variant(monkeypatch, f'em_l3_fit_mb=0,em_l3_mb={mb},em_streams={streams}')
        got = hygiene(hctx, call, f'em blocks, streams={streams}')
    finally:
        _variant(monkeypatch, '')
    err = float(np.max(np.abs(got['posterior'] - oracle.gss_block(Y, act, iters, post))))
    print(f'em blocks, streams={streams}: {err:.2e}')
    assert err < EM_TOL


def test_cacgmm_guided_with_weights(hctx):
    D, T, F, K, iters, post = 7, 200, 4, 4, 6, 1        # of test_gpu_guided.SHAPES
    rng, Y, act = _scene_of(D, T, F, K)
    init, mask = _per_frequency_guidance(rng, act, F)

    def call(ctx):
        from pb_chime5_amd import ops
        return {'posterior': ops.cacgmm_posteriors_guided(
            Y, init.transpose(1, 2, 0), mask.transpose(1, 2, 0), iters, post, ctx=ctx)}
    got = hygiene(hctx, call, 'guided em')
    err = float(np.max(np.abs(got['posterior'] - _oracle_guided(Y, init, mask, iters, post))))
    print(f'guided em: {err:.2e}')
    assert err < EM_TOL


@pytest.mark.parametrize('variant', ['', 'estep_lds'])
@pytest.mark.parametrize('cell_', [spr.CELLS[0], spr.CELLS[2]], ids=str)
def test_cacgmm_shared_prior(hctx, monkeypatch, cell_, variant):
    """The register and the LDS form of the prior E-step, PRIOR_MAX_SLICES planes of partial
    column sums and the per-tile sums of gamma."""
    D, T, F, K, iterations, post = cell_
    seed = spr.seed_of(cell_, 'weak')
    Y, act = spr.parity_scene(D, T, F, K, seed)
    init, mask = spr.form_guidance('weak', act, F, seed)

    def call(ctx):
        from pb_chime5_amd import ops
        posterior, prior = ops.cacgmm_posteriors_shared_prior(Y, init, mask, iterations, post,
                                                              return_prior=True, ctx=ctx)
        return {'posterior': posterior, 'prior': prior}
    try:
        _variant(monkeypatch, variant)
        got = hygiene(hctx, call, f'shared prior {cell_} [{variant}]')
    finally:
        _variant(monkeypatch, '')
    want, want_prior = spr.reference(cell_, 'weak', seed)
    err = float(np.max(np.abs(got['posterior'] - want)))
    perr = float(np.max(np.abs(got['prior'] - want_prior)))
    print(f'shared prior {cell_} [{variant}]: posteriors {err:.2e}, prior {perr:.2e}')
    assert err < EM_TOL and perr < EM_TOL


def _model_errors(got, want):
    precision, log_det, weight = cm_ref.dense(want)
    got = got.normalized()
    return (float(np.max(_rel_fro(got.precision, precision))),
            float(np.max(np.abs(got.log_determinant - log_det))),
            float(np.max(np.abs(got.weight - weight))))


def test_cacgmm_model_fit_predict_refit_log_likelihood(hctx):
    sc = cm_ref.NONFLOORED[0]
    D, T, F, K, iters = sc
    Y, act = cm_ref.scene(D, T, F, K)

    models = {}

    def call(ctx):
        from pb_chime5_amd import ops
        first = ops.cacgmm_fit(Y, None, act, iters, ctx=ctx)
        posterior, loglik = ops.cacgmm_predict(first, Y, act, log_likelihood=True, ctx=ctx)
        refit = ops.cacgmm_fit(Y, None, act, 2, model=first, ctx=ctx)
        out = {'posterior': posterior, 'loglik': loglik}
        for name, m in (('fit', first), ('refit', refit)):
            out.update({f'{name} precision': m.precision, f'{name} log_det': m.log_determinant,
                        f'{name} weight': m.weight})
        models.update(fit=first, refit=refit)
        return out
    got = hygiene(hctx, call, f'model {sc}')
    want = cm_ref.oracle_fit(*sc)
    for name, w in (('fit', want), ('refit', cm_ref.oracle_fit(D, T, F, K, iters + 2))):
        e_p, e_l, e_w = _model_errors(models[name], w)
        print(f'model {sc} {name}: precision {e_p:.1e} log_det {e_l:.1e} weight {e_w:.1e}')
        assert e_p <= BAR_PRECISION and e_l <= BAR_LOG_DET and e_w <= BAR_WEIGHT
    mask = cm_ref.mask_fkt(act, F)
    posterior = want.predict(cm_ref.to_ftd(Y), source_activity_mask=mask).transpose(1, 2, 0)
    err = float(np.max(np.abs(got['posterior'] - posterior)))
    ll = cm_ref.log_likelihood(want, Y, mask)
    fin = np.isfinite(ll)
    assert np.array_equal(np.isneginf(got['loglik']), np.isneginf(ll))
    lerr = float(np.max(np.abs(got['loglik'][fin] - ll[fin]) / np.maximum(1.0, np.abs(ll[fin]))))
    print(f'model {sc}: predict {err:.1e}, log-likelihood {lerr:.1e}')
    assert err < EM_TOL and lerr <= LOGLIK_TOL


# ================================================================== beamformers
@pytest.mark.parametrize('D', [1, 7, 24, 29])
def test_mvdr(hctx, D):
    _, want = cell(('mvdr', D))
    got = hygiene(hctx, _mvdr_call(D), f'mvdr D={D}')
    for ban in (False, True):
        err = rel_err(got[f'ban={ban}'], want[f'ban={ban}'])
        print(f'mvdr D={D} ban={ban}: {err:.2e}')
        assert got[f'ref ban={ban}'] == want['ref'] and err < BF_TOL


def test_gev(hctx):
    (Y, xm, nm), want = cell(('gev', 12))

    def call(ctx):
        from pb_chime5_amd import ops
        return {f'ban={ban}': ops.gev_from_masks(Y, xm, nm, ban=ban, ctx=ctx) for ban in (False, True)}
    got = hygiene(hctx, call, 'gev D=12')
    for ban in (False, True):
        assert rel_err(np.abs(got[f'ban={ban}']), want[f'ban={ban}']) < GEV_TOL


def test_mvdr_segments_with_a_fallback_segment(hctx):
    D, T, F, L, c = 4, 300, 6, 64, 0        # of test_gpu_segments.STAGE_SCENES: 20 % fall back
    Y, xm, nm = seg_scene(D, T, F)
    assert sr.mass_margin(xm, nm, L, c, SEG_MIN_MASS) > 1e-6

    def call(ctx):
        from pb_chime5_amd import ops
        out = {}
        for ban in (False, True):
            got, ref, fallbacks = ops.mvdr_souden_segments_from_masks(
                Y, xm, nm, ban=ban, segment_frames=L, segment_context=c, min_mass=SEG_MIN_MASS,
                return_ref_channel=True, return_fallbacks=True, ctx=ctx)
            out.update({f'ban={ban}': got, f'ref ban={ban}': ref, f'fallbacks ban={ban}': fallbacks})
        return out
    got = hygiene(hctx, call, 'segment-wise mvdr')
    for ban in (False, True):
        want, det = sr.mvdr_souden_segments(Y, xm, nm, ban, L, c, SEG_MIN_MASS)
        assert int(det['fallbacks'].sum()) > 0
        assert got[f'ref ban={ban}'] == det['ref_channel']
        assert got[f'fallbacks ban={ban}'] == int(det['fallbacks'].sum())
        assert rel_err(got[f'ban={ban}'], want) < BF_TOL


@pytest.mark.parametrize('fallback', [False, True])
def test_lcmv(hctx, fallback):
    """The LCMV, and with the interferer silent in one frequency its masked fallback."""
    D, T, F, f0 = 5, 130, 4, 2              # of test_gpu_lcmv
    Y, xm, im, nm, _ = lcmv_scene(D, T, F)
    min_mass = 0.0
    if fallback:
        im = im.copy()
        im[:, f0] = 0.0
        min_mass = 2 * D

    def call(ctx):
        from pb_chime5_amd import ops
        out = {}
        for ban in (False, True):
            got, ref, fallbacks = ops.lcmv_souden_from_masks(
                Y, xm, im, nm, ban=ban, min_mass=min_mass, return_ref_channel=True,
                return_fallbacks=True, ctx=ctx)
            out.update({f'ban={ban}': got, f'ref ban={ban}': ref, f'fallbacks ban={ban}': fallbacks})
        return out
    got = hygiene(hctx, call, f'lcmv fallback={fallback}')
    for ban in (False, True):
        want, det = lr.lcmv_souden_from_masks(Y, xm, im, nm, ban, min_mass)
        assert got[f'ref ban={ban}'] == det['ref_channel']
        assert got[f'fallbacks ban={ban}'] == int(fallback)
        assert rel_err(got[f'ban={ban}'], want) <= BF_TOL


@pytest.mark.parametrize('scene', [(4, 130, 3, 3, 2), (12, 333, 3, 10, 2)], ids=str)
def test_wpd(hctx, scene):
    D, T, F, taps, delay = scene
    Y, m, g = wpd_scene(*scene)

    def call(ctx):
        from pb_chime5_amd import ops
        out = {}
        for iterations in (1, 2):
            got, ref, pivots = ops.wpd_souden_from_masks(
                Y, m, ban=True, taps=taps, delay=delay, iterations=iterations, frame_gate=g,
                return_ref_channel=True, return_zero_pivots=True, ctx=ctx)
            out.update({f'X {iterations}': got, f'ref {iterations}': ref,
                        f'pivots {iterations}': pivots})
        return out
    got = hygiene(hctx, call, f'wpd {scene}')
    for iterations in (1, 2):
        want, det = wpd_reference(scene, True, iterations, None)
        err = rel_err(got[f'X {iterations}'], want)
        print(f'wpd {scene} iterations={iterations}: {err:.2e}')
        assert got[f'ref {iterations}'] == det['ref_channel'] and got[f'pivots {iterations}'] == 0
        assert err <= WPD_BAR


# ================================================================== channel selection, activity
def test_channel_selection(hctx):
    D, T, F, B = 5, 37, 4, 2                # the smallest of test_gpu_channel_select.SHAPES
    _, Obs, W, scores, V = chsel_case(D, T, F, B)
    keep = 4

    def call(ctx):
        from pb_chime5_amd import ops
        got, gotV = ops.channel_scores(Obs, bank=W, return_band_variances=True, ctx=ctx)
        sel, channels = ops.select_channels(Obs, keep, bank=W, ctx=ctx)
        return {'scores': got, 'band variances': gotV, 'selected': sel,
                'channels': np.asarray(channels), 'status': ctx.last_selected_channels()}
    got = hygiene(hctx, call, 'channel selection')
    assert float(np.max(np.abs(got['scores'] - scores) / np.abs(scores))) <= CHSEL_BAR
    assert float(np.max(np.abs(got['band variances'] - V) / np.abs(V))) <= CHSEL_BAR
    want = cs_ref.pick(scores, keep)
    assert np.array_equal(got['channels'], want) and got['status'] == list(want)
    assert np.array_equal(got['selected'], Obs[want])


@pytest.mark.parametrize('D,T,F,K', [(2, 1, 1, 1), (5, 65, 4, 3)])
def test_posterior_activity(hctx, D, T, F, K):
    _, _, Obs, post, w, scores, power = pact_case(D, T, F, K, True)

    def call(ctx):
        from pb_chime5_amd import ops
        got, gotp = ops.posterior_activity(Obs, post, w, return_power=True, ctx=ctx)
        return {'scores': got, 'power': gotp}
    got = hygiene(hctx, call, f'posterior activity {(D, T, F, K)}')
    pact_within(got['scores'], scores, F, D, 'scores')
    pact_within(got['power'], power, F, D, 'power')


# ================================================================== fused entries
FUSED_KW = dict(wpe_taps=5, bss_iterations=8)       # of test_gpu_pipeline.test_tiny_with_wpe_vs_oracle
FUSED_CONTEXT = 4096
SIZE, SHIFT = 1024, 256
DETAILS = ('Obs', 'acitivity_freq', 'posterior', 'target_mask', 'distortion_mask', 'X_hat')


@functools.lru_cache(maxsize=None)
def _utterance():
    """Six channels as two arrays of three, three speakers and noise, T = 97 frames; the samples
    are rounded to 2^-15 so that the pcm16 twins see the same numbers."""
    from pb_chime5_amd import synthetic
    u = synthetic.tiny(num_channels=6, num_samples=24000, num_speakers=3, context=FUSED_CONTEXT)
    pcm = np.clip(np.round(u.obs / np.max(np.abs(u.obs)) * 20000), -32768, 32767).astype(np.int16)
    obs = pcm / 2.0 ** 15
    obs.setflags(write=False)
    pcm.setflags(write=False)
    return u, obs, pcm


def _frames():
    from pb_chime5_amd import ops
    return ops.samples_to_stft_frames(FUSED_CONTEXT, SIZE, SHIFT, fading=True)


def _with_details(x, det, **more):
    out = {'x_hat': x, 'ref_channel': det['ref_channel'], **more}
    out.update({k: det[k] for k in DETAILS if k in det})
    return out


def _host_entry(ctx, obs, act, target, **kw):
    """gss_enhance_observation_host: host buffers in and out, its own device blocks inside."""
    from pb_chime5_amd import ops
    from pb_chime5_amd._capi import c_void_p
    params = ops.params_for(ops.make_params(**kw), obs.shape[0], 2)
    ops._prepare_windows(ctx, SIZE, SHIFT, None)
    obs = np.ascontiguousarray(obs, np.float64)
    act = np.ascontiguousarray(act != 0, np.uint8)
    T = ops.stft_frames(obs.shape[1], SIZE, SHIFT, True)
    out = np.full(int(ctx.lib.gss_istft_num_samples(T, SIZE, SHIFT, 1)), np.nan)
    ctx._check(ctx.lib.gss_enhance_observation_host(
        ctx.handle, ctypes.byref(params), obs.ctypes.data_as(c_void_p), obs.shape[0], obs.shape[1],
        act.ctypes.data_as(c_void_p), act.shape[0], act.shape[1], int(target), FUSED_CONTEXT,
        FUSED_CONTEXT, out.ctypes.data_as(c_void_p)), 'gss_enhance_observation_host')
    return out


# the one-target entries of ops._FUSED_ENTRIES (with their pcm16 twins) and the four with a
# head of their own; 'select' runs the joint WPE (a selection breaks the arrays), every other
# entry the per-array WPE of two arrays
FUSED = ['plain', 'plain_pcm16', 'host', 'guided', 'targets', 'targets_pcm16', 'activity',
         'select', 'select_pcm16', 'wpe_online', 'segments', 'lcmv', 'wpd']


def _targets(target):
    """S = 3 of the K = 4 classes: the target first, then the noise class and another speaker."""
    return [target] + [k for k in (3, 1, 0) if k != target][:2]


def _fused_call(entry):
    u, obs, pcm = _utterance()
    act, target, c = u.activity_array, u.target_index, FUSED_CONTEXT
    samples = pcm if entry.endswith('pcm16') else obs
    args = (samples, act, target, c, c)
    kw = dict(FUSED_KW, wpe_arrays=2)

    def call(ctx):
        from pb_chime5_amd import ops
        common = dict(debug=True, ctx=ctx, **kw)
        if entry in ('plain', 'plain_pcm16'):
            if entry == 'plain':
                return _with_details(*ops.enhance_observation(*args, **common))
            # (ops.enhance_observation takes float64; the twin through the resident utterance)
            params = ops.params_for(ops.make_params(**FUSED_KW), 6, 2)
            ops._prepare_windows(ctx, SIZE, SHIFT, None)
            utt = ops.ResidentUtterance(ctx, pcm, act, params, pcm=True)
            bufs, taps = ops._debug_taps(utt)
            utt.enqueue(target, c, c, taps)
            return _with_details(*ops._one_target_result(utt, bufs, True))
        if entry == 'host':
            return {'x_hat': _host_entry(ctx, obs, act, target, **FUSED_KW)}
        if entry == 'guided':
            T = ops.stft_frames(obs.shape[1], SIZE, SHIFT, True)
            actf = oracle.activity_time_to_frequency(act, SIZE, SHIFT, True, stft_pad=True)[:, :T]
            return _with_details(*ops.enhance_observation_guided(obs, None, actf, target, c, c,
                                                                 **common))
        if entry in ('targets', 'targets_pcm16'):
            x, det = ops.enhance_observation_targets(samples, act, _targets(target), c, c, **common)
            return _with_details(x, {**det, 'ref_channel': np.asarray(det['ref_channel'])},
                                 status=ctx.last_ref_channels(3))
        if entry == 'activity':
            x, scores, power, det = ops.enhance_observation_activity(
                *args, freq_weights=pa_ref.weights(SIZE // 2 + 1), **common)
            return _with_details(x, det, scores=scores, power=power)
        if entry in ('select', 'select_pcm16'):
            x, det = ops.enhance_observation_select(*args, keep=5, debug=True, ctx=ctx, **FUSED_KW)
            return _with_details(x, det, channels=det['selected_channels'])
        if entry == 'wpe_online':
            return _with_details(*ops.enhance_observation_wpe_online(*args, **common))
        if entry == 'segments':
            x, det = ops.enhance_observation_segments(*args, segment_frames=64, **common)
            return _with_details(x, det, fallbacks=det['segment_fallbacks'])
        if entry == 'lcmv':
            x, det = ops.enhance_observation_lcmv(*args, **common)
            return _with_details(x, det, interferer=det['interferer'], fallbacks=det['lcmv_fallbacks'],
                                 interferer_mask=det['interferer_mask'])
        assert entry == 'wpd'
        x, det = ops.enhance_observation_wpd(*args, **common)
        return _with_details(x, det, pivots=det['wpd_zero_pivots'])
    return call


@functools.lru_cache(maxsize=None)
def _fused_oracle(channels=None):
    """The oracle on the utterance: per-array WPE of two arrays, or (a selection) the joint WPE
    on the kept channels."""
    u, obs, _ = _utterance()
    wpe_fn = _oracle_per_array(oracle.wpe_block, 2) if channels is None else None
    rows = obs if channels is None else obs[list(channels)]
    return oracle.enhance_observation(rows, u.activity_array, u.target_index, u.ex, **FUSED_KW,
                                      return_details=True, gss_fn=oracle.gss_block_batched,
                                      wpe_fn=wpe_fn)


_PLAIN = {}


def _plain(ctx):
    """The plain call with the mode off, once: what the entries that differ from it in one
    stage are compared with, bit for bit."""
    if 'out' not in _PLAIN:
        _PLAIN['out'] = _fused_call('plain')(ctx)
    return _PLAIN['out']


def _against_oracle(got, channels=None):
    want, wdet = _fused_oracle(channels)
    errs = (rel_err(np.abs(got['X_hat']), np.abs(wdet['X_hat'])), rel_err(got['x_hat'], want))
    print(f'fused vs oracle: |X_hat| {errs[0]:.1e}, x_hat {errs[1]:.1e}, ref '
          f'{got["ref_channel"]} / {wdet["ref_channel"]}')
    assert got['ref_channel'] == wdet['ref_channel']
    assert errs[0] < TOL_STFT_MAG and errs[1] < X_TOL


@pytest.mark.parametrize('entry', FUSED)
def test_fused_entry(hctx, entry):
    from pb_chime5_amd import ops
    u, obs, pcm = _utterance()
    act, target, c = u.activity_array, u.target_index, FUSED_CONTEXT
    got = hygiene(hctx, _fused_call(entry), f'fused {entry}')
    assert np.all(np.isfinite(got['x_hat']))
    plain = _plain(hctx)
    front = ('Obs', 'acitivity_freq', 'posterior')
    sf = ef = _frames()
    if entry == 'plain':
        _against_oracle(got)
        assert not same_bits(got, plain)
    elif entry in ('plain_pcm16', 'guided'):
        # the twin on samples that are multiples of 2^-15; the guided call fed the frame activity
        assert not same_bits(got, {k: plain[k] for k in got})
    elif entry == 'host':
        assert _bits(got['x_hat']) == _bits(plain['x_hat'])
    elif entry in ('targets', 'targets_pcm16'):
        # row s is the one-target call for target s, taps and status words included
        assert not same_bits({k: got[k] for k in front}, {k: plain[k] for k in front})
        for s, t in enumerate(_targets(target)):
            one = plain if t == target else _with_details(*ops.enhance_observation(
                obs, act, t, c, c, debug=True, ctx=hctx, wpe_arrays=2, **FUSED_KW))
            assert _bits(got['x_hat'][s]) == _bits(one['x_hat']), t
            for k in ('target_mask', 'distortion_mask', 'X_hat'):
                assert _bits(got[k][s]) == _bits(one[k]), (t, k)
            assert got['ref_channel'][s] == one['ref_channel'] == got['status'][s], t
    elif entry == 'activity':
        assert not same_bits({k: got[k] for k in plain}, plain)
        s, p = ops.posterior_activity(plain['Obs'], plain['posterior'],
                                      pa_ref.weights(SIZE // 2 + 1), return_power=True, ctx=hctx)
        assert _bits(got['scores']) == _bits(s) and _bits(got['power']) == _bits(p)
        rs, rp = pa_ref.posterior_activity(np.ascontiguousarray(plain['Obs'].transpose(2, 1, 0)),
                                           np.ascontiguousarray(plain['posterior'].transpose(2, 0, 1)),
                                           pa_ref.weights(SIZE // 2 + 1))
        pact_within(got['scores'], rs, SIZE // 2 + 1, 6, 'fused scores')
        pact_within(got['power'], rp, SIZE // 2 + 1, 6, 'fused power')
    elif entry in ('select', 'select_pcm16'):
        Y = oracle.stft(obs, SIZE, SHIFT).transpose(2, 1, 0)
        scores, _ = cs_ref.channel_scores(np.ascontiguousarray(Y), cs_ref.mel_bank(40, SIZE))
        assert list(got['channels']) == list(cs_ref.pick(scores, 5))
        _against_oracle(got, tuple(int(ch) for ch in got['channels']))
    elif entry == 'wpe_online':
        # (documented identity of the fused call: its Obs tap has the bits of the stage)
        stage = ops.wpe_online_dtf(ops.stft(obs, SIZE, SHIFT, ctx=hctx), FUSED_KW['wpe_taps'], 2,
                                   arrays=2, ctx=hctx)
        assert _bits(got['Obs']) == _bits(stage)
        Xr, _ = wr.online_wpe(wr.to_ftd(oracle.stft(obs, SIZE, SHIFT)), FUSED_KW['wpe_taps'], 2,
                              ops.WPE_ONLINE_ALPHA, 2)
        print(f'fused online wpe: Obs vs reference {rel_err(wr.to_ftd(got["Obs"]), Xr):.1e}')
        assert rel_err(wr.to_ftd(got['Obs']), Xr) < ONLINE_OBS_TOL
        # everything behind the WPE runs in its released bytes: |x_hat| against the oracle's stages
        # with the reference in the place of the WPE block (wr.pipe_enhance on this utterance)

        def wpe_fn(Obs, taps, delay, iterations, psd_context):
            return wr.to_dtf(wr.online_wpe(wr.to_ftd(Obs), taps, delay, ops.WPE_ONLINE_ALPHA, 2)[0])
        want, wdet = oracle.enhance_observation(obs, act, target, u.ex, **FUSED_KW, return_details=True,
                                                wpe_fn=wpe_fn, gss_fn=oracle.gss_block_batched)
        err = wr.abs_rel_err(got['x_hat'], want)
        print(f'fused online wpe: |x_hat| vs the oracle chain {err:.1e}, ref {got["ref_channel"]} / '
              f'{wdet["ref_channel"]}')
        assert got['ref_channel'] == wdet['ref_channel'] and err < wr.X_TOL
    else:
        # a beamformer of its own behind the plain call's front: that stage's reference on the taps
        assert not same_bits({k: got[k] for k in front}, {k: plain[k] for k in front})
        if entry == 'segments':
            want, det = sr.mvdr_souden_segments(got['Obs'], got['target_mask'],
                                                got['distortion_mask'], True, 64, 0, None)
            assert got['fallbacks'] == int(det['fallbacks'].sum())
            bar = BF_TOL
        elif entry == 'lcmv':
            xm, im, nm = lr.masks_from_posteriors(got['posterior'], target, got['interferer'], sf, ef)
            assert got['interferer'] >= 0 and np.array_equal(got['interferer_mask'], im)
            want, det = lr.lcmv_souden_from_masks(got['Obs'], xm, im, nm, True, 2 * 6)
            assert got['fallbacks'] == int(det['fallbacks'].sum())
            bar = BF_TOL
        else:
            raw = ops.stft(obs, SIZE, SHIFT, ctx=hctx)
            want, det = wpd_ref.wpd_souden_from_masks(
                raw, got['target_mask'], True, taps=FUSED_KW['wpe_taps'], delay=2, iterations=1,
                frame_gate=wpd_ref.context_gate(raw.shape[1], sf, ef))
            assert got['pivots'] == 0
            bar = WPD_BAR
        err = rel_err(got['X_hat'], want)
        print(f'fused {entry}: X_hat vs the stage reference on the taps {err:.1e}')
        assert got['ref_channel'] == det['ref_channel'] and err <= bar
        # ... and the iSTFT into the poisoned output, as test_gpu_segments holds its fused call
        assert rel_err(got['x_hat'], oracle.istft(got['X_hat'], SIZE, SHIFT)) < ISTFT_TOL
