"""The CACGMM with a frequency-shared prior on the GPU (gss_cacgmm_shared_prior,
ops.cacgmm_posteriors_shared_prior / cacgmm_posteriors_blind, GSS(shared_prior=True),
Enhancer.enhance_observation_blind).

The reference for every number is tests/shared_prior_reference.py: the untouched oracle's
CACGMMTrainer with the mixture weight averaged over the frequencies instead of over time.  The
bar is EM_TOL = 1e-7 of tests/test_gpu_specialisations.py, on posteriors and prior alike, and the
scenes are chosen by that file's rule: a seed is kept only if the reference's own output moves at
least 100 x less than the bar under a last-bit change of the input (spr.SEEDS; seed 0 passed in
every cell, the reference moves by at most 8.3e-11; tests/test_shared_prior_api.py re-checks a
sample on the CPU)."""
import ctypes

import numpy as np
import pytest

import gss_oracle as oracle
import shared_prior_reference as spr
from conftest import rel_err

pytestmark = pytest.mark.gpu

EM_TOL = spr.EM_TOL


def _run(ctx, cell, form, **kw):
    """ops.cacgmm_posteriors_shared_prior on a parity cell -> posterior (K,T,F), prior (K,T)."""
    from pb_chime5_amd import ops
    D, T, F, K, iterations, post = cell
    seed = spr.seed_of(cell, form)
    Y, act = spr.parity_scene(D, T, F, K, seed)
    init, mask = spr.form_guidance(form, act, F, seed)
    if init.ndim == 3:
        init = init.transpose(1, 2, 0)          # (F,K,T) -> the operators' (K,T,F)
    return ops.cacgmm_posteriors_shared_prior(Y, init, mask, iterations, post, return_prior=True,
                                              ctx=ctx, **kw)


# ------------------------------------------------------------------ parity with the reference
@pytest.mark.parametrize('form', spr.FORMS)
@pytest.mark.parametrize('cell', spr.CELLS, ids=lambda c: '-'.join(map(str, c)))
def test_posteriors_and_prior_match_the_reference(gpu_ctx, cell, form):
    want, want_prior = spr.reference(cell, form, spr.seed_of(cell, form))
    got, prior = _run(gpu_ctx, cell, form)
    assert got.shape == want.shape and prior.shape == want_prior.shape
    err, perr = float(np.max(np.abs(got - want))), float(np.max(np.abs(prior - want_prior)))
    print(f'shared prior {cell} {form}: posteriors {err:.2e}, prior {perr:.2e}')
    assert err < EM_TOL and perr < EM_TOL


@pytest.mark.parametrize('cell', [spr.CELLS[0], spr.CELLS[1], spr.CELLS[5]],
                         ids=lambda c: '-'.join(map(str, c)))
def test_lds_form_of_the_estep_at_the_register_form_shapes(gpu_ctx, monkeypatch, cell):
    """D = 4, 24 and 12 with 2 <= K <= 6 take the register form of the E-step; GSS_VARIANT=estep_lds
    sends them through the form every other shape takes.  Both are held to the reference."""
    want, want_prior = spr.reference(cell, 'weak', spr.seed_of(cell, 'weak'))
    reg = _run(gpu_ctx, cell, 'weak')
    try:
        monkeypatch.setenv('GSS_VARIANT', 'estep_lds')
        got, prior = _run(gpu_ctx, cell, 'weak')
    finally:
        monkeypatch.delenv('GSS_VARIANT', raising=False)
        _run(gpu_ctx, spr.CELLS[7], 'blind')      # (the library re-reads the variable)
    err, perr = float(np.max(np.abs(got - want))), float(np.max(np.abs(prior - want_prior)))
    print(f'shared prior {cell} weak [estep_lds]: posteriors {err:.2e}, prior {perr:.2e}; the '
          f'two forms differ by {float(np.max(np.abs(got - reg[0]))):.2e}')
    assert err < EM_TOL and perr < EM_TOL


@pytest.mark.parametrize('cell', spr.REG_CELLS, ids=lambda c: f'D{c[0]}-K{c[3]}')
def test_every_register_form_instantiation(gpu_ctx, cell):
    """em_estep_prior_reg_kernel<K, D, fit | predict> for every (D, K) the dispatch can select,
    weakly guided (a masked fit, an unmasked predict), against the reference."""
    want, want_prior = spr.reference(cell, 'weak', spr.seed_of(cell, 'weak'))
    got, prior = _run(gpu_ctx, cell, 'weak')
    err, perr = float(np.max(np.abs(got - want))), float(np.max(np.abs(prior - want_prior)))
    print(f'shared prior, register form D={cell[0]} K={cell[3]}: posteriors {err:.2e}, '
          f'prior {perr:.2e}')
    assert err < EM_TOL and perr < EM_TOL


@pytest.mark.parametrize('per_frequency', [False, True], ids=['KT', 'FKT'])
@pytest.mark.parametrize('cell', spr.MASK_ONLY_CELLS, ids=lambda c: '-'.join(map(str, c)))
def test_mask_only_start(gpu_ctx, cell, per_frequency):
    """No initialisation: the 1 : 1e-10 table is derived from the mask on the device, and the
    first prior is that table ((K,T) mask) or its mean over f ((F,K,T) mask)."""
    from pb_chime5_amd import ops
    D, T, F, K, iterations, post = cell
    want, want_prior, mask = spr.mask_only_reference(cell, per_frequency)
    Y, _ = spr.parity_scene(D, T, F, K, 0)
    mask_ktf = mask.transpose(1, 2, 0) if per_frequency else mask
    got, prior = ops.cacgmm_posteriors_shared_prior(Y, None, mask_ktf, iterations, post,
                                                    return_prior=True, ctx=gpu_ctx)
    err, perr = float(np.max(np.abs(got - want))), float(np.max(np.abs(prior - want_prior)))
    print(f'shared prior {cell} mask only, (F,K,T) mask {per_frequency}: posteriors {err:.2e}, '
          f'prior {perr:.2e}')
    assert err < EM_TOL and perr < EM_TOL
    # one M-step (one iteration, post 1): the prior handed back is the derived table itself / its
    # mean over f
    _, first = ops.cacgmm_posteriors_shared_prior(Y, None, mask_ktf, 1, 1, return_prior=True,
                                                  ctx=gpu_ctx)
    table = np.where(mask, 1.0, 1e-10)
    table = table / table.sum(axis=-2, keepdims=True)
    if per_frequency:
        assert float(np.max(np.abs(first - table.mean(axis=0)))) < 1e-15
    else:
        assert np.array_equal(first, table)


def test_one_array_takes_the_multi_launch_path(gpu_ctx):
    """D = 4, K = 3 is the one-launch kernel's shape; its frequencies never meet, so the shared
    prior must not reach it: the E-steps are the prior's own, one per iteration plus the predict."""
    cell = spr.CELLS[0]
    assert cell[0] == 4 and 2 <= cell[3] <= 6
    gpu_ctx.profile_reset()
    gpu_ctx.profile_enable(True)
    try:
        _run(gpu_ctx, cell, 'blind')
        report = gpu_ctx.profile_report()
    finally:
        gpu_ctx.profile_enable(False)
        gpu_ctx.profile_reset()
    assert 'em_onchip' not in report and 'em_estep' not in report, sorted(report)
    assert report['em_estep_prior']['calls'] == cell[4]
    assert report['em_predict_prior']['calls'] == 1
    assert report['em_prior_update']['calls'] == cell[4]


def test_one_class_gives_exactly_one(gpu_ctx):
    """K = 1 at (D, T, F) = (4, 327, 3): the posteriors are exactly 1.0.  The prior handed back
    is the one of the last M-step: the initialisation (exactly 1.0) after one iteration, the
    clipped affiliation 1 - 1e-10 of the reference after more."""
    from pb_chime5_amd import ops
    Y, _ = spr.parity_scene(4, 327, 3, 3, 0)
    for iterations, want_prior in ((1, 1.0), (3, 1.0 - 1e-10)):
        posterior, prior = ops.cacgmm_posteriors_blind(Y, 1, iterations, return_prior=True,
                                                       ctx=gpu_ctx)
        ref, ref_prior = spr.shared_prior_block(Y, ops.blind_initialization(1, 327, 0), None,
                                                iterations, 1)
        assert np.all(ref == 1.0) and np.all(ref_prior == want_prior)
        assert posterior.shape == (1, 327, 3) and np.all(posterior == 1.0)
        assert prior.shape == (1, 327) and np.all(prior == want_prior)


def test_the_prior_is_really_used(gpu_ctx):
    """The same inputs through the per-frequency model give other posteriors."""
    from pb_chime5_amd import ops
    cell = spr.CELLS[1]
    D, T, F, K, iterations, post = cell
    assert (D, T, F, K) == (24, 327, 3, 5)
    Y, act = spr.parity_scene(D, T, F, K, spr.seed_of(cell, 'blind'))
    init, _ = spr.form_guidance('blind', act, F, spr.seed_of(cell, 'blind'))
    shared, _ = _run(gpu_ctx, cell, 'blind')
    per_f = ops.cacgmm_posteriors_guided(Y, init, None, iterations, post, ctx=gpu_ctx)
    assert float(np.max(np.abs(shared - per_f))) > 1e-3


# ------------------------------------------------------------------ determinism
@pytest.mark.parametrize('cell', [spr.CELLS[1], spr.CELLS[5], spr.CELLS[6]],
                         ids=lambda c: '-'.join(map(str, c)))
def test_same_call_same_bits_whatever_the_block_settings(gpu_ctx, monkeypatch, cell):
    """No atomics: twice the same bits, prior included; and the frequency-block settings of the
    per-frequency EM do not reach this mode (one block on one stream)."""
    first = _run(gpu_ctx, cell, 'random')
    again = _run(gpu_ctx, cell, 'random')
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    try:
        for text in ('em_streams=2', 'em_streams=2,em_l3_mb=1,em_l3_fit_mb=0', 'em_unfused'):
            monkeypatch.setenv('GSS_VARIANT', text)
            other = _run(gpu_ctx, cell, 'random')
            assert np.array_equal(first[0], other[0]) and np.array_equal(first[1], other[1]), text
    finally:
        monkeypatch.delenv('GSS_VARIANT', raising=False)
        _run(gpu_ctx, spr.CELLS[7], 'blind')      # (the library re-reads the variable)


# ------------------------------------------------------------------ workspace of a fresh context
def _raw(ctx, Y_d, F, T, D, g, K, iterations, post, g_d, p_d):
    from pb_chime5_amd import _capi
    return ctx.lib.gss_cacgmm_shared_prior(
        ctx.handle, _capi.c_void_p(Y_d.ptr), F, T, D, ctypes.byref(g) if g is not None else None,
        K, iterations, post, _capi.c_void_p(g_d.ptr), _capi.c_void_p(p_d.ptr if p_d else None))


@pytest.mark.parametrize('D,K', [(4, 4), (24, 5)])
def test_fresh_context_never_runs_out_of_workspace(gpu_ctx, D, K):
    """A context that has never grown its arena: the reserve covers what the mode adds (the
    1 MiB rounding of a warm arena would hide a short reserve)."""
    from pb_chime5_amd import _capi
    F, frames = 513, (100, 1163, 2172, 2891, 4000)
    Tmax = max(frames)
    rng = np.random.default_rng(D)
    flat = rng.standard_normal(2 * 513 * 64 * D)
    Y_d = gpu_ctx.to_device(np.resize(flat, 2 * F * Tmax * D).view(np.complex128))
    init_d = gpu_ctx.to_device(rng.uniform(0.01, 1.0, size=(K, Tmax)))
    g_d = gpu_ctx.empty(8 * F * K * Tmax)
    p_d = gpu_ctx.empty(8 * K * Tmax)
    g = _capi.GssGuidance(init_dev=init_d.ptr, init_f_stride=0, init_k_stride=Tmax)
    for T in frames:
        for prior_d in (p_d, None):
            ctx = _capi.Context(0)
            try:
                status = _raw(ctx, Y_d, F, T, D, g, K, 1, 1, g_d, prior_d)
                assert status != _capi.GSS_ERR_NOMEM, (T, ctx.lib.gss_last_error(ctx.handle))
                ctx._check(status, f'gss_cacgmm_shared_prior T={T}')
                ctx.synchronize()
            finally:
                ctx.close()


# ------------------------------------------------------------------ error paths
def test_guidance_errors_are_the_guided_calls_and_leave_the_context_usable(gpu_ctx):
    from pb_chime5_amd import _capi, ops
    cell = spr.CELLS[0]
    D, T, F, K, iterations, post = cell
    Y, act = spr.parity_scene(D, T, F, K, 0)
    init, _ = spr.form_guidance('random', act, F, 0)
    ctx = gpu_ctx
    Y_d, _ = ops._obs_to_device_ftd(ctx, Y)
    init_d = ctx.to_device(init)
    mask_d = ctx.to_device(np.repeat(act[None], F, axis=0).astype(np.uint8))
    g_d, p_d = ctx.empty(8 * F * K * T), ctx.empty(8 * K * T)

    def guidance(**kw):
        base = dict(init_dev=init_d.ptr, mask_dev=mask_d.ptr, init_f_stride=K * T,
                    init_k_stride=T, mask_f_stride=K * T, mask_k_stride=T)
        return _capi.GssGuidance(**{**base, **kw})

    def good(prior_d=p_d):
        ctx._check(_raw(ctx, Y_d, F, T, D, guidance(), K, iterations, post, g_d, prior_d),
                   'gss_cacgmm_shared_prior')
        return ctx.to_host(g_d, (F, K, T), np.float64)
    want = good()
    want_prior = ctx.to_host(p_d, (K, T), np.float64)
    ref, ref_prior = spr.shared_prior_block(Y, init, np.repeat(act[None], F, axis=0), iterations,
                                            post)
    assert np.max(np.abs(want.transpose(1, 2, 0) - ref)) < EM_TOL
    assert np.max(np.abs(want_prior - ref_prior)) < EM_TOL
    cases = [
        (None, 'guidance is NULL'),
        (guidance(init_dev=None, mask_dev=None), 'init_dev and mask_dev are both NULL'),
        (guidance(init_f_stride=K * T - 1), 'init_f_stride'),
        (guidance(mask_f_stride=K * T - 1), 'mask_f_stride'),
        (guidance(init_k_stride=T - 1), 'init_k_stride'),
        (guidance(mask_f_stride=0, mask_k_stride=T - 1), 'mask_k_stride'),
        (guidance(init_f_stride=-K * T), 'init_f_stride'),
    ]
    for g, match in cases:
        status = _raw(ctx, Y_d, F, T, D, g, K, iterations, post, g_d, p_d)
        assert status == _capi.GSS_ERR_INVALID, match
        with pytest.raises(ValueError, match=match):
            ctx._check(status, 'gss_cacgmm_shared_prior')
        assert np.array_equal(good(), want), match
    with pytest.raises(ValueError, match='iterations'):
        ctx._check(_raw(ctx, Y_d, F, T, D, guidance(), K, 0, post, g_d, p_d), 'shared_prior')
    with pytest.raises(AssertionError, match='K < 20'):
        ctx._check(_raw(ctx, Y_d, F, T, D, guidance(), 20, iterations, post, g_d, p_d),
                   'shared_prior')
    # prior_dev = NULL is accepted and changes nothing
    assert np.array_equal(good(None), want)
    assert np.array_equal(ctx.to_host(p_d, (K, T), np.float64), want_prior)


# ------------------------------------------------------------------ what the method is for
def test_blind_separation_keeps_every_bin_consistent(gpu_ctx):
    """The s = 0, D = 4 run of the issue's table (F = 129, T = 1003, K = 3, 20 iterations)
    through ops.cacgmm_posteriors_blind: within the bar of the reference, and all 129 bins give
    each speaker the class the prior gives them (the reference's margin: a correlation gap of
    0.68)."""
    from pb_chime5_amd import ops
    Obs, truth, _, want, want_prior = spr.table_run(0, 4)
    got, prior = ops.cacgmm_posteriors_blind(Obs, spr.TABLE_K, spr.TABLE_ITERATIONS, seed=100,
                                             return_prior=True, ctx=gpu_ctx)
    err, perr = float(np.max(np.abs(got - want))), float(np.max(np.abs(prior - want_prior)))
    share, gap, corr = spr.bins_consistent(got, prior, truth)
    print(f'blind, table run s=0 D=4: posteriors {err:.2e}, prior {perr:.2e}; {share:.3f} of the '
          f'bins consistent, smallest gap {gap:.2f}, corr(prior, truth) {corr[0]:.2f} {corr[1]:.2f}')
    assert err < 1e-7 and perr < 1e-7
    assert share == 1.0 and got.shape[2] == 129
    assert min(corr) >= 0.6


# ------------------------------------------------------------------ the front doors
def test_gss_block_with_the_flag_equals_the_op(gpu_ctx):
    from pb_chime5_amd import core, ops
    cell = spr.CELLS[5]
    D, T, F, K, iterations, post = cell
    Y, act = spr.parity_scene(D, T, F, K, 0)
    weights = act * np.random.default_rng(3).uniform(0.2, 1.0, size=act.shape)
    gss = core.GSS(iterations=iterations, iterations_post=post, shared_prior=True)
    block = gss(Y, weights, debug=True)
    init, mask = ops.guidance_from_activity(weights)
    op, prior = ops.cacgmm_posteriors_shared_prior(Y, init, mask, iterations, post,
                                                   return_prior=True, ctx=gpu_ctx)
    assert rel_err(block, op) < 1e-10
    assert rel_err(gss.locals['prior'], prior) < 1e-10
    ref, _ = spr.shared_prior_block(Y, init, mask, iterations, post)
    assert float(np.max(np.abs(block - ref))) < EM_TOL
    with pytest.raises(NotImplementedError, match='shared_prior'):
        gss.locals['learned']
    # off: the per-frequency model, as before
    off = core.GSS(iterations=iterations, iterations_post=post)(Y, weights)
    assert np.array_equal(off, ops.cacgmm_posteriors_guided(Y, init, mask, iterations, post,
                                                            ctx=gpu_ctx))


def test_enhance_observation_blind_against_the_oracle_stages(gpu_ctx):
    """synthetic.tiny (4 channels, 12000 samples), 2 WPE taps, 3 EM iterations, against oracle
    stft -> wpe_block -> the reference -> masks -> beamform_mvdr_souden_from_masks -> istft.
    The chain's own |x_hat| moves by 2.4e-10 ... 3.7e-10 per class under a last-bit change of
    the samples (seed 0 kept by the rule); the bar is the 1e-4 of the end-to-end tests."""
    from pb_chime5_amd import core
    from pb_chime5_amd import posterior_activity as pact
    import posterior_activity_reference as par
    b = spr.BLIND
    u = spr.blind_scene()
    want, want_prior, Obs, posterior = spr.blind_reference()
    enh = core.get_enhancer(wpe_tabs=b['wpe_taps'], wpe_delay=b['wpe_delay'],
                            wpe_iterations=b['wpe_iterations'], bss_iterations=b['iterations'],
                            stft_size=b['stft_size'], stft_shift=b['stft_shift'])
    out = enh.enhance_observation_blind(u.obs, b['num_speakers'], ex=u.ex)
    K = b['num_speakers'] + 1
    assert isinstance(out, core.BlindSeparation)
    assert out.x_hat.shape == want.shape == (K, want.shape[1])
    errs = [spr.abs_rel_err(out.x_hat[k], want[k]) for k in range(K)]
    perr = float(np.max(np.abs(out.prior - want_prior)))
    print(f'enhance_observation_blind: |x_hat| rel err per class '
          f'{" ".join(f"{e:.2e}" for e in errs)}, prior {perr:.2e}')
    assert max(errs) < spr.X_TOL
    assert perr < EM_TOL
    _, power = par.posterior_activity(Obs.transpose(2, 1, 0), posterior.transpose(2, 0, 1))
    active = pact.decide(want_prior, power, None)
    assert out.active.dtype == bool and np.array_equal(out.active, active)
    assert out.intervals == [pact.frames_to_intervals(active[k], b['stft_size'], b['stft_shift'],
                                                      True, u.obs.shape[-1]) for k in range(K)]
    # a rule of the caller's reaches the decision
    strict = pact.ActivityRule(on=0.9, off=0.8)
    again = enh.enhance_observation_blind(u.obs, b['num_speakers'], ex=u.ex, rule=strict)
    assert np.array_equal(again.x_hat, out.x_hat)
    assert np.array_equal(again.active, pact.decide(want_prior, power, strict))


def test_enhance_example_blind_loads_no_annotation(gpu_ctx, monkeypatch):
    """From an example of a session that has no annotation: the audio is loaded, nothing is asked
    of the activity, and the result is `enhance_observation_blind` with the context trimmed and
    the intervals clipped to the utterance and moved to the recording's clock."""
    from pb_chime5_amd import core
    from pb_chime5_amd import posterior_activity as pact
    b = spr.BLIND
    u = spr.blind_scene()
    N, context, window_start = u.obs.shape[1], 2048, 700000
    clock = {'U03': window_start}

    def on(value):
        return {'original': value, 'observation': {k: v + value for k, v in clock.items()}}
    ex = {'session_id': 'S99', 'example_id': 'x', 'reference_array': 'U03',
          'audio_path': {'observation': {'U03': 'u03.wav'}},
          'start': on(0), 'end': on(N), 'start_orig': on(context), 'end_orig': on(N - context),
          'num_samples_orig': {'original': N - 2 * context, 'observation': {'U03': N - 2 * context}}}
    loads = []

    def load_audio(path, start, stop, dtype=np.float64):
        loads.append((path, start, stop))
        return u.obs.astype(dtype)
    monkeypatch.setattr(core, 'load_audio', load_audio)

    class NoAnnotation:
        def __getitem__(self, key):
            raise KeyError(f'no annotation for {key}')
    enh = core.get_enhancer(multiarray=False, context_samples=context, wpe_tabs=b['wpe_taps'],
                            wpe_delay=b['wpe_delay'], wpe_iterations=b['wpe_iterations'],
                            bss_iterations=b['iterations'])
    enh.activity = NoAnnotation()
    out = enh.enhance_example_blind(ex, b['num_speakers'])
    assert loads == [('u03.wav', window_start, window_start + N)]
    whole = enh.enhance_observation_blind(u.obs, b['num_speakers'], ex=ex)
    assert np.array_equal(out.x_hat, whole.x_hat[:, context:N - context])
    assert np.array_equal(out.prior, whole.prior) and np.array_equal(out.active, whole.active)
    assert out.intervals == [
        [(window_start + a, window_start + c)
         for a, c in pact.clip_intervals(row, context, N - context)] for row in whole.intervals]
    want = spr.blind_reference()[0]
    assert max(spr.abs_rel_err(out.x_hat[k], want[k, context:N - context])
               for k in range(want.shape[0])) < spr.X_TOL
