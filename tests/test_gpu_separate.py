"""The fused annotation-free window call (gss_separate_observation; ops.separate_observation,
Enhancer.enhance_observation_blind(fused=True)) and the recording driver built on it and on the
link (Enhancer.enhance_recording_blind).

The window call is held to the NumPy reference of tests/shared_prior_reference.py on its blind
scene: prior and posteriors to EM_TOL of `spr.blind_reference()`, x_hat to X_TOL of the same
reference's stages WITHOUT its context frames -- `spr.blind_reference()` zeroes the masks on the
context of the scene's example, and the fused call has no context frames (with ``ex`` and
``bf_drop_context`` it raises), so its own x_hat is printed against it, not asserted.  The
driver's mappings are asked to EQUAL those of `link_reference.recording_reference` on the periodic
scene, whose links are decided by margins of at least 0.1 (tests/golden/link_periodic.npz holds
that reference's results; tests/test_link_api.py re-derives them on the CPU)."""
import ctypes
import functools

import numpy as np
import pytest

import gss_oracle as oracle
import link_reference as lr
import shared_prior_reference as spr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

c_void_p = ctypes.c_void_p


def _blind_enhancer(**kw):
    from pb_chime5_amd import core
    b = spr.BLIND
    return core.get_enhancer(wpe_tabs=b['wpe_taps'], wpe_delay=b['wpe_delay'],
                             wpe_iterations=b['wpe_iterations'], bss_iterations=b['iterations'],
                             stft_size=b['stft_size'], stft_shift=b['stft_shift'], **kw)


@functools.lru_cache(maxsize=None)
def _reference_without_context():
    """The stages of `spr.blind_enhance` on the reference's own post-WPE Obs and posteriors, the
    masks taken as they are: x_hat (K,N)."""
    b = spr.BLIND
    _, _, Obs, posterior = spr.blind_reference()
    K = posterior.shape[0]
    return np.stack([oracle.istft(oracle.beamform_mvdr_souden_from_masks(
        Obs, posterior[k], np.sum(np.delete(posterior, k, axis=0), axis=0), ban=True),
        b['stft_size'], b['stft_shift'], fading=True) for k in range(K)])


# ------------------------------------------------------------------ the window call
def test_fused_window_against_the_reference_and_the_stage_path(gpu_ctx):
    from pb_chime5_amd import core
    b = spr.BLIND
    u = spr.blind_scene()
    with_context, want_prior, _, _ = spr.blind_reference()
    want = _reference_without_context()
    K = b['num_speakers'] + 1
    enh = _blind_enhancer()
    out = enh.enhance_observation_blind(u.obs, b['num_speakers'], fused=True)
    stage = enh.enhance_observation_blind(u.obs, b['num_speakers'])
    assert isinstance(out, core.BlindSeparation)
    assert out.x_hat.shape == stage.x_hat.shape == want.shape
    errs = [spr.abs_rel_err(out.x_hat[k], want[k]) for k in range(K)]
    stage_errs = [spr.abs_rel_err(out.x_hat[k], stage.x_hat[k]) for k in range(K)]
    ctx_errs = [spr.abs_rel_err(out.x_hat[k], with_context[k]) for k in range(K)]
    perr = float(np.max(np.abs(out.prior - want_prior)))
    stage_perr = float(np.max(np.abs(out.prior - stage.prior)))
    print(f'fused window: |x_hat| rel err per class vs the reference '
          f'{" ".join(f"{e:.2e}" for e in errs)}, vs the stage path '
          f'{" ".join(f"{e:.2e}" for e in stage_errs)} (vs the reference WITH its context frames '
          f'{" ".join(f"{e:.2e}" for e in ctx_errs)}: not asserted); prior {perr:.2e}, vs the '
          f'stage path {stage_perr:.2e}')
    assert max(errs) < spr.X_TOL and max(stage_errs) < spr.X_TOL
    assert perr < spr.EM_TOL and stage_perr < spr.EM_TOL
    assert np.array_equal(out.active, stage.active) and out.intervals == stage.intervals
    # the same call gives the same bits; the default is the stage path
    again = enh.enhance_observation_blind(u.obs, b['num_speakers'], fused=True)
    assert again.x_hat.tobytes() == out.x_hat.tobytes()
    default = enh.enhance_observation_blind(u.obs, b['num_speakers'], fused=False)
    assert default.x_hat.tobytes() == stage.x_hat.tobytes()


def test_operator_posteriors_power_and_taps(gpu_ctx):
    from pb_chime5_amd import ops
    b = spr.BLIND
    u = spr.blind_scene()
    _, want_prior, _, want_posterior = spr.blind_reference()
    K = b['num_speakers'] + 1
    params = ops.make_params(stft_size=b['stft_size'], stft_shift=b['stft_shift'],
                             wpe_taps=b['wpe_taps'], wpe_delay=b['wpe_delay'],
                             wpe_iterations=b['wpe_iterations'], bss_iterations=b['iterations'])
    T = ops.stft_frames(u.obs.shape[1], b['stft_size'], b['stft_shift'], True)
    init = ops.blind_initialization(K, T, 0)
    x_hat, prior, power, posterior, details = ops.separate_observation(
        u.obs, init, params=params, return_posterior=True, debug=True, ctx=gpu_ctx)
    gerr = float(np.max(np.abs(posterior - want_posterior)))
    perr = float(np.max(np.abs(prior - want_prior)))
    print(f'separate_observation: posteriors {gerr:.2e}, prior {perr:.2e}')
    assert posterior.shape == want_posterior.shape and gerr < spr.EM_TOL and perr < spr.EM_TOL
    assert details['posterior'].tobytes() == posterior.tobytes()
    assert 'acitivity_freq' not in details
    # the power is that of the posterior activity on the call's own observation and posteriors
    _, want_power = ops.posterior_activity(details['Obs'], details['posterior'], None,
                                           return_power=True, ctx=gpu_ctx)
    assert power.tobytes() == want_power.tobytes()
    # the prior is the operator's, the per-class taps are those of the targets call
    _, op_prior = ops.cacgmm_posteriors_blind(details['Obs'], K, b['iterations'], seed=0,
                                              return_prior=True, ctx=gpu_ctx)
    assert op_prior.tobytes() == prior.tobytes()
    assert details['target_mask'].shape == (K, T, b['stft_size'] // 2 + 1)
    np.testing.assert_array_equal(details['target_mask'], posterior)
    want = _reference_without_context()
    assert max(spr.abs_rel_err(x_hat[k], want[k]) for k in range(K)) < spr.X_TOL
    # without the optional outputs: the same signals
    plain = ops.separate_observation(u.obs, init, params=params, ctx=gpu_ctx)
    assert len(plain) == 3 and plain[0].tobytes() == x_hat.tobytes()


def _raw_separate(ctx, params, obs_d, D, N, init_d, K, out_d, prior_d, power_d, gamma_d, taps=None):
    def ptr(buf):
        return c_void_p(buf.ptr if buf is not None else None)
    return ctx.lib.gss_separate_observation(
        ctx.handle, ctypes.byref(params) if params is not None else None, ptr(obs_d), D, N,
        ptr(init_d), K, ptr(out_d), ptr(prior_d), ptr(power_d), ptr(gamma_d),
        ctypes.byref(taps) if taps is not None else None)


@pytest.mark.parametrize('D,K,frames', [(4, 3, (19, 64, 100, 327, 941, 1163, 2172, 2891)),
                                        (24, 5, (327, 941, 2172))], ids=('D4', 'D24'))
def test_fresh_context_never_runs_out_of_workspace(gpu_ctx, D, K, frames):
    """A context that has never grown its arena: the call's own workspace function covers every
    stage, with and without the optional outputs (F = 513)."""
    from pb_chime5_amd import _capi, ops
    size, shift = 1024, 256
    params = ops.make_params(stft_size=size, stft_shift=shift, wpe_iterations=1, bss_iterations=1)
    F = size // 2 + 1
    rng = np.random.default_rng(D)
    Tmax = max(frames)
    Nmax = (Tmax - 3) * shift
    obs_d = gpu_ctx.to_device(rng.standard_normal((D, Nmax)))
    init_d = gpu_ctx.to_device(rng.uniform(0.01, 1.0, size=(K, Tmax)))
    out_d, prior_d = gpu_ctx.empty(8 * K * Nmax), gpu_ctx.empty(8 * K * Tmax)
    power_d, gamma_d = gpu_ctx.empty(8 * Tmax), gpu_ctx.empty(8 * F * K * Tmax)
    for T in frames:
        N = (T - 3) * shift
        assert ops.stft_frames(N, size, shift, True) == T
        for optional in (True, False):
            ctx = _capi.Context(0)
            try:
                ops._prepare_windows(ctx, size, shift, None)
                assert ctx.workspace_bytes() == 0
                status = _raw_separate(ctx, params, obs_d, D, N, init_d, K, out_d, prior_d,
                                       power_d if optional else None,
                                       gamma_d if optional else None)
                assert status != _capi.GSS_ERR_NOMEM, (T, ctx.lib.gss_last_error(ctx.handle))
                ctx._check(status, f'gss_separate_observation T={T}')
                ctx.synchronize()
                assert ctx.workspace_bytes() > 0
            finally:
                ctx.close()


def test_unsupported_options_and_argument_errors(gpu_ctx):
    from pb_chime5_amd import _capi, ops
    ctx = gpu_ctx
    b = spr.BLIND
    u = spr.blind_scene()
    D, N = u.obs.shape
    K = 3
    size, shift = b['stft_size'], b['stft_shift']
    T = ops.stft_frames(N, size, shift, True)
    init = ops.blind_initialization(K, T, 0)
    params = ops.make_params(stft_size=size, stft_shift=shift, wpe_taps=2, wpe_iterations=1,
                             bss_iterations=1)
    # the per-array WPE is the one option gss_params can ask for that the call does not have
    per_array = ops.make_params(stft_size=size, stft_shift=shift, wpe_taps=2, wpe_iterations=1,
                                bss_iterations=1, wpe_arrays=2)
    with pytest.raises(NotImplementedError, match='per-array WPE'):
        ops.separate_observation(u.obs, init, params=per_array, ctx=ctx)
    # without WPE the field is not read
    no_wpe = ops.make_params(stft_size=size, stft_shift=shift, wpe=False, bss_iterations=1,
                             wpe_arrays=2)
    ops.separate_observation(u.obs, init, params=no_wpe, ctx=ctx)
    win = ops.ResidentSeparation(ctx, u.obs, init, params)
    good = dict(params=params, obs_d=win.obs_d, D=D, N=N, init_d=win.init_d, K=K, out_d=win.out_d,
                prior_d=win.prior_d, power_d=win.power_d, gamma_d=win.gamma_d)
    taps = _capi.GssDebugTaps(act_frames=win.power_d.ptr)
    no_iterations = ops.make_params(stft_size=size, stft_shift=shift, bss_iterations=0)
    cases = [
        (dict(params=None), _capi.GSS_ERR_INVALID, 'params is NULL'),
        (dict(obs_d=None), _capi.GSS_ERR_INVALID, 'bad arguments'),
        (dict(init_d=None), _capi.GSS_ERR_INVALID, 'bad arguments'),
        (dict(out_d=None), _capi.GSS_ERR_INVALID, 'bad arguments'),
        (dict(prior_d=None), _capi.GSS_ERR_INVALID, 'prior_dev is NULL'),
        (dict(N=0), _capi.GSS_ERR_INVALID, 'bad arguments'),
        (dict(K=0), _capi.GSS_ERR_INVALID, 'K=0'), (dict(K=20), _capi.GSS_ERR_INVALID, 'K=20'),
        (dict(D=1), _capi.GSS_ERR_UNSUPPORTED, 'D=1'),
        (dict(D=33), _capi.GSS_ERR_UNSUPPORTED, 'D=33'),
        (dict(taps=taps), _capi.GSS_ERR_INVALID, 'act_frames must be NULL'),
        (dict(params=no_iterations), _capi.GSS_ERR_INVALID, 'iterations=0'),
        (dict(params=per_array), _capi.GSS_ERR_UNSUPPORTED, 'wpe_arrays=2'),
    ]
    for kw, code, match in cases:
        status = _raw_separate(ctx, **{**good, **kw})
        assert status == code, match
        with pytest.raises((ValueError, NotImplementedError, AssertionError), match=match):
            ctx._check(status, 'gss_separate_observation')
    # the context is usable afterwards
    ctx._check(_raw_separate(ctx, **good), 'gss_separate_observation')
    x_hat, prior, power = win.result()
    assert np.all(np.isfinite(x_hat)) and np.all(np.isfinite(prior)) and np.all(power >= 0)


def test_poisoned_workspace_changes_nothing():
    """The window call under gss_debug_workspace in both fill patterns on a fresh context: no
    guard is touched and every output has the bits of the plain run."""
    from pb_chime5_amd import _capi, ops
    b = spr.BLIND
    u = spr.blind_scene()
    K = 3
    params = ops.make_params(stft_size=b['stft_size'], stft_shift=b['stft_shift'],
                             wpe_taps=b['wpe_taps'], wpe_delay=b['wpe_delay'],
                             wpe_iterations=b['wpe_iterations'], bss_iterations=b['iterations'])
    T = ops.stft_frames(u.obs.shape[1], b['stft_size'], b['stft_shift'], True)
    init = ops.blind_initialization(K, T, 0)
    ctx = _capi.Context(0)
    try:
        def run():
            return ops.separate_observation(u.obs, init, params=params, return_posterior=True,
                                            ctx=ctx)
        plain = run()
        for pattern in (0x00, 0xFF):
            ctx.debug_workspace(pattern)
            try:
                got = run()
                count, text, _ = ctx.debug_workspace_report()
            finally:
                ctx.debug_workspace(None)
            assert count == 0, text
            for name, a, c in zip(('x_hat', 'prior', 'power', 'posterior'), got, plain):
                assert a.tobytes() == c.tobytes(), (name, pattern)
    finally:
        ctx.close()


# ------------------------------------------------------------------ the recording driver
def _scene_enhancer():
    from pb_chime5_amd import core
    s = lr.SCENE
    return core.get_enhancer(wpe=False, bss_iterations=s['iterations'], stft_size=s['stft_size'],
                             stft_shift=s['stft_shift'])


@functools.lru_cache(maxsize=None)
def _recording(start):
    s = lr.SCENE
    obs, _ = lr.periodic_scene()
    return _scene_enhancer().enhance_recording_blind(
        obs, s['num_speakers'], window_samples=s['window_samples'], hop_samples=s['hop_samples'],
        seed=100 + lr.SCENE_SEED, start=start)


@pytest.mark.parametrize('start', ('fresh', 'carry'))
def test_recording_keeps_one_class_per_speaker(gpu_ctx, start):
    from pb_chime5_amd import core
    golden = np.load(GOLDEN / 'link_periodic.npz')
    want = golden[f'{start}_mappings']
    assert float(np.min(golden[f'{start}_margins'])) >= lr.MIN_MARGIN
    rec = _recording(start)
    assert isinstance(rec, core.BlindRecording)
    s = lr.SCENE
    obs, acts = lr.periodic_scene()
    n, K = want.shape
    N = obs.shape[1]
    assert rec.windows == lr.window_plan(N, s['window_samples'], s['hop_samples'])
    assert rec.x_hat.shape == (K, N) and rec.mappings.shape == rec.link_scores.shape == (n, K)
    assert rec.prior.shape == rec.active.shape == golden[f'{start}_prior'].shape
    print(f'recording {start}: mappings {rec.mappings.tolist()} (reference {want.tolist()}), '
          f'link scores {np.round(rec.link_scores[1:], 3).tolist()}, stitched prior vs the '
          f'reference {float(np.max(np.abs(rec.prior - golden[f"{start}_prior"]))):.2e}')
    np.testing.assert_array_equal(rec.mappings, want)
    np.testing.assert_array_equal(rec.mappings[0], np.arange(K))
    assert np.all(np.isnan(rec.link_scores[0])) and np.all(np.isfinite(rec.link_scores[1:]))
    if start == 'fresh':
        assert np.any(rec.mappings != np.arange(K))
    # each speaker's best class of the stitched prior is its best class in every window
    truth = lr.frame_truth(acts)
    whole = [k for k, _ in lr.best_classes(rec.prior, truth)]
    assert whole[0] != whole[1]
    assert whole == golden[f'{start}_best'].tolist()
    H = s['hop_samples'] // s['stft_shift']
    T_w = (s['window_samples'] + s['stft_size']) // s['stft_shift'] - 1
    for w in range(n):
        span = slice(w * H, w * H + T_w)
        # (inside a window the stitched prior is that window's linked prior, faded at the ends)
        mine = [k for k, _ in lr.best_classes(rec.prior[:, span], truth[:, span])]
        assert mine == whole, (w, mine, whole)
    assert len(rec.intervals) == K


def test_recording_is_the_stitch_of_its_windows(gpu_ctx):
    """x_hat equals a NumPy cross-fade of the per-window fused calls taken by the reported
    mappings (the start='fresh' run: every window starts from its own table), and the link
    scores are the link operator's on those windows' posteriors."""
    s = lr.SCENE
    obs, _ = lr.periodic_scene()
    rec = _recording('fresh')
    enh = _scene_enhancer()
    pieces, priors = [], []
    for w, (a, b) in enumerate(rec.windows):
        out = enh.enhance_observation_blind(obs[:, a:b], s['num_speakers'],
                                            seed=100 + lr.SCENE_SEED + w, fused=True)
        pieces.append(out.x_hat[rec.mappings[w], :b - a])
        priors.append(out.prior[rec.mappings[w]])
    want = lr.stitch_by_blend(pieces, [a for a, _ in rec.windows], obs.shape[1])
    err = float(np.max(np.abs(rec.x_hat - want)) / np.max(np.abs(want)))
    H = s['hop_samples'] // s['stft_shift']
    want_prior = lr.stitch_by_blend(priors, [w * H for w in range(len(priors))], rec.prior.shape[1])
    perr = float(np.max(np.abs(rec.prior - want_prior)))
    print(f'recording vs the stitch of its windows: x_hat {err:.2e} relative, prior {perr:.2e}')
    assert err <= 1e-15 and perr <= 1e-15


def test_short_recording_is_the_window_call(gpu_ctx):
    s = lr.SCENE
    obs, _ = lr.periodic_scene()
    short = np.ascontiguousarray(obs[:, :20001])
    enh = _scene_enhancer()
    for start in ('carry', 'fresh'):
        rec = enh.enhance_recording_blind(short, s['num_speakers'],
                                          window_samples=s['window_samples'],
                                          hop_samples=s['hop_samples'], seed=5, start=start)
        one = enh.enhance_observation_blind(short, s['num_speakers'], seed=5, fused=True)
        assert rec.windows == [(0, 20001)]
        assert rec.x_hat.tobytes() == np.ascontiguousarray(one.x_hat[:, :20001]).tobytes()
        assert rec.prior.tobytes() == one.prior.tobytes()
        assert np.array_equal(rec.active, one.active) and rec.intervals == one.intervals
        assert rec.mappings.tolist() == [[0, 1, 2]] and np.all(np.isnan(rec.link_scores))
