"""WPD convolutional beamformer (gss_wpd_weights, gss_wpe_weighted, gss_wpd_souden,
gss_enhance_observation_wpd) on the GPU against the plain-NumPy reference
(tests/wpd_reference.py): stage parity, the weights, the weighted WPE step
and its identity with gss_wpe, the orthogonality invariant, the gate, a silent frequency, the fused
pipeline and its block path, the workspace of a fresh context, the error codes of the C entry
points and the two pivot counters."""
import ctypes
import functools

import numpy as np
import pytest

import wpd_reference as wr
from conftest import rel_err

pytestmark = pytest.mark.gpu

STAGE_BAR = 1e-9        # the project's stage bar


@functools.lru_cache(maxsize=None)
def _scene(D, T, F, taps, delay):
    Y, m, g = wr.scene(np.random.default_rng(1000 * D + T), D, T, F, taps, delay)
    for a in (Y, m, g):
        a.setflags(write=False)
    assert g[0] == 0 and g[-1] == 0 and g.sum() < T - 2      # context on both sides
    return Y, m, g


@functools.lru_cache(maxsize=None)
def _reference(scene, ban, iterations, ref_channel):
    D, T, F, taps, delay = scene
    Y, m, g = _scene(*scene)
    want, det = wr.wpd_souden_from_masks(Y, m, ban, taps=taps, delay=delay, iterations=iterations,
                                         frame_gate=g, ref_channel=ref_channel)
    # a badly drawn scene fails loudly
    assert np.linalg.cond(det['phi_a']).max() <= 1e5, np.linalg.cond(det['phi_a'])
    assert np.all(np.isfinite(want))
    want.setflags(write=False)
    return want, det


# ------------------------------------------------------------------ 1. stage parity
@pytest.mark.parametrize('named', [False, True], ids=['chosen', 'named'])
@pytest.mark.parametrize('iterations', [1, 2])
@pytest.mark.parametrize('ban', [False, True])
@pytest.mark.parametrize('scene', wr.STAGE_SCENES, ids=str)
def test_stage_matches_the_reference(gpu_ctx, scene, ban, iterations, named):
    """max|X_hat - ref| <= 1e-9 max|ref|, the reference channel equal as an integer; with the
    channel chosen and with another one named."""
    from pb_chime5_amd import ops
    D, T, F, taps, delay = scene
    Y, m, g = _scene(*scene)
    _, chosen = _reference(scene, ban, iterations, None)
    name = (chosen['ref_channel'] + 1) % D if named else None
    want, det = _reference(scene, ban, iterations, name)
    got, ref, pivots = ops.wpd_souden_from_masks(
        Y, m, ban=ban, taps=taps, delay=delay, iterations=iterations, frame_gate=g,
        ref_channel=name, return_ref_channel=True, return_zero_pivots=True, ctx=gpu_ctx)
    print(f'{scene} ban={ban} iterations={iterations} named={named}: rel err '
          f'{rel_err(got, want):.1e}, ref {ref} / {det["ref_channel"]}')
    assert ref == det['ref_channel'] == gpu_ctx.last_ref_channel()
    assert pivots == 0
    assert rel_err(got, want) <= STAGE_BAR
    if named:       # the channel matters
        assert rel_err(got, _reference(scene, ban, iterations, None)[0]) > 1e-3


# ------------------------------------------------------------------ 2. weights
@pytest.mark.parametrize('scene', wr.STAGE_SCENES + [(1, 70, 2, 2, 1)], ids=str)
def test_weights_from_both_sources(gpu_ctx, scene):
    """Both sources against NumPy at 1e-13, gated and not; a frequency without power and a gate
    that removes every frame give all-zero weights."""
    from pb_chime5_amd import ops
    D, T, F, taps, delay = scene
    Y, m, g = _scene(*scene)
    Yf = Y.transpose(2, 0, 1)
    for gate in (g, None):
        ones = np.ones(T) if gate is None else gate
        for floor in (1e-3, 1.0):
            want = wr.weights(wr.masked_power(Yf, m.T), ones, floor)
            got = ops.wpd_weights(Y, m, frame_gate=gate, power_floor=floor, ctx=gpu_ctx)
            assert rel_err(got, want) <= 1e-13, (scene, floor, rel_err(got, want))
            assert np.all(got[:, ones == 0] == 0) and np.all(got[:, ones != 0] > 0)
        xh = np.ascontiguousarray(Y[0]) * m
        want = wr.weights(np.abs(xh.T) ** 2, ones)
        got = ops.wpd_weights(X_hat=xh, frame_gate=gate, ctx=gpu_ctx)
        assert rel_err(got, want) <= 1e-13, (scene, rel_err(got, want))
    # a silent frequency, in both sources; the others are untouched
    Y0 = Y.copy()
    Y0[:, :, 1] = 0
    got = ops.wpd_weights(Y0, m, frame_gate=g, ctx=gpu_ctx)
    assert np.all(got[1] == 0)
    assert np.array_equal(got[0], ops.wpd_weights(Y, m, frame_gate=g, ctx=gpu_ctx)[0])
    got = ops.wpd_weights(X_hat=np.ascontiguousarray(Y0[0]), frame_gate=g, ctx=gpu_ctx)
    assert np.all(got[1] == 0) and np.all(got[0, g != 0] > 0)
    # power on gated-out frames only is no power
    Y1 = Y.copy()
    Y1[:, g != 0, 1] = 0
    assert np.all(ops.wpd_weights(Y1, m, frame_gate=g, ctx=gpu_ctx)[1] == 0)
    # a gate that removes all frames
    none = np.zeros(T)
    assert np.all(ops.wpd_weights(Y, m, frame_gate=none, ctx=gpu_ctx) == 0)
    assert np.all(ops.wpd_weights(X_hat=np.ascontiguousarray(Y[0]), frame_gate=none,
                                  ctx=gpu_ctx) == 0)


def test_weights_of_a_mask_with_100_db_of_dynamic_range(gpu_ctx):
    from pb_chime5_amd import ops
    scene = (5, 130, 4, 3, 2)
    D, T, F, _, _ = scene
    Y, _, g = _scene(*scene)
    rng = np.random.default_rng(100)
    m = 10.0 ** rng.uniform(-10, 0, size=(T, F))
    m[rng.integers(0, T, 6), rng.integers(0, F, 6)] = [1.0, 1e-10, 1.0, 1e-10, 1.0, 1e-10]
    assert np.isclose(m.max() / m.min(), 1e10, rtol=1e-12)
    for floor in (1e-3, 1e-12):
        want = wr.weights(wr.masked_power(Y.transpose(2, 0, 1), m.T), g, floor)
        got = ops.wpd_weights(Y, m, frame_gate=g, power_floor=floor, ctx=gpu_ctx)
        print(f'floor {floor:g}: weights span {got.max() / got[got > 0].min():.1e}, rel err '
              f'{rel_err(got, want):.1e}, worst element '
              f'{np.max(np.abs(got - want)[want > 0] / want[want > 0]):.1e}')
        # every element on its own scale: the small weights are held to the bar too
        assert np.max(np.abs(got - want)[want > 0] / want[want > 0]) <= 1e-13
        assert np.array_equal(got == 0, want == 0)


# ------------------------------------------------------------------ 3. weighted WPE step
@pytest.mark.parametrize('scene', wr.STAGE_SCENES, ids=str)
def test_weighted_wpe_step(gpu_ctx, scene):
    """One step with arbitrary weights against the oracle at 1e-9, and fed with
    gss_wpe_inverse_power the bits of gss_wpe(iterations=1)."""
    from pb_chime5_amd import ops
    D, T, F, taps, delay = scene
    Y, m, g = _scene(*scene)
    Yf = Y.transpose(2, 0, 1)
    a = wr.weights(wr.masked_power(Yf, m.T), g)
    want, _ = wr.wpe_step(Yf, a, taps, delay)
    got = ops.wpe_weighted(Y, a, taps, delay, ctx=gpu_ctx)
    assert gpu_ctx.last_wpe_zero_pivots() == 0
    print(f'{scene}: weighted step rel err {rel_err(got, want.transpose(1, 2, 0)):.1e}')
    assert rel_err(got, want.transpose(1, 2, 0)) <= STAGE_BAR
    w = ops.get_power_inverse(Yf, ctx=gpu_ctx)
    assert np.array_equal(ops.wpe_weighted(Y, w, taps, delay, ctx=gpu_ctx),
                          ops.wpe_dtf(Y, taps, delay, iterations=1, ctx=gpu_ctx))


# ------------------------------------------------------------------ 4. the invariant
@pytest.mark.parametrize('scene', wr.STAGE_SCENES, ids=str)
def test_output_is_orthogonal_to_the_tap_window(gpu_ctx, scene):
    """rho (wpd_reference.orthogonality) <= 1e-9 on the device's WPD output and >= 1e-2 for
    gss_wpe (3 iterations) + gss_mvdr_souden on the same scene.  On the CPU the values were
    <= 2e-13 and >= 0.08.  Cannot pass without the feature."""
    from pb_chime5_amd import ops
    D, T, F, taps, delay = scene
    Y, m, g = _scene(*scene)
    a = ops.wpd_weights(Y, m, frame_gate=g, ctx=gpu_ctx)
    x = ops.wpd_souden_from_masks(Y, m, taps=taps, delay=delay, frame_gate=g, ctx=gpu_ctx)
    rho = wr.orthogonality(Y, a, x, taps, delay)
    Z = ops.wpe_dtf(Y, taps, delay, iterations=3, ctx=gpu_ctx)
    old = ops.mvdr_souden_from_masks(Z, m * g[:, None], (1 - m) * g[:, None], ctx=gpu_ctx)
    rho_old = wr.orthogonality(Y, a, old, taps, delay)
    print(f'{scene}: rho WPD {rho:.1e}, WPE + MVDR {rho_old:.1e}')
    assert rho <= 1e-9
    assert rho_old >= 1e-2


# ------------------------------------------------------------------ 5. gate, repeatability
@pytest.mark.parametrize('iterations', [1, 2])
def test_gated_frames_do_not_matter_and_calls_repeat(gpu_ctx, iterations):
    from pb_chime5_amd import ops
    scene = (5, 130, 4, 3, 2)
    D, T, F, taps, delay = scene
    Y, m, g = _scene(*scene)
    kw = dict(ban=True, taps=taps, delay=delay, iterations=iterations, frame_gate=g, ctx=gpu_ctx)
    x = ops.wpd_souden_from_masks(Y, m, **kw)
    assert np.array_equal(ops.wpd_souden_from_masks(Y, m, **kw), x)
    m2 = m.copy()
    m2[g == 0] = np.random.default_rng(5).uniform(0, 1, size=(int((g == 0).sum()), F))
    assert not np.array_equal(m2, m)
    assert np.array_equal(ops.wpd_souden_from_masks(Y, m2, **kw), x)
    # the gate itself matters
    assert rel_err(ops.wpd_souden_from_masks(Y, m, **{**kw, 'frame_gate': None}), x) > 1e-6
    a = ops.wpd_weights(Y, m, frame_gate=g, ctx=gpu_ctx)
    assert np.array_equal(ops.wpd_weights(Y, m2, frame_gate=g, ctx=gpu_ctx), a)


# ------------------------------------------------------------------ 6. a silent frequency
@pytest.mark.parametrize('iterations', [1, 2])
@pytest.mark.parametrize('ban', [False, True])
def test_a_frequency_that_is_zero_in_every_channel(gpu_ctx, ban, iterations):
    """p_max = 0 there: a = 0, the MVDR of two all-zero masks -- 0, or NaN under `ban` --, in
    the reference and on the device, at the same positions; the other frequencies at the bar.
    The zero rows of R are zeroed pivots, counted in the WPD's word and not in the WPE's."""
    from pb_chime5_amd import ops
    scene = (5, 130, 4, 3, 2)
    D, T, F, taps, delay = scene
    Y, m, g = _scene(*scene)
    Y = Y.copy()
    Y[:, :, 2] = 0
    want, det = wr.wpd_souden_from_masks(Y, m, ban, taps=taps, delay=delay, iterations=iterations,
                                         frame_gate=g)
    before = gpu_ctx.last_wpe_zero_pivots()
    got, ref, pivots = ops.wpd_souden_from_masks(
        Y, m, ban=ban, taps=taps, delay=delay, iterations=iterations, frame_gate=g,
        return_ref_channel=True, return_zero_pivots=True, ctx=gpu_ctx)
    assert ref == det['ref_channel']
    assert pivots == iterations * taps * D
    assert gpu_ctx.last_wpe_zero_pivots() == before
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.all(np.isnan(want[:, 2])) if ban else np.all(want[:, 2] == 0)
    live = [0, 1, 3]
    assert np.all(np.isfinite(got[:, live]))
    assert rel_err(got[:, live], want[:, live]) <= STAGE_BAR
    if not ban:
        assert np.all(got[:, 2] == 0)


# ------------------------------------------------------------------ 9. error codes
def test_c_abi_argument_errors_name_the_field(gpu_ctx):
    from pb_chime5_amd import _capi, ops
    ctx = gpu_ctx
    F, T, D = 3, 130, 4
    buf = ctx.empty(16 * F * T * 32)
    p = _capi.c_void_p(buf.ptr)
    INVALID = _capi.GSS_ERR_INVALID
    good = dict(taps=3, delay=2, iterations=1, ban=1, power_floor=1e-3)
    bad_fields = ((dict(taps=0), 'taps'), (dict(delay=-1), 'delay'), (dict(iterations=0), 'iterations'),
                  (dict(power_floor=0.0), 'power_floor'), (dict(power_floor=1.5), 'power_floor'),
                  (dict(power_floor=-1e-3), 'power_floor'),
                  (dict(power_floor=float('nan')), 'power_floor'),
                  (dict(power_floor=float('inf')), 'power_floor'))

    def error():
        return ctx.lib.gss_last_error(ctx.handle).decode()

    def stage(bf=good, D=D, ref=-1, Y=p, mask=p, out=p):
        bf = _capi.GssBfWpd(**bf) if bf is not None else None
        return ctx.lib.gss_wpd_souden(ctx.handle, Y, F, T, D, mask, None,
                                      ctypes.byref(bf) if bf is not None else None, ref, out, None)
    for bad, word in bad_fields:
        assert stage({**good, **bad}) == INVALID, bad
        assert word in error(), (bad, error())
    for kw, word in ((dict(bf=None), 'wpd'), (dict(D=30), 'D < 30'), (dict(D=0), 'D=0'),
                     (dict(ref=D), 'ref_channel'), (dict(ref=-2), 'ref_channel'),
                     (dict(Y=None), 'Y_dev'), (dict(mask=None), 'target_mask_dev'),
                     (dict(out=None), 'Xhat_dev')):
        assert stage(**kw) == INVALID, kw
        assert word in error(), (kw, error())

    def weights(Y=p, mask=p, xhat=None, floor=1e-3, out=p, D=D):
        return ctx.lib.gss_wpd_weights(ctx.handle, Y, F, T, D, mask, xhat, None, floor, out)
    for kw, word in ((dict(out=None), 'weights_dev'), (dict(Y=None), 'neither'),
                     (dict(mask=None), 'neither'), (dict(floor=0.0), 'power_floor'),
                     (dict(floor=float('nan')), 'power_floor'), (dict(floor=2.0), 'power_floor'),
                     (dict(D=30), 'D < 30')):
        assert weights(**kw) == INVALID, kw
        assert word in error(), (kw, error())
    assert weights(Y=None, mask=None, xhat=p) == 0

    def step(Y=p, w=p, out=p, taps=3, delay=2):
        return ctx.lib.gss_wpe_weighted(ctx.handle, Y, F, T, D, taps, delay, w, out)
    for kw in (dict(Y=None), dict(w=None), dict(out=None), dict(taps=0), dict(delay=-1)):
        assert step(**kw) == INVALID, kw

    ops._prepare_windows(ctx, 1024, 256)
    big = ctx.empty(8 * 4 * 4096)
    q = _capi.c_void_p(big.ptr)

    def fused(bf=good, params=None, D=4, target=0):
        params = params or ops.make_params()
        bf = _capi.GssBfWpd(**bf) if bf is not None else None
        return ctx.lib.gss_enhance_observation_wpd(
            ctx.handle, ctypes.byref(params), q, D, 4096, q, 2, 4096, target, 0, 0,
            ctypes.byref(bf) if bf is not None else None, q, None)
    for name in ('gev_ban', 'ch2', 'sum'):
        assert fused(params=ops.make_params(bf=name)) == _capi.GSS_ERR_UNSUPPORTED, name
    assert fused(None) == INVALID and 'wpd' in error()
    assert fused(D=30) == INVALID and 'D < 30' in error()
    assert fused(target=2) == INVALID and 'target_index' in error()
    for bad, word in bad_fields:
        assert fused({**good, **bad}) == INVALID, bad
        assert word in error(), (bad, error())

    out64 = ctypes.c_int64(-1)
    assert ctx.lib.gss_last_wpd_zero_pivots(ctx.handle, None) == INVALID
    assert ctx.lib.gss_last_wpd_zero_pivots(ctx.handle, ctypes.byref(out64)) == 0 <= out64.value


# ------------------------------------------------------------------ 7. fused
FUSED = dict(stft_size=256, stft_shift=64, wpe_tabs=2, wpe_iterations=2, bss_iterations=5)


@functools.lru_cache(maxsize=None)
def _fused_scene(D, speakers=3):
    from pb_chime5_amd import synthetic
    # (a few hundred frames of 64 samples; sensor noise 30 dB below the speech keeps the WPE and
    # Phi_a well conditioned, as in the small pipeline tests)
    return synthetic.tiny(seed=40 + D, num_channels=D, num_samples=19200, num_speakers=speakers,
                          context=2048, noise=3e-2)


FUSED_CASES = [(6, dict(bf='wpdSouden_ban')), (6, dict(bf='wpdSouden_ban', bf_wpd_iterations=2)),
               (4, dict(bf='wpdSouden')), (4, dict(bf='wpdSouden_ban', wpe=False)),
               (4, dict(bf='wpdSouden_ban', postfilter='mask_mul')),
               (4, dict(bf='wpdSouden_ban', bf_drop_context=False)),
               (4, dict(bf='wpdSouden_ban', bf_wpd_taps=5, bf_wpd_delay=1, bf_wpd_power_floor=1e-2))]


@pytest.mark.parametrize('D,options', FUSED_CASES, ids=str)
def test_fused_call_against_the_composition_of_stages_and_reference(gpu_ctx, D, options):
    """Enhancer.enhance_observation(bf='wpdSouden*') against STFT -> WPE -> posteriors (the
    existing stage operators) -> reference masks -> reference WPD ON THE RAW STFT -> iSTFT:
    |X_hat| and x_hat at 1e-6 relative; the block path (stage calls on the raw STFT) equals the
    fused call at 1e-9 -- the bars tests/test_gpu_lcmv.py uses for the same two comparisons."""
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import get_enhancer, start_end_context_frames
    from pb_chime5_amd.database.chime5 import activity_time_to_frequency
    u = _fused_scene(D)
    keys = list(u.activity)
    target = keys.index(u.speaker_id)
    enh = get_enhancer(**{**FUSED, **options})
    assert enh._fusable()
    got = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, debug=True)
    det = enh.enhance_observation_locals['details']
    wpd_pivots, wpe_pivots = det['wpd_zero_pivots'], enh._ctx().last_wpe_zero_pivots()

    size, shift = FUSED['stft_size'], FUSED['stft_shift']
    raw = ops.stft(u.obs, size, shift, ctx=gpu_ctx)
    Obs = raw
    if options.get('wpe', True):
        Obs = ops.wpe_dtf(raw, taps=2, delay=2, iterations=2, ctx=gpu_ctx)
    actf = activity_time_to_frequency(np.array(list(u.activity.values())),
                                      stft_window_length=size, stft_shift=shift,
                                      stft_fading=True, stft_pad=True)
    posterior = ops.cacgmm_posteriors(Obs, actf, iterations=5, ctx=gpu_ctx)
    drop = options.get('bf_drop_context', True)
    sf, ef = start_end_context_frames(u.ex, size, shift, True)
    assert sf > 0 and ef > 0
    xm, nm = wr.masks_from_posteriors(posterior, target, sf, ef, drop)
    gate = wr.context_gate(raw.shape[1], sf, ef) if drop else None
    ban = options['bf'] == 'wpdSouden_ban'
    X_want, wdet = wr.wpd_souden_from_masks(
        raw, xm, ban, taps=options.get('bf_wpd_taps', 2), delay=options.get('bf_wpd_delay', 2),
        iterations=options.get('bf_wpd_iterations', 1),
        power_floor=options.get('bf_wpd_power_floor', 1e-3), frame_gate=gate)
    assert np.linalg.cond(wdet['phi_a']).max() <= 1e8
    if options.get('postfilter') == 'mask_mul':
        X_want = X_want * xm
    want = ops.istft(X_want, size, shift, ctx=gpu_ctx)
    err = rel_err(np.abs(det['X_hat']), np.abs(X_want))
    print(f'D={D} {options}: |X_hat| rel err {err:.1e}, x_hat {rel_err(got, want):.1e}, ref '
          f'{det["ref_channel"]} / {wdet["ref_channel"]}, cond(Phi_a) '
          f'{np.linalg.cond(wdet["phi_a"]).max():.1e}')
    assert det['ref_channel'] == wdet['ref_channel'] == enh._ctx().last_ref_channel()
    assert wpd_pivots == 0 == wpe_pivots
    assert err <= 1e-6
    assert rel_err(got, want) <= 1e-6
    # the taps keep their meaning: the input of the mixture model, the masks of the MVDR call
    assert rel_err(det['Obs'], Obs) <= 1e-9
    assert np.array_equal(det['target_mask'],
                          wr.masks_from_posteriors(det['posterior'], target, sf, ef, drop)[0])
    assert rel_err(det['target_mask'], xm) <= 1e-9
    assert rel_err(det['distortion_mask'], nm) <= 1e-9
    # the block path
    blocks = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, fused=False,
                                     debug=True)
    print(f'D={D} {options}: block path vs fused {rel_err(blocks, got):.1e}')
    assert rel_err(blocks, got) <= 1e-9
    # it is another signal than WPE + MVDR
    if options == dict(bf='wpdSouden_ban'):
        plain = get_enhancer(**FUSED, bf='mvdrSouden_ban')
        assert rel_err(got, plain.enhance_observation(u.obs, u.activity, u.speaker_id,
                                                      ex=u.ex)) > 1e-3


def test_fused_call_with_wpe_per_array(gpu_ctx):
    """wpe_per_array only shapes the WPE that feeds the mixture model: the WPD works on the copy
    of the raw STFT that the fused call keeps beside it."""
    from pb_chime5_amd.core import get_enhancer
    u = _fused_scene(6)
    enh = get_enhancer(**FUSED, bf='wpdSouden_ban', wpe_per_array=True,
                       multiarray='outer_array_mics')
    got = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, wpe_arrays=3)
    blocks = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, wpe_arrays=3,
                                     fused=False)
    joint = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, wpe_arrays=1)
    print(f'per-array WPE: block path vs fused {rel_err(blocks, got):.1e}, vs joint '
          f'{rel_err(got, joint):.1e}')
    assert np.all(np.isfinite(got)) and rel_err(blocks, got) <= 1e-9
    assert rel_err(got, joint) > 1e-6


def test_wrapper_and_block_reach_the_wpd_kernels(gpu_ctx):
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import Beamformer
    from pb_chime5_amd.speech_enhancement.beamforming_wrapper import beamform_wpd_souden_from_masks
    scene = (5, 130, 4, 3, 2)
    D, T, F, taps, delay = scene
    Y, m, g = _scene(*scene)
    for ban in (False, True):
        direct = ops.wpd_souden_from_masks(Y, m, ban=ban, taps=taps, delay=delay, frame_gate=g,
                                           ctx=gpu_ctx)
        kw = dict(ban=ban, taps=taps, delay=delay, frame_gate=g)
        assert np.array_equal(beamform_wpd_souden_from_masks(Y, m, **kw), direct)
        assert np.array_equal(beamform_wpd_souden_from_masks(
            Y[None], np.broadcast_to(m, (1, D, T, F)), **kw), direct)
        assert np.array_equal(beamform_wpd_souden_from_masks(
            Y, np.broadcast_to(m, (D, T, F)), **kw), direct)
    block = Beamformer('wpdSouden_ban', 'mask_mul', wpd_taps=taps, wpd_delay=delay)
    assert np.array_equal(block(Y * 0.5, m, 1 - m, raw_obs=Y, frame_gate=g), direct * m)
    # raw_obs defaults to Obs
    assert np.array_equal(block(Y, m, 1 - m, frame_gate=g), direct * m)


# ------------------------------------------------------------------ 8. workspace
WORKSPACE_FRAMES = tuple(range(70, 70 + 12 * 7, 7)) + (1000,)


@pytest.mark.parametrize('D', [4, 24])
def test_fresh_context_over_a_sweep_of_lengths(gpu_ctx, D):
    """A context that has never grown its arena, for a sweep of N at the smallest STFT size the
    pipeline tests use (64 / 16): a frame adds so little that the sweep meets the 1 MiB rounding
    of the arena at many offsets, and the reserve formula decides -- the raw STFT beside the
    per-array WPE's output, the gate and the WPD's own workspace (10 taps against the WPE's 2:
    its solve is the largest stage) included.  Stage call and fused call."""
    from pb_chime5_amd import _capi, ops
    K, size, shift = 3, 64, 16
    F = size // 2 + 1
    analysis = ops.analysis_window(size)
    synthesis = ops.synthesis_window(analysis, shift)
    samples = []
    for t in WORKSPACE_FRAMES:
        n = max(t * shift - size - 3 * shift, shift)
        while ops.stft_frames(n, size, shift, True) < t:
            n += 1
        assert ops.stft_frames(n, size, shift, True) == t
        samples.append(n)
    Nmax, Tmax = max(samples), max(WORKSPACE_FRAMES)
    rng = np.random.default_rng(D)
    obs_d = gpu_ctx.to_device(rng.standard_normal((D, Nmax)))
    act = rng.random((K, Nmax)) < 0.7
    act[-1] = True
    act_d = gpu_ctx.to_device(act.astype(np.uint8))
    out_d = gpu_ctx.empty(8 * int(gpu_ctx.lib.gss_istft_num_samples(Tmax, size, shift, 1)))
    Y_d = gpu_ctx.to_device(rng.standard_normal(2 * F * Tmax * D).view(np.complex128))
    m_d = gpu_ctx.to_device(rng.uniform(0.05, 0.95, size=F * Tmax))
    X_d = gpu_ctx.empty(16 * F * Tmax)
    p = _capi.c_void_p
    bf = ops.check_bf_wpd(10, 2, 2, 1e-3, True, D)
    for i, (N, T) in enumerate(zip(samples, WORKSPACE_FRAMES)):
        params = ops.make_params(stft_size=size, stft_shift=shift, wpe=i % 3 != 2, wpe_taps=2,
                                 wpe_iterations=1, bss_iterations=1,
                                 wpe_arrays=2 if i % 3 == 1 else 0)
        for fused in (False, True):
            ctx = _capi.Context(0)
            try:
                if fused:
                    ctx.set_windows(size, shift, analysis, synthesis)
                    status = ctx.lib.gss_enhance_observation_wpd(
                        ctx.handle, ctypes.byref(params), p(obs_d.ptr), D, N, p(act_d.ptr), K, Nmax,
                        0, 5 * shift, 4 * shift, ctypes.byref(bf), p(out_d.ptr), None)
                else:
                    status = ctx.lib.gss_wpd_souden(
                        ctx.handle, p(Y_d.ptr), F, T, D, p(m_d.ptr), None, ctypes.byref(bf), -1,
                        p(X_d.ptr), None)
                assert status != _capi.GSS_ERR_NOMEM, (N, fused, ctx.lib.gss_last_error(ctx.handle))
                ctx._check(status, f'WPD N={N} fused={fused}')
                assert 0 <= ctx.last_ref_channel() < D
            finally:
                ctx.close()


# ------------------------------------------------------------------ 10. the two pivot counters
def test_the_pivot_counters_of_wpe_and_wpd_are_separate(gpu_ctx):
    """A dead microphone zeroes pivots in every solve.  After the fused call
    gss_last_wpe_zero_pivots is the WPE stage's count -- the one the same pipeline with the MVDR
    reports -- and gss_last_wpd_zero_pivots the WPD's -- the one the stage call on the raw STFT
    reports; with different taps and iterations they differ."""
    from pb_chime5_amd import ops, synthetic
    u = synthetic.tiny(seed=3, num_channels=6, num_samples=24000, num_speakers=2)
    obs = u.obs.copy()
    obs[2] = 0.0
    cs = ce = 2048
    kw = dict(stft_size=256, stft_shift=64, wpe=True, wpe_taps=4, wpe_iterations=2,
              bss_iterations=3, ctx=gpu_ctx)
    ops.enhance_observation(obs, u.activity_array, u.target_index, cs, ce, **kw)
    wpe_count = gpu_ctx.last_wpe_zero_pivots()
    x_hat, det = ops.enhance_observation_wpd(obs, u.activity_array, u.target_index, cs, ce,
                                             taps=3, delay=2, iterations=3, debug=True, **kw)
    assert np.all(np.isfinite(x_hat))
    fused_wpe, fused_wpd = gpu_ctx.last_wpe_zero_pivots(), det['wpd_zero_pivots']
    raw = ops.stft(obs, 256, 64, ctx=gpu_ctx)
    sf = ops.samples_to_stft_frames(cs, 256, 64, fading=True)
    gate = wr.context_gate(raw.shape[1], sf, sf)
    _, stage_wpd = ops.wpd_souden_from_masks(raw, det['target_mask'], ban=True, taps=3, delay=2,
                                             iterations=3, frame_gate=gate,
                                             return_zero_pivots=True, ctx=gpu_ctx)
    print(f'zero pivots: WPE stage {wpe_count}, after the fused WPD call {fused_wpe}; WPD '
          f'{fused_wpd}, stage call {stage_wpd}')
    assert fused_wpe == wpe_count > 0
    assert fused_wpd == stage_wpd > 0
    assert fused_wpd != fused_wpe
    # a later WPE call does not touch the WPD's word
    ops.wpe_dtf(raw, 4, 2, 1, ctx=gpu_ctx)
    assert gpu_ctx.last_wpd_zero_pivots() == fused_wpd
    assert 0 < gpu_ctx.last_wpe_zero_pivots() < wpe_count
