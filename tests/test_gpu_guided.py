"""Weighted and per-frequency guidance of the CACGMM on the GPU (gss_cacgmm_guided,
gss_enhance_observation_guided, GSS.__call__ with weights, Enhancer.enhance_observation_guided).

The reference for every number is the untouched oracle: `_oracle_guided` calls
CACGMMTrainer.fit / predict the way oracle.gss_block_batched does, with any (F,K,T)
initialisation and mask."""
import ctypes

import numpy as np
import pytest

import gss_oracle as oracle
from conftest import rel_err
from test_gpu_stages import _scene

pytestmark = pytest.mark.gpu

# (D, T, F, K, iterations, post): scenes and seeds as test_cacgmm_matches_oracle
SHAPES = [(4, 300, 6, 3, 5, 1), (4, 100, 6, 3, 3, 0), (2, 64, 3, 2, 4, 1), (7, 200, 4, 4, 6, 1),
          (24, 400, 3, 5, 10, 1), (12, 333, 3, 5, 8, 0), (4, 900, 4, 5, 8, 2), (4, 900, 4, 6, 20, 1),
          (6, 129, 3, 8, 4, 1)]


def _oracle_guided(Y, init_fkt, mask_fkt, iterations, post):
    """Y (D,T,F), initialisation (F,K,T), mask (F,K,T) bool or None -> posterior (K,T,F): the
    steps of oracle.gss_block_batched."""
    trainer = oracle.CACGMMTrainer()
    y = np.ascontiguousarray(Y.transpose(2, 1, 0))  # (F, T, D)
    cur = trainer.fit(y, init_fkt, iterations=iterations, source_activity_mask=mask_fkt)
    if post != 0:
        if post != 1:
            cur = trainer.fit(y, cur, iterations=post - 1)
        aff = cur.predict(y)
    else:
        aff = cur.predict(y, source_activity_mask=mask_fkt)
    return aff.transpose(1, 2, 0)


def _scene_of(D, T, F, K):
    rng = np.random.default_rng(D + T + K)
    Y, act = _scene(rng, D, T, F, K)
    return rng, Y, act


def _per_frequency_guidance(rng, act, F):
    """Mask (F,K,T): the activity, class 0 dropped on the first T/3 frames of the upper half of
    the bins (the last class stays on); initialisation U(0.01, 1) * where(mask, 1, 1e-10)
    normalised over k."""
    K, T = act.shape
    mask = np.repeat(act[None], F, axis=0)
    mask[F // 2:, 0, :T // 3] = False
    init = rng.uniform(0.01, 1.0, size=(F, K, T)) * np.where(mask, 1.0, 1e-10)
    init /= init.sum(axis=1, keepdims=True)
    return init, mask


# ------------------------------------------------------------------ 1. nothing existing moves
@pytest.mark.parametrize('D,T,F,K,iters', [
    (4, 700, 3, 5, 6), (4, 257, 2, 2, 5), (4, 513, 2, 6, 4),      # one launch (em_onchip4_kernel)
    (4, 300, 3, 8, 4),                                            # D = 4, more classes than it takes
    (7, 200, 4, 4, 5), (24, 400, 3, 5, 6), (12, 333, 3, 5, 4), (6, 129, 3, 9, 3)])
@pytest.mark.parametrize('post', [0, 1, 2])
def test_binary_guidance_equals_the_unweighted_call_bit_for_bit(gpu_ctx, D, T, F, K, iters, post):
    """{NULL, act, 0, 0, 0, T} is gss_cacgmm: the same kernels read the same bytes."""
    from pb_chime5_amd import ops
    _, Y, act = _scene_of(D, T, F, K)
    want = ops.cacgmm_posteriors(Y, act, iters, post, ctx=gpu_ctx)
    got = ops.cacgmm_posteriors_guided(Y, None, act, iters, post, ctx=gpu_ctx)
    assert np.array_equal(got, want)


def _tiny(D):
    """A synthetic.tiny scene and the pipeline's parameters for it.  24 channels: the recipe of
    test_other_channel_and_class_counts -- enough frames per unknown of the WPE (T = 253,
    taps * D = 48) and sensor noise 30 dB below the speech.  (With tiny's default noise of
    1e-3, three point sources on 24 microphones leave the WPE's normal equations singular to
    rounding: the oracle's own |X_hat| then moves by 2e-3 when the samples change in the last
    bit; on this scene it moves by 7e-8 and cond(Phi_N) < 1e8 in every bin.)"""
    from pb_chime5_amd import synthetic
    if D == 4:
        return synthetic.tiny(seed=5, num_channels=4, num_samples=24000, num_speakers=3,
                              context=2048), dict(wpe_taps=4, wpe_iterations=3, bss_iterations=6)
    return synthetic.tiny(seed=6, num_channels=24, num_samples=64000, num_speakers=3,
                          context=4096, noise=3e-2), dict(wpe_taps=2, wpe_iterations=2,
                                                          bss_iterations=6)


def _context_samples(u):
    return (u.ex['start_orig']['original'] - u.ex['start']['original'],
            u.ex['end']['original'] - u.ex['end_orig']['original'])


def _frame_activity(u, T):
    return oracle.activity_time_to_frequency(u.activity_array, 1024, 256, True, stft_pad=True)[:, :T]


@pytest.mark.parametrize('D', [4, 24])
def test_fused_guided_call_fed_the_frame_activity_is_the_fused_call(gpu_ctx, D):
    from pb_chime5_amd import ops
    u, kw = _tiny(D)
    cs, ce = _context_samples(u)
    x, det = ops.enhance_observation(u.obs, u.activity_array, u.target_index, cs, ce,
                                     debug=True, ctx=gpu_ctx, **kw)
    T = det['Obs'].shape[1]
    actf = _frame_activity(u, T)
    assert np.array_equal(actf, det['acitivity_freq'])
    gx, gdet = ops.enhance_observation_guided(u.obs, None, actf, u.target_index, cs, ce,
                                              debug=True, ctx=gpu_ctx, **kw)
    assert np.array_equal(gx, x)
    for key in ('Obs', 'posterior', 'target_mask', 'distortion_mask', 'X_hat'):
        assert np.array_equal(gdet[key], det[key]), key
    assert gdet['ref_channel'] == det['ref_channel']
    assert 'acitivity_freq' not in gdet


# ------------------------------------------------------------------ 2. weights reach the model
@pytest.mark.parametrize('D,T,F,K,iters,post', SHAPES)
def test_weighted_activity_through_the_gss_block(gpu_ctx, D, T, F, K, iters, post):
    """GSS.__call__ with a float activity: the weights are the initial affiliations, as in the
    reference (core.py:156-159) -- it used to binarise them.  1e-7: the bar of
    test_cacgmm_matches_oracle (the oracle moves by at most 7e-11 on these shapes when
    observation and initialisation change in the last bit)."""
    from pb_chime5_amd.core import GSS
    rng, Y, act = _scene_of(D, T, F, K)
    w = act * rng.uniform(0.05, 1.0, size=act.shape)
    got = GSS(iterations=iters, iterations_post=post)(Y, w)
    want = oracle.gss_block_batched(Y, w, iters, post)
    binarised = oracle.gss_block_batched(Y, w != 0, iters, post)
    err, gap = np.max(np.abs(got - want)), np.max(np.abs(binarised - want))
    print(f'D={D} T={T} K={K}: vs oracle {err:.1e}; weighted vs binarised oracle {gap:.1e}')
    assert got.shape == want.shape == (K, T, F)
    # the case tells a weighted from a binarised run: the gap is orders above the tolerance
    assert gap > 1e-3
    assert err < 1e-7
    assert np.max(np.abs(got.sum(axis=0) - 1)) < 1e-12 or post == 0


# ------------------------------------------------------------------ 3. per-frequency guidance
@pytest.mark.parametrize('D,T,F,K,iters,post', SHAPES)
def test_per_frequency_mask_and_initialisation(gpu_ctx, D, T, F, K, iters, post):
    from pb_chime5_amd import ops
    rng, Y, act = _scene_of(D, T, F, K)
    init, mask = _per_frequency_guidance(rng, act, F)
    got = ops.cacgmm_posteriors_guided(Y, init.transpose(1, 2, 0), mask.transpose(1, 2, 0),
                                       iters, post, ctx=gpu_ctx)
    want = _oracle_guided(Y, init, mask, iters, post)
    err = np.max(np.abs(got - want))
    print(f'D={D} T={T} K={K} post={post}: per-frequency guidance vs oracle {err:.1e}')
    assert got.shape == want.shape == (K, T, F)
    assert err < 1e-7
    if post == 0:
        assert np.all(got[~mask.transpose(1, 2, 0)] == 0)
    else:
        assert np.max(np.abs(got.sum(axis=0) - 1)) < 1e-12


@pytest.mark.parametrize('D,T,F,K,iters,post', SHAPES)
def test_per_frequency_initialisation_without_a_mask(gpu_ctx, D, T, F, K, iters, post):
    """fit(y, initialization, source_activity_mask=None) + unmasked predict (post >= 1)."""
    from pb_chime5_amd import ops
    post = max(post, 1)
    rng, Y, act = _scene_of(D, T, F, K)
    init, _ = _per_frequency_guidance(rng, act, F)
    got = ops.cacgmm_posteriors_guided(Y, init.transpose(1, 2, 0), None, iters, post, ctx=gpu_ctx)
    want = _oracle_guided(Y, init, None, iters, post)
    err = np.max(np.abs(got - want))
    print(f'D={D} T={T} K={K} post={post}: unmasked fit vs oracle {err:.1e}')
    assert err < 1e-7
    assert np.max(np.abs(got.sum(axis=0) - 1)) < 1e-12


@pytest.mark.parametrize('streams', [1, 2])
def test_per_frequency_guidance_over_blocks_of_frequencies(gpu_ctx, monkeypatch, streams):
    """The frequency-blocked EM (forced as in test_cacgmm_over_blocks_of_frequencies): every
    block reads its own rows of a per-frequency mask and initialisation."""
    from pb_chime5_amd import ops
    D, T, F, K, iters, post = 12, 333, 45, 5, 6, 0
    rng = np.random.default_rng(D + T + F)
    Y, act = _scene(rng, D, T, F, K)
    init, mask = _per_frequency_guidance(rng, act, F)
    # every frequency its own mask: class 1 off on a stretch that moves with f
    for f in range(F):
        mask[f, 1, 3 * f:3 * f + 40] = False
    args = (Y, init.transpose(1, 2, 0), mask.transpose(1, 2, 0), iters, post)
    whole = ops.cacgmm_posteriors_guided(*args, ctx=gpu_ctx)
    per_f_mb = (16 * D + 8 * K) * T / 2 ** 20
    for fb in (8, 16):
        mb = int(np.ceil(per_f_mb * fb * streams))
        monkeypatch.setenv('GSS_VARIANT', f'em_l3_fit_mb=0,em_l3_mb={max(mb, 1)},em_streams={streams}')
        blocked = ops.cacgmm_posteriors_guided(*args, ctx=gpu_ctx)
        monkeypatch.delenv('GSS_VARIANT')
        assert np.max(np.abs(blocked - whole)) < 1e-9, (fb, np.max(np.abs(blocked - whole)))
        assert np.all(blocked[~mask.transpose(1, 2, 0)] == 0)
    assert np.max(np.abs(blocked - _oracle_guided(Y, init, mask, iters, post))) < 1e-7


# ------------------------------------------------------------------ 4. explicit initialisation
@pytest.mark.parametrize('D,T,F,K,iters,post', SHAPES)
def test_explicit_initialisation_of_the_activity_gives_the_unweighted_posteriors(
        gpu_ctx, D, T, F, K, iters, post):
    from pb_chime5_amd import ops
    _, Y, act = _scene_of(D, T, F, K)
    init, mask = ops.guidance_from_activity(act)
    want = ops.cacgmm_posteriors(Y, act, iters, post, ctx=gpu_ctx)
    got = ops.cacgmm_posteriors_guided(Y, np.repeat(init[..., None], F, axis=-1), mask, iters, post,
                                       ctx=gpu_ctx)
    err = np.max(np.abs(got - want))
    print(f'D={D} T={T} K={K}: explicit initialisation vs the unweighted call {err:.1e}')
    assert err <= 1e-12


# ------------------------------------------------------------------ 5. fused
@pytest.mark.parametrize('D', [4, 24])
def test_fused_guided_pipeline_with_weights(gpu_ctx, D):
    """Enhancer.enhance_observation_guided with weighted frame guidance against the oracle's
    stft -> wpe_block -> CACGMM from the weighted initialisation -> masks -> MVDR + BAN ->
    istft; the block path agrees with the fused one; the taps hold the guided posteriors."""
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import get_enhancer
    u, kw = _tiny(D)
    T = ops.stft_frames(u.obs.shape[1], 1024, 256, True)
    rng = np.random.default_rng(D)
    actf = _frame_activity(u, T)
    guidance = {spk: a * rng.uniform(0.05, 1.0, size=T) for spk, a in zip(u.activity, actf)}
    w = np.array(list(guidance.values()))

    def gss_fn(Obs, activity_freq, iterations, iterations_post):
        init, mask = oracle.gss_initialization(w)
        return _oracle_guided(Obs, init[None], mask[None], iterations, iterations_post)
    want, wdet = oracle.enhance_observation(u.obs, u.activity_array, u.target_index, u.ex,
                                            return_details=True, gss_fn=gss_fn, **kw)
    plain = oracle.enhance_observation(u.obs, u.activity_array, u.target_index, u.ex,
                                       gss_fn=oracle.gss_block_batched, **kw)

    enh = get_enhancer(wpe_tabs=kw['wpe_taps'], wpe_iterations=kw['wpe_iterations'],
                       bss_iterations=kw['bss_iterations'])
    assert enh._fusable()
    got = enh.enhance_observation_guided(u.obs, guidance, u.speaker_id, ex=u.ex, debug=True)
    loc = enh.enhance_observation_locals
    assert got.shape == want.shape
    err = rel_err(np.abs(loc['X_hat']), np.abs(wdet['X_hat']))
    print(f'D={D}: |X_hat| rel err {err:.1e}, x_hat {rel_err(got, want):.1e}; weighted vs '
          f'unweighted oracle {rel_err(plain, want):.1e}')
    assert err <= 1e-4
    assert loc['details']['ref_channel'] == wdet['ref_channel']
    assert rel_err(plain, want) > 1e-3          # the weights matter in this scene
    # the taps hold the guided posteriors: those of the stage call on the tapped observation
    init, mask = ops.guidance_from_activity(w)
    stage = ops.cacgmm_posteriors_guided(loc['Obs'], init, mask, kw['bss_iterations'], 1, ctx=gpu_ctx)
    assert np.array_equal(loc['details']['posterior'], stage)
    ref = gss_fn(wdet['Obs'], None, kw['bss_iterations'], 1)
    assert np.max(np.abs(loc['details']['posterior'] - ref)) < 1e-4
    assert 'acitivity_freq' not in loc['details']

    blocks = enh.enhance_observation_guided(u.obs, guidance, u.speaker_id, ex=u.ex, fused=False,
                                            debug=True)
    print(f'D={D}: block path vs fused {rel_err(blocks, got):.1e}')
    assert rel_err(blocks, got) < 1e-10
    assert np.array_equal(enh.gss_block.locals['initialization'], init)
    assert np.array_equal(enh.gss_block.locals['source_active_mask'], mask)


def test_fused_guided_pipeline_with_a_per_frequency_initialisation(gpu_ctx):
    """A (T,F) initialisation per speaker (what a neural mask estimator gives) and the (T,)
    activity as the mask, fused against the blocks."""
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import get_enhancer
    u, kw = _tiny(4)
    T = ops.stft_frames(u.obs.shape[1], 1024, 256, True)
    rng = np.random.default_rng(11)
    actf = _frame_activity(u, T)
    guidance = dict(zip(u.activity, actf))
    init = rng.uniform(0.01, 1.0, size=(len(guidance), T, 513)) * np.where(actf, 1.0, 1e-10)[..., None]
    init /= init.sum(axis=0, keepdims=True)
    initialization = dict(zip(u.activity, init))
    enh = get_enhancer(wpe_tabs=kw['wpe_taps'], wpe_iterations=kw['wpe_iterations'],
                       bss_iterations=kw['bss_iterations'])
    fused = enh.enhance_observation_guided(u.obs, guidance, u.speaker_id, ex=u.ex,
                                           initialization=initialization, debug=True)
    loc = enh.enhance_observation_locals
    want = _oracle_guided(loc['Obs'], init.transpose(2, 0, 1),
                          np.repeat(actf[None], 513, axis=0), kw['bss_iterations'], 1)
    assert np.max(np.abs(loc['details']['posterior'] - want)) < 1e-7
    blocks = enh.enhance_observation_guided(u.obs, guidance, u.speaker_id, ex=u.ex,
                                            initialization=initialization, fused=False)
    assert rel_err(blocks, fused) < 1e-10
    plain = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex)
    assert rel_err(plain, fused) > 1e-6


# ------------------------------------------------------------------ 6. strides and errors
def _raw_guided(ctx, Y, K, iters, post, init=None, init_strides=(0, 0), mask=None,
                mask_strides=(0, 0), descriptor=True):
    """gss_cacgmm_guided on flat host tables with explicit (f, k) strides -> gamma (F,K,T)."""
    from pb_chime5_amd import _capi, ops
    Y_d, (D, T, F) = ops._obs_to_device_ftd(ctx, Y)
    init_d = ctx.to_device(np.ascontiguousarray(init, np.float64)) if init is not None else None
    mask_d = ctx.to_device(np.ascontiguousarray(mask, np.uint8)) if mask is not None else None
    g = _capi.GssGuidance(init_dev=init_d.ptr if init_d else None,
                          mask_dev=mask_d.ptr if mask_d else None,
                          init_f_stride=init_strides[0], init_k_stride=init_strides[1],
                          mask_f_stride=mask_strides[0], mask_k_stride=mask_strides[1])
    g_d = ctx.empty(8 * F * K * T)
    ctx._check(ctx.lib.gss_cacgmm_guided(
        ctx.handle, _capi.c_void_p(Y_d.ptr), F, T, D, ctypes.byref(g) if descriptor else None, K,
        iters, post, _capi.c_void_p(g_d.ptr)), 'gss_cacgmm_guided')
    return ctx.to_host(g_d, (F, K, T), np.float64)


@pytest.mark.parametrize('D,T,F,K', [(4, 300, 5, 3), (24, 200, 4, 5), (7, 130, 4, 4)])
def test_strided_tables_equal_their_contiguous_forms(gpu_ctx, D, T, F, K):
    rng, Y, act = _scene_of(D, T, F, K)
    init, mask = _per_frequency_guidance(rng, act, F)
    mask8 = mask.astype(np.uint8)
    want = _raw_guided(gpu_ctx, Y, K, 4, 0, init, (K * T, T), mask8, (K * T, T))
    # rows padded to a k stride > T (the padding holds what must not be read: NaN / 1)
    ks = T + 13
    init_p = np.full((F, K, ks), np.nan)
    init_p[..., :T] = init
    mask_p = np.ones((F, K, ks), np.uint8)
    mask_p[..., :T] = mask8
    got = _raw_guided(gpu_ctx, Y, K, 4, 0, init_p, (K * ks, ks), mask_p, (K * ks, ks))
    assert np.array_equal(got, want)
    # ... and frequencies padded too
    fs = K * ks + 7
    init_q = np.full((F, fs), np.nan)
    init_q[:, :K * ks] = init_p.reshape(F, -1)
    mask_q = np.ones((F, fs), np.uint8)
    mask_q[:, :K * ks] = mask_p.reshape(F, -1)
    got = _raw_guided(gpu_ctx, Y, K, 4, 0, init_q, (fs, ks), mask_q, (fs, ks))
    assert np.array_equal(got, want)
    # one (K,T) table with f stride 0 = the table repeated for every frequency
    rep = _raw_guided(gpu_ctx, Y, K, 4, 0, np.repeat(init[:1], F, axis=0), (K * T, T),
                      np.repeat(mask8[:1], F, axis=0), (K * T, T))
    one = _raw_guided(gpu_ctx, Y, K, 4, 0, init[0], (0, T), mask8[0], (0, T))
    assert np.array_equal(one, rep)
    assert not np.array_equal(one, want)


def test_guidance_errors_name_the_argument_and_leave_the_context_usable(gpu_ctx):
    D, T, F, K = 4, 200, 3, 3
    rng, Y, act = _scene_of(D, T, F, K)
    init, mask = _per_frequency_guidance(rng, act, F)
    mask8 = mask.astype(np.uint8)
    good = dict(init=init, init_strides=(K * T, T), mask=mask8, mask_strides=(K * T, T))
    want = _raw_guided(gpu_ctx, Y, K, 3, 1, **good)
    cases = [
        (dict(good, descriptor=False), 'guidance is NULL'),
        (dict(), 'init_dev and mask_dev are both NULL'),
        (dict(good, init_strides=(K * T - 1, T)), 'init_f_stride'),
        (dict(good, mask_strides=(K * T - 1, T)), 'mask_f_stride'),
        (dict(good, init_strides=(K * T, T - 1)), 'init_k_stride'),
        (dict(good, mask_strides=(0, T - 1)), 'mask_k_stride'),
        (dict(good, init_strides=(-K * T, T)), 'init_f_stride'),
    ]
    for kwargs, match in cases:
        with pytest.raises(ValueError, match=match):
            _raw_guided(gpu_ctx, Y, K, 3, 1, **kwargs)
        assert np.array_equal(_raw_guided(gpu_ctx, Y, K, 3, 1, **good), want), match
    # the limits of K, D and the iterations are gss_cacgmm's
    with pytest.raises(AssertionError, match='K < 20'):
        _raw_guided(gpu_ctx, Y, 20, 3, 1, **good)
    with pytest.raises(ValueError, match='iterations'):
        _raw_guided(gpu_ctx, Y, K, 0, 1, **good)
    # the strides of a table that is not given are not read
    only_mask = _raw_guided(gpu_ctx, Y, K, 3, 1, mask=mask8, mask_strides=(K * T, T),
                            init_strides=(5, 1))
    assert np.max(np.abs(only_mask.sum(axis=1) - 1)) < 1e-12


def _fused_raw(ctx, params, obs_d, D, N, K, g, out_d, taps=None):
    from pb_chime5_amd import _capi
    return ctx.lib.gss_enhance_observation_guided(
        ctx.handle, ctypes.byref(params), _capi.c_void_p(obs_d.ptr), D, N,
        ctypes.byref(g) if g is not None else None, K, 0, 0, 0, _capi.c_void_p(out_d.ptr),
        ctypes.byref(taps) if taps is not None else None)


def test_fused_guidance_errors(gpu_ctx):
    from pb_chime5_amd import _capi, ops
    D, N, K = 4, 20000, 3
    ctx = gpu_ctx
    params = ops.make_params(wpe_taps=2, bss_iterations=2)
    ops._prepare_windows(ctx, 1024, 256, None)
    T = ops.stft_frames(N, 1024, 256, True)
    rng = np.random.default_rng(1)
    obs_d = ctx.to_device(rng.standard_normal((D, N)))
    mask_d = ctx.to_device(np.ones((K, T), np.uint8))
    out_d = ctx.empty(8 * int(ctx.lib.gss_istft_num_samples(T, 1024, 256, 1)))

    def guidance(**kw):
        return _capi.GssGuidance(**{**dict(mask_dev=mask_d.ptr, mask_k_stride=T), **kw})
    act_tap = ctx.empty(K * T)
    cases = [
        (None, None, 'guidance is NULL'),
        (guidance(mask_dev=None), None, 'both NULL'),
        (guidance(mask_k_stride=T - 1), None, 'mask_k_stride'),
        (guidance(mask_f_stride=K * T - 1), None, 'mask_f_stride'),
        (guidance(init_dev=mask_d.ptr, init_k_stride=T - 1), None, 'init_k_stride'),
        (guidance(init_dev=mask_d.ptr, init_k_stride=T, init_f_stride=1), None, 'init_f_stride'),
        (guidance(), _capi.GssDebugTaps(act_frames=act_tap.ptr), 'act_frames'),
    ]
    for g, taps, match in cases:
        status = _fused_raw(ctx, params, obs_d, D, N, K, g, out_d, taps)
        assert status == _capi.GSS_ERR_INVALID, match
        with pytest.raises(ValueError, match=match):
            ctx._check(status, 'gss_enhance_observation_guided')
        ctx._check(_fused_raw(ctx, params, obs_d, D, N, K, guidance(), out_d),
                   'gss_enhance_observation_guided')
    ctx.synchronize()


# ------------------------------------------------------------------ 7. workspace of a fresh context
def _sweep_frames():
    frames = [int(t) + (int(t) % 64 == 0) for t in np.linspace(100, 4000, 42)]
    assert len(frames) >= 40 and all(t % 64 for t in frames)
    return frames


@pytest.mark.parametrize('D,K', [(4, 4), (24, 5)])
def test_fresh_context_over_a_sweep_of_frames_stage_call(gpu_ctx, D, K):
    """A context that has never grown its arena, for every T: the reserve covers what the
    guided EM allocates (the 1 MiB rounding of a warm arena would hide a short reserve)."""
    from pb_chime5_amd import _capi
    F, frames = 513, _sweep_frames()
    rng = np.random.default_rng(D)
    # one observation and one set of tables for the longest T, in HBM once; shorter calls read
    # the head of them as (F,T,D) / with the strides of the longest
    Tmax = max(frames)
    flat = rng.standard_normal(2 * 513 * 64 * D)
    Y = np.resize(flat, 2 * F * Tmax * D).view(np.complex128)
    Y_d = gpu_ctx.to_device(Y)
    mask = rng.random((F, K, Tmax)) < 0.7
    mask[:, -1] = True
    init = rng.uniform(0.01, 1.0, size=(F, K, Tmax))
    mask_d, init_d = gpu_ctx.to_device(mask.astype(np.uint8)), gpu_ctx.to_device(init)
    g_d = gpu_ctx.empty(8 * F * K * Tmax)
    g = _capi.GssGuidance(init_dev=init_d.ptr, mask_dev=mask_d.ptr, init_f_stride=K * Tmax,
                          init_k_stride=Tmax, mask_f_stride=K * Tmax, mask_k_stride=Tmax)
    for T in frames:
        ctx = _capi.Context(0)
        try:
            status = ctx.lib.gss_cacgmm_guided(ctx.handle, _capi.c_void_p(Y_d.ptr), F, T, D,
                                               ctypes.byref(g), K, 1, 1, _capi.c_void_p(g_d.ptr))
            assert status != _capi.GSS_ERR_NOMEM, (T, ctx.lib.gss_last_error(ctx.handle))
            ctx._check(status, f'gss_cacgmm_guided T={T}')
            ctx.synchronize()
        finally:
            ctx.close()


@pytest.mark.parametrize('D,K,wpe', [(4, 4, True), (4, 4, False), (24, 5, True), (24, 5, False)])
def test_fresh_context_over_a_sweep_of_frames_fused_call(gpu_ctx, D, K, wpe):
    from pb_chime5_amd import _capi, ops
    F = 513
    params = ops.make_params(wpe=wpe, wpe_taps=2, wpe_iterations=1, bss_iterations=1)
    analysis = ops.analysis_window(1024)
    synthesis = ops.synthesis_window(analysis, 256)
    samples = []
    for t in _sweep_frames():
        n = t * 256 - 700
        while ops.stft_frames(n, 1024, 256, True) % 64 == 0:
            n += 256
        samples.append(n)
    Tmax = ops.stft_frames(max(samples), 1024, 256, True)
    rng = np.random.default_rng(D)
    obs_d = gpu_ctx.to_device(rng.standard_normal((D, max(samples))))     # (D,N): its head
    mask = rng.random((F, K, Tmax)) < 0.7
    mask[:, -1] = True
    mask_d = gpu_ctx.to_device(mask.astype(np.uint8))
    init_d = gpu_ctx.to_device(rng.uniform(0.01, 1.0, size=(F, K, Tmax)))
    out_d = gpu_ctx.empty(8 * int(gpu_ctx.lib.gss_istft_num_samples(Tmax, 1024, 256, 1)))
    g = _capi.GssGuidance(init_dev=init_d.ptr, mask_dev=mask_d.ptr, init_f_stride=K * Tmax,
                          init_k_stride=Tmax, mask_f_stride=K * Tmax, mask_k_stride=Tmax)
    for N in samples:
        ctx = _capi.Context(0)
        try:
            ctx.set_windows(1024, 256, analysis, synthesis)
            status = _fused_raw(ctx, params, obs_d, D, N, K, g, out_d)
            assert status != _capi.GSS_ERR_NOMEM, (N, ctx.lib.gss_last_error(ctx.handle))
            ctx._check(status, f'gss_enhance_observation_guided N={N}')
            ctx.synchronize()
        finally:
            ctx.close()
