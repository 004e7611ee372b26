"""Posterior activity on the GPU (pact_sums / pact_scores behind gss_posterior_activity and
gss_enhance_observation_activity) against tests/posterior_activity_reference.py.

The bar between the device and the NumPy reference is derived there, not measured: every sum is
of non-negative terms, n = 2 F D of them, so any order is within about (n - 1) 2^-53 relative
and |got - want| <= 4 (2 F D + 8) 2^-53 want holds for scores and power."""
import ctypes
import functools

import numpy as np
import pytest

import posterior_activity_reference as ref

pytestmark = pytest.mark.gpu

# (D, T, F, K): one frame; T either side of the 64-frame tile; F below, not a multiple of and
# well above the number of frequency shares; both limits of K and D
SHAPES = [(2, 1, 1, 1), (2, 63, 3, 2), (5, 65, 4, 3), (12, 130, 7, 5), (32, 70, 2, 4),
          (24, 200, 33, 19), (24, 333, 257, 5)]


@functools.lru_cache(maxsize=None)
def _case(D, T, F, K, weighted):
    """Scene Y (F,T,D), gamma (F,K,T), their views for `ops`, the weights and the reference's
    scores and power; computed once and shared (read-only)."""
    Y, gamma = ref.scene(D, T, F, K)
    w = ref.weights(F) if weighted else None
    scores, power = ref.posterior_activity(Y, gamma, w)
    Obs = np.ascontiguousarray(Y.transpose(2, 1, 0))
    post = np.ascontiguousarray(gamma.transpose(1, 2, 0))
    for a in (Y, gamma, Obs, post, scores, power) + (() if w is None else (w,)):
        a.setflags(write=False)
    return Y, gamma, Obs, post, w, scores, power


def _within(got, want, F, D, what):
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want)
    worst = float(np.max(err / np.where(want > 0, want, 1.0)))
    print(f'{what}: worst relative deviation {worst:.2e}, bar {ref.bar(F, D):.2e}')
    assert np.all(err <= ref.bar(F, D) * want), what


def _raw(ctx, Y, gamma, w=None, want_power=True):
    """gss_posterior_activity on host arrays already in the device layouts: Y (F,T,D), gamma
    (F,K,T).  No other library call than copies touches the context."""
    from pb_chime5_amd._capi import c_void_p
    F, T, D = Y.shape
    K = gamma.shape[1]
    Y_d = ctx.to_device(np.ascontiguousarray(Y, dtype=np.complex128))
    g_d = ctx.to_device(np.ascontiguousarray(gamma, dtype=np.float64))
    w_d = ctx.to_device(np.ascontiguousarray(w, dtype=np.float64)) if w is not None else None
    s_d, p_d = ctx.empty(8 * K * T), ctx.empty(8 * T)
    ctx._check(ctx.lib.gss_posterior_activity(
        ctx.handle, c_void_p(Y_d.ptr), c_void_p(g_d.ptr), F, K, T, D,
        c_void_p(w_d.ptr) if w_d is not None else None, c_void_p(s_d.ptr),
        c_void_p(p_d.ptr) if want_power else None), 'gss_posterior_activity')
    scores = ctx.to_host(s_d, (K, T), np.float64)
    return scores, (ctx.to_host(p_d, (T,), np.float64) if want_power else None)


# ------------------------------------------------------------------ 1. stage parity
@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('D,T,F,K', SHAPES)
def test_scores_and_power_match_the_reference(gpu_ctx, D, T, F, K, weighted):
    from pb_chime5_amd import ops
    _, _, Obs, post, w, scores, power = _case(D, T, F, K, weighted)
    got, gotp = ops.posterior_activity(Obs, post, w, return_power=True, ctx=gpu_ctx)
    _within(got, scores, F, D, f'{(D, T, F, K)} scores')
    _within(gotp, power, F, D, f'{(D, T, F, K)} power')
    assert np.all(got >= 0) and np.all(got <= 1 + ref.bar(F, D))
    only = ops.posterior_activity(Obs, post, w, ctx=gpu_ctx)      # power_dev = NULL
    assert only.tobytes() == got.tobytes()


# ------------------------------------------------------------------ 2. exact values
def test_exact_zeros_and_scaling(gpu_ctx):
    from pb_chime5_amd import ops
    D, T, F, K = 5, 65, 4, 3
    Y, gamma, _, _, _, _, _ = _case(D, T, F, K, False)
    Y, gamma = Y.copy(), gamma.copy()
    Y[:, 9, :] = 0                          # a frame that is zero in every channel
    Y[:, 64, :] = 0                         # (and one in the last, ragged tile)
    gamma[:, 1, 20] = 0                     # a class whose posterior is 0 in a frame
    gamma[:, 2, 64] = 0
    Obs = np.ascontiguousarray(Y.transpose(2, 1, 0))
    post = np.ascontiguousarray(gamma.transpose(1, 2, 0))
    scores, power = ops.posterior_activity(Obs, post, return_power=True, ctx=gpu_ctx)
    for t in (9, 64):
        assert power[t] == 0.0 and np.all(scores[:, t] == 0.0) and not np.signbit(power[t])
    assert scores[1, 20] == 0.0 and scores[0, 20] > 0 and power[20] > 0
    assert np.all(np.isfinite(scores)) and np.all(np.isfinite(power))
    want, wantp = ref.posterior_activity(Y, gamma)
    _within(scores, want, F, D, 'zeros: scores')
    _within(power, wantp, F, D, 'zeros: power')

    # all-zero weights: everything exactly 0
    s0, p0 = ops.posterior_activity(Obs, post, np.zeros(F), return_power=True, ctx=gpu_ctx)
    assert not s0.any() and not p0.any()

    # Y * 2^5: the same score bits, power times exactly 2^10
    for w in (None, ref.weights(F)):
        a, pa = ops.posterior_activity(Obs, post, w, return_power=True, ctx=gpu_ctx)
        b, pb = ops.posterior_activity(Obs * 32.0, post, w, return_power=True, ctx=gpu_ctx)
        assert a.tobytes() == b.tobytes()
        assert np.array_equal(pb, pa * 1024.0)


# ------------------------------------------------------------------ 3. the same bits every time
@pytest.mark.parametrize('D,T,F,K', [(12, 130, 7, 5), (24, 333, 257, 5)])
def test_the_same_call_gives_the_same_bits_on_a_warm_and_a_fresh_context(gpu_ctx, D, T, F, K):
    from pb_chime5_amd import _capi
    Y, gamma, _, _, w, _, _ = _case(D, T, F, K, True)
    a, pa = _raw(gpu_ctx, Y, gamma, w)
    b, pb = _raw(gpu_ctx, Y, gamma, w)
    assert a.tobytes() == b.tobytes() and pa.tobytes() == pb.tobytes()
    fresh = _capi.Context(0)
    try:
        c, pc = _raw(fresh, Y, gamma, w)
    finally:
        fresh.close()
    assert a.tobytes() == c.tobytes() and pa.tobytes() == pc.tobytes()


@pytest.mark.parametrize('T', [4097, 20001])
def test_workspace_on_a_fresh_context(T):
    """The arena of a fresh context is reserved from the call's own term alone; at these shapes
    the partial planes (16 resp. 6 shares of 20 x T doubles: 10 and 18 MiB) are far more than the
    1 MiB the reserve is rounded up to, so a missing term is GSS_ERR_NOMEM (MemoryError) here."""
    from pb_chime5_amd import _capi
    D, F, K = 2, 16, 19
    Y, gamma, _, _, _, scores, power = _case(D, T, F, K, False)
    ctx = _capi.Context(0)
    try:
        assert ctx.workspace_bytes() == 0
        got, gotp = _raw(ctx, Y, gamma)
        assert ctx.workspace_bytes() >= 8 * 4 * (K + 1) * T
    finally:
        ctx.close()
    _within(got, scores, F, D, f'T={T} scores')
    _within(gotp, power, F, D, f'T={T} power')


# ------------------------------------------------------------------ 4. the fused call
def _utterance(D):
    from pb_chime5_amd import synthetic
    if D == 4:
        return synthetic.tiny(seed=5, num_channels=4, num_samples=24000, num_speakers=3,
                              context=2048), dict(wpe_taps=4, wpe_iterations=3, bss_iterations=6)
    return synthetic.tiny(seed=6, num_channels=D, num_samples=32000, num_speakers=3, context=4096,
                          noise=3e-2), dict(wpe_taps=2, wpe_iterations=2, bss_iterations=6)


def _contexts(u):
    return (u.ex['start_orig']['original'] - u.ex['start']['original'],
            u.ex['end']['original'] - u.ex['end_orig']['original'])


DETAILS = ('Obs', 'acitivity_freq', 'posterior', 'target_mask', 'distortion_mask', 'X_hat',
           'ref_channel')


@pytest.mark.parametrize('D', [4, 12])
def test_fused_call_is_the_plain_call_plus_the_stage_bit_for_bit(gpu_ctx, D):
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import get_enhancer
    u, kw = _utterance(D)
    cs, ce = _contexts(u)
    args = (u.obs, u.activity_array, u.target_index, cs, ce)
    x, det = ops.enhance_observation(*args, debug=True, ctx=gpu_ctx, **kw)
    w = ref.weights(513)
    for weights in (None, w):
        xa, scores, power, adet = ops.enhance_observation_activity(
            *args, freq_weights=weights, debug=True, ctx=gpu_ctx, **kw)
        assert xa.tobytes() == x.tobytes()
        for key in DETAILS:
            assert np.array_equal(adet[key], det[key]), key
        # the stage on the tapped Obs_ftd and gamma
        s, p = ops.posterior_activity(det['Obs'], det['posterior'], weights, return_power=True,
                                      ctx=gpu_ctx)
        assert scores.tobytes() == s.tobytes() and power.tobytes() == p.tobytes()
        xb, sb, pb = ops.enhance_observation_activity(*args, freq_weights=weights, ctx=gpu_ctx,
                                                      **kw)
        assert (xb.tobytes(), sb.tobytes(), pb.tobytes()) == \
            (x.tobytes(), scores.tobytes(), power.tobytes())
    K, T = det['posterior'].shape[:2]
    assert scores.shape == (K, T) and power.shape == (T,)
    total = np.sum(ops.posterior_activity(det['Obs'], det['posterior'], ctx=gpu_ctx), axis=0)
    assert np.max(np.abs(total - 1)) < 1e-9                     # normalised posteriors

    # the Enhancer: the fused path is that call, the block path the stage on the blocks
    enh = get_enhancer(wpe_tabs=kw['wpe_taps'], wpe_iterations=kw['wpe_iterations'],
                       bss_iterations=kw['bss_iterations'])
    assert enh._fusable()
    xe, act = enh.enhance_observation_activity(u.obs, u.activity, u.speaker_id, ex=u.ex,
                                               freq_weights=w)
    assert xe.tobytes() == x.tobytes()
    assert act.scores.tobytes() == scores.tobytes() and act.power.tobytes() == power.tobytes()
    assert act.keys == tuple(u.activity) and act.target_index == u.target_index
    assert (act.start_context_frames, act.end_context_frames) == tuple(
        ops.samples_to_stft_frames(c, 1024, 256, fading=True) for c in (cs, ce))


@pytest.mark.parametrize('D', [4, 12])
def test_block_path_reports_the_same_within_the_bar(gpu_ctx, D):
    """fused=False: `ops.posterior_activity` on the blocks' Obs and posterior, against the fused
    call; the bar of the stage parity."""
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import get_enhancer
    u, kw = _utterance(D)
    cs, ce = _contexts(u)
    w = ref.weights(513)
    _, scores, power = ops.enhance_observation_activity(
        u.obs, u.activity_array, u.target_index, cs, ce, freq_weights=w, ctx=gpu_ctx, **kw)
    enh = get_enhancer(wpe_tabs=kw['wpe_taps'], wpe_iterations=kw['wpe_iterations'],
                       bss_iterations=kw['bss_iterations'])
    xp = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, fused=False)
    xk, blocks = enh.enhance_observation_activity(u.obs, u.activity, u.speaker_id, ex=u.ex,
                                                  freq_weights=w, fused=False)
    assert xk.tobytes() == xp.tobytes()
    assert blocks.keys == tuple(u.activity) and blocks.target_index == u.target_index
    _within(blocks.scores, scores, 513, D, f'D={D} block path: scores')
    _within(blocks.power, power, 513, D, f'D={D} block path: power')


# ------------------------------------------------------------------ 5. it tracks the truth
def test_scores_track_the_truth(gpu_ctx):
    """The target is annotated over 1.5 s but speaks only in the first half of it.  On the CPU
    (oracle posteriors, NumPy reference: test_posterior_activity_api.py) its mean score is 0.67
    over the spoken frames and 0.003 over the silent annotated ones.  Ordering only."""
    from pb_chime5_amd import ops
    u, spoken, silent = ref.truth_scene(4)
    _, scores, power = ops.enhance_observation_activity(
        u.obs, u.activity_array, u.target_index, 0, 0, ctx=gpu_ctx, **ref.TRUTH_PARAMS)
    assert scores.shape == (3, len(spoken))
    a, b = scores[0, spoken].mean(), scores[0, silent].mean()
    print(f'target: mean score {a:.4f} over the spoken frames, {b:.4f} over the silent annotated')
    assert a > b


# ------------------------------------------------------------------ 6. errors through the ABI
def test_abi_errors_name_the_argument_and_leave_the_context_usable(gpu_ctx):
    from pb_chime5_amd import ops
    from pb_chime5_amd._capi import c_void_p
    ctx, lib = gpu_ctx, gpu_ctx.lib
    D, T, F, K = 5, 65, 4, 3
    Y, gamma, _, _, _, scores, _ = _case(D, T, F, K, False)
    # (every buffer has room for the largest sizes named below, should a check ever let one
    # through: 33 channels, 20 classes)
    Y_d, g_d = ctx.empty(16 * F * T * 33), ctx.empty(8 * F * 20 * T)
    ctx.upload(Y_d, Y)
    ctx.upload(g_d, gamma)
    s_d, p_d = ctx.empty(8 * 20 * T), ctx.empty(8 * T)

    def stage(Y=Y_d.ptr, gamma=g_d.ptr, F=F, K=K, T=T, D=D, scores=s_d.ptr):
        ctx._check(lib.gss_posterior_activity(
            ctx.handle, c_void_p(Y), c_void_p(gamma), F, K, T, D, None, c_void_p(scores),
            c_void_p(p_d.ptr)), 'gss_posterior_activity')

    for bad, name in ((dict(Y=None), 'Y_dev'), (dict(gamma=None), 'gamma_dev'),
                      (dict(scores=None), 'scores_dev'), (dict(K=20), 'K=20'), (dict(K=0), 'K=0'),
                      (dict(D=33), 'D=33'), (dict(D=0), 'D=0'), (dict(F=0), 'F=0'),
                      (dict(T=0), 'T=0'), (dict(T=-1), 'T=-1')):
        with pytest.raises(ValueError, match=name):
            stage(**bad)
    stage()
    _within(ctx.to_host(s_d, (K, T), np.float64), scores, F, D, 'after the errors')

    u, kw = _utterance(4)
    cs, ce = _contexts(u)
    p = ops.make_params(**kw)
    ops._prepare_windows(ctx, p.stft_size, p.stft_shift)
    utt = ops.ResidentUtterance(ctx, u.obs, u.activity_array, p)
    fs_d, fp_d = ctx.empty(8 * 20 * utt.T), ctx.empty(8 * utt.T)

    def fused(params=p, obs=utt.obs_d.ptr, act=utt.act_d.ptr, out=utt.out_d.ptr, scores=fs_d.ptr,
              K=utt.K, D=utt.D, N=utt.N):
        ctx._check(lib.gss_enhance_observation_activity(
            ctx.handle, ctypes.byref(params) if params is not None else None, c_void_p(obs), D, N,
            c_void_p(act), K, utt.N_act, u.target_index, cs, ce, None, c_void_p(out),
            c_void_p(scores), c_void_p(fp_d.ptr), None), 'gss_enhance_observation_activity')

    for bad, name in ((dict(params=None), 'params'), (dict(obs=None), 'obs_dev'),
                      (dict(act=None), 'act_dev'), (dict(out=None), 'out_dev'),
                      (dict(scores=None), 'scores_dev'), (dict(K=20), 'K=20'), (dict(K=0), 'K=0'),
                      (dict(D=33), 'D=33'), (dict(D=0), 'D=0'), (dict(N=0), 'N=0')):
        with pytest.raises(ValueError, match=name):
            fused(**bad)
    fused()
    x = utt.result()
    want = ops.enhance_observation(u.obs, u.activity_array, u.target_index, cs, ce, ctx=ctx, **kw)
    assert x.tobytes() == want.tobytes()


# ------------------------------------------------------------------ 7. the profile names them
def test_profile_report_lists_the_two_kernels(gpu_ctx):
    from pb_chime5_amd import ops
    _, _, Obs, post, _, _, _ = _case(12, 130, 7, 5, False)
    gpu_ctx.profile_reset()
    gpu_ctx.profile_enable(True)
    try:
        ops.posterior_activity(Obs, post, ctx=gpu_ctx)
        report = gpu_ctx.profile_report()
    finally:
        gpu_ctx.profile_enable(False)
        gpu_ctx.profile_reset()
    assert report['pact_sums']['calls'] == 1 and report['pact_scores']['calls'] == 1
