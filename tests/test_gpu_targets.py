"""Several targets of one window from one separation (gss_enhance_observation_targets,
ops.enhance_observation_targets, Enhancer.enhance_observation_speakers) on the GPU.

The contract is bit identity: row s of a targets call, and each per-target block of its debug
taps, equals the single-target call for target_index[s] with that target's contexts on the same
inputs and params.  test_gpu_pipeline.py holds the single-target call to the oracle for the
target speaker of each scene; test_config2_every_speaker_vs_oracle below does the same for
every speaker of config 2, which no single-target test covers."""
import numpy as np
import pytest

import gss_oracle as oracle
from conftest import rel_err
from pb_chime5_amd import ops, synthetic
from pb_chime5_amd._capi import Context, c_void_p

pytestmark = pytest.mark.gpu

SMALL = dict(wpe=True, wpe_taps=4, bss_iterations=5)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _check_rows(ctx, u, targets, starts, ends, debug=True, obs=None, **kw):
    """One targets call against len(targets) single calls, every row and tap bit for bit."""
    obs = u.obs if obs is None else obs
    act = u.activity_array
    S = len(targets)
    starts = ops.target_contexts(starts, S)
    ends = ops.target_contexts(ends, S)
    res = ops.enhance_observation_targets(obs, act, targets, starts, ends, debug=debug, ctx=ctx,
                                          **kw)
    x, det = res if debug else (res, None)
    assert x.shape[0] == S
    for s, t in enumerate(targets):
        one = ops.enhance_observation(obs, act, t, starts[s], ends[s], debug=debug, ctx=ctx, **kw)
        xs, ds = one if debug else (one, None)
        assert _same(x[s], xs), (s, t)
        if not debug:
            continue
        for key in ('target_mask', 'distortion_mask', 'X_hat'):
            assert _same(det[key][s], ds[key]), (s, t, key)
        assert det['ref_channel'][s] == ds['ref_channel'], (s, t)
        if s == 0:
            for key in ('Obs', 'posterior', 'acitivity_freq'):
                assert _same(det[key], ds[key]), key
    return x, det


@pytest.fixture(scope='module')
def tiny():
    return synthetic.tiny(num_channels=4, num_samples=16000, num_speakers=2, context=2048)


@pytest.mark.parametrize('drop', [True, False])
@pytest.mark.parametrize('targets,starts,ends', [
    ([0], 2048, 2048),
    ([2, 0], [0, 2048], [4096, 1024]),          # the garbage class, permuted
    ([1, 2], 3000, [0, 5000]),                  # K - 1, non-contiguous with the one left out
    ([2, 0, 1], [1000, 0, 2048], [0, 3000, 2048]),   # all K, permuted
])
def test_tiny_rows_are_single_calls(gpu_ctx, tiny, targets, starts, ends, drop):
    _check_rows(gpu_ctx, tiny, targets, starts, ends, bf_drop_context=drop, **SMALL)


@pytest.mark.parametrize('postfilter', [None, 'mask_mul'])
@pytest.mark.parametrize('bf', ['mvdrSouden_ban', 'ch2', 'sum', 'gev_ban'])
@pytest.mark.parametrize('scene', ['tiny', 'config1'])
def test_every_beamformer_and_postfilter(gpu_ctx, tiny, scene, bf, postfilter):
    if scene == 'tiny':
        u, kw = tiny, dict(SMALL)
    else:
        u, kw = synthetic.config1(context=8000), dict(wpe=False, bss_iterations=5)
    _check_rows(gpu_ctx, u, [1, 0, 2], [2048, 0, 4096], [0, 2048, 1024], bf=bf,
                postfilter=postfilter, **kw)


def test_outer_mics_scene_with_per_array_wpe(gpu_ctx):
    """12 channels (6 arrays x the 2 outer microphones), WPE per array."""
    u = synthetic.tiny(seed=3, num_channels=12, num_samples=24000, num_speakers=3, context=4000)
    _check_rows(gpu_ctx, u, [3, 1, 0, 2], 4000, [4000, 0, 2000, 4000], wpe_arrays=6, **SMALL)
    _check_rows(gpu_ctx, u, [2], 0, 0, debug=False, wpe_arrays=6, **SMALL)


@pytest.fixture(scope='module')
def config2():
    return synthetic.config2()


@pytest.mark.parametrize('bf', ['mvdrSouden_ban', 'gev_ban'])
@pytest.mark.parametrize('targets', [[0], [4, 1], [3, 0, 2, 1], [0, 1, 2, 3, 4]])
def test_config2_rows_are_single_calls(gpu_ctx, config2, targets, bf):
    ctx_samples = config2.ex['start_orig']['original']
    debug = len(targets) == 5 and bf == 'mvdrSouden_ban'
    starts = [ctx_samples - 16000 * s for s in range(len(targets))]
    _check_rows(gpu_ctx, config2, targets, starts, ctx_samples, debug=debug, bf=bf)


@pytest.mark.parametrize('targets', [
    [5, 0, 11, 3, 8, 1],                                  # S = 6: the 8-target apply
    [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0],               # S = K = 12: the 19-target apply
])
def test_many_targets(gpu_ctx, targets):
    """K = 12 (11 speakers + Noise): the larger instantiations of mvdr_apply_targets and the
    per-target status words and mask arguments beyond five targets."""
    u = synthetic.tiny(seed=12, num_channels=6, num_samples=24000, num_speakers=11,
                       context=2048, noise=3e-2)
    assert u.activity_array.shape[0] == 12
    starts = [512 * (i % 5) for i in range(len(targets))]
    _check_rows(gpu_ctx, u, targets, starts, 2048, **SMALL)
    _check_rows(gpu_ctx, u, targets, 0, 0, debug=False, bf='gev_ban', **SMALL)
    ops.enhance_observation_targets(u.obs, u.activity_array, targets, 0, 0, ctx=gpu_ctx, **SMALL)
    refs = gpu_ctx.last_ref_channels(len(targets))
    assert len(refs) == len(targets) and min(refs) >= 0 and max(refs) < 6


def test_config2_every_speaker_vs_oracle(gpu_ctx, config2, oracle_pool, ref_mismatches):
    """All four speakers of BASELINE configs[1] (24 ch, 15 s, K = 5) from one targets call,
    against the oracle on all 513 bins, stage by stage as test_gpu_pipeline's
    test_config2_stagewise_vs_oracle_on_frequency_subset does for the target speaker: the
    oracle's WPE once on the STFT (worker pool), its EM once on the GPU's dereverberated tensor,
    its beamformer once per speaker on that tensor with the oracle's own masks.  Each speaker's
    reference channel goes through the tie certification of test_gpu_pipeline (session-wide
    `ref_mismatches`); its enhanced STFT magnitude is held to TOL_STFT_MAG against the oracle's
    beamformer -- on every bin when fed the GPU's masks, and on the bins where the literal
    float64 oracle is meaningful (cond(Phi_N) < 1e8) when fed the oracle's masks."""
    from test_gpu_pipeline import TOL_STFT_MAG, _check_ref_channel_or_tie
    u = config2
    cs = u.ex['start_orig']['original']
    ce = u.ex['end']['original'] - u.ex['end_orig']['original']
    speakers = [0, 1, 2, 3]
    x, det = ops.enhance_observation_targets(u.obs, u.activity_array, speakers, cs, ce,
                                             debug=True, ctx=gpu_ctx)
    T = det['Obs'].shape[1]
    # WPE: the oracle's on the STFT, every bin
    X_want = oracle_pool.wpe_block(oracle.stft(u.obs), 10, 2, 3)
    wpe_err = (np.linalg.norm(det['Obs'] - X_want, axis=(0, 1))
               / np.linalg.norm(X_want, axis=(0, 1)))
    cache = {}

    def gss_once(Obs, act, **kw):      # the oracle's EM, once, on the GPU's tensor
        if 'gss' not in cache:
            cache['gss'] = oracle_pool.gss_block(Obs, act, **kw)
        return cache['gss'].copy()

    for s, k in enumerate(speakers):
        _, wdet = oracle.enhance_observation(u.obs, u.activity_array, k, u.ex,
                                             return_details=True, gss_fn=gss_once,
                                             wpe_fn=lambda *a: det['Obs'].copy())
        if s == 0:
            assert np.array_equal(det['acitivity_freq'], wdet['activity_freq'][:, :T])
            post_err = np.max(np.abs(det['posterior'] - cache['gss']))
            print('config 2 front: WPE per-bin error max %.2e, posteriors max %.2e'
                  % (wpe_err.max(), post_err))
            assert wpe_err.max() < 1e-6
            assert post_err < 1e-4
        one = {key: det[key][s] for key in ('target_mask', 'distortion_mask', 'X_hat')}
        one.update(Obs=det['Obs'], ref_channel=int(det['ref_channel'][s]))
        same = _check_ref_channel_or_tie(gpu_ctx, one, wdet, ('config2 speaker', k),
                                         ref_mismatches)
        # the oracle's beamformer on the GPU's own tensor and masks: every bin
        X_stage, bdet = oracle.beamform_mvdr_souden_from_masks(
            det['Obs'], one['target_mask'], one['distortion_mask'], ban=True,
            return_details=True)
        if bdet['ref_channel'] != one['ref_channel']:
            # (a certified tie above: the oracle's beamformer with the GPU's channel)
            w = oracle.get_mvdr_vector_souden(bdet['cov_x'], bdet['cov_n'],
                                              ref_channel=one['ref_channel'], eps=1e-10)
            X_stage = oracle.apply_beamforming_vector(
                oracle.blind_analytic_normalization(w, bdet['cov_n']),
                det['Obs'].transpose(2, 0, 1)).T
        stage_err = rel_err(np.abs(one['X_hat']), np.abs(X_stage))
        # with the oracle's masks, where the literal oracle is meaningful
        good = np.linalg.cond(wdet['cov_n']) < 1e8
        assert good.any()
        err = rel_err(np.abs(one['X_hat'][:, good]), np.abs(wdet['X_hat'][:, good]))
        print('config 2 speaker %d: ref %d (oracle %d), |X_hat| error %.2e (all bins, GPU masks), '
              '%.2e (%d bins, oracle masks)' % (k, one['ref_channel'], wdet['ref_channel'],
                                                stage_err, err, good.sum()))
        assert stage_err < TOL_STFT_MAG, k
        if same:
            assert err < TOL_STFT_MAG, k
        assert rel_err(x[s], oracle.istft(one['X_hat'])) < 1e-11
        assert np.all(np.isfinite(x[s]))


def test_pcm16_entry_is_the_f64_entry_on_scaled_samples(gpu_ctx, tiny):
    pcm = np.clip(np.round(tiny.obs * 2 ** 15), -2 ** 15, 2 ** 15 - 1).astype(np.int16)
    act = tiny.activity_array
    a = ops.enhance_observation_targets(pcm, act, [2, 1, 0], 2048, 2048, ctx=gpu_ctx, **SMALL)
    b = ops.enhance_observation_targets(pcm.astype(np.float64) / 2 ** 15, act, [2, 1, 0], 2048,
                                        2048, ctx=gpu_ctx, **SMALL)
    assert _same(a, b)


@pytest.mark.parametrize('hint', [0, 1])
def test_utterances_in_flight_hint(gpu_ctx, config2, hint):
    """The hint puts half of the WPE stage on the second stream: the same bits either way."""
    gpu_ctx.set_utterances_in_flight(hint)
    try:
        _check_rows(gpu_ctx, config2, [1, 3], 0, 0, debug=False)
    finally:
        gpu_ctx.set_utterances_in_flight(0)


def test_nan_channel_raises_like_the_single_call_and_context_recovers(gpu_ctx, tiny):
    act = tiny.activity_array
    bad = tiny.obs.copy()
    bad[1, 5000] = np.nan
    with pytest.raises(AssertionError):
        ops.enhance_observation(bad, act, 0, 2048, 2048, ctx=gpu_ctx, **SMALL)
    with pytest.raises(AssertionError, match='P02'):
        ops.enhance_observation_targets(bad, act, [1, 0], 2048, 2048, ctx=gpu_ctx,
                                        target_names=['P02', 'P01'], **SMALL)
    _check_rows(gpu_ctx, tiny, [1, 0], 2048, 2048, debug=False, **SMALL)


def test_gev_failure_of_one_target(gpu_ctx, tiny):
    """A context that covers the whole window leaves target 1 with an all-zero noise mask: its
    noise PSD is not positive definite, the single call raises LinAlgError, so does the targets
    call (naming it), and the other target still gets its output."""
    act = tiny.activity_array
    n = tiny.obs.shape[1]
    kw = dict(SMALL, bf='gev_ban')
    with pytest.raises(np.linalg.LinAlgError):
        ops.enhance_observation(tiny.obs, act, 1, n, 0, ctx=gpu_ctx, **kw)
    with pytest.raises(np.linalg.LinAlgError, match='speaker B'):
        ops.enhance_observation_targets(tiny.obs, act, [0, 1], [2048, n], [2048, 0], ctx=gpu_ctx,
                                        target_names=['speaker A', 'speaker B'], **kw)
    refs = gpu_ctx.last_ref_channels(2)
    assert refs[0] == 0 and refs[1] <= -2
    assert gpu_ctx.last_ref_channel() == refs[0]
    # the other target finished: its row (read without the host's raise) is its single call
    utt = ops.ResidentUtterance(gpu_ctx, tiny.obs, act, ops.make_params(**kw))
    out_d = gpu_ctx.empty(8 * 2 * utt.n_out)
    utt.enqueue_targets([0, 1], [2048, n], [2048, 0], out_d)
    rows = gpu_ctx.to_host(out_d, (2, utt.n_out), np.float64)
    assert gpu_ctx.last_ref_channels(2) == refs
    assert np.all(np.isfinite(rows[0])) and np.all(np.isnan(rows[1]))
    assert _same(rows[0], ops.enhance_observation(tiny.obs, act, 0, 2048, 2048, ctx=gpu_ctx,
                                                  **kw))
    _check_rows(gpu_ctx, tiny, [0, 1], 2048, 2048, debug=False, **kw)


def test_status_words_of_a_call_without_beamformer(gpu_ctx, tiny):
    """A 'ch2' targets call runs no beamformer: afterwards only S = 1 (the word
    gss_last_ref_channel reads) is accepted, not stale words of an earlier call."""
    act = tiny.activity_array
    ops.enhance_observation_targets(tiny.obs, act, [0, 1, 2], 0, 0, ctx=gpu_ctx, **SMALL)
    assert len(gpu_ctx.last_ref_channels(3)) == 3
    ops.enhance_observation_targets(tiny.obs, act, [0, 1, 2], 0, 0, ctx=gpu_ctx, bf='ch2',
                                    **SMALL)
    with pytest.raises(ValueError):
        gpu_ctx.last_ref_channels(2)
    assert gpu_ctx.last_ref_channels(1) == [gpu_ctx.last_ref_channel()]


def test_enhancer_speakers_match_enhance_observation(gpu_ctx, tiny):
    from pb_chime5_amd.core import get_enhancer
    enh = get_enhancer(wpe=True, wpe_tabs=4, bss_iterations=5, context_samples=2048)
    enh.device_id = 0
    out = enh.enhance_observation_speakers(tiny.obs, tiny.activity, ex=tiny.ex)
    assert list(out) == ['P01', 'P02']
    for spk, x in out.items():
        want = enh.enhance_observation(tiny.obs, tiny.activity, spk, ex=tiny.ex)
        assert _same(x, want), spk


# ---------------------------------------------------------------- fresh-context sweeps
def _samples_for_frames(T):
    N = max(256 * (T - 4), 1)
    while ops.stft_frames(N, 1024, 256, True) < T:
        N += 1
    assert ops.stft_frames(N, 1024, 256, True) == T
    return N


def _fresh_scene(rng, D, K, T):
    N = _samples_for_frames(T)
    obs = rng.standard_normal((D, N)) * 0.1
    act = np.zeros((K, N), dtype=bool)
    act[-1] = True
    for k in range(K - 1):
        a = int(rng.integers(0, N // 2))
        act[k, a:a + N // 2] = True
    return obs, act


SWEEP = [(4, 4, T) for T in (300, 451, 700, 999, 1200, 1500, 1777, 2172, 2500, 3000, 3500,
                             4000)] + [(24, 5, T) for T in (300, 1100, 2172, 4000)]


@pytest.mark.parametrize('D,K,T', SWEEP)
def test_fresh_context_sweep_has_enough_workspace(D, K, T):
    """A new context per call sizes its workspace from scratch: every entry that runs the EM
    must reserve what cacgmm_run allocates (the zero-frame tile flags included)."""
    rng = np.random.default_rng(T + 10 * D)
    obs, act = _fresh_scene(rng, D, K, T)
    params = dict(wpe=False, bss_iterations=2)
    F = 513
    # gss_cacgmm on the STFT of the window
    ctx = Context(0)
    try:
        ops._prepare_windows(ctx, 1024, 256)
        x_d = ctx.to_device(obs)
        act_d = ctx.to_device(ops.activity_time_to_frequency_device(act, 1024, 256, True,
                                                                    ctx=ctx).astype(np.uint8))
        Y_d = ctx.empty(16 * F * T * D)
        g_d = ctx.empty(8 * F * K * T)
        ctx._check(ctx.lib.gss_stft(ctx.handle, c_void_p(x_d.ptr), D, obs.shape[1], 1,
                                    c_void_p(Y_d.ptr)), 'gss_stft')
        ctx._check(ctx.lib.gss_cacgmm(ctx.handle, c_void_p(Y_d.ptr), F, T, D, c_void_p(act_d.ptr),
                                      K, 2, 1, c_void_p(g_d.ptr)), 'gss_cacgmm')
        ctx.synchronize()
    finally:
        ctx.close()
    ctx = Context(0)
    try:
        one = ops.enhance_observation(obs, act, 0, 0, 0, ctx=ctx, **params)
    finally:
        ctx.close()
    ctx = Context(0)
    try:
        both = ops.enhance_observation_targets(obs, act, [0, K - 1], 0, 0, ctx=ctx, **params)
    finally:
        ctx.close()
    assert _same(both[0], one)
