"""Per-array WPE (gss_params.wpe_arrays = A > 1, get_enhancer(wpe_per_array=True)) on the GPU:
the stage (gss_wpe_arrays) against the per-array wpe_v8 of the device and of the oracle, the
fused pipeline against the oracle with a per-array WPE, the block path, A = 1, and the session
driver.  Semantics: the reference's WPE.__call__(Obs, stack=False) (core.py:71-79) on the
morph('ACN->A*CN') channel order of enhance_example -- array a is channels a C ... a C + C - 1."""
import numpy as np
import pytest

import gss_oracle as oracle
from conftest import rel_err
from test_chime5_frontdoor import _enhancer, corpus_dev, fixture_dev  # noqa: F401 (fixtures)
from test_gpu_pipeline import TOL_STFT_MAG, _beamformer_all_bins_with_referee
from test_gpu_stages import _reverberant

pytestmark = pytest.mark.gpu


def _oracle_per_array(wpe_block, A):
    """``wpe_fn`` for oracle.enhance_observation: wpe_block on each array's channels."""
    def wpe_fn(Obs, taps, delay, iterations, psd_context):
        C = Obs.shape[0] // A
        return np.concatenate([wpe_block(Obs[a * C:(a + 1) * C], taps, delay, iterations,
                                         psd_context) for a in range(A)])
    return wpe_fn


def _contexts(u):
    return u.ex['start_orig']['original'], u.ex['end']['original'] - u.ex['end_orig']['original']


# ---------------------------------------------------------------- stage
@pytest.mark.parametrize('psd_context', [0, 2])
@pytest.mark.parametrize('C', [1, 2, 4])
@pytest.mark.parametrize('A', [2, 6])
def test_stage_is_wpe_v8_per_array_bit_for_bit(gpu_ctx, A, C, psd_context):
    """gss_wpe_arrays on (F, T, A C) = ops.wpe_v8 on the (A, F, C, T) view, bit for bit (the
    same per-bin arithmetic on the same bins, only their order differs), and within the WPE
    stage tolerance of the oracle's wpe_v8 applied to each array."""
    from pb_chime5_amd import ops
    rng = np.random.default_rng(100 * A + 10 * C + psd_context)
    D, T, F, taps, delay, iters = A * C, 347, 9, 5, 2, 3
    Y = _reverberant(rng, D, T, F)
    got = ops.wpe_arrays_dtf(Y, A, taps, delay, iters, psd_context, ctx=gpu_ctx)
    assert got.shape == (D, T, F)
    assert gpu_ctx.last_wpe_zero_pivots() == 0
    view = Y.reshape(A, C, T, F).transpose(0, 3, 1, 2)                       # (A, F, C, T)
    want = ops.wpe_v8(view, taps, delay, iters, psd_context, ctx=gpu_ctx)
    want = want.transpose(0, 2, 3, 1).reshape(D, T, F)
    assert np.array_equal(got.view(np.float64), want.view(np.float64))
    ref = _oracle_per_array(oracle.wpe_block, A)(Y, taps, delay, iters, psd_context)
    err = rel_err(got, ref)
    print(f'per-array WPE A={A} C={C} psd_context={psd_context}: {err:.2e} against the oracle')
    assert err < 1e-7       # (the stage bound of test_config2_stagewise_vs_oracle_on_...)
    # the arrays really are independent: the joint WPE is something else
    joint = ops.wpe_dtf(Y, taps, delay, iters, psd_context, ctx=gpu_ctx)
    assert rel_err(joint, got) > 1e-6


def test_stage_one_array_and_no_iterations(gpu_ctx):
    """A = 1 is gss_wpe itself (bit for bit); iterations = 0 hands the input back."""
    from pb_chime5_amd import ops
    rng = np.random.default_rng(5)
    Y = _reverberant(rng, 6, 200, 5)
    assert np.array_equal(ops.wpe_arrays_dtf(Y, 1, 4, 2, 2, ctx=gpu_ctx),
                          ops.wpe_dtf(Y, 4, 2, 2, ctx=gpu_ctx))
    assert np.array_equal(ops.wpe_arrays_dtf(Y, 3, 4, 2, 0, ctx=gpu_ctx), Y)


def test_wpe_block_stack_false_is_one_device_call(gpu_ctx, monkeypatch):
    """WPE.__call__(Obs4, stack=False): one gss_wpe_arrays call instead of a loop over arrays."""
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import WPE
    rng = np.random.default_rng(9)
    Obs = _reverberant(rng, 8, 260, 6).reshape(2, 4, 260, 6)
    calls = []
    real = ops.wpe_arrays_dtf
    monkeypatch.setattr(ops, 'wpe_dtf', lambda *a, **k: calls.append('wpe_dtf'))
    monkeypatch.setattr(ops, 'wpe_arrays_dtf',
                        lambda *a, **k: calls.append('wpe_arrays_dtf') or real(*a, **k))
    got = WPE(taps=3, delay=2, iterations=2, psd_context=0)(Obs, stack=False)
    assert calls == ['wpe_arrays_dtf'] and got.shape == Obs.shape
    want = np.array([oracle.wpe_block(o, 3, 2, 2) for o in Obs])
    assert np.max(np.abs(got - want)) / np.max(np.abs(Obs)) < 1e-9


# ---------------------------------------------------------------- pipeline
def test_config2_per_array_end_to_end_vs_oracle(gpu_ctx, oracle_pool):
    """The bench scene (BASELINE configs[1], 6 arrays x 4 channels, all 513 bins) with WPE per
    array, against the oracle with wpe_block per array, held to the per-bin rules of
    test_gpu_pipeline.py::test_config2_end_to_end_vs_oracle; prints the WPE stage's
    GPU - oracle / oracle self-noise ratio (joint WPE: median 1.98)."""
    from pb_chime5_amd import ops, synthetic
    u = synthetic.config2()
    cs = u.ex['start_orig']['original']
    x_hat, det = ops.enhance_observation(u.obs, u.activity_array, u.target_index, cs, cs,
                                         debug=True, ctx=gpu_ctx, wpe_arrays=6)
    kw = dict(return_details=True, gss_fn=oracle_pool.gss_block,
              wpe_fn=_oracle_per_array(oracle_pool.wpe_block, 6))
    want, wdet = oracle.enhance_observation(u.obs, u.activity_array, u.target_index, u.ex, **kw)
    assert rel_err(det['Obs'], wdet['Obs']) < 1e-6
    assert det['ref_channel'] == wdet['ref_channel']
    glob = rel_err(np.abs(det['X_hat']), np.abs(wdet['X_hat']))
    print('config 2 per-array: global |X_hat| error %.2e, x_hat %.2e, after WPE %.2e'
          % (glob, rel_err(x_hat, want), rel_err(det['Obs'], wdet['Obs'])))
    assert glob < 3e-5
    assert rel_err(x_hat, want) < 3e-5
    rng = np.random.default_rng(0)
    obs2 = u.obs * (1 + 2e-16 * rng.standard_normal(u.obs.shape))
    _, wdet2 = oracle.enhance_observation(obs2, u.activity_array, u.target_index, u.ex, **kw)
    A, B, B2 = np.abs(det['X_hat']), np.abs(wdet['X_hat']), np.abs(wdet2['X_hat'])
    nb = np.linalg.norm(B, axis=0)
    loud = nb ** 2 > np.max(nb ** 2) * 1e-8
    err = np.linalg.norm(A - B, axis=0) / nb
    self_f = np.linalg.norm(B2 - B, axis=0) / nb
    tol = np.maximum(TOL_STFT_MAG, 10.0 * self_f)
    relaxed = loud & (err >= TOL_STFT_MAG)
    print('config 2 per-array per-bin |X_hat| error: median %.2e, max %.2e; %d of %d bins above 1e-4'
          % (np.median(err[loud]), err[loud].max(), int((err[loud] > TOL_STFT_MAG).sum()),
             int(loud.sum())))
    assert loud.all()
    assert np.all(err[loud] < tol[loud]), np.flatnonzero(loud & (err >= tol))
    assert relaxed.sum() <= 2 and err[loud].max() < 1e-3
    wpe_err = np.linalg.norm(det['Obs'] - wdet['Obs'], axis=(0, 1))
    wpe_self = np.linalg.norm(wdet2['Obs'] - wdet['Obs'], axis=(0, 1))
    ratio = wpe_err / np.maximum(wpe_self, 1e-300)
    print('per-array WPE output, GPU - oracle over oracle self-noise per bin: median %.2f, '
          'max %.2f (bin %d)' % (np.median(ratio), ratio.max(), int(np.argmax(ratio))))
    assert np.median(ratio) < 3.0 and ratio.max() < 5.0


def test_config5_outer_mics_per_array_gev_all_bins(gpu_ctx, oracle_pool):
    """BASELINE configs[4] (120 s, 6 arrays x 2 outer microphones, 40 EM iterations, GEV + BAN,
    T = 7503) with WPE per array, every bin, judged by the rules of
    test_gpu_pipeline.py::_scene_all_bins (WPE and posteriors per bin; the beamformer against
    the literal oracle where cond(Phi_N) < 1e8, through the extended-precision referee beyond)."""
    from pb_chime5_amd import ops, synthetic
    u = synthetic.config5()
    cs, ce = _contexts(u)
    x_hat, det = ops.enhance_observation(u.obs, u.activity_array, u.target_index, cs, ce,
                                         debug=True, ctx=gpu_ctx, bf='gev_ban',
                                         bss_iterations=40, wpe_arrays=6)
    assert det['Obs'].shape == (12, 7503, 513)
    _, wdet = oracle.enhance_observation(
        u.obs, u.activity_array, u.target_index, u.ex, return_details=True, bf='gev_ban',
        bss_iterations=40, gss_fn=oracle_pool.gss_block,
        wpe_fn=_oracle_per_array(oracle_pool.wpe_block, 6))
    T = det['Obs'].shape[1]
    assert np.array_equal(det['acitivity_freq'], wdet['activity_freq'][:, :T])
    nrm = np.linalg.norm(wdet['Obs'], axis=(0, 1))
    wpe_err = np.linalg.norm(det['Obs'] - wdet['Obs'], axis=(0, 1)) / nrm
    post_err = np.max(np.abs(det['posterior'] - np.where(wdet['masks'] == 0, det['posterior'],
                                                         wdet['masks'])), axis=(0, 1))
    print('config 5 per-array: after WPE per-bin error max %.2e median %.2e; posteriors max %.2e'
          % (wpe_err.max(), np.median(wpe_err), post_err.max()))
    assert wpe_err.max() < 1e-6
    assert post_err.max() < 1e-4
    masks = det['posterior'].copy()
    sf, ef = oracle.start_end_context_frames(u.ex, 1024, 256, True)
    masks[:, :sf] = 0
    if ef > 0:
        masks[:, -ef:] = 0
    assert np.array_equal(det['target_mask'], masks[u.target_index])
    # _scene_all_bins's beamformer rule: the literal oracle within 1e-4 wherever cond(Phi_N) <
    # 1e8 (here: every bin -- the extended-precision referee is only needed beyond that, and its
    # pivot-free elimination hits exact zeros on this scene), the referee elsewhere
    tm, dm = det['target_mask'], det['distortion_mask']
    cond = np.linalg.cond(oracle.get_power_spectral_density_matrix(
        det['Obs'].transpose(2, 0, 1), dm.T))
    strict = cond < 1e8
    X_lit = oracle.beamform_gev_from_masks(det['Obs'], tm, dm, ban=True)
    n = lambda a: np.linalg.norm(a, axis=0)
    e_lit = n(np.abs(det['X_hat']) - np.abs(X_lit)) / n(np.abs(X_lit))
    print('config 5 per-array: cond(Phi_N) < 1e8 in %d of %d bins; |X_hat| vs literal oracle '
          'max %.2e' % (strict.sum(), strict.size, e_lit[strict].max()))
    assert np.all(e_lit[strict] < TOL_STFT_MAG), np.flatnonzero(strict & (e_lit >= TOL_STFT_MAG))
    if not strict.all():
        _beamformer_all_bins_with_referee(gpu_ctx, det, u, 'gev_ban')
    assert rel_err(x_hat, oracle.istft(det['X_hat'])) < 1e-11
    assert np.all(np.isfinite(x_hat))


def test_fused_equals_block_path_and_oracle(gpu_ctx):
    """get_enhancer(multiarray=True, wpe_per_array=True): the fused pipeline, the block path
    (WPE(..., stack=False) on the (A, C, T, F) view) and the oracle agree; the option changes
    the result (it is not the joint WPE)."""
    from pb_chime5_amd import synthetic
    from pb_chime5_amd.core import get_enhancer
    u = synthetic.tiny(seed=31, num_channels=12, num_samples=24000, num_speakers=3, context=4096)
    enh = get_enhancer(multiarray=True, wpe_tabs=4, bss_iterations=6, wpe_per_array=True)
    assert enh.wpe_arrays(u.ex, 12) == 3
    a = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, fused=True)
    b = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, fused=False, debug=True)
    assert rel_err(a, b) < 1e-10
    assert enh.wpe_block.locals['Obs'].shape[:2] == (3, 4)
    c = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, wpe_arrays=3)
    assert np.array_equal(a, c)
    want = oracle.enhance_observation(u.obs, u.activity_array, u.target_index, u.ex, wpe_taps=4,
                                      bss_iterations=6, gss_fn=oracle.gss_block_batched,
                                      wpe_fn=_oracle_per_array(oracle.wpe_block, 3))
    assert rel_err(a, want) < 1e-5
    joint = get_enhancer(multiarray=True, wpe_tabs=4, bss_iterations=6).enhance_observation(
        u.obs, u.activity, u.speaker_id, ex=u.ex)
    assert rel_err(joint, a) > 1e-4


def test_one_array_is_bit_identical_to_the_default(gpu_ctx):
    """multiarray=False with wpe_per_array=True (A = 1) is the default pipeline, bit for bit --
    also when the caller names one array, through the fused call and the staged pipeline."""
    from pb_chime5_amd import ops, synthetic
    from pb_chime5_amd.core import get_enhancer
    u = synthetic.tiny(seed=32, num_channels=4, num_samples=32000, num_speakers=3, context=4096)
    base = get_enhancer(wpe_tabs=5, bss_iterations=6).enhance_observation(
        u.obs, u.activity, u.speaker_id, ex=u.ex)
    enh = get_enhancer(wpe_tabs=5, bss_iterations=6, wpe_per_array=True)
    assert enh.wpe_arrays(u.ex, 4) == 1
    assert np.array_equal(enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex), base)
    cs, ce = _contexts(u)
    kw = dict(wpe_taps=5, bss_iterations=6, ctx=gpu_ctx)
    x0 = ops.enhance_observation(u.obs, u.activity_array, u.target_index, cs, ce, **kw)
    x1 = ops.enhance_observation(u.obs, u.activity_array, u.target_index, cs, ce, wpe_arrays=1,
                                 **kw)
    assert np.array_equal(x0, x1)


def test_two_sets_of_bins_and_in_flight_pipeline_give_the_same_bits(gpu_ctx, monkeypatch):
    """The WPE stage's two-stream split runs over virtual bins (frequency, array): the same bits
    as one stream; the utterance pipeline (per-utterance A) equals the one-at-a-time call."""
    from pb_chime5_amd import ops, synthetic
    u = synthetic.tiny(seed=33, num_channels=8, num_samples=40000, num_speakers=3, context=4096)
    cs, ce = _contexts(u)
    kw = dict(wpe_taps=6, bss_iterations=5, ctx=gpu_ctx, wpe_arrays=2)
    one = ops.enhance_observation(u.obs, u.activity_array, u.target_index, cs, ce, **kw)
    monkeypatch.setenv('GSS_VARIANT', 'wpe_halves=1')
    two = ops.enhance_observation(u.obs, u.activity_array, u.target_index, cs, ce, **kw)
    monkeypatch.delenv('GSS_VARIANT')
    assert np.array_equal(one, two)
    pipe = ops.UtterancePipeline(ops.make_params(wpe_taps=6, bss_iterations=5), depth=2,
                                 first_ctx=gpu_ctx)
    try:
        pipe.enqueue('a', u.obs, u.activity_array, u.target_index, cs, ce, wpe_arrays=2)
        pipe.enqueue('b', u.obs, u.activity_array, u.target_index, cs, ce)
        (_, xa), (_, xb) = pipe.pop(), pipe.pop()
    finally:
        pipe.close()
    assert np.array_equal(xa, one)
    joint = ops.enhance_observation(u.obs, u.activity_array, u.target_index, cs, ce, wpe_taps=6,
                                    bss_iterations=5, ctx=gpu_ctx)
    assert np.array_equal(xb, joint) and not np.array_equal(xa, xb)


# ---------------------------------------------------------------- sessions
@pytest.mark.parametrize('loaders,inflight', [(3, 2)])
def test_dev_session_per_array_equals_example_loop(corpus_dev, fixture_dev, tmp_path, loaders,  # noqa: F811
                                                   inflight):
    """enhance_session(['S02', 'S09'], wpe_per_array=True) -- 6 arrays (24 ch) and 5 arrays
    (20 ch) in one run, A taken from each example -- writes the same bytes as the loop of
    enhance_example with the same setting; and not the bytes of the joint WPE."""
    sessions = fixture_dev['corpus']['session_id']
    a, b, c = tmp_path / 'seq', tmp_path / 'pipe', tmp_path / 'joint'
    seq = _enhancer(corpus_dev, fixture_dev, wpe_per_array=True)
    seq.inflight = 1
    seq.enhance_session(sessions, a)
    pipe = _enhancer(corpus_dev, fixture_dev, wpe_per_array=True)
    pipe.inflight, pipe.loaders = inflight, loaders
    pipe.enhance_session(sessions, b)
    joint = _enhancer(corpus_dev, fixture_dev)
    joint.enhance_session(sessions, c)
    files = sorted(p.relative_to(a) for p in a.rglob('*.wav'))
    assert len(files) == len(fixture_dev['examples'])
    assert files == sorted(p.relative_to(b) for p in b.rglob('*.wav'))
    for rel in files:
        assert (a / rel).read_bytes() == (b / rel).read_bytes(), rel
    assert any((a / rel).read_bytes() != (c / rel).read_bytes() for rel in files)


def test_rttm_front_door_runs_per_array_on_the_outer_mics(gpu_ctx, tmp_path):
    """core_chime6_rttm with multiarray='outer_array_mics', wpe_per_array=True (a flat list of
    channel files: A = D / 2), through the command line and against the oracle."""
    from pb_chime5_amd.core_chime6_rttm import get_enhancer
    from pb_chime5_amd.scripts import enhance_rttm
    from test_rttm_frontdoor import _make_chime6_dir
    root, rttm_file, _ = _make_chime6_dir(tmp_path)
    out = tmp_path / 'out'
    enhance_rttm.main([
        '--chime6-dir', str(root), '--database-rttm', str(rttm_file), '--session-id', 'S02',
        '--out', str(out), '--context-samples', '4000', '--wpe-tabs', '2',
        '--bss-iterations', '3', '--multiarray', 'outer_array_mics', '--wpe-per-array'])
    wavs = sorted((out / 'audio' / 'dev').glob('*.wav'))
    assert len(wavs) == 3
    enh = get_enhancer(database_rttm=[str(rttm_file)], activity_rttm=[str(rttm_file)],
                       chime6_dir=root, multiarray='outer_array_mics', context_samples=4000,
                       wpe_tabs=2, bss_iterations=3, wpe_per_array=True)
    ex = enh.get_dataset('S02')[1]
    assert ex['audio_data'].shape[0] == 6 and enh.wpe_arrays(ex, 6) == 3
    act = {k: v[ex['start']:ex['end']] for k, v in enh.activity['S02'].items()}
    oex = {'start': {'original': ex['start']}, 'start_orig': {'original': ex['start_orig']},
           'end_orig': {'original': ex['end_orig']}, 'end': {'original': ex['end']}}
    want = oracle.enhance_observation(ex['audio_data'], np.array(list(act.values())), 0, oex,
                                      wpe_taps=2, bss_iterations=3,
                                      gss_fn=oracle.gss_block_batched,
                                      wpe_fn=_oracle_per_array(oracle.wpe_block, 3))
    want = want[4000:4000 + 12000]
    got = enh.enhance_example(ex)
    assert got.shape == want.shape == (12000,)
    assert rel_err(got, want) < 1e-6
