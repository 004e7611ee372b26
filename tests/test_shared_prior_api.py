"""The CACGMM with a frequency-shared prior (gss_cacgmm_shared_prior; pb_bss
weight_constant_axis=-3) without a GPU: what the method does, on the NumPy reference
(tests/shared_prior_reference.py); the reference's invariants; the host-side checks of the
operators and the front doors; header and binding."""
import re

import numpy as np
import pytest

import gss_oracle as oracle
import shared_prior_reference as spr
from conftest import REPO

HEADER = (REPO / 'include' / 'gss_hip.h').read_text()


@pytest.fixture
def no_context(monkeypatch):
    """Any attempt to create or fetch a device context fails the test."""
    from pb_chime5_amd import _capi, ops

    def boom(*a, **k):
        raise AssertionError('device work before the argument check')
    monkeypatch.setattr(_capi, 'default_context', boom)
    monkeypatch.setattr(ops, 'default_context', boom)
    monkeypatch.setattr(_capi.Context, '__init__', boom)


# ------------------------------------------------------------------ what the method is for
@pytest.mark.parametrize('seed,D', spr.TABLE_RUNS)
def test_the_shared_prior_keeps_a_class_the_same_speaker_in_every_bin(seed, D):
    """Two speakers, three classes, a start that is no annotation ((K,T) uniform noise for every
    frequency), 20 iterations.  With the shared prior EVERY frequency gives each speaker the class
    the prior gives them, and the prior follows each speaker's true frame activity (>= 0.6: a
    loose floor that only tells 'tracks the speaker' from 'does not'; measured 0.74 ... 0.86).
    The per-frequency model from the same start does not: fewer than all bins agree (measured
    0.39 ... 0.92)."""
    Obs, truth, init, posterior, prior = spr.table_run(seed, D)
    assert Obs.shape == (D, 1003, 129)
    share, gap, corr = spr.bins_consistent(posterior, prior, truth)
    print(f's={seed} D={D}: shared prior {share:.3f} of the bins, smallest gap {gap:.2f}, '
          f'corr(prior, truth) {corr[0]:.2f} {corr[1]:.2f}')
    assert share == 1.0
    assert min(corr) >= 0.6
    per_f = spr.per_frequency_block(Obs, init, spr.TABLE_ITERATIONS)
    share_f, _, _ = spr.bins_consistent(per_f, per_f.mean(axis=2), truth)
    print(f's={seed} D={D}: per-frequency weights {share_f:.3f} of the bins')
    assert share_f < 1.0


# ------------------------------------------------------------------ invariants of the reference
CELL = (6, 90, 5, 3)        # D, T, F, K


def _cell(form, iterations=3, post=1, cell=CELL):
    D, T, F, K = cell
    Y, act = spr.parity_scene(D, T, F, K, 0)
    init, mask = spr.form_guidance(form, act, F, 0)
    return Y, init, mask, spr.shared_prior_block(Y, init, mask, iterations, post)


@pytest.mark.parametrize('form', spr.FORMS)
@pytest.mark.parametrize('post', [0, 1, 2])
def test_reference_posteriors_and_prior_are_distributions(form, post):
    _, _, mask, (posterior, prior) = _cell(form, post=post)
    live = np.ones(posterior.shape[1:], bool)
    if mask is not None and post == 0:
        live = np.broadcast_to(mask.any(axis=0)[:, None], live.shape)
    assert np.max(np.abs(posterior.sum(axis=0) - 1)[live]) <= 1e-12
    # the prior is a mean of affiliations clipped to [1e-10, 1 - 1e-10]
    assert np.max(np.abs(prior.sum(axis=0) - 1)) <= 1e-9
    assert prior.shape == posterior.shape[:2] and np.all(prior > 0)


def test_reference_first_prior_is_the_initialisation():
    """One iteration: the prior of the only M-step is the (K,T) table itself, the mean over f of
    an (F,K,T) one."""
    D, T, F, K = CELL
    Y, act = spr.parity_scene(D, T, F, K, 0)
    init, _ = spr.form_guidance('blind', act, F, 0)
    assert np.array_equal(spr.shared_prior_block(Y, init, None, 1, 1)[1], init)
    init3, _ = spr.form_guidance('random', act, F, 0)
    assert np.array_equal(spr.shared_prior_block(Y, init3, None, 1, 1)[1], init3.mean(axis=0))


def test_reference_reversing_the_frequencies_reverses_the_output():
    Y, init, mask, (posterior, prior) = _cell('random')
    back, prior_back = spr.shared_prior_block(Y[:, :, ::-1], init[::-1], None, 3, 1)
    assert np.max(np.abs(back[:, :, ::-1] - posterior)) <= 1e-12
    assert np.max(np.abs(prior_back - prior)) <= 1e-12


def test_reference_one_class_gives_ones():
    """K = 1: the posteriors are exactly 1 (w / w); the prior is the mean of the clipped
    affiliation of the last fit step, 1 - 1e-10 -- and exactly 1 after a single iteration, whose
    prior is the initialisation."""
    from pb_chime5_amd import ops
    D, T, F, _ = CELL
    Y, _ = spr.parity_scene(D, T, F, 3, 0)
    init = ops.blind_initialization(1, T, 0)
    assert np.all(init == 1.0)
    posterior, prior = spr.shared_prior_block(Y, init, None, 1, 1)
    assert np.all(posterior == 1.0) and np.all(prior == 1.0)
    posterior, prior = spr.shared_prior_block(Y, init, None, 3, 1)
    assert np.all(posterior == 1.0) and np.all(prior == 1.0 - 1e-10)


def test_reference_masked_entries_are_exactly_zero_with_post_0():
    _, _, mask, (posterior, _) = _cell('weak', post=0)
    off = ~np.broadcast_to(mask[:, :, None], posterior.shape)
    assert off.any() and np.all(posterior[off] == 0.0)
    _, _, _, (unmasked, _) = _cell('weak', post=1)
    assert np.all(unmasked[off] > 0.0)


def test_the_kept_seeds_are_stable_for_the_reference():
    """A sample of tests/test_gpu_shared_prior.py's cells, re-checked here: the reference moves
    at least 100 x less than the bar under a last-bit change of its input."""
    for cell, form in [(spr.CELLS[0], 'blind'), (spr.CELLS[1], 'random'), (spr.CELLS[2], 'weak'),
                       (spr.CELLS[5], 'blind'), (spr.CELLS[7], 'weak')]:
        moved = spr.reference_movement(cell, form, spr.seed_of(cell, form))
        print(f'{cell} {form}: seed {spr.seed_of(cell, form)}, the reference moves by {moved:.1e}')
        assert moved * spr.STABILITY_MARGIN <= spr.EM_TOL


# ------------------------------------------------------------------ host checks
def test_blind_initialization():
    from pb_chime5_amd import ops
    a = ops.blind_initialization(3, 1003, 100)
    assert a.shape == (3, 1003) and a.dtype == np.float64
    assert np.all(a > 0)
    assert np.max(np.abs(a.sum(axis=0) - 1)) <= 4e-16
    assert np.array_equal(a, ops.blind_initialization(3, 1003, 100))
    assert not np.array_equal(a, ops.blind_initialization(3, 1003, 101))
    # the definition, to the bit
    u = np.random.default_rng(100).uniform(size=(3, 1003))
    assert np.array_equal(a, u / u.sum(axis=0, keepdims=True))
    assert ops.blind_initialization(19, 1, np.int64(5)).shape == (19, 1)


@pytest.mark.parametrize('args', [(0, 10), (20, 10), (-1, 10), (3, 0), (3, -5), (3.0, 10), (3, 10.0),
                                  (True, 10), (3, 10, 1.5), (3, 10, '0'), (3, 10, None),
                                  (3, 10, -1), (3, 10, True)])
def test_blind_initialization_refuses(args):
    from pb_chime5_amd import ops
    with pytest.raises(ValueError):
        ops.blind_initialization(*args)


def _obs(D=4, T=30, F=5):
    rng = np.random.default_rng(0)
    return rng.standard_normal((D, T, F)) + 1j * rng.standard_normal((D, T, F))


BAD_SHARED = [
    (dict(), 'both None'),
    (dict(initialization=np.ones((3, 29))), 'frames'),
    (dict(initialization=np.ones((3, 30, 4))), 'frequencies'),
    (dict(initialization=np.ones((3,))), 'neither'),
    (dict(initialization=np.ones((3, 30)), source_activity_mask=np.ones((2, 30))), 'classes'),
    (dict(initialization=np.ones((20, 30))), 'classes outside'),
    (dict(initialization=np.ones((3, 30)), iterations=0), 'iterations'),
    (dict(initialization=np.ones((3, 30)), iterations=2.0), 'iterations'),
    (dict(initialization=np.ones((3, 30)), iterations_post=-1), 'iterations_post'),
    (dict(initialization=np.ones((3, 30)), iterations_post=True), 'iterations_post'),
]


@pytest.mark.parametrize('kw,match', BAD_SHARED, ids=[m for _, m in BAD_SHARED])
def test_shared_prior_op_refuses_before_any_device_work(no_context, kw, match):
    from pb_chime5_amd import ops
    with pytest.raises(ValueError, match=match):
        ops.cacgmm_posteriors_shared_prior(_obs(), **kw)


@pytest.mark.parametrize('obs,match', [
    (np.zeros((4, 30), complex), r'not \(D,T,F\)'), (np.zeros((4, 30, 5)), 'complex'),
    (np.zeros((1, 30, 5), complex), 'channels'), (np.zeros((33, 30, 5), complex), 'channels'),
    (np.zeros((4, 0, 5), complex), 'no frames')])
def test_both_ops_refuse_a_bad_observation(no_context, obs, match):
    from pb_chime5_amd import ops
    with pytest.raises(ValueError, match=match):
        ops.cacgmm_posteriors_shared_prior(obs, np.ones((3, 30)))
    with pytest.raises(ValueError, match=match):
        ops.cacgmm_posteriors_blind(obs, 3)


@pytest.mark.parametrize('kw', [dict(num_classes=0), dict(num_classes=20), dict(num_classes=2.0),
                                dict(num_classes=3, seed=0.5), dict(num_classes=3, iterations=0),
                                dict(num_classes=3, iterations='20')])
def test_blind_op_refuses_before_any_device_work(no_context, kw):
    from pb_chime5_amd import ops
    with pytest.raises(ValueError):
        ops.cacgmm_posteriors_blind(_obs(), **kw)


# ------------------------------------------------------------------ front doors
REFUSED = [('bf_segment_frames', dict(bf_segment_frames=64)),
           ('bf_null_interferer', dict(bf_null_interferer=True)),
           ('channel_keep', dict(channel_keep=3)),
           ('wpdSouden', dict(bf='wpdSouden_ban')), ('wpdSouden', dict(bf='wpdSouden')),
           ('wpe_per_array', dict(wpe_per_array=True, multiarray=True))]


@pytest.mark.parametrize('option,kw', REFUSED, ids=[str(k) for _, k in REFUSED])
def test_blind_methods_refuse_the_options_they_are_not_built_for(no_context, option, kw):
    from pb_chime5_amd import core
    enh = core.get_enhancer(**kw)
    with pytest.raises(NotImplementedError, match=option):
        enh.enhance_observation_blind(np.zeros((4, 4000)), 2)
    with pytest.raises(NotImplementedError, match=option):
        enh.enhance_example_blind({'speaker_id': 'A'}, 2)


@pytest.mark.parametrize('kw', [dict(num_speakers=0), dict(num_speakers=19), dict(num_speakers=2.0),
                                dict(num_speakers=True), dict(num_speakers=2, seed=1.5),
                                dict(num_speakers=2, seed=-1)])
def test_blind_method_refuses_bad_arguments_before_any_device_work(no_context, kw):
    from pb_chime5_amd import core
    with pytest.raises(ValueError):
        core.get_enhancer().enhance_observation_blind(np.zeros((4, 4000)), **kw)
    with pytest.raises(ValueError, match=r'\(D,N\)'):
        core.get_enhancer().enhance_observation_blind(np.zeros(4000), 2)


def test_gss_without_the_flag_dispatches_exactly_as_before(monkeypatch):
    """shared_prior defaults to False, and then GSS.__call__ never reaches the new op: a 0/1
    activity takes the unweighted call, weights the guided one, with the arguments of before."""
    from pb_chime5_amd import core, ops
    calls = []
    monkeypatch.setattr(ops, 'cacgmm_posteriors',
                        lambda *a, **k: calls.append(('plain', a, k)) or 'plain')
    monkeypatch.setattr(ops, 'cacgmm_posteriors_guided',
                        lambda *a, **k: calls.append(('guided', a, k)) or 'guided')
    monkeypatch.setattr(ops, 'cacgmm_posteriors_shared_prior',
                        lambda *a, **k: calls.append(('shared', a, k)) or ('shared', 'prior'))
    gss = core.GSS(iterations=7, iterations_post=2)
    assert gss.shared_prior is False
    assert core.get_enhancer().gss_block.shared_prior is False
    Obs = _obs()
    act = np.ones((3, 30), bool)
    act[0, :10] = False
    assert gss(Obs, act) == 'plain'
    assert calls[-1][0] == 'plain' and calls[-1][1][0] is Obs and calls[-1][1][1] is act
    assert calls[-1][2] == dict(iterations=7, iterations_post=2)
    weights = np.where(act, 0.3, 0.0)
    assert gss(Obs, weights) == 'guided'
    kind, a, k = calls[-1]
    init, mask = ops.guidance_from_activity(weights)
    assert kind == 'guided' and a[0] is Obs and k == dict(iterations=7, iterations_post=2)
    assert np.array_equal(a[1], init) and np.array_equal(a[2], mask)
    assert [c[0] for c in calls] == ['plain', 'guided']
    # with the flag every kind of activity takes the new op
    on = core.GSS(iterations=7, iterations_post=2, shared_prior=True)
    for activity in (act, weights):
        assert on(Obs, activity) == 'shared'
        kind, a, k = calls[-1]
        init, mask = ops.guidance_from_activity(activity)
        assert kind == 'shared' and a[0] is Obs
        assert np.array_equal(a[1], init) and np.array_equal(a[2], mask)
        assert k == dict(iterations=7, iterations_post=2, return_prior=True)
    on(Obs, act, debug=True)
    assert on.locals['prior'] == 'prior' and 'learned' in on.locals
    with pytest.raises(NotImplementedError, match='shared_prior'):
        on.locals['learned']


def test_entry_point_in_header_binding_and_library():
    from pb_chime5_amd import _capi, build
    assert re.search(r'\bint\s+gss_cacgmm_shared_prior\s*\(', HEADER)
    assert 'gss_cacgmm_shared_prior' in _capi.SIGNATURES
    restype, argtypes = _capi.SIGNATURES['gss_cacgmm_shared_prior']
    guided = _capi.SIGNATURES['gss_cacgmm_guided']
    assert restype is guided[0] and argtypes == guided[1] + [_capi.c_void_p]
    assert hasattr(_capi.load_library(), 'gss_cacgmm_shared_prior')
    assert 'cacgmm_prior.hip' in build.SOURCES
    assert _capi.GSS_ABI_VERSION == 7 and '#define GSS_ABI_VERSION 7' in HEADER
    comment = HEADER[HEADER.index('ABI revision of this header'):HEADER.index('#define GSS_ABI_VERSION')]
    assert 'gss_cacgmm_shared_prior' in comment


def test_a_library_without_the_symbol_is_named_in_the_error(monkeypatch):
    from pb_chime5_amd import _capi
    monkeypatch.setitem(_capi.SIGNATURES, 'gss_cacgmm_shared_prior_absent',
                        _capi.SIGNATURES['gss_cacgmm_shared_prior'])
    with pytest.raises(_capi.GssError, match='gss_cacgmm_shared_prior_absent'):
        _capi.load_library(_capi.LIB_PATH)


# ------------------------------------------------------------------ examples without an annotation
N, CONTEXT, WINDOW_START = 32000, 8000, 160000


class _NoAnnotation:
    def __getitem__(self, key):
        raise KeyError(f'no annotation for {key}')


def _blind_front_doors():
    from pb_chime5_amd import core, core_chime6, core_chime6_rttm as rttm
    clocks = {'U01': WINDOW_START + 777, 'U02': WINDOW_START}

    def on(value):
        return {'original': 500000 + value, 'observation': {k: v + value for k, v in clocks.items()}}
    ex5 = {'session_id': 'S99', 'example_id': 'x', 'reference_array': 'U02',
           'audio_path': {'observation': {'U01': 'u01.wav', 'U02': 'u02.wav'}},
           'start': on(0), 'end': on(N), 'start_orig': on(CONTEXT), 'end_orig': on(N - CONTEXT),
           'num_samples_orig': {'original': N - 2 * CONTEXT,
                                'observation': {k: N - 2 * CONTEXT for k in clocks}}}
    ex6 = {'session_id': 'S99', 'example_id': 'x', 'reference_array': 'U02',
           'audio_path': {'observation': {'U01': 'u01.wav', 'U02': 'u02.wav'}},
           'start': WINDOW_START, 'end': WINDOW_START + N, 'start_orig': WINDOW_START + CONTEXT,
           'end_orig': WINDOW_START + N - CONTEXT, 'num_samples': N,
           'num_samples_orig': N - 2 * CONTEXT}
    exr = dict(ex6, audio_data=np.zeros((4, N)))
    del exr['reference_array'], exr['audio_path']
    enh_r = rttm.Enhancer(
        db=None, context_samples=CONTEXT, multiarray='outer_array_mics', reference_array=None,
        wpe_block=None, activity=None, gss_block=rttm.GSS(iterations=2, iterations_post=1),
        bf_drop_context=True, bf_block=rttm.Beamformer(type='mvdrSouden_ban', postfilter=None),
        stft_size=1024, stft_shift=256, stft_fading=True)
    return [(core, core.get_enhancer(multiarray='outer_array_mics', context_samples=CONTEXT), ex5, 4),
            (core_chime6, core_chime6.get_enhancer(multiarray='outer_array_mics',
                                                   context_samples=CONTEXT), ex6, 4),
            (rttm, enh_r, exr, 4)]


def test_enhance_example_blind_asks_nothing_of_the_annotation(no_context, monkeypatch):
    """No speaker id in the example, an activity store that raises on every lookup: the three
    front doors load the audio alone, hand it to `enhance_observation_blind`, trim the context and
    put the intervals, clipped to the utterance, on the recording's clock."""
    from pb_chime5_amd import core
    for module, enh, ex, channels in _blind_front_doors():
        if hasattr(module, 'load_audio'):
            monkeypatch.setattr(module, 'load_audio', lambda path, start, stop, dtype=np.float64:
                                np.zeros((4, stop - start), dtype))
        enh.activity = _NoAnnotation()
        seen = {}

        def stub(obs, num_speakers, ex=None, **kw):
            seen.update(shape=np.shape(obs), num_speakers=num_speakers, kw=kw, ex=ex)
            return core.BlindSeparation(
                np.tile(np.arange(N, dtype=float), (3, 1)), np.full((3, 5), 1 / 3),
                np.zeros((3, 5), bool), [[(100, 9000)], [(7000, 20000), (23000, 31000)], []])
        monkeypatch.setattr(enh, 'enhance_observation_blind', stub)
        assert 'speaker_id' not in ex
        out = enh.enhance_example_blind(ex, 2, seed=4)
        assert seen['shape'] == (channels, N) and seen['num_speakers'] == 2
        assert seen['kw'] == dict(seed=4) and seen['ex'] is ex
        assert np.array_equal(out.x_hat, np.tile(np.arange(CONTEXT, N - CONTEXT, dtype=float), (3, 1)))
        assert out.intervals == [
            [(WINDOW_START + 8000, WINDOW_START + 9000)],
            [(WINDOW_START + 8000, WINDOW_START + 20000), (WINDOW_START + 23000, WINDOW_START + 24000)],
            []], module.__name__
        assert out.prior.shape == (3, 5)
        # the annotated methods still ask for it
        monkeypatch.undo()
