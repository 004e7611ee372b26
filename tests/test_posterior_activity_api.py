"""Posterior activity (gss_posterior_activity, gss_enhance_observation_activity,
pb_chime5_amd.posterior_activity, Enhancer.enhance_*_activity): the NumPy reference itself, the
decision rule, the interval and RTTM arithmetic, the argument checks, the C ABI and the front
doors, without a GPU."""
import inspect

import numpy as np
import pytest

from conftest import REPO

import posterior_activity_reference as ref

SYMBOLS = ('gss_posterior_activity', 'gss_enhance_observation_activity')


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize('D,T,F,K', [(2, 1, 1, 1), (5, 65, 4, 3), (12, 130, 7, 5)])
def test_reference_scores_of_normalised_posteriors_sum_to_one(D, T, F, K):
    Y, gamma = ref.scene(D, T, F, K)
    for w in (None, ref.weights(F)):
        scores, power = ref.posterior_activity(Y, gamma, w)
        assert scores.shape == (K, T) and power.shape == (T,)
        assert np.all(power > 0)
        assert np.all(scores >= 0) and np.all(scores <= 1 + 1e-12)
        assert np.max(np.abs(np.sum(scores, axis=0) - 1)) <= 10 * ref.bar(F, D)


def test_reference_silent_frame_scores_zero():
    Y, gamma = ref.scene(4, 20, 6, 3)
    Y[:, 7, :] = 0
    scores, power = ref.posterior_activity(Y, gamma)
    assert power[7] == 0.0 and np.all(scores[:, 7] == 0.0)
    assert np.all(np.isfinite(scores)) and np.all(power[np.arange(20) != 7] > 0)


def test_reference_one_hot_weights_reproduce_that_frequencys_posteriors():
    Y, gamma = ref.scene(3, 33, 5, 4)
    for f in range(5):
        w = np.zeros(5)
        w[f] = 2.5
        scores, power = ref.posterior_activity(Y, gamma, w)
        assert np.max(np.abs(scores - gamma[f])) <= 4 * 2.0 ** -53
        assert np.allclose(power, 2.5 * np.sum(np.abs(Y[f]) ** 2, axis=-1), rtol=1e-14)


def test_reference_tracks_the_truth_on_the_scene_of_the_gpu_test():
    """The scene of test_gpu_posterior_activity.py::test_scores_track_the_truth, on the CPU:
    posteriors from oracle/gss_oracle.py, scores from the NumPy reference.  The target's mean
    score is 0.67 over the frames it speaks in and 0.003 over the annotated frames it is
    silent in."""
    import gss_oracle as oracle
    u, spoken, silent = ref.truth_scene(4)
    _, det = oracle.enhance_observation(
        u.obs, u.activity_array, 0, ex=u.ex, bf_drop_context=False, return_details=True,
        gss_fn=oracle.gss_block_batched, **ref.TRUTH_PARAMS)
    scores, _ = ref.posterior_activity(det['Obs'].transpose(2, 1, 0),
                                       det['masks'].transpose(2, 0, 1))
    assert scores.shape == (3, len(spoken)) and spoken.sum() > 30 and silent.sum() > 30
    a, b = scores[0, spoken].mean(), scores[0, silent].mean()
    print(f'reference: spoken {a:.4f}, silent {b:.4f}')
    assert a > b


# ------------------------------------------------------------------ the rule
def _decide(row, power=None, **rule):
    from pb_chime5_amd.posterior_activity import ActivityRule, decide
    row = np.asarray(row, dtype=float)
    power = np.ones(len(row)) if power is None else np.asarray(power, dtype=float)
    base = dict(median_frames=1, on=0.5, off=0.35, min_off_frames=0, min_on_frames=0)
    base.update(rule)
    return decide(row[None], power, ActivityRule(**base))[0].astype(int).tolist()


def test_decide_hysteresis():
    # starts off; on at >= on; stays on while >= off; 0.4 alone never switches on
    assert _decide([0.4, 0.5, 0.4, 0.35, 0.34, 0.4, 0.49, 0.6]) == [0, 1, 1, 1, 0, 0, 0, 1]
    assert _decide([0.9, 0.2, 0.9], on=0.9, off=0.9) == [1, 0, 1]


def test_decide_power_floor_comes_first():
    row = [0.9, 0.9, 0.9, 0.9]
    assert _decide(row, power=[1.0, 0.009, 0.01, 100.0]) == [1, 1, 1, 1]
    assert _decide(row, power=[1.0, 0.009, 0.01, 100.0], power_floor=1e-2) == [1, 0, 0, 1]
    assert _decide(row, power=[1.0, 0.999, 1.0, 100.0], power_floor=1e-2) == [1, 0, 1, 1]
    # before the median: a zeroed frame takes part in it (and is outvoted here)
    assert _decide([0.9] * 5, power=[1, 1, 0, 1, 1], power_floor=0.5, median_frames=3) == \
        [1, 1, 1, 1, 1]
    assert _decide([0.9] * 5, power=[1, 1, 0, 1, 1], power_floor=0.5) == [1, 1, 0, 1, 1]


def test_decide_running_median_is_clipped_at_both_edges():
    from pb_chime5_amd.posterior_activity import running_median
    x = np.array([[0.9, 0.1, 0.2, 0.8, 0.7, 0.0, 1.0]])
    got = running_median(x, 3)
    want = [np.median(v) for v in ([0.9, 0.1], [0.9, 0.1, 0.2], [0.1, 0.2, 0.8], [0.2, 0.8, 0.7],
                                   [0.8, 0.7, 0.0], [0.7, 0.0, 1.0], [0.0, 1.0])]
    assert np.array_equal(got[0], want)
    got5 = running_median(x, 5)[0]
    assert got5[0] == np.median([0.9, 0.1, 0.2]) and got5[1] == np.median([0.9, 0.1, 0.2, 0.8])
    assert got5[-1] == np.median([0.7, 0.0, 1.0]) and got5[-2] == np.median([0.8, 0.7, 0.0, 1.0])
    assert np.array_equal(running_median(x, 1), x)
    # through decide: a single-frame spike goes, a single-frame hole closes; the first frame's
    # window is its two frames (median of [0.9, 0.1] = 0.5 >= on)
    assert _decide([0.9, 0.1, 0.1, 0.9, 0.1, 0.9, 0.9, 0.1, 0.9, 0.9], median_frames=3) == \
        [1, 0, 0, 0, 1, 1, 1, 1, 1, 1]


def test_decide_fills_short_gaps_between_on_runs_only():
    row = [0, 1, 1, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0]
    assert _decide(row, min_off_frames=3) == [0, 1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 0, 0]
    assert _decide(row, min_off_frames=4) == [0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0]
    assert _decide(row, min_off_frames=2) == row          # (a gap of min_off_frames stays)


def test_decide_drops_short_on_runs_after_the_filling():
    row = [1, 0, 0, 1, 1, 1, 0, 1, 0, 0, 0, 1, 1]
    assert _decide(row, min_on_frames=3) == [0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    assert _decide(row, min_on_frames=2) == [0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1]
    # filled first: 1 + gap + 3 + gap + 1 is one run of 8 and survives
    assert _decide(row, min_off_frames=3, min_on_frames=6) == \
        [1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]


def test_decide_shapes_and_defaults():
    from pb_chime5_amd.posterior_activity import ActivityRule, decide
    r = ActivityRule()
    assert (r.median_frames, r.on, r.off, r.min_off_frames, r.min_on_frames, r.power_floor) == \
        (11, 0.5, 0.35, 8, 8, 0.0)
    assert 'not measurements' in ActivityRule.__doc__
    scores = np.zeros((3, 40))
    scores[1, 10:30] = 0.8
    got = decide(scores, np.ones(40))
    assert got.dtype == bool and got.shape == (3, 40)
    assert got[1].tolist() == [False] * 10 + [True] * 20 + [False] * 10 and not got[[0, 2]].any()
    assert scores[1, 10] == 0.8                                  # (the input is not written)
    with pytest.raises(ValueError, match='power'):
        decide(scores, np.ones(39))
    with pytest.raises(ValueError, match='scores'):
        decide(scores[0], np.ones(40))


@pytest.mark.parametrize('bad', [
    dict(median_frames=0), dict(median_frames=4), dict(median_frames=-3), dict(median_frames=3.0),
    dict(median_frames=True), dict(on=0.3, off=0.4), dict(off=0.0), dict(off=-0.1), dict(on=1.5),
    dict(on=float('nan')), dict(off=float('nan')), dict(on='0.5'), dict(min_off_frames=-1),
    dict(min_on_frames=-1), dict(min_on_frames=2.5), dict(power_floor=-1e-3),
    dict(power_floor=1.0), dict(power_floor=float('inf'))])
def test_bad_rules_are_value_errors(bad):
    from pb_chime5_amd.posterior_activity import ActivityRule
    with pytest.raises(ValueError, match=next(iter(bad))):
        ActivityRule(**bad)


def test_good_rules():
    from pb_chime5_amd.posterior_activity import ActivityRule
    ActivityRule(median_frames=1, on=1.0, off=1.0, min_off_frames=0, min_on_frames=0)
    ActivityRule(median_frames=np.int64(3), on=0.5, off=0.5, power_floor=0.999)


# ------------------------------------------------------------------ frames -> samples
def _row(T, *runs):
    row = np.zeros(T, bool)
    for a, b in runs:
        row[a:b] = True
    return row


def test_frames_to_intervals_with_fading():
    from pb_chime5_amd.posterior_activity import frames_to_intervals
    # size 1024, shift 256, fading: pad 768, centre of frame t = 256 t - 256
    got = frames_to_intervals(_row(100, (10, 20), (50, 51)), 1024, 256, True, 100000)
    assert got == [(256 * 10 - 384, 256 * 20 - 384), (256 * 50 - 384, 256 * 51 - 384)]
    # adjacent runs (seen as two rows of a decision) meet without overlap
    a = frames_to_intervals(_row(100, (10, 20)), 1024, 256, True, 100000)
    b = frames_to_intervals(_row(100, (20, 30)), 1024, 256, True, 100000)
    assert a[0][1] == b[0][0]
    # an odd shift: [c_a - shift // 2, c_(b-1) + shift - shift // 2)
    got = frames_to_intervals(_row(50, (4, 6), (6, 9)), 20, 5, True, 1000)
    assert got == [(4 * 5 - 15 + 10 - 2, 8 * 5 - 15 + 10 + 5 - 2)]
    a = frames_to_intervals(_row(50, (4, 6)), 20, 5, True, 1000)
    b = frames_to_intervals(_row(50, (6, 9)), 20, 5, True, 1000)
    assert a == [(13, 23)] and b == [(23, 38)]


def test_frames_to_intervals_without_fading():
    from pb_chime5_amd.posterior_activity import frames_to_intervals
    got = frames_to_intervals(_row(100, (0, 3), (10, 20)), 1024, 256, False, 100000)
    assert got == [(512 - 128, 256 * 2 + 512 + 128), (256 * 10 + 384, 256 * 20 + 384)]


def test_frames_to_intervals_clips_and_drops():
    from pb_chime5_amd.posterior_activity import frames_to_intervals
    # with fading the first frames lie before sample 0: clipped, and dropped when nothing is left
    assert frames_to_intervals(_row(100, (0, 1)), 1024, 256, True, 100000) == []
    assert frames_to_intervals(_row(100, (0, 2)), 1024, 256, True, 100000) == [(0, 128)]
    assert frames_to_intervals(_row(100, (0, 4), (90, 100)), 1024, 256, True, 23000) == \
        [(0, 640), (256 * 90 - 384, 23000)]
    assert frames_to_intervals(_row(100, (95, 100)), 1024, 256, True, 23000) == []
    assert frames_to_intervals(_row(100), 1024, 256, True, 23000) == []
    assert frames_to_intervals(_row(5, (0, 5)), 1024, 256, True, 300) == [(0, 300)]
    with pytest.raises(ValueError, match='active_row'):
        frames_to_intervals(np.zeros((2, 5), bool), 1024, 256, True, 300)


# ------------------------------------------------------------------ RTTM
def test_write_rttm_round_trips_through_from_rttm(tmp_path):
    from pb_chime5_amd.database.chime5.rttm import from_rttm
    from pb_chime5_amd.posterior_activity import write_rttm
    spans = {'P05': [(12345, 20001), (160000, 160001)], 'P06': [(0, 7), (3 * 16000, 5 * 16000)]}
    path = tmp_path / 'S02.rttm'
    assert write_rttm(path, 'S02', spans) == 4
    lines = path.read_text().splitlines()
    assert lines[0] == 'SPEAKER S02 1 0.7715625 0.4785 <NA> <NA> P05 <NA> <NA>'
    assert lines[1] == 'SPEAKER S02 1 10 0.0000625 <NA> <NA> P05 <NA> <NA>'
    assert lines[3] == 'SPEAKER S02 1 3 2 <NA> <NA> P06 <NA> <NA>'
    assert all('e' not in line.lower().replace('speaker', '') for line in lines)
    back = from_rttm(path)
    assert set(back) == {'S02'} and set(back['S02']) == set(spans)
    for speaker, want in spans.items():
        assert [tuple(i) for i in back['S02'][speaker].normalized_intervals] == want
    # several files: overlapping lines are united, no merge step
    other = tmp_path / 'b.rttm'
    write_rttm(other, 'S02', {'P05': [(20000, 30000)]})
    union = from_rttm([path, other])['S02']['P05']
    assert [tuple(i) for i in union.normalized_intervals] == [(12345, 30000), (160000, 160001)]
    # an empty decision is an empty file
    assert write_rttm(other, 'S02', {'P05': []}) == 0 and from_rttm(other) == {}


def test_write_rttm_refuses_what_has_no_exact_form(tmp_path):
    from pb_chime5_amd.posterior_activity import write_rttm
    with pytest.raises(ValueError, match='exact'):
        write_rttm(tmp_path / 'x.rttm', 'S', {'A': [(1, 3)]}, sample_rate=44100)
    with pytest.raises(ValueError, match='empty'):
        write_rttm(tmp_path / 'x.rttm', 'S', {'A': [(5, 5)]})
    write_rttm(tmp_path / 'x.rttm', 'S', {'A': [(1, 3)]}, sample_rate=8000)
    assert (tmp_path / 'x.rttm').read_text().split()[3:5] == ['0.000125', '0.00025']


# ------------------------------------------------------------------ argument checks
@pytest.fixture
def no_context(monkeypatch):
    """Any attempt to create or fetch a device context fails the test."""
    from pb_chime5_amd import _capi, ops

    def boom(*a, **k):
        raise AssertionError('device work before the argument check')
    monkeypatch.setattr(_capi, 'default_context', boom)
    monkeypatch.setattr(ops, 'default_context', boom)
    monkeypatch.setattr(_capi.Context, '__init__', boom)


BAD_WEIGHTS = [np.ones(4), np.ones((5, 1)), np.ones((1, 5)), 1.0, [1, 1, 1, 1, -1e-300],
               [1, 1, float('nan'), 1, 1], [1, float('inf'), 1, 1, 1], ['a'] * 5, np.ones(5) * 1j]


@pytest.mark.parametrize('w', BAD_WEIGHTS, ids=range(len(BAD_WEIGHTS)))
def test_bad_freq_weights_are_value_errors_before_any_device_work(no_context, w):
    from pb_chime5_amd import core, ops
    Obs, post = np.ones((2, 7, 5), complex), np.ones((3, 7, 5))
    with pytest.raises(ValueError, match='freq_weights'):
        ops.posterior_activity(Obs, post, w)
    with pytest.raises(ValueError, match='freq_weights'):
        ops.check_freq_weights(w, 5)
    with pytest.raises(ValueError, match='freq_weights'):
        ops.enhance_observation_activity(np.zeros((2, 4000)), np.ones((2, 4000), bool), 0, 0, 0,
                                         freq_weights=w, stft_size=8, stft_shift=2)
    enh = core.get_enhancer(stft_size=8, stft_shift=2)
    with pytest.raises(ValueError, match='freq_weights'):
        enh.enhance_observation_activity(np.zeros((2, 4000)), {'A': np.ones(4000, bool)}, 'A',
                                         freq_weights=w)


def test_good_freq_weights():
    from pb_chime5_amd import ops
    assert ops.check_freq_weights(None, 5) is None
    w = ops.check_freq_weights([0, 1, 2, 0, 0.5], 5)
    assert w.dtype == np.float64 and w.flags.c_contiguous and w.tolist() == [0, 1, 2, 0, 0.5]
    assert ops.check_freq_weights(np.zeros(3, np.float32), 3).dtype == np.float64


def test_bad_shapes_are_value_errors_before_any_device_work(no_context):
    from pb_chime5_amd import ops
    Obs, post = np.ones((2, 7, 5), complex), np.ones((3, 7, 5))
    for a, b, name in ((Obs[0], post, 'Obs'), (Obs, post[0], 'posterior'),
                       (Obs[None], post, 'Obs'), (Obs, post[:, :6], 'differ'),
                       (Obs, post[:, :, :4], 'differ'), (Obs[:, :0], post[:, :0], 'empty'),
                       (Obs, post[:0], 'empty')):
        with pytest.raises(ValueError, match=name):
            ops.posterior_activity(a, b)
    with pytest.raises(ValueError, match='obs'):
        ops.enhance_observation_activity(np.zeros(4000), np.ones((2, 4000), bool), 0, 0, 0)


def test_signatures_and_defaults():
    from pb_chime5_amd import core, ops
    sig = inspect.signature(ops.posterior_activity).parameters
    assert list(sig) == ['Obs', 'posterior', 'freq_weights', 'return_power', 'ctx']
    assert (sig['freq_weights'].default, sig['return_power'].default, sig['ctx'].default) == \
        (None, False, None)
    assert sig['ctx'].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(ops.enhance_observation_activity).parameters
    plain = inspect.signature(ops.enhance_observation).parameters
    assert [n for n in sig if n != 'freq_weights'] == list(plain)
    assert sig['freq_weights'].default is None and sig['debug'].default is False
    sig = inspect.signature(core.Enhancer.enhance_observation_activity).parameters
    assert list(sig)[:5] == ['self', 'obs', 'ex_array_activity', 'speaker_id', 'ex']
    assert sig['freq_weights'].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(core.Enhancer.enhance_example_activity).parameters
    assert list(sig) == ['self', 'ex', 'rule', 'freq_weights']
    from pb_chime5_amd import core_chime6, core_chime6_rttm
    for cls in (core.Enhancer, core_chime6.Enhancer, core_chime6_rttm.Enhancer):
        assert inspect.signature(cls.enhance_session).parameters['refined_rttm'].default is False


# ------------------------------------------------------------------ header and binding
def test_the_built_library_exports_the_activity_entry_points():
    from pb_chime5_amd import _capi
    lib = _capi.load_library()
    header = (REPO / 'include' / 'gss_hip.h').read_text()
    for name in SYMBOLS:
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
        assert f'int {name}(' in header, name
    assert len(_capi.SIGNATURES['gss_posterior_activity'][1]) == 10
    assert len(_capi.SIGNATURES['gss_enhance_observation_activity'][1]) == 16
    assert 'NOT inspected' in header                     # the weight table
    # entry points only: the revision is the one the per-array WPE pinned
    assert _capi.GSS_ABI_VERSION == 7 and lib.gss_abi_version() == 7
    assert '#define GSS_ABI_VERSION 7' in header
    from pb_chime5_amd import build
    assert 'posterior_activity.hip' in build.SOURCES


# ------------------------------------------------------------------ front doors
def _enhancers(**kw):
    from pb_chime5_amd import core, core_chime6
    return [mod.get_enhancer(**kw) for mod in (core, core_chime6)]


@pytest.mark.parametrize('option,kw', [
    ('bf_segment_frames', dict(bf_segment_frames=64)),
    ('bf_null_interferer', dict(bf_null_interferer=True)),
    ('channel_keep', dict(channel_keep=3))])
def test_refused_combinations_name_the_option_before_any_device_work(no_context, tmp_path,
                                                                     option, kw):
    obs, act = np.zeros((4, 4000)), {'A': np.ones(4000, bool), 'Noise': np.ones(4000, bool)}
    for enh in _enhancers(**kw):
        with pytest.raises(NotImplementedError, match=option):
            enh.enhance_observation_activity(obs, act, 'A')
        with pytest.raises(NotImplementedError, match=option):
            enh.enhance_example_activity({'speaker_id': 'A'})
        with pytest.raises(NotImplementedError, match=option):
            enh.enhance_session('S02', tmp_path / 'never', refined_rttm=True)
        assert not (tmp_path / 'never').exists()


def test_the_speakers_methods_refuse_the_activity(no_context):
    obs, act = np.zeros((4, 4000)), {'A': np.ones(4000, bool), 'Noise': np.ones(4000, bool)}
    for enh in _enhancers():
        with pytest.raises(NotImplementedError, match='posterior_activity'):
            enh.enhance_observation_speakers(obs, act, posterior_activity=True)
        with pytest.raises(NotImplementedError, match='posterior_activity'):
            enh.enhance_example_speakers({'speaker_id': 'A'}, posterior_activity=True)


def test_rttm_front_door_refuses_the_same():
    from pb_chime5_amd import core_chime6_rttm as m
    enh = m.Enhancer(
        db=None, context_samples=0, multiarray='outer_array_mics', reference_array=None,
        wpe_block=None, activity=m.Activity(), gss_block=m.GSS(iterations=1, iterations_post=1,
                                                               verbose=False),
        bf_drop_context=True, bf_block=m.Beamformer(type='mvdrSouden_ban', postfilter=None,
                                                    segment_frames=64),
        stft_size=1024, stft_shift=256, stft_fading=True)
    with pytest.raises(NotImplementedError, match='bf_segment_frames'):
        enh.enhance_session('S02', 'never', refined_rttm=True)
    with pytest.raises(NotImplementedError, match='bf_segment_frames'):
        enh.enhance_example_activity({})


def test_command_line_has_the_switch():
    from pb_chime5_amd.scripts import enhance_rttm
    src = inspect.getsource(enhance_rttm)
    assert "'--refined-rttm'" in src and 'refined_rttm' in src


# ------------------------------------------------------------------ the recording's clock
N, CONTEXT, WINDOW_START = 40000, 8000, 123456


class _FakeCtx:
    def set_utterances_in_flight(self, n):
        pass


def _stub_device(monkeypatch, enh, runs, seen):
    """The fused device call replaced: the target's score is 0.9 in the frames of ``runs``."""
    from pb_chime5_amd import ops
    T = ops.stft_frames(N, 1024, 256, True)

    def fake(obs, activity, target_index, start_ctx, end_ctx, *, freq_weights=None, params=None,
             ctx=None, wpe_arrays=None, **kw):
        seen.update(target_index=target_index, contexts=(start_ctx, end_ctx),
                    freq_weights=freq_weights, shape=np.shape(obs))
        scores = np.full((np.shape(activity)[0], T), 0.05)
        scores[target_index] = np.where(_row(T, *runs), 0.9, 0.05)
        return np.arange(N, dtype=float), scores, np.ones(T)
    monkeypatch.setattr(ops, 'enhance_observation_activity', fake)
    monkeypatch.setattr(type(enh), '_ctx', lambda self: _FakeCtx())
    obs = np.zeros((4, N))
    activity = {'P01': np.ones(N, bool), 'P02': np.ones(N, bool), 'Noise': np.ones(N, bool)}
    monkeypatch.setattr(type(enh), '_prepare_example',
                        lambda self, ex, dtype=np.float64: (obs, activity, ex['speaker_id']))
    return T


RUNS = [(20, 60), (100, 150)]
# frames [a, b) -> samples [256 a - 384, 256 b - 384) of the window; the utterance's own span is
# [CONTEXT, N - CONTEXT); then the window's first sample on the recording's clock
WANT = [(WINDOW_START + 8000, WINDOW_START + 256 * 60 - 384),
        (WINDOW_START + 256 * 100 - 384, WINDOW_START + 32000)]


def _check_mapping(enh, ex, monkeypatch):
    seen = {}
    T = _stub_device(monkeypatch, enh, RUNS, seen)
    x_hat, intervals = enh.enhance_example_activity(ex)
    assert intervals == WANT
    assert np.array_equal(x_hat, np.arange(CONTEXT, N - CONTEXT, dtype=float))   # trimmed
    assert seen == dict(target_index=1, contexts=(CONTEXT, CONTEXT), freq_weights=None,
                        shape=(4, N))
    # the report of the observation call
    x, act = enh.enhance_observation_activity(np.zeros((4, N)), {
        'P01': np.ones(N, bool), 'P02': np.ones(N, bool), 'Noise': np.ones(N, bool)}, 'P02', ex=ex,
        freq_weights=np.ones(513))
    assert act.keys == ('P01', 'P02', 'Noise') and act.target_index == 1
    assert act.scores.shape == (3, T) and act.power.shape == (T,)
    assert (act.start_context_frames, act.end_context_frames) == (
        enh_frames(CONTEXT), enh_frames(CONTEXT))
    assert seen['freq_weights'].shape == (513,)
    # a rule of one's own reaches `decide`
    from pb_chime5_amd.posterior_activity import ActivityRule
    none = enh.enhance_example_activity(ex, rule=ActivityRule(on=0.95, off=0.95))[1]
    assert none == []


def enh_frames(samples):
    from pb_chime5_amd import ops
    return ops.samples_to_stft_frames(samples, 1024, 256, fading=True)


def test_chime5_json_front_door_maps_to_the_reference_arrays_clock(monkeypatch):
    from pb_chime5_amd import core
    enh = core.get_enhancer(multiarray=True, context_samples=CONTEXT)
    # the arrays of a CHiME-5 example run on clocks of their own: the reference array's counts
    clocks = {'U01': WINDOW_START + 777, 'U02': WINDOW_START}
    ex = {
        'session_id': 'S02', 'speaker_id': 'P02', 'example_id': 'x', 'reference_array': 'U02',
        'start': {'original': 500000, 'observation': clocks},
        'end': {'original': 500000 + N, 'observation': {k: v + N for k, v in clocks.items()}},
        'start_orig': {'original': 500000 + CONTEXT,
                       'observation': {k: v + CONTEXT for k, v in clocks.items()}},
        'end_orig': {'original': 500000 + N - CONTEXT,
                     'observation': {k: v + N - CONTEXT for k, v in clocks.items()}},
        'num_samples_orig': {'original': N - 2 * CONTEXT,
                             'observation': {k: N - 2 * CONTEXT for k in clocks}},
    }
    _check_mapping(enh, ex, monkeypatch)


def _one_clock_example():
    return {'session_id': 'S02', 'speaker_id': 'P02', 'example_id': 'x',
            'reference_array': 'U02', 'start': WINDOW_START, 'end': WINDOW_START + N,
            'start_orig': WINDOW_START + CONTEXT, 'end_orig': WINDOW_START + N - CONTEXT,
            'num_samples': N, 'num_samples_orig': N - 2 * CONTEXT}


def test_chime6_json_front_door_maps_with_its_one_clock(monkeypatch):
    from pb_chime5_amd import core_chime6
    enh = core_chime6.get_enhancer(multiarray=True, context_samples=CONTEXT)
    _check_mapping(enh, _one_clock_example(), monkeypatch)


def test_rttm_front_door_maps_with_its_one_clock(monkeypatch, tmp_path):
    from pb_chime5_amd import core_chime6_rttm as m
    enh = m.Enhancer(
        db=None, context_samples=CONTEXT, multiarray='outer_array_mics', reference_array=None,
        wpe_block=m.WPE(taps=10, delay=2, iterations=3, psd_context=0), activity=m.Activity(),
        gss_block=m.GSS(iterations=20, iterations_post=1, verbose=False), bf_drop_context=True,
        bf_block=m.Beamformer(type='mvdrSouden_ban', postfilter=None),
        stft_size=1024, stft_shift=256, stft_fading=True)
    ex = _one_clock_example()
    del ex['reference_array']                             # an RTTM example names none
    _check_mapping(enh, ex, monkeypatch)

    # the session loop writes <example_id>.rttm next to the WAV, file id = the session id
    from pb_chime5_amd import mapping
    from pb_chime5_amd.database.chime5.rttm import from_rttm
    dataset = mapping.session_to_dataset['S02']
    (tmp_path / dataset).mkdir()
    written = []
    monkeypatch.setattr(type(enh), '_write',
                        lambda self, ex, x_hat, audio_dir: written.append(len(x_hat)))
    enh._enhance_and_write([ex], tmp_path, refined_rttm=True)
    assert written == [N - 2 * CONTEXT]
    back = from_rttm(tmp_path / dataset / 'x.rttm')
    assert [tuple(i) for i in back['S02']['P02'].normalized_intervals] == WANT
