"""WPD convolutional beamformer (gss_wpd_souden, get_enhancer(bf='wpdSouden_ban')): the C ABI, the
argument checks, the parameter plumbing, the front doors and the NumPy reference itself
(tests/wpd_reference.py: the factorised form against the direct solve), without a GPU."""
import ctypes
import inspect

import numpy as np
import pytest

import wpd_reference as wr
from conftest import REPO

SYMBOLS = ('gss_wpe_weighted', 'gss_wpd_weights', 'gss_wpd_souden', 'gss_last_wpd_zero_pivots',
           'gss_enhance_observation_wpd')


def test_the_built_library_exports_the_wpd_entry_points():
    from pb_chime5_amd import _capi
    lib = _capi.load_library()
    header = (REPO / 'include' / 'gss_hip.h').read_text()
    for name in SYMBOLS:
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
        assert f'int {name}(' in header, name
    # entry points only: the revision is the one the per-array WPE pinned
    assert _capi.GSS_ABI_VERSION == 7 and lib.gss_abi_version() == 7


def test_descriptor_layout_is_the_header_struct():
    from pb_chime5_amd import _capi
    header = (REPO / 'include' / 'gss_hip.h').read_text()
    for decl in ('int taps, delay, iterations, ban;', 'double power_floor;', '} gss_bf_wpd;'):
        assert decl in header, decl
    S = _capi.GssBfWpd
    assert [n for n, _ in S._fields_] == ['taps', 'delay', 'iterations', 'ban', 'power_floor']
    assert [getattr(S, n).offset for n, _ in S._fields_] == [0, 4, 8, 12, 16]
    assert ctypes.sizeof(S) == 24


@pytest.fixture
def no_context(monkeypatch):
    """Any attempt to create or fetch a device context fails the test."""
    from pb_chime5_amd import _capi, ops

    def boom(*a, **k):
        raise AssertionError('device work before the argument check')
    monkeypatch.setattr(_capi, 'default_context', boom)
    monkeypatch.setattr(ops, 'default_context', boom)
    monkeypatch.setattr(_capi.Context, '__init__', boom)


# ------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize('scene', wr.STAGE_SCENES, ids=str)
def test_factorised_and_direct_form_agree(scene):
    """One WPE step with 1 / target power, then the wMPDR, against the direct solve of the stacked
    (taps + 1) D system: <= 1e-10 on every stage scene of the GPU tests (measured 1e-15 ...
    1e-12); the scenes are well conditioned, or this fails loudly."""
    D, T, F, taps, delay = scene
    assert T >= 2 * (taps + 1) * D or D < 24
    Y, m, g = wr.scene(np.random.default_rng(1000 * D + T), *scene)
    assert g[:7].sum() == 0 and g[-5:].sum() == 0 and g[7:-5].all()
    assert m.min() >= 1e-10 and m.max() <= 1
    x, det = wr.wpd_souden_from_masks(Y, m, taps=taps, delay=delay, frame_gate=g)
    assert np.linalg.cond(det['phi_a']).max() <= 1e5
    xd = wr.direct(Y, m, det['a'], taps, delay, det['ref_channel'], g)
    err = np.abs(x - xd).max() / np.abs(xd).max()
    rho = wr.orthogonality(Y, det['a'], x, taps, delay)
    print(f'{scene}: factorised vs direct {err:.1e}, rho {rho:.1e}')
    assert err <= 1e-10
    assert rho <= 1e-9
    # the gate: the weights vanish on the context, and the mask there does not matter
    assert np.all(det['a'][:, g == 0] == 0) and np.all(det['a'][:, g != 0] > 0)
    m2 = m.copy()
    m2[g == 0] = 0.5
    assert np.array_equal(wr.wpd_souden_from_masks(Y, m2, taps=taps, delay=delay,
                                                   frame_gate=g)[0], x)


def test_reference_weights():
    p = np.array([[4.0, 1.0, 1e-6, 8.0], [0.0, 0.0, 0.0, 5.0]])
    gate = np.array([1, 1, 1, 0])
    a = wr.weights(p, gate, 1e-3)
    assert np.array_equal(a[0], [0.25, 1.0, 1 / 4e-3, 0.0])     # the gated-out 8 is no maximum
    assert np.all(a[1] == 0)                                      # power on gated-out frames only
    assert np.all(wr.weights(p, np.zeros(4), 1e-3) == 0)
    assert np.array_equal(wr.weights(p, np.ones(4), 1.0)[0], np.full(4, 1 / 8))


# ------------------------------------------------------------------ argument checks
def test_check_bf_wpd():
    from pb_chime5_amd import ops
    bf = ops.check_bf_wpd()
    assert (bf.taps, bf.delay, bf.iterations, bf.ban, bf.power_floor) == (10, 2, 1, 0, 1e-3)
    bf = ops.check_bf_wpd(3, 0, 4, 1.0, True, 29)
    assert (bf.taps, bf.delay, bf.iterations, bf.ban, bf.power_floor) == (3, 0, 4, 1, 1.0)
    assert ops.WPD_POWER_FLOOR == 1e-3
    for kw, word in ((dict(taps=0), 'taps'), (dict(taps=2.0), 'taps'), (dict(taps=True), 'taps'),
                     (dict(delay=-1), 'delay'), (dict(delay=None), 'delay'),
                     (dict(iterations=0), 'iterations'), (dict(iterations='2'), 'iterations'),
                     (dict(power_floor=0), 'power_floor'), (dict(power_floor=1.01), 'power_floor'),
                     (dict(power_floor=-1e-3), 'power_floor'),
                     (dict(power_floor=float('nan')), 'power_floor'),
                     (dict(power_floor=float('inf')), 'power_floor'),
                     (dict(power_floor=None), 'power_floor'), (dict(num_channels=0), 'num_channels')):
        with pytest.raises(ValueError, match=word):
            ops.check_bf_wpd(**kw)
    with pytest.raises(AssertionError, match='D < 30'):
        ops.check_bf_wpd(num_channels=30)
    for kw, word in ((dict(bf='mvdrSouden_ban'), 'mvdrSouden_ban'), (dict(bf='gev_ban'), 'gev_ban'),
                     (dict(segment_frames=64), 'bf_segment_frames'),
                     (dict(null_interferer=True), 'bf_null_interferer'),
                     (dict(channel_keep=3), 'channel_keep'), (dict(multi_target=True), 'targets'),
                     (dict(activity=True), 'activity')):
        with pytest.raises(NotImplementedError, match=word):
            ops.check_bf_wpd(**kw)
    for bf in ('wpdSouden', 'wpdSouden_ban'):
        ops.check_bf_wpd(bf=bf)


def test_stage_argument_errors_before_any_device_work(no_context):
    from pb_chime5_amd import ops
    Y = np.zeros((4, 130, 3), complex)
    m = np.zeros((130, 3))
    for kw, word in ((dict(taps=0), 'taps'), (dict(delay=-1), 'delay'),
                     (dict(iterations=0), 'iterations'), (dict(power_floor=2.0), 'power_floor'),
                     (dict(ref_channel=4), 'ref_channel'), (dict(ref_channel=-1), 'ref_channel'),
                     (dict(frame_gate=np.ones(129)), 'frame_gate')):
        with pytest.raises(ValueError, match=word):
            ops.wpd_souden_from_masks(Y, m, **kw)
    with pytest.raises(ValueError, match='Y'):
        ops.wpd_souden_from_masks(Y[0], m)
    with pytest.raises(ValueError, match='X_mask'):
        ops.wpd_souden_from_masks(Y, m[:-1])
    with pytest.raises(AssertionError, match='D < 30'):
        ops.wpd_souden_from_masks(np.zeros((30, 130, 3), complex), m)
    with pytest.raises(ValueError, match='power_floor'):
        ops.wpd_weights(Y, m, power_floor=0.0)
    with pytest.raises(ValueError, match='either'):
        ops.wpd_weights(Y)
    with pytest.raises(ValueError, match='either'):
        ops.wpd_weights(Y, m, X_hat=m)
    with pytest.raises(ValueError, match='X_mask'):
        ops.wpd_weights(Y, m.T)
    with pytest.raises(ValueError, match='weights'):
        ops.wpe_weighted(Y, np.ones((130, 3)))
    with pytest.raises(ValueError, match='taps'):
        ops.wpe_weighted(Y, np.ones((3, 130)), taps=0)


def test_fused_argument_errors_before_any_device_work(no_context):
    from pb_chime5_amd import ops
    obs, act = np.zeros((4, 4096)), np.ones((3, 4096), bool)
    with pytest.raises(ValueError, match='obs'):
        ops.enhance_observation_wpd(obs[0], act, 0, 0, 0)
    for kw, word in ((dict(taps=0), 'taps'), (dict(delay=-2), 'delay'),
                     (dict(iterations=0), 'iterations'), (dict(power_floor=0.0), 'power_floor')):
        with pytest.raises(ValueError, match=word):
            ops.enhance_observation_wpd(obs, act, 0, 0, 0, **kw)
    for bf in ('gev_ban', 'ch2', 'sum'):
        with pytest.raises(NotImplementedError, match=bf):
            ops.enhance_observation_wpd(obs, act, 0, 0, 0, bf=bf)
    with pytest.raises(AssertionError, match='D < 30'):
        ops.enhance_observation_wpd(np.zeros((30, 4096)), act, 0, 0, 0)
    with pytest.raises(ValueError, match='wpe_arrays'):
        ops.enhance_observation_wpd(obs, act, 0, 0, 0, wpe_arrays=3)


def test_signatures_and_defaults():
    from pb_chime5_amd import ops
    from pb_chime5_amd.speech_enhancement import beamforming_wrapper
    sig = inspect.signature(beamforming_wrapper.beamform_wpd_souden_from_masks).parameters
    assert list(sig)[:3] == ['Y', 'X_mask', 'ban']
    assert [(k, sig[k].default) for k in ('ban', 'taps', 'delay', 'iterations', 'power_floor',
                                          'frame_gate')] == \
        [('ban', False), ('taps', 10), ('delay', 2), ('iterations', 1), ('power_floor', 1e-3),
         ('frame_gate', None)]
    for k in ('taps', 'delay', 'iterations', 'power_floor', 'frame_gate'):
        assert sig[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    sig = inspect.signature(ops.wpd_souden_from_masks).parameters
    assert (sig['taps'].default, sig['delay'].default, sig['iterations'].default,
            sig['power_floor'].default) == (10, 2, 1, 1e-3)


# ------------------------------------------------------------------ wrapper and block
def test_wrapper_shape_rules(monkeypatch):
    """2-, 3- and 4-dimensional masks (median over channels), NotImplementedError(shape)
    otherwise: what reaches the operator."""
    from pb_chime5_amd import ops
    from pb_chime5_amd.speech_enhancement.beamforming_wrapper import beamform_wpd_souden_from_masks
    seen = []

    def fake(Y, X_mask, **kw):
        seen.append((np.array(Y), np.array(X_mask), kw))
        return 'x'
    monkeypatch.setattr(ops, 'wpd_souden_from_masks', fake)
    rng = np.random.default_rng(0)
    D, T, F = 3, 7, 2
    Y = rng.standard_normal((D, T, F)) + 0j
    m3 = rng.uniform(size=(D, T, F))
    gate = np.ones(T)
    assert beamform_wpd_souden_from_masks(Y, m3[0], True, taps=4, delay=1, iterations=2,
                                          power_floor=0.5, frame_gate=gate) == 'x'
    assert beamform_wpd_souden_from_masks(Y, m3) == 'x'
    assert beamform_wpd_souden_from_masks(Y[None], m3[None]) == 'x'
    for got_Y, _, _ in seen:
        assert np.array_equal(got_Y, Y)
    assert np.array_equal(seen[0][1], m3[0])
    assert np.array_equal(seen[1][1], np.median(m3, axis=0))
    assert np.array_equal(seen[2][1], np.median(m3, axis=0))
    kw = seen[0][2]
    assert (kw['ban'], kw['taps'], kw['delay'], kw['iterations'], kw['power_floor']) == \
        (True, 4, 1, 2, 0.5) and kw['frame_gate'] is gate
    kw = seen[1][2]
    assert (kw['ban'], kw['taps'], kw['delay'], kw['iterations'], kw['power_floor'],
            kw['frame_gate']) == (False, 10, 2, 1, 1e-3, None)
    with pytest.raises(NotImplementedError):
        beamform_wpd_souden_from_masks(Y, m3[0, 0])
    with pytest.raises(AssertionError):
        beamform_wpd_souden_from_masks(np.zeros((30, T, F), complex), m3[0])


def test_beamformer_types(no_context):
    from pb_chime5_amd.core import Beamformer
    plain = Beamformer('mvdrSouden_ban', None)
    assert plain.wpd is None
    assert (plain.wpd_taps, plain.wpd_delay, plain.wpd_iterations, plain.wpd_power_floor) == \
        (10, 2, 1, 1e-3)
    assert Beamformer('wpdSouden', None).wpd == dict(taps=10, delay=2, iterations=1,
                                                     power_floor=1e-3, ban=False)
    assert Beamformer('wpdSouden_ban', 'mask_mul', wpd_taps=4, wpd_delay=1, wpd_iterations=3,
                      wpd_power_floor=0.1).wpd == dict(taps=4, delay=1, iterations=3,
                                                       power_floor=0.1, ban=True)
    # the fields are unread by the other types
    assert Beamformer('ch2', None, wpd_taps=0).wpd is None
    for kw, word in ((dict(wpd_taps=0), 'taps'), (dict(wpd_delay=-1), 'delay'),
                     (dict(wpd_iterations=0), 'iterations'), (dict(wpd_power_floor=0), 'power_floor')):
        with pytest.raises(ValueError, match=word):
            Beamformer('wpdSouden_ban', None, **kw)
    with pytest.raises(NotImplementedError, match='bf_segment_frames'):
        Beamformer('wpdSouden_ban', None, segment_frames=64)
    with pytest.raises(NotImplementedError, match='bf_null_interferer'):
        Beamformer('wpdSouden', None, null_interferer=True)
    Y, m = np.zeros((4, 70, 3), complex), np.zeros((70, 3))
    with pytest.raises(ValueError, match='raw_obs'):
        plain(Y, m, m, raw_obs=Y)
    with pytest.raises(ValueError, match='frame_gate'):
        plain(Y, m, m, frame_gate=np.ones(70))
    with pytest.raises(ValueError, match='interferer_mask'):
        Beamformer('wpdSouden', None)(Y, m, m, interferer_mask=m)


def test_beamformer_call_hands_over_the_raw_stft(monkeypatch):
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import Beamformer
    seen = []

    def fake(Y, X_mask, **kw):
        seen.append((Y, X_mask, kw))
        return np.ones(np.shape(X_mask), complex)
    monkeypatch.setattr(ops, 'wpd_souden_from_masks', fake)
    D, T, F = 4, 70, 3
    Obs, raw = np.zeros((D, T, F), complex), np.ones((D, T, F), complex)
    m = np.full((T, F), 0.25)
    gate = np.ones(T)
    out = Beamformer('wpdSouden_ban', 'mask_mul', wpd_taps=3)(Obs, m, 1 - m, raw_obs=raw,
                                                              frame_gate=gate)
    assert np.array_equal(out, m)
    assert np.array_equal(seen[0][0], raw) and np.array_equal(seen[0][1], m)
    kw = seen[0][2]
    assert (kw['ban'], kw['taps'], kw['delay'], kw['iterations'], kw['power_floor']) == \
        (True, 3, 2, 1, 1e-3) and kw['frame_gate'] is gate
    Beamformer('wpdSouden', None)(Obs, m, 1 - m)
    assert np.array_equal(seen[1][0], Obs) and seen[1][2]['ban'] is False


# ------------------------------------------------------------------ front doors
def test_every_front_door_has_the_keywords_and_carries_them():
    from pb_chime5_amd import core, core_chime6, core_chime6_rttm
    for mod in (core, core_chime6, core_chime6_rttm):
        sig = inspect.signature(mod.get_enhancer).parameters
        assert [sig[k].default for k in ('bf_wpd_taps', 'bf_wpd_delay', 'bf_wpd_iterations',
                                         'bf_wpd_power_floor')] == [None, None, 1, 1e-3], mod.__name__
    for mod in (core, core_chime6):
        assert mod.get_enhancer().bf_block == core.Beamformer('mvdrSouden_ban', None)
        assert mod.get_enhancer()._bf_wpd() is None
        # None means the WPE block's taps / delay
        enh = mod.get_enhancer(bf='wpdSouden_ban', wpe_tabs=7, wpe_delay=3, wpe_per_array=True,
                               multiarray=True)
        assert type(enh.bf_block) is core.Beamformer and enh._fusable()
        assert enh._bf_wpd() == dict(taps=7, delay=3, iterations=1, power_floor=1e-3, ban=True)
        assert enh._params().bf == 0 and enh._params().wpe_taps == 7
        enh = mod.get_enhancer(bf='wpdSouden', bf_wpd_taps=5, bf_wpd_delay=1, bf_wpd_iterations=2,
                               bf_wpd_power_floor=0.01, wpe=False, postfilter='mask_mul')
        assert enh._bf_wpd() == dict(taps=5, delay=1, iterations=2, power_floor=0.01, ban=False)
        assert enh.bf_block == core.Beamformer('wpdSouden', 'mask_mul', wpd_taps=5, wpd_delay=1,
                                               wpd_iterations=2, wpd_power_floor=0.01)
        for kw, word in ((dict(bf_segment_frames=256), 'bf_segment_frames'),
                         (dict(bf_null_interferer=True), 'bf_null_interferer'),
                         (dict(channel_keep=3), 'channel_keep')):
            with pytest.raises(NotImplementedError, match=word):
                mod.get_enhancer(bf='wpdSouden_ban', **kw)
        # WPD settings with another beamformer are a combination nobody reads
        for bf in ('mvdrSouden_ban', 'gev_ban', 'ch2', 'sum'):
            with pytest.raises(NotImplementedError, match=bf):
                mod.get_enhancer(bf=bf, bf_wpd_iterations=2)
            with pytest.raises(NotImplementedError, match=bf):
                mod.get_enhancer(bf=bf, bf_wpd_taps=10)
        for kw, word in ((dict(bf_wpd_taps=0), 'taps'), (dict(bf_wpd_delay=-1), 'delay'),
                         (dict(bf_wpd_iterations=0), 'iterations'),
                         (dict(bf_wpd_power_floor=0.0), 'power_floor')):
            with pytest.raises(ValueError, match=word):
                mod.get_enhancer(bf='wpdSouden_ban', **kw)


def test_rttm_front_door_takes_the_type(tmp_path):
    from pb_chime5_amd import core
    from pb_chime5_amd.core_chime6_rttm import get_enhancer
    from test_rttm_frontdoor import _make_chime6_dir
    root, rttm, _ = _make_chime6_dir(tmp_path)
    kw = dict(database_rttm=[str(rttm)], activity_rttm=[str(rttm)], chime6_dir=root,
              multiarray='outer_array_mics')
    enh = get_enhancer(**kw, bf='wpdSouden_ban', bf_wpd_iterations=2)
    assert enh.bf_block == core.Beamformer('wpdSouden_ban', None, wpd_iterations=2)
    assert get_enhancer(**kw).bf_block == core.Beamformer('mvdrSouden_ban', None)


def test_command_lines_parse_the_keys(monkeypatch):
    from pb_chime5_amd.scripts import run, kaldi_run, kaldi_run_rttm, enhance_rttm
    cfg = run.main(['print_config', 'with', 'bf=wpdSouden_ban', 'bf_wpd_iterations=2',
                    'bf_wpd_taps=5', 'bf_wpd_power_floor=0.01'])
    assert (cfg['bf'], cfg['bf_wpd_iterations'], cfg['bf_wpd_taps'], cfg['bf_wpd_delay'],
            cfg['bf_wpd_power_floor']) == ('wpdSouden_ban', 2, 5, None, 0.01)
    cfg = run.main(['print_config'])
    assert (cfg['bf_wpd_taps'], cfg['bf_wpd_delay'], cfg['bf_wpd_iterations'],
            cfg['bf_wpd_power_floor']) == (None, None, 1, 1e-3)
    assert kaldi_run.main(['print_config', 'with', 'bf=wpdSouden_ban', 'bf_wpd_iterations=2'])[
        'bf_wpd_iterations'] == 2
    assert kaldi_run_rttm.main(['print_config', 'with', 'database_rttm=a.rttm',
                                'bf=wpdSouden', 'bf_wpd_delay=1'])['bf_wpd_delay'] == 1

    from pb_chime5_amd import core_chime6_rttm, parallel
    seen = {}

    class Stop(Exception):
        pass

    def fake_get_enhancer(**kw):
        seen.update(kw)
        raise Stop
    monkeypatch.setattr(core_chime6_rttm, 'get_enhancer', fake_get_enhancer)
    monkeypatch.setattr(parallel, 'init', lambda *a, **k: None)
    monkeypatch.setattr(parallel, 'device_index', lambda: 0)
    base = ['--chime6-dir', 'x', '--database-rttm', 'a.rttm', '--out', 'o']
    with pytest.raises(Stop):
        enhance_rttm.main(base + ['--bf', 'wpdSouden_ban', '--bf-wpd-taps', '5', '--bf-wpd-delay',
                                  '1', '--bf-wpd-iterations', '2', '--bf-wpd-power-floor', '0.01'])
    assert (seen['bf'], seen['bf_wpd_taps'], seen['bf_wpd_delay'], seen['bf_wpd_iterations'],
            seen['bf_wpd_power_floor']) == ('wpdSouden_ban', 5, 1, 2, 0.01)
    seen.clear()
    with pytest.raises(Stop):
        enhance_rttm.main(base)
    assert (seen['bf_wpd_taps'], seen['bf_wpd_delay'], seen['bf_wpd_iterations'],
            seen['bf_wpd_power_floor']) == (None, None, 1, 1e-3)


def test_guided_multi_target_and_activity_methods_refuse_the_type(no_context, tmp_path):
    from pb_chime5_amd.core import get_enhancer
    enh = get_enhancer(bf='wpdSouden_ban')
    obs = np.zeros((4, 4096))
    act = {'P01': np.ones(4096, bool), 'Noise': np.ones(4096, bool)}
    with pytest.raises(NotImplementedError, match='wpdSouden_ban'):
        enh.enhance_observation_guided(obs, {'P01': np.ones(19), 'Noise': np.ones(19)}, 'P01')
    with pytest.raises(NotImplementedError, match='wpdSouden_ban'):
        enh.enhance_observation_speakers(obs, act, ['P01'])
    with pytest.raises(NotImplementedError, match='wpdSouden_ban'):
        enh.enhance_example_speakers({})
    with pytest.raises(NotImplementedError, match='wpdSouden_ban'):
        enh.enhance_observation_activity(obs, act, 'P01')
    with pytest.raises(NotImplementedError, match='wpdSouden_ban'):
        enh.enhance_example_activity({})
    with pytest.raises(NotImplementedError, match='refined_rttm'):
        enh.enhance_session('S02', tmp_path / 'audio', refined_rttm=True)
    assert not (tmp_path / 'audio').exists()


def test_session_takes_one_utterance_at_a_time(monkeypatch, tmp_path):
    """The pipelined pcm16 path is out of the WPD's scope: `_enhance_and_write` goes through
    `enhance_example`, as it does for the segment-wise beamformer."""
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import get_enhancer
    enh = get_enhancer(bf='wpdSouden_ban')
    assert enh.inflight > 1 and enh._fusable()
    done = []
    monkeypatch.setattr(type(enh), 'enhance_example', lambda self, ex: done.append(ex) or 'x')
    monkeypatch.setattr(type(enh), '_write', lambda self, ex, x, d: done.append((ex, x)))

    def boom(*a, **k):
        raise AssertionError('the pipelined path')
    monkeypatch.setattr(ops, 'UtterancePipeline', boom)
    enh._enhance_and_write([{'example_id': 'a'}, {'example_id': 'b'}], tmp_path)
    assert done == [{'example_id': 'a'}, ({'example_id': 'a'}, 'x'),
                    {'example_id': 'b'}, ({'example_id': 'b'}, 'x')]


def test_fused_call_gets_the_settings_and_the_block_path_the_raw_stft(monkeypatch):
    from pb_chime5_amd import core, ops
    seen = {}

    def fake(obs, activity, target, start, end, **kw):
        seen.update(kw, target=target, start=start, end=end)
        return np.zeros(8)
    monkeypatch.setattr(ops, 'enhance_observation_wpd', fake)

    class Ctx:
        def set_utterances_in_flight(self, n):
            pass
    monkeypatch.setattr(core.Enhancer, '_ctx', lambda self: Ctx())
    enh = core.get_enhancer(bf='wpdSouden', wpe_tabs=4, bf_wpd_iterations=3, bf_wpd_power_floor=0.5,
                            bf_drop_context=False)
    act = {'P01': np.ones(4096, bool), 'P02': np.ones(4096, bool), 'Noise': np.ones(4096, bool)}
    enh.enhance_observation(np.zeros((4, 4096)), act, 'P02')
    assert (seen['taps'], seen['delay'], seen['iterations'], seen['power_floor'], seen['ban']) == \
        (4, 2, 3, 0.5, False)
    assert (seen['target'], seen['start'], seen['end'], seen['wpe_arrays']) == (1, 0, 0, 1)
    assert seen['params'].bf == 0 and seen['params'].wpe_taps == 4

    # the block path: the beamformer block gets the STFT before WPE and the gate of the context
    calls = []
    enh = core.get_enhancer(bf='wpdSouden_ban', stft_size=64, stft_shift=16)
    T, F = 30, 33
    raw = np.full((4, T, F), 2 + 0j)
    monkeypatch.setattr(core.Enhancer, 'stft', lambda self, x: raw)
    monkeypatch.setattr(core.Enhancer, 'istft', lambda self, X: X)
    monkeypatch.setattr(core.Enhancer, '_blocks_wpe', lambda self, Obs, debug, A: Obs * 0.5)
    monkeypatch.setattr(core, 'activity_time_to_frequency', lambda a, **k: np.ones((3, T), bool))
    monkeypatch.setattr(core.GSS, '__call__',
                        lambda self, Obs, act, debug=False: np.full((3, T, F), 1 / 3))
    monkeypatch.setattr(core.Beamformer, '__call__',
                        lambda self, Obs, **kw: calls.append((Obs, kw)) or kw['target_mask'])
    ex = dict(start_orig=64, start=0, end=4096, end_orig=4096 - 48)
    out = enh.enhance_observation(np.zeros((4, 4096)), act, 'P01', ex=ex, fused=False)
    Obs, kw = calls[0]
    assert np.all(Obs == 1 + 0j) and kw['raw_obs'] is raw
    sf, ef = core.start_end_context_frames(ex, 64, 16, True)
    assert sf > 0 and ef > 0
    assert np.array_equal(kw['frame_gate'], wr.context_gate(T, sf, ef))
    assert np.all(out[:sf] == 0) and np.all(out[sf:T - ef] == 1 / 3)
