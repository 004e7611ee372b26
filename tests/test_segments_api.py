"""Segment-wise MVDR (gss_mvdr_souden_segments, get_enhancer(bf_segment_frames=...)): the C
ABI, the argument checks, the parameter plumbing and the front doors, without a GPU."""
import ctypes
import inspect

import numpy as np
import pytest

from conftest import REPO

SYMBOLS = ('gss_mvdr_souden_segments', 'gss_enhance_observation_segments',
           'gss_last_segment_fallbacks')


def test_the_built_library_exports_the_segment_entry_points():
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
    for decl in ('int64_t segment_frames;', 'int32_t context_segments;', 'double min_mass;',
                 '} gss_bf_segments;'):
        assert decl in header, decl
    S = _capi.GssBfSegments
    assert [n for n, _ in S._fields_] == ['segment_frames', 'context_segments', 'min_mass']
    assert (S.segment_frames.offset, S.context_segments.offset, S.min_mass.offset) == (0, 8, 16)
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


BAD_SEGMENTS = [
    dict(segment_frames=0), dict(segment_frames=-64), dict(segment_frames=63),
    dict(segment_frames=100), dict(segment_frames=64.0), dict(segment_frames=True),
    dict(segment_frames='64'), dict(segment_frames=None),
    dict(segment_frames=64, segment_context=-1), dict(segment_frames=64, segment_context=0.5),
    dict(segment_frames=64, segment_context=True),
    dict(segment_frames=64, min_mass=-1.0), dict(segment_frames=64, min_mass=np.nan),
    dict(segment_frames=64, min_mass=np.inf), dict(segment_frames=64, min_mass='8'),
]


@pytest.mark.parametrize('bad', BAD_SEGMENTS, ids=lambda b: ','.join(f'{k}={v!r}' for k, v in b.items()))
def test_bad_segment_settings_are_value_errors_before_any_device_work(no_context, bad):
    from pb_chime5_amd import ops
    Y = np.zeros((4, 130, 3), complex)
    m = np.zeros((130, 3))
    name = [k for k in bad if k != 'segment_frames' or len(bad) == 1][-1]
    with pytest.raises(ValueError, match=name):
        ops.mvdr_souden_segments_from_masks(Y, m, m, **bad)
    with pytest.raises(ValueError, match=name):
        ops.enhance_observation_segments(np.zeros((4, 4096)), np.ones((2, 4096), bool), 0, 0, 0,
                                         **bad)


def test_other_argument_errors_before_any_device_work(no_context):
    from pb_chime5_amd import ops
    Y = np.zeros((4, 130, 3), complex)
    m = np.zeros((130, 3))
    with pytest.raises(TypeError):          # segment_frames is required
        ops.mvdr_souden_segments_from_masks(Y, m, m)
    with pytest.raises(ValueError, match='Y'):
        ops.mvdr_souden_segments_from_masks(Y[0], m, m, segment_frames=64)
    with pytest.raises(ValueError, match='X_mask'):
        ops.mvdr_souden_segments_from_masks(Y, m[:-1], m, segment_frames=64)
    with pytest.raises(ValueError, match='N_mask'):
        ops.mvdr_souden_segments_from_masks(Y, m, m.T, segment_frames=64)
    for ref in (-1, 4):
        with pytest.raises(ValueError, match='ref_channel'):
            ops.mvdr_souden_segments_from_masks(Y, m, m, segment_frames=64, ref_channel=ref)
    with pytest.raises(ValueError, match='obs'):
        ops.enhance_observation_segments(np.zeros(4096), np.ones((2, 4096), bool), 0, 0, 0,
                                         segment_frames=64)
    for bf in ('gev_ban', 'ch2', 'sum'):
        with pytest.raises(NotImplementedError, match=bf):
            ops.enhance_observation_segments(np.zeros((4, 4096)), np.ones((2, 4096), bool), 0,
                                             0, 0, segment_frames=64, bf=bf)


def test_min_mass_defaults_to_twice_the_channels():
    from pb_chime5_amd import ops
    seg = ops.check_bf_segments(256, 1, None, 12)
    assert (seg.segment_frames, seg.context_segments, seg.min_mass) == (256, 1, 24.0)
    assert ops.check_bf_segments(64, 0, 0, 12).min_mass == 0.0
    assert ops.check_bf_segments(np.int64(128), np.int32(2), 8, 12).min_mass == 8.0
    sig = inspect.signature(ops.mvdr_souden_segments_from_masks).parameters
    assert sig['segment_frames'].default is inspect.Parameter.empty
    assert sig['segment_frames'].kind is inspect.Parameter.KEYWORD_ONLY
    assert (sig['ban'].default, sig['segment_context'].default, sig['min_mass'].default,
            sig['ref_channel'].default, sig['return_ref_channel'].default,
            sig['return_fallbacks'].default) == (False, 0, None, None, False, False)
    assert 'a choice, not a measurement' in ops.mvdr_souden_segments_from_masks.__doc__


def test_beamformer_defaults_are_untouched():
    from pb_chime5_amd.core import Beamformer
    from pb_chime5_amd.speech_enhancement import beamforming_wrapper
    bf = Beamformer('mvdrSouden_ban', None)
    assert (bf.type, bf.postfilter) == ('mvdrSouden_ban', None)
    assert (bf.segment_frames, bf.segment_context, bf.segment_min_mass) == (None, 0, None)
    assert bf.segments is None
    assert bf == Beamformer(type='mvdrSouden_ban', postfilter=None)
    assert bf != Beamformer('mvdrSouden_ban', None, segment_frames=256)
    # every type is still constructible without segments
    for t in ('gev_ban', 'ch2', 'sum'):
        assert Beamformer(t, 'mask_mul').segments is None
    sig = inspect.signature(beamforming_wrapper.beamform_mvdr_souden_from_masks).parameters
    assert (sig['segment_frames'].default, sig['segment_context'].default,
            sig['segment_min_mass'].default) == (None, 0, None)
    assert sig['segment_frames'].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(sig)[:4] == ['Y', 'X_mask', 'N_mask', 'ban']


def test_beamformer_with_segments():
    from pb_chime5_amd.core import Beamformer
    bf = Beamformer('mvdrSouden_ban', None, segment_frames=256, segment_context=1)
    assert bf.segments == dict(segment_frames=256, segment_context=1, min_mass=None)
    for t in ('gev_ban', 'ch2', 'sum', 'nonsense'):
        with pytest.raises(NotImplementedError, match=t):
            Beamformer(type=t, postfilter=None, segment_frames=256)
    with pytest.raises(ValueError, match='segment_frames'):
        Beamformer('mvdrSouden_ban', None, segment_frames=100)
    with pytest.raises(ValueError, match='segment_context'):
        Beamformer('mvdrSouden_ban', None, segment_frames=128, segment_context=-2)
    with pytest.raises(ValueError, match='min_mass'):
        Beamformer('mvdrSouden_ban', None, segment_frames=128, segment_min_mass=-1)


def test_every_front_door_has_segments_off_by_default_and_carries_them():
    from pb_chime5_amd import core, core_chime6, core_chime6_rttm
    for mod in (core, core_chime6, core_chime6_rttm):
        sig = inspect.signature(mod.get_enhancer).parameters
        assert (sig['bf_segment_frames'].default, sig['bf_segment_context'].default,
                sig['bf_segment_min_mass'].default) == (None, 0, None), mod.__name__
    for mod in (core, core_chime6):
        assert mod.get_enhancer().bf_block == core.Beamformer('mvdrSouden_ban', None)
        enh = mod.get_enhancer(bf_segment_frames=256, bf_segment_context=1)
        assert type(enh.bf_block) is core.Beamformer and enh._fusable()
        assert enh.bf_block == core.Beamformer('mvdrSouden_ban', None, 256, 1, None)
        assert enh._bf_segments() == dict(segment_frames=256, segment_context=1, min_mass=None)
        assert mod.get_enhancer(bf_segment_frames=64, bf_segment_min_mass=3.5) \
            .bf_block.segment_min_mass == 3.5
        with pytest.raises(NotImplementedError, match='gev_ban'):
            mod.get_enhancer(bf='gev_ban', bf_segment_frames=256)


def test_rttm_front_door_takes_segments(tmp_path):
    from pb_chime5_amd import core
    from pb_chime5_amd.core_chime6_rttm import get_enhancer
    from test_rttm_frontdoor import _make_chime6_dir
    root, rttm, _ = _make_chime6_dir(tmp_path)
    kw = dict(database_rttm=[str(rttm)], activity_rttm=[str(rttm)], chime6_dir=root,
              multiarray='outer_array_mics')
    enh = get_enhancer(**kw, bf_segment_frames=256, bf_segment_context=1)
    assert enh.bf_block == core.Beamformer('mvdrSouden_ban', None, 256, 1, None)
    assert get_enhancer(**kw).bf_block == core.Beamformer('mvdrSouden_ban', None)


def test_command_lines_parse_the_keys(monkeypatch):
    from pb_chime5_amd.scripts import run, kaldi_run, kaldi_run_rttm, enhance_rttm
    cfg = run.main(['print_config', 'with', 'bf_segment_frames=256', 'bf_segment_context=1'])
    assert (cfg['bf_segment_frames'], cfg['bf_segment_context'],
            cfg['bf_segment_min_mass']) == (256, 1, None)
    cfg = run.main(['print_config'])
    assert (cfg['bf_segment_frames'], cfg['bf_segment_context'],
            cfg['bf_segment_min_mass']) == (None, 0, None)
    cfg = kaldi_run.main(['print_config', 'with', 'bf_segment_frames=128',
                          'bf_segment_min_mass=6.5'])
    assert (cfg['bf_segment_frames'], cfg['bf_segment_min_mass']) == (128, 6.5)
    cfg = kaldi_run_rttm.main(['print_config', 'with', 'database_rttm=a.rttm',
                               'bf_segment_frames=64', 'bf_segment_context=2'])
    assert (cfg['bf_segment_frames'], cfg['bf_segment_context']) == (64, 2)

    # enhance_rttm: the options reach get_enhancer
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
        enhance_rttm.main(base + ['--bf-segment-frames', '256', '--bf-segment-context', '1'])
    assert (seen['bf_segment_frames'], seen['bf_segment_context']) == (256, 1)
    seen.clear()
    with pytest.raises(Stop):
        enhance_rttm.main(base)
    assert (seen['bf_segment_frames'], seen['bf_segment_context']) == (None, 0)


def test_guided_and_multi_target_methods_refuse_segments(no_context):
    from pb_chime5_amd.core import get_enhancer
    enh = get_enhancer(bf_segment_frames=256)
    obs = np.zeros((4, 4096))
    act = {'P01': np.ones(4096, bool), 'Noise': np.ones(4096, bool)}
    with pytest.raises(NotImplementedError, match='bf_segment_frames'):
        enh.enhance_observation_guided(obs, {'P01': np.ones(19), 'Noise': np.ones(19)}, 'P01')
    with pytest.raises(NotImplementedError, match='bf_segment_frames'):
        enh.enhance_observation_speakers(obs, act, ['P01'])
    with pytest.raises(NotImplementedError, match='bf_segment_frames'):
        enh.enhance_example_speakers({})


def test_session_loop_is_one_utterance_at_a_time_with_segments(tmp_path, monkeypatch):
    """`_enhance_and_write` takes its one-at-a-time loop (enhance_example per example) for an
    enhancer with segments: the pipelined pcm16 path has no segment twin."""
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import get_enhancer
    enh = get_enhancer(bf_segment_frames=256)
    assert enh.inflight > 1 and enh._fusable()
    calls = []
    monkeypatch.setattr(type(enh), 'enhance_example', lambda self, ex: calls.append(ex) or 'x')
    monkeypatch.setattr(type(enh), '_write', lambda self, ex, x, d: calls.append((ex, x)))

    def no_pipeline(*a, **k):
        raise AssertionError('the pipelined path was taken')
    monkeypatch.setattr(ops, 'UtterancePipeline', no_pipeline)
    enh._enhance_and_write(['a', 'b'], tmp_path)
    assert calls == ['a', ('a', 'x'), 'b', ('b', 'x')]


def test_reference_helper_windows():
    """The NumPy reference's segment arithmetic (tests/segments_reference.py)."""
    from segments_reference import segment_windows
    assert segment_windows(300, 64, 0) == [((0, 64), (0, 64)), ((64, 128), (64, 128)),
                                           ((128, 192), (128, 192)), ((192, 256), (192, 256)),
                                           ((256, 300), (256, 300))]
    assert segment_windows(300, 64, 1)[0] == ((0, 64), (0, 128))
    assert segment_windows(300, 64, 1)[4] == ((256, 300), (192, 300))
    assert segment_windows(300, 64, 9) == [((a, min(a + 64, 300)), (0, 300))
                                           for a in range(0, 300, 64)]
    assert segment_windows(100, 128, 0) == [((0, 100), (0, 100))]
