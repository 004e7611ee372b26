"""Envelope-variance channel selection (gss_channel_scores, gss_select_channels,
gss_enhance_observation_select, get_enhancer(channel_keep=...)): the C ABI, the argument checks,
the band table, the parameter plumbing and the NumPy reference itself, without a GPU."""
import ctypes
import inspect
import math

import numpy as np
import pytest

from conftest import REPO

import channel_select_reference as ref

SYMBOLS = ('gss_channel_scores', 'gss_select_channels', 'gss_last_selected_channels',
           'gss_enhance_observation_select', 'gss_enhance_observation_select_pcm16')


def test_the_built_library_exports_the_selection_entry_points():
    from pb_chime5_amd import _capi
    lib = _capi.load_library()
    header = (REPO / 'include' / 'gss_hip.h').read_text()
    for name in SYMBOLS:
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
        assert f'int {name}(' in header, name
    # entry points only: the revision is the one the per-array WPE pinned
    assert _capi.GSS_ABI_VERSION == 7 and lib.gss_abi_version() == 7
    assert '#define GSS_ABI_VERSION 7' in header


def test_descriptor_layout_is_the_header_struct():
    from pb_chime5_amd import _capi
    header = (REPO / 'include' / 'gss_hip.h').read_text()
    for decl in ('const double *bank_dev;', 'int32_t bands;', 'int32_t keep;', 'double floor;',
                 '} gss_channel_select;'):
        assert decl in header, decl
    order = [header.index(d) for d in ('const double *bank_dev;', 'int32_t bands;',
                                       'int32_t keep;', 'double floor;', '} gss_channel_select;')]
    assert order == sorted(order)
    S = _capi.GssChannelSelect
    assert [n for n, _ in S._fields_] == ['bank_dev', 'bands', 'keep', 'floor']
    assert (S.bank_dev.offset, S.bands.offset, S.keep.offset, S.floor.offset) == (0, 8, 12, 16)
    assert ctypes.sizeof(S) == 24
    # the existing descriptors keep their layouts
    assert ctypes.sizeof(_capi.GssParams) == 14 * 4
    assert ctypes.sizeof(_capi.GssDebugTaps) == 7 * ctypes.sizeof(ctypes.c_void_p)


@pytest.fixture
def no_context(monkeypatch):
    """Any attempt to create or fetch a device context fails the test."""
    from pb_chime5_amd import _capi, ops

    def boom(*a, **k):
        raise AssertionError('device work before the argument check')
    monkeypatch.setattr(_capi, 'default_context', boom)
    monkeypatch.setattr(ops, 'default_context', boom)
    monkeypatch.setattr(_capi.Context, '__init__', boom)


BAD_KEEP = [0, -1, True, False, '3', '0.8', None, float('nan'), 0.0, -0.5, 1.5, 2.0, np.nan,
            np.float64(0.0), np.int64(0), [3], float('inf')]


@pytest.mark.parametrize('keep', BAD_KEEP, ids=repr)
def test_bad_keep_is_a_value_error_before_any_device_work(no_context, keep):
    from pb_chime5_amd import ops
    with pytest.raises(ValueError, match='keep'):
        ops.check_channel_keep(keep, 8)
    with pytest.raises(ValueError, match='keep'):
        ops.select_channels(np.zeros((4, 20, 5), complex), keep)
    with pytest.raises(ValueError, match='keep'):
        ops.enhance_observation_select(np.zeros((4, 4096)), np.ones((2, 4096), bool), 0, 0, 0,
                                       keep=keep)
    if keep is not None:            # (None is "no selection" for the enhancer)
        from pb_chime5_amd.core import get_enhancer
        with pytest.raises(ValueError, match='keep'):
            get_enhancer(channel_keep=keep)


def test_keep_counts_and_shares():
    from pb_chime5_amd import ops
    assert [ops.check_channel_keep(k, 24) for k in (1, 20, 24, 25, 1000, np.int32(7))] == \
        [1, 20, 24, 24, 24, 7]
    for D in range(1, 33):
        assert ops.check_channel_keep(1.0, D) == D
        assert ops.check_channel_keep(0.8, D) == max(1, math.ceil(round(0.8 * D, 9))), D
        assert ops.check_channel_keep(1e-6, D) == 1
        assert ops.check_channel_keep(np.float64(0.5), D) == max(1, math.ceil(D / 2))
    # ceil of the share: 0.8 of 24 is 19.2 -> 20; 0.8 of 20 is 16 (not 17: 0.8 * 20 in float64
    # is 16.000000000000004)
    assert ops.check_channel_keep(0.8, 24) == 20 and ops.check_channel_keep(0.8, 20) == 16
    assert ops.check_channel_keep(0.75, 12) == 9
    # without a channel count the value is only checked
    assert ops.check_channel_keep(5) == 5 and ops.check_channel_keep(0.25) == 0.25


@pytest.mark.parametrize('bad,name', [
    (dict(bands=0), 'bands'), (dict(bands=65), 'bands'), (dict(bands=4.0), 'bands'),
    (dict(bands=True), 'bands'), (dict(bands='4'), 'bands'), (dict(bands=None), 'bands'),
    (dict(floor=-1e-3), 'floor'), (dict(floor=1.0), 'floor'), (dict(floor=np.nan), 'floor'),
    (dict(floor=np.inf), 'floor'), (dict(floor='0'), 'floor'), (dict(floor=True), 'floor'),
    (dict(floor=None), 'floor'),
    (dict(bank=np.ones((3, 4))), 'bank'), (dict(bank=np.ones((65, 5))), 'bank'),
    (dict(bank=np.ones(5)), 'bank'), (dict(bank=np.ones((0, 5))), 'bank'),
    (dict(bank=-np.ones((3, 5))), 'bank'), (dict(bank=np.full((3, 5), np.nan)), 'bank'),
    (dict(bank=np.ones((2, 3, 5))), 'bank'), (dict(bank='mel'), 'bank'),
], ids=lambda v: v if isinstance(v, str) else ','.join(
    f'{k}={getattr(x, "shape", x)!r}' for k, x in v.items()))
def test_bad_settings_are_value_errors_before_any_device_work(no_context, bad, name):
    from pb_chime5_amd import ops
    Y = np.zeros((4, 20, 5), complex)
    with pytest.raises(ValueError, match=name):
        ops.channel_scores(Y, **bad)
    with pytest.raises(ValueError, match=name):
        ops.select_channels(Y, 2, **bad)
    if 'bank' not in bad:
        with pytest.raises(ValueError, match=name):
            ops.enhance_observation_select(np.zeros((4, 4096)), np.ones((2, 4096), bool), 0, 0,
                                           0, keep=2, **bad)
    if 'bands' in bad:
        with pytest.raises(ValueError, match=name):
            ops.mel_bank(bad['bands'], 1024)


def test_other_argument_errors_before_any_device_work(no_context):
    from pb_chime5_amd import ops
    with pytest.raises(ValueError, match='Obs'):
        ops.channel_scores(np.zeros((20, 5), complex))
    with pytest.raises(ValueError, match='Obs'):
        ops.select_channels(np.zeros((4, 0, 5), complex), 2)
    with pytest.raises(ValueError, match='obs'):
        ops.enhance_observation_select(np.zeros(4096), np.ones((2, 4096), bool), 0, 0, 0, keep=2)
    with pytest.raises(ValueError, match='bank'):       # a bank for another STFT size
        ops.enhance_observation_select(np.zeros((4, 4096)), np.ones((2, 4096), bool), 0, 0, 0,
                                       keep=2, bank=np.ones((3, 5)))
    with pytest.raises(TypeError):                      # keep is required
        ops.enhance_observation_select(np.zeros((4, 4096)), np.ones((2, 4096), bool), 0, 0, 0)
    for size in (0, 1, 1023, 512.0, '1024', True):
        with pytest.raises(ValueError, match='stft_size'):
            ops.mel_bank(40, size)
    for rate in (0, -16000, np.nan, '16000'):
        with pytest.raises(ValueError, match='sample_rate'):
            ops.mel_bank(40, 1024, rate)
    with pytest.raises(NotImplementedError, match='ch2'):
        ops.enhance_observation_select(np.zeros((4, 4096)), np.ones((2, 4096), bool), 0, 0, 0,
                                       keep=3, bf='ch2')
    with pytest.raises(NotImplementedError, match='wpe_arrays'):
        ops.enhance_observation_select(np.zeros((4, 4096)), np.ones((2, 4096), bool), 0, 0, 0,
                                       keep=3, wpe_arrays=2)


def test_signatures_and_defaults():
    from pb_chime5_amd import ops
    sig = inspect.signature(ops.channel_scores).parameters
    assert list(sig)[:5] == ['Obs', 'bank', 'bands', 'floor', 'return_band_variances']
    assert (sig['bank'].default, sig['bands'].default, sig['floor'].default,
            sig['return_band_variances'].default, sig['ctx'].default) == \
        (None, 40, 1e-10, False, None)
    sig = inspect.signature(ops.select_channels).parameters
    assert list(sig)[:2] == ['Obs', 'keep'] and sig['keep'].default is inspect.Parameter.empty
    sig = inspect.signature(ops.enhance_observation_select).parameters
    assert sig['keep'].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig['keep'].default is inspect.Parameter.empty
    assert inspect.signature(ops.mel_bank).parameters['sample_rate'].default == 16000
    for fn, name in ((ops.ResidentUtterance.enqueue, 'channel_select'),
                     (ops.UtterancePipeline.enqueue_staged, 'channel_select')):
        assert inspect.signature(fn).parameters[name].default is None


# ------------------------------------------------------------------ the band table
def test_mel_bank():
    from pb_chime5_amd import ops
    W = ops.mel_bank(40, 1024)
    assert W.shape == (40, 513) and W.dtype == np.float64
    assert np.all(W >= 0) and np.all(np.isfinite(W))
    for b, row in enumerate(W):
        peak = int(np.argmax(row))
        assert 0 < row[peak] <= 1, b
        assert np.sum(row == row[peak]) == 1, b                # one maximum ...
        assert np.all(np.diff(row[:peak + 1]) >= 0), b          # ... reached by a rise ...
        assert np.all(np.diff(row[peak:]) <= 0), b              # ... left by a fall
    for b in range(39):
        assert np.any((W[b] > 0) & (W[b + 1] > 0)), b           # neighbours overlap
        assert np.argmax(W[b]) < np.argmax(W[b + 1]), b
    # the outer edges are 0 and sample_rate / 2 (the latter through the mel scale and back)
    assert np.all(W[:, 0] == 0) and np.all(W[:, -1] < 1e-12)
    assert np.max(np.abs(W - ref.mel_bank(40, 1024))) <= 1e-15
    for bands, size, rate in ((1, 16, 16000), (8, 64, 8000), (64, 4096, 48000), (23, 512, 16000)):
        got = ops.mel_bank(bands, size, rate)
        assert got.shape == (bands, size // 2 + 1)
        assert np.max(np.abs(got - ref.mel_bank(bands, size, rate))) <= 1e-15
    # the HTK mel scale: the middle edge of one band over 0 .. 8 kHz
    one = ops.mel_bank(1, 4096)
    mid = 700.0 * (10.0 ** (0.5 * 2595.0 * np.log10(1 + 8000 / 700.0) / 2595.0) - 1.0)
    assert abs(np.argmax(one[0]) * 16000 / 4096 - mid) <= 16000 / 4096


def test_channel_select_object():
    from pb_chime5_amd import ops
    sel = ops.ChannelSelect(0.8, 513)
    assert sel.bands == 40 and sel.floor == 1e-10 and sel.keep == 0.8
    assert np.array_equal(sel.bank, ops.mel_bank(40, 1024))
    assert sel.count(24) == 20 and sel.count(4) == 4 and sel.count(1) == 1
    bank = np.abs(np.random.default_rng(0).standard_normal((3, 9)))
    sel = ops.ChannelSelect(5, 9, bank, floor=0)
    assert sel.bands == 3 and sel.count(4) == 4 and sel.count(12) == 5 and sel.floor == 0.0
    assert np.array_equal(sel.bank, bank) and sel.bank.flags.c_contiguous


# ------------------------------------------------------------------ plumbing
def test_every_front_door_has_the_selection_off_by_default_and_carries_it():
    from pb_chime5_amd import core, core_chime6, core_chime6_rttm
    for mod in (core, core_chime6, core_chime6_rttm):
        sig = inspect.signature(mod.get_enhancer).parameters
        assert (sig['channel_keep'].default, sig['channel_bands'].default) == (None, 40), mod
    sig = inspect.signature(core.Enhancer).parameters
    assert (sig['channel_keep'].default, sig['channel_bands'].default) == (None, 40)
    for mod in (core, core_chime6):
        enh = mod.get_enhancer()
        assert enh.channel_keep is None and enh._channel_select() is None
        enh = mod.get_enhancer(channel_keep=0.8, channel_bands=24, multiarray=True)
        assert (enh.channel_keep, enh.channel_bands) == (0.8, 24) and enh._fusable()
        sel = enh._channel_select()
        assert sel is enh._channel_select()             # one object: one copy of its table in HBM
        assert sel.bands == 24 and sel.bank.shape == (24, 513) and sel.count(24) == 20
        assert mod.get_enhancer(channel_keep=20).channel_keep == 20
        assert mod.get_enhancer(channel_keep=3, stft_size=512, stft_shift=128) \
            ._channel_select().bank.shape == (40, 257)
        with pytest.raises(ValueError, match='bands'):
            mod.get_enhancer(channel_keep=3, channel_bands=65)


def test_rttm_front_door_takes_the_selection(tmp_path):
    from pb_chime5_amd.core_chime6_rttm import get_enhancer
    from test_rttm_frontdoor import _make_chime6_dir
    root, rttm, _ = _make_chime6_dir(tmp_path)
    kw = dict(database_rttm=[str(rttm)], activity_rttm=[str(rttm)], chime6_dir=root,
              multiarray='outer_array_mics')
    enh = get_enhancer(**kw, channel_keep=0.75)
    assert enh.channel_keep == 0.75 and enh._channel_select().count(12) == 9
    assert get_enhancer(**kw).channel_keep is None
    with pytest.raises(NotImplementedError, match='wpe_per_array'):
        get_enhancer(**kw, channel_keep=4, wpe_per_array=True)


def test_forbidden_combinations_raise_when_the_object_is_built():
    from pb_chime5_amd import core, core_chime6
    for mod in (core, core_chime6):
        with pytest.raises(NotImplementedError, match='wpe_per_array'):
            mod.get_enhancer(channel_keep=0.8, wpe_per_array=True, multiarray=True)
        with pytest.raises(NotImplementedError, match='ch2'):
            mod.get_enhancer(channel_keep=0.8, bf='ch2')
        with pytest.raises(NotImplementedError, match='bf_segment_frames'):
            mod.get_enhancer(channel_keep=0.8, bf_segment_frames=256)
        # each of them alone is still fine
        mod.get_enhancer(wpe_per_array=True, multiarray=True)
        mod.get_enhancer(bf='ch2')
        mod.get_enhancer(bf_segment_frames=256)
        mod.get_enhancer(channel_keep=0.8, bf='sum')
        mod.get_enhancer(channel_keep=0.8, bf='gev_ban', postfilter='mask_mul')


def test_guided_and_multi_speaker_methods_refuse_the_selection(no_context):
    from pb_chime5_amd.core import get_enhancer
    enh = get_enhancer(channel_keep=3)
    obs = np.zeros((4, 4096))
    act = {'P01': np.ones(4096, bool), 'Noise': np.ones(4096, bool)}
    with pytest.raises(NotImplementedError, match='channel_keep'):
        enh.enhance_observation_guided(obs, {'P01': np.ones(19), 'Noise': np.ones(19)}, 'P01')
    with pytest.raises(NotImplementedError, match='channel_keep'):
        enh.enhance_observation_speakers(obs, act, ['P01'])
    with pytest.raises(NotImplementedError, match='channel_keep'):
        enh.enhance_example_speakers({})


def test_command_lines_parse_the_keys(monkeypatch):
    from pb_chime5_amd.scripts import run, kaldi_run, kaldi_run_rttm, enhance_rttm
    cfg = run.main(['print_config', 'with', 'channel_keep=0.75', 'channel_bands=24'])
    assert (cfg['channel_keep'], cfg['channel_bands']) == (0.75, 24)
    cfg = run.main(['print_config'])
    assert (cfg['channel_keep'], cfg['channel_bands']) == (None, 40)
    cfg = kaldi_run.main(['print_config', 'with', 'channel_keep=20'])
    assert cfg['channel_keep'] == 20 and type(cfg['channel_keep']) is int
    cfg = kaldi_run_rttm.main(['print_config', 'with', 'database_rttm=a.rttm',
                               'channel_keep=0.8'])
    assert cfg['channel_keep'] == 0.8

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
    for text, want in (('0.8', 0.8), ('20', 20)):
        with pytest.raises(Stop):
            enhance_rttm.main(base + ['--channel-keep', text, '--channel-bands', '32'])
        assert (seen['channel_keep'], seen['channel_bands']) == (want, 32)
        assert type(seen['channel_keep']) is type(want)
        seen.clear()
    with pytest.raises(Stop):
        enhance_rttm.main(base)
    assert (seen['channel_keep'], seen['channel_bands']) == (None, 40)


def test_session_stays_pipelined_with_the_selection(tmp_path, monkeypatch):
    """`_enhance_and_write` keeps its pipelined path for an enhancer with channel_keep (unlike
    the segment-wise beamformer) and hands the selection to every enqueue_staged."""
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import get_enhancer
    enh = get_enhancer(channel_keep=0.75)
    assert enh.inflight > 1 and enh._fusable()

    class Taken(Exception):
        pass

    def pipeline(*a, **k):
        raise Taken
    monkeypatch.setattr(ops, 'UtterancePipeline', pipeline)
    monkeypatch.setattr(type(enh), '_ctx', lambda self: None)
    monkeypatch.setattr(type(enh), 'enhance_example',
                        lambda self, ex: pytest.fail('one utterance at a time'))
    with pytest.raises(Taken):
        enh._enhance_and_write(['a', 'b'], tmp_path)


# ------------------------------------------------------------------ the reference itself
SCENES = [(4, 100, 6, 3), (5, 37, 4, 2), (7, 200, 17, 5), (12, 333, 33, 8), (29, 150, 9, 4)]


def _bank(B, F):
    return ref.random_bank(np.random.default_rng(100 * B + F), B, F)


@pytest.mark.parametrize('D,T,F,B', SCENES)
def test_reference_scores_are_bounded_and_gain_invariant(D, T, F, B):
    """Scores lie in [0, B] and do not depend on a channel's gain: 1e-12 (measured: at most
    7e-15 on these scenes under gains of 10^-3 / 10^3)."""
    Y, W = ref.scene(D, T, F), _bank(B, F)
    s, V = ref.channel_scores(Y, W)
    assert s.shape == (D,) and V.shape == (B, D)
    assert np.all(s >= 0) and np.all(s <= B) and np.all(V >= 0)
    assert np.isclose(np.max(V / V.max(axis=1, keepdims=True), axis=1), 1).all()
    gain = 10.0 ** np.random.default_rng(D).choice([-3.0, 3.0], size=D)
    s2, _ = ref.channel_scores(Y * gain, W)
    dev = np.max(np.abs(s2 - s) / s)
    print(f'gain deviation {dev:.1e}')
    assert dev < 1e-12
    for keep in (1, math.ceil(0.8 * D), D - 1, D):
        assert np.array_equal(ref.pick(s2, keep), ref.pick(s, keep))


def test_reference_dead_channel_scores_zero_and_ranks_last():
    D, T, F, B = 7, 200, 17, 5
    Y, W = ref.scene(D, T, F), _bank(B, F)
    Y[:, :, 3] = 0
    s, V = ref.channel_scores(Y, W)
    assert s[3] == 0.0 and np.all(V[:, 3] == 0.0) and np.all(np.isfinite(s))
    assert np.all(np.delete(s, 3) > 0)
    assert 3 not in ref.pick(s, D - 1) and list(ref.pick(s, D)) == list(range(D))
    # an all-zero band row contributes nothing
    W0 = W.copy()
    W0[2] = 0
    s0, V0 = ref.channel_scores(Y, W0)
    assert np.all(V0[2] == 0)
    assert np.allclose(s0, ref.scores_from_variances(np.delete(V, 2, axis=0)), rtol=1e-13)
    # everything dead: all scores 0, the lowest indices are kept
    sz, _ = ref.channel_scores(np.zeros_like(Y), W)
    assert np.all(sz == 0) and list(ref.pick(sz, 3)) == [0, 1, 2]


def test_reference_pick_rules():
    assert list(ref.pick([0.1, 0.9, 0.5, 0.7], 2)) == [1, 3]           # ascending channel order
    assert list(ref.pick([3.0, 1.0, 3.0, 3.0, 2.0], 2)) == [0, 2]      # ties: the lower index
    assert list(ref.pick([3.0, 1.0, 3.0, 3.0, 2.0], 4)) == [0, 2, 3, 4]
    assert list(ref.pick([np.nan, 0.0, np.inf, 1.0], 2)) == [1, 3]     # non-finite below finite
    assert list(ref.pick([np.nan, 0.0, np.inf, 1.0], 3)) == [0, 1, 3]  # ... and by index among them
    assert list(ref.pick([np.nan, 0.0, -np.inf, 1.0], 4)) == [0, 1, 2, 3]
    assert list(ref.pick([5.0], 1)) == [0]
    for keep in range(1, 9):
        got = ref.pick(np.random.default_rng(keep).uniform(size=8), keep)
        assert len(got) == keep and np.all(np.diff(got) > 0)
    assert ref.boundary_gap([1.0, 0.5, 0.25], 1) == 0.5
    assert ref.boundary_gap([1.0, 0.5, 0.25], 3) == np.inf


def test_reference_select_gathers_in_channel_order():
    D, T, F, B = 5, 37, 4, 2
    Y, W = ref.scene(D, T, F), _bank(B, F)
    Ysel, channels = ref.select(Y, W, 3)
    assert Ysel.shape == (F, T, 3) and np.all(np.diff(channels) > 0)
    assert np.array_equal(Ysel, Y[:, :, channels])
