"""Several targets of one stream without a GPU: the composed NumPy reference against the
single-target reference of tests/stream_reference.py, its independence of the cuts, the seeds of
the new cells, the argument errors of `StreamingEnhancer(targets=)` and `Enhancer.stream(targets=)`
-- all raised before the GPU is touched --, the checkpoint refusals and the new C-ABI rows."""
import numpy as np
import pytest

import stream_reference as sr
import stream_targets_reference as tr


def _equal_states(a, b, what):
    a, b = tr.state_arrays(a), tr.state_arrays(b)
    assert sorted(a) == sorted(b), what
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize('name', ['a', 'h'])
def test_row_s_is_the_single_target_reference_with_that_target(name, monkeypatch):
    x, activity = tr.scene(name, tr.seed_of(name))
    x_hat, taps, states = tr.reference(name, tr.seed_of(name))
    assert taps['fallbacks'] == ((0,) * len(tr.TARGETS[name]), 0)
    for s, target in enumerate(tr.TARGETS[name]):
        monkeypatch.setitem(sr.SETTINGS, 'target', target)
        one_x, one_taps, one_states = sr.compose_whole(name, x, activity)
        assert np.array_equal(x_hat[s], one_x), (name, target)
        for k in ('target_mask', 'distortion_mask', 'X_hat'):
            assert np.array_equal(taps[k][s], one_taps[k]), (name, target, k)
        for k in ('Obs', 'gamma'):
            assert np.array_equal(taps[k], one_taps[k]), (name, target, k)
        for k, v in one_states['bf'].items():
            assert np.array_equal(states['bf'][s][k], v), (name, target, k)
        for stage in ('wpe', 'em'):
            for k, v in (one_states[stage] or {}).items():
                assert np.array_equal(states[stage][k], v), (name, stage, k)
    # different targets are different signals
    assert not np.array_equal(x_hat[0], x_hat[1])


@pytest.mark.parametrize('name', ['a', 'm'])
def test_the_composed_reference_does_not_depend_on_the_cuts(name):
    x, activity = tr.scene(name, tr.seed_of(name))
    x_hat, taps, states = tr.reference(name, tr.seed_of(name))
    for part, cuts in tr.partitions(name).items():
        xs, ts, ss = tr.compose_stream(name, x, activity, tr.TARGETS[name], cuts)
        assert np.array_equal(xs, x_hat), (name, part)
        for k in ('Obs', 'gamma', 'target_mask', 'distortion_mask', 'X_hat'):
            assert np.array_equal(ts[k], taps[k]), (name, part, k)
        assert ts['fallbacks'] == taps['fallbacks']
        _equal_states(ss, states, (name, part))


@pytest.mark.parametrize('name', sorted(tr.SEEDS))
def test_the_new_cells_keep_the_first_stable_seed(name):
    assert tr.choose_seed(name) == tr.seed_of(name)
    moved, x_moved = tr.reference_movement(name, tr.seed_of(name))
    print(f'{name}: gamma / X_hat / states move {moved:.1e}, |x_hat| {x_moved:.1e}')
    assert moved * tr.STABILITY_MARGIN <= tr.TOL and x_moved * tr.STABILITY_MARGIN <= tr.X_TOL


@pytest.mark.parametrize('name', ['a', 'f', 'h'])
def test_the_shared_cells_are_stable_for_every_target(name):
    assert tr.is_stable(name, tr.seed_of(name))


def test_the_fallback_scene_separates_the_targets():
    import online_mvdr_reference as mref
    Y, gamma, state, beta, targets, counts = tr.fallback_scene()
    assert np.all(gamma >= 0) and np.all(np.isfinite(gamma)) and counts[1] > 0
    for target, count in zip(targets, counts):
        mx, mn = tr.masks(gamma, target)
        assert mref.online_mvdr(Y, mx, mn, beta, 0, True, state=state)[3] == count


# ------------------------------------------------------------------ the constructor
OK = dict(stft_size=64, stft_shift=16, wpe_taps=2, wpe_delay=1)


def test_constructor_errors_are_raised_before_the_gpu_is_touched():
    from pb_chime5_amd.streaming import StreamingEnhancer
    for bad, match in ((dict(targets=1), 'sequence'), (dict(targets='01'), 'sequence'),
                       (dict(targets=()), '1 to 8'), (dict(targets=[]), '1 to 8'),
                       (dict(targets=tuple(range(9)), num_classes=8), '1 to 8'),
                       (dict(targets=(0, 1, 0)), 'twice'), (dict(targets=(0, 3)), r'\[0, 3\)'),
                       (dict(targets=(-1,)), r'\[0, 3\)'), (dict(targets=(0.5,)), 'integer'),
                       (dict(targets=(True,)), 'integer'),
                       (dict(targets=(0, 1), target=1), 'together with target')):
        args = dict(num_channels=4, num_classes=3, **OK)
        args.update(bad)
        with pytest.raises(ValueError, match=match):
            StreamingEnhancer(**args)
    enh = StreamingEnhancer(4, 3, targets=[2, 0], **OK)
    assert enh.targets == (2, 0) and enh.target == 0 and enh.stream is None and enh.ctx is None
    assert enh.fallbacks == {'mvdr': 0, 'cacgmm': 0, 'mvdr_targets': [0, 0]}
    assert StreamingEnhancer(4, 8, targets=range(8), **OK).targets == tuple(range(8))
    # without targets nothing changes
    one = StreamingEnhancer(4, 3, target=1, **OK)
    assert one.targets is None and one.fallbacks == {'mvdr': 0, 'cacgmm': 0}


def test_a_stream_of_targets_that_took_nothing_ends_empty():
    from pb_chime5_amd.streaming import StreamingEnhancer
    enh = StreamingEnhancer(4, 3, targets=(0, 2), **OK)
    with pytest.raises(ValueError, match='block'):
        enh.process(np.zeros((3, 40)), np.ones((3, 40), bool))
    out, details = enh.flush(debug=True)
    assert out.shape == (2, 0) and details is None and enh.stream is None
    with pytest.raises(RuntimeError, match='reset'):
        enh.flush()


def test_check_online_targets():
    from pb_chime5_amd import ops
    assert ops.check_online_targets([np.int64(1), 0]) == (1, 0)
    assert ops.check_online_targets(np.array([3, 1]), 4) == (3, 1)
    with pytest.raises(ValueError, match='num_classes'):
        ops.check_online_targets((-1,))
    with pytest.raises(ValueError, match=r'\[0, 2\)'):
        ops.check_online_targets((2,), 2)


# ------------------------------------------------------------------ Enhancer.stream
def _get_enhancer(**kw):
    from pb_chime5_amd.core import get_enhancer
    args = dict(gss_online=True, bf_online=True, wpe_online=True)
    args.update(kw)
    return get_enhancer(**args)


def test_enhancer_stream_takes_names_and_indices():
    enh = _get_enhancer(stft_size=512, stft_shift=128, postfilter='mask_mul')
    s = enh.stream(6, ['P01', 'P02', 'Noise'], targets=['P02', 'P01'], ref_channel=2)
    assert (s.D, s.K, s.targets, s.ref_channel, s.postfilter) == (6, 3, (1, 0), 2, 'mask_mul')
    assert s.speakers == ['P01', 'P02', 'Noise'] and s.fused
    assert enh.stream(4, 3, targets=(2, 0), fused=False).targets == (2, 0)
    with pytest.raises(ValueError, match="'P03' is not one of speakers"):
        enh.stream(6, ['P01', 'P02'], targets=['P01', 'P03'])
    with pytest.raises(ValueError, match='sequence of names'):
        enh.stream(6, ['P01', 'P02'], targets='P01')
    with pytest.raises(ValueError, match='targets together with target'):
        enh.stream(6, ['P01', 'P02'], 'P01', targets=['P02'])
    with pytest.raises(ValueError, match='targets together with target'):
        enh.stream(6, 3, 1, targets=(0, 2))
    with pytest.raises(ValueError, match='twice'):
        enh.stream(6, 3, targets=(1, 1))
    with pytest.raises(ValueError, match='speakers'):
        enh.stream(6, targets=(0, 1))
    # the single target stays what it was
    assert enh.stream(6, 3, 2).targets is None and enh.stream(6, 3, 2).target == 2


def test_the_three_front_doors_take_the_keyword(tmp_path):
    from pb_chime5_amd import core, core_chime6, core_chime6_rttm
    from test_rttm_frontdoor import _make_chime6_dir
    root, rttm, _ = _make_chime6_dir(tmp_path)
    online = dict(gss_online=True, bf_online=True, wpe_online=True)
    doors = {'core': core.get_enhancer(**online),
             'core_chime6': core_chime6.get_enhancer(**online),
             'core_chime6_rttm': core_chime6_rttm.get_enhancer(
                 database_rttm=[str(rttm)], activity_rttm=[str(rttm)], chime6_dir=root,
                 multiarray='outer_array_mics', **online)}
    for name, enh in doors.items():
        s = enh.stream(4, ['P05', 'P06', 'Noise'], targets=['Noise', 'P05'])
        assert (s.D, s.K, s.targets, s.target) == (4, 3, (2, 0), 0), name
        assert enh.stream(4, 3, targets=[1]).targets == (1,), name
        with pytest.raises(ValueError, match='twice'):
            enh.stream(4, 3, targets=(0, 0))
        with pytest.raises(ValueError, match='targets together with target'):
            enh.stream(4, 3, 0, targets=(1,))


@pytest.mark.parametrize('setting,kw', [
    ('gss_online', dict(gss_online=False, bf_online=False, wpe_online=False)),
    ('bf_online', dict(bf_online=False, wpe_online=False)),
    ('wpe_online', dict(wpe_online=False)),
    ('stft_fading', dict(stft_fading=False)),
], ids=lambda v: v if isinstance(v, str) else '')
def test_enhancer_stream_keeps_its_refusals(setting, kw):
    with pytest.raises(NotImplementedError, match=f'stream with {setting}'):
        _get_enhancer(**kw).stream(4, 3, targets=(0, 1))


def test_enhancer_stream_keeps_refusing_the_whole_window_options():
    from pb_chime5_amd.core import get_enhancer
    cases = {
        "bf='ch2'": dict(gss_online=True, bf='ch2'),
        'channel_keep': dict(wpe_online=True, channel_keep=2),
        'bf_segment_frames': dict(wpe_online=True, bf_segment_frames=64),
        'bf_null_interferer': dict(wpe_online=True, bf_null_interferer=True),
        "bf='wpdSouden_ban'": dict(bf='wpdSouden_ban'),
    }
    for setting, kw in cases.items():
        with pytest.raises(NotImplementedError, match='stream with') as err:
            get_enhancer(**kw).stream(4, 3, targets=(0, 1))
        assert setting.split('=')[0] in str(err.value), (setting, str(err.value))


# ------------------------------------------------------------------ checkpoints
def test_checkpoint_refusals_before_the_gpu_is_touched():
    from pb_chime5_amd.streaming import StreamingEnhancer
    multi = dict(targets=[0, 2], stream={}, em={}, bf={}, tails=np.zeros((2, 48)), wpe={})
    single = dict(stream={}, em={}, bf={}, wpe={})
    cases = ((StreamingEnhancer(4, 3, targets=(0, 1), **OK), multi, r'targets=\(0, 2\)'),
             (StreamingEnhancer(4, 3, targets=(2, 0), **OK), multi, r'targets=\(0, 2\)'),
             (StreamingEnhancer(4, 3, targets=(0, 1, 2), **OK), multi, r'targets=\(0, 2\)'),
             (StreamingEnhancer(4, 3, **OK), multi, 'with targets='),
             (StreamingEnhancer(4, 3, targets=(0, 2), **OK), single, 'without targets='))
    for enh, host, match in cases:
        with pytest.raises(ValueError, match=match):
            enh.from_host(host)
        assert enh.stream is None and enh.ctx is None


# ------------------------------------------------------------------ the C ABI
def test_the_library_declares_the_targets_entries():
    import ctypes
    from pb_chime5_amd import _capi
    names = ('gss_mvdr_online_targets', 'gss_last_mvdr_online_fallbacks_targets',
             'gss_istft_stream_targets', 'gss_stream_block_targets')
    assert set(names) <= set(_capi.SIGNATURES)
    assert not [n for n in names if n.startswith('gss_enhance_observation')]
    assert _capi.GSS_ABI_VERSION == 7
    lib = _capi.load_library()
    for name in names:
        assert hasattr(lib, name), name
    # the block call is gss_stream_block's with the tails, a table of targets and S in it
    one, many = _capi.SIGNATURES['gss_stream_block'][1], _capi.SIGNATURES['gss_stream_block_targets'][1]
    assert len(many) == len(one) + 2
    assert many[:7] == one[:7] and many[8:12] == one[7:11]
    assert many[12:14] == [ctypes.POINTER(ctypes.c_int32), ctypes.c_int] and many[14:] == one[12:]
