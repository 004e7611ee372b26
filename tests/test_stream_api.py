"""The sample-block stream without a GPU: the NumPy stream reference against the oracle to the bit,
its composition with the references of the three online stages, the geometry helpers, the refusals
of `Enhancer.stream` and the argument errors of `StreamingEnhancer`."""
import numpy as np
import pytest

import gss_oracle as oracle
import stream_reference as sr

GEOMETRIES = ((64, 16), (48, 12), (1024, 256))


def _cuts(N):
    cuts = [(N,), sr.random_cuts(N, 1), sr.random_cuts(N, 2, pieces=12)]
    if N == 1001:
        cuts += [(1, 15, 16, 17, 0, 500, 452), (255, 255, 255, 236)]
    return cuts


@pytest.mark.parametrize('size,shift', GEOMETRIES)
def test_the_stream_reference_is_the_oracle_to_the_bit(size, shift):
    rng = np.random.default_rng([size, shift])
    for N in (1, shift - 1, shift, 500, 1001):
        x = rng.standard_normal((2, N))
        activity = rng.random((3, N)) < 0.2
        Yo = oracle.stft(x, size, shift, fading=True)
        fo = oracle.activity_time_to_frequency(activity, size, shift, True)[:, :Yo.shape[1]]
        X = Yo[0] * (1 + 0.25j) + Yo[1]
        xo = oracle.istft(X, size, shift, fading=True)[:N]
        for cuts in _cuts(N):
            Y, f = sr.stream_stft(x, activity, size, shift, cuts)
            assert Y.shape == Yo.shape and np.array_equal(Y, Yo), (N, cuts)
            assert np.array_equal(f, fo), (N, cuts)
        T = X.shape[0]
        for frame_cuts in ((T,), (1,) * T, sr.random_cuts(T, 4, pieces=5)):
            out = sr.stream_istft(X, N, size, shift, frame_cuts)
            assert out.shape == xo.shape and np.array_equal(out, xo), (N, frame_cuts)


@pytest.mark.parametrize('name', ['a', 'c', 'e', 'h'])
def test_the_composed_reference_does_not_depend_on_the_cuts(name):
    x, activity = sr.scene(name, sr.seed_of(name))
    x_hat, taps, states = sr.reference(name, sr.seed_of(name))
    assert taps['fallbacks'] == (0, 0)
    for part, cuts in sr.partitions(name).items():
        xs, ts, ss = sr.compose_stream(name, x, activity, cuts)
        assert np.array_equal(xs, x_hat), (name, part)
        for k in ('Obs', 'gamma', 'target_mask', 'distortion_mask', 'X_hat'):
            assert np.array_equal(ts[k], taps[k]), (name, part, k)
        a, b = sr.state_arrays(states), sr.state_arrays(ss)
        assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a), (name, part)


@pytest.mark.parametrize('name', sorted(sr.CELLS))
def test_parity_scenes_are_stable(name):
    """Every cell keeps the first seed at which the composed reference moves at least 100x less
    than the bars under a last-bit change of the samples."""
    assert sr.choose_seed(name) == sr.seed_of(name)
    moved, x_moved = sr.reference_movement(name, sr.seed_of(name))
    print(f'{name}: gamma / X_hat / states move {moved:.1e}, |x_hat| {x_moved:.1e}')
    assert moved * sr.STABILITY_MARGIN <= sr.TOL and x_moved * sr.STABILITY_MARGIN <= sr.X_TOL


def test_geometry_helpers():
    from pb_chime5_amd import ops
    for W, H in GEOMETRIES + ((64, 32),):
        counts = (0, 1, H - 1, H, H + 1, W - 1, W, W + 1, 1000, 240000)
        for M in counts:
            want = oracle.stft_frames(M, W, H, fading=True) * H - M
            assert ops.stream_flush_samples(M, W, H) == want == sr.flush_samples(M, W, H)
            # a flushed stream has the frames of the whole signal and at least M samples out
            assert (M + want) // H == oracle.stft_frames(M, W, H, fading=True)
            assert ops.stream_num_samples_out(0, M + want, W, H) >= M
            for n in counts:
                frames = (M + n) // H - M // H
                out = max(0, (M + n) // H * H - (W - H)) - max(0, M // H * H - (W - H))
                assert ops.stream_num_frames(M, n, W, H) == frames == sr.num_frames(M, n, W, H)
                assert ops.stream_num_samples_out(M, n, W, H) == out == sr.num_samples_out(M, n, W, H)
            # the latency: what went in and has not come out
            assert M - sr.emitted(M, W, H) == (M if M // H * H < W - H else W - H + M % H)
    for bad in (dict(size=64, shift=24), dict(size=0, shift=16), dict(size=64, shift=0)):
        with pytest.raises(ValueError):
            ops.stream_num_frames(0, 1, **bad)
    with pytest.raises(ValueError, match='received'):
        ops.stream_num_frames(-1, 1, 64, 16)
    with pytest.raises(ValueError, match='n='):
        ops.stream_num_samples_out(0, -1, 64, 16)


def test_the_library_declares_the_stream():
    from pb_chime5_amd import _capi, build
    assert 'stream.hip' in build.SOURCES
    names = ('gss_stream_init', 'gss_stream_num_frames', 'gss_stream_num_samples_out',
             'gss_stream_flush_samples', 'gss_stft_stream', 'gss_istft_stream', 'gss_stream_block')
    assert set(names) <= set(_capi.SIGNATURES)
    # no new fused entry: the stream is not a row of the binding's call table
    assert not [n for n in names if n.startswith('gss_enhance_observation')]
    assert _capi.GSS_ABI_VERSION == 7


def _get_enhancer(**kw):
    from pb_chime5_amd.core import get_enhancer
    args = dict(gss_online=True, bf_online=True, wpe_online=True)
    args.update(kw)
    return get_enhancer(**args)


def test_enhancer_stream_builds_from_the_enhancers_settings():
    enh = _get_enhancer(wpe_tabs=4, wpe_delay=3, stft_size=512, stft_shift=128, gss_forget=0.98,
                        bf_forget=0.97, bf_loading=0.5, postfilter='mask_mul')
    s = enh.stream(6, ['P01', 'P02', 'Noise'], 'P02', ref_channel=2)
    assert (s.D, s.K, s.target, s.ref_channel, s.size, s.shift) == (6, 3, 1, 2, 512, 128)
    assert (s.wpe, s.wpe_taps, s.wpe_delay, s.wpe_alpha) == (True, 4, 3, enh.wpe_block.alpha)
    assert (s.gss_forget, s.bf_forget, s.bf_loading, s.postfilter) == (0.98, 0.97, 0.5, 'mask_mul')
    assert s.fused and s.guided and s.speakers == ['P01', 'P02', 'Noise']
    assert s.latency_samples == 0 and s.samples_in == s.samples_out == 0
    assert enh.stream(4, 3, 0, fused=False).fused is False
    assert _get_enhancer(wpe=False, wpe_online=False).stream(4, 2, 1).wpe is False
    with pytest.raises(ValueError, match='target'):
        enh.stream(6, ['P01', 'P02'], 'P03')
    with pytest.raises(ValueError, match='speakers'):
        enh.stream(6)
    with pytest.raises(ValueError, match='target'):
        enh.stream(6, 3)


@pytest.mark.parametrize('setting,kw', [
    ('gss_online', dict(gss_online=False, bf_online=False, wpe_online=False)),
    ('bf_online', dict(bf_online=False, wpe_online=False)),
    ('wpe_online', dict(wpe_online=False)),
    ('stft_fading', dict(stft_fading=False)),
], ids=lambda v: v if isinstance(v, str) else '')
def test_enhancer_stream_refuses_what_it_is_not_built_for(setting, kw):
    with pytest.raises(NotImplementedError, match=f'stream with {setting}'):
        _get_enhancer(**kw).stream(4, 3, 0)


def test_enhancer_stream_refuses_the_whole_window_options():
    """Settings that the online stages already refuse at construction never reach `stream`; the
    ones an enhancer can be built with are refused there, naming the setting."""
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
            get_enhancer(**kw).stream(4, 3, 0)
        assert setting.split('=')[0] in str(err.value), (setting, str(err.value))


def test_streaming_enhancer_argument_errors():
    from pb_chime5_amd.streaming import StreamingEnhancer
    ok = dict(stft_size=64, stft_shift=16, wpe_taps=2, wpe_delay=1)
    for bad, match in ((dict(num_channels=0), 'num_channels'), (dict(num_channels=33), 'num_channels'),
                       (dict(num_classes=0), 'num_classes'), (dict(num_classes=9), 'num_classes'),
                       (dict(target=3), 'target'), (dict(target=-1), 'target'),
                       (dict(ref_channel=4), 'ref_channel'), (dict(ref_channel=-1), 'ref_channel'),
                       (dict(stft_shift=24), 'shift'), (dict(wpe_alpha=0.0), 'alpha'),
                       (dict(wpe_taps=0), 'taps'), (dict(wpe_arrays=3), 'arrays'),
                       (dict(gss_forget=1.5), 'forget'), (dict(gss_prior_mass=0.0), 'prior_mass'),
                       (dict(bf_forget=0.0), 'forget'), (dict(bf_loading=-1.0), 'loading'),
                       (dict(fused=1), 'fused'), (dict(model='a model'), 'model'),
                       (dict(speakers=['a', 'a', 'b']), 'speakers')):
        args = dict(num_channels=4, num_classes=3, **ok)
        args.update(bad)
        with pytest.raises(ValueError, match=match):
            StreamingEnhancer(**args)
    with pytest.raises(ValueError, match='num_classes'):
        StreamingEnhancer(4, **ok)
    for bad in (dict(stft_shift=64), dict(stft_size=6000, stft_shift=1500), dict(postfilter='wiener'),
                dict(wpe_taps=200)):
        with pytest.raises(NotImplementedError):
            StreamingEnhancer(4, 3, **dict(ok, **bad))


def test_process_checks_the_block_before_any_device_work():
    from pb_chime5_amd.streaming import StreamingEnhancer
    enh = StreamingEnhancer(4, 3, stft_size=64, stft_shift=16, wpe_taps=2, wpe_delay=1,
                            speakers=['a', 'b', 'n'])
    x, act = np.zeros((4, 40)), np.ones((3, 40), bool)
    for block, activity, match in ((x[:3], act, 'block'), (x[0], act, 'block'), (x, act[:2], 'activity'),
                                   (x, act[:, :39], 'activity'), (x, None, 'activity: missing'),
                                   (x, dict(a=act[0], b=act[1]), 'tracks'),
                                   (x, dict(a=act[0], b=act[1], n=act[2][:5]), 'activity')):
        with pytest.raises(ValueError, match=match):
            enh.process(block, activity)
    assert enh.samples_in == 0 and enh.stream is None       # nothing reached the device
    # a stream that took nothing ends empty; process is an error until reset
    assert enh.flush().shape == (0,)
    for call in (lambda: enh.process(x, act), enh.flush):
        with pytest.raises(RuntimeError, match='reset'):
            call()
    enh.reset()
    with pytest.raises(ValueError, match='block'):
        enh.process(x[:3], act)


def test_stream_state_checks():
    from pb_chime5_amd import ops
    with pytest.raises(ValueError, match='num_channels'):
        ops.check_stream(0, 3, 64, 16)
    with pytest.raises(ValueError, match='num_classes'):
        ops.check_stream(4, 9, 64, 16)
    with pytest.raises(NotImplementedError, match='overlapping'):
        ops.check_stream(4, 3, 64, 64)
    assert ops.check_stream(4, 0, 1024, 256) == (4, 0, 1024, 256)
    assert ops.StreamState._shapes(4, 0, 64, 16) == {'x_hist': (4, 64), 'ola_tail': (48,)}
    assert ops.StreamState._shapes(4, 3, 64, 16)['act_hist'] == (3, 64)
    for host, match in ((dict(x_hist=np.zeros(5), size=64, shift=16, received=0, frames_out=0), 'x_hist'),
                        (dict(x_hist=np.zeros((2, 64)), size=64, shift=16, received=10, frames_out=1),
                         'frames_out'),
                        (dict(x_hist=np.zeros((2, 64)), size=64, shift=16, received=-1, frames_out=0),
                         'received')):
        with pytest.raises(ValueError, match=match):
            ops.StreamState.from_host(host)
    for fn in (ops.stft_stream, ops.istft_stream):
        with pytest.raises(ValueError, match='StreamState'):
            fn(np.zeros((1, 4)), state=None)
