"""Several speakers of one window (gss_enhance_observation_targets,
Enhancer.enhance_observation_speakers): speaker-id resolution, contexts, the block path and the
C ABI declarations -- everything that needs no GPU."""
import numpy as np
import pytest

import gss_oracle as oracle


def _activity(keys, n=4096):
    return {k: np.ones(n, bool) for k in keys}


@pytest.mark.parametrize('garbage_class,garbage', [
    (True, ['Noise']), (False, ['Noise']), (2, ['Noise0', 'Noise1']), (None, [])])
def test_default_speakers_leave_out_the_garbage_tracks(garbage_class, garbage):
    from pb_chime5_amd.core import get_enhancer
    enh = get_enhancer(activity_garbage_class=garbage_class)
    act = _activity(['P05', 'P02', 'P07'] + garbage)
    assert enh.speaker_ids_of(act) == ['P05', 'P02', 'P07']
    # explicit ids keep their order, garbage tracks may be asked for
    assert enh.speaker_ids_of(act, ('P07', 'P05')) == ['P07', 'P05']
    if garbage:
        assert enh.speaker_ids_of(act, [garbage[0], 'P02']) == [garbage[0], 'P02']


@pytest.mark.parametrize('ids,match', [
    (['P01', 'P09'], 'not in the activity'), (['P01', 'P01'], 'twice'), ([], 'no speaker')])
def test_bad_speaker_ids_raise_before_device_work(monkeypatch, ids, match):
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import get_enhancer
    enh = get_enhancer()
    calls = []
    monkeypatch.setattr(ops, 'enhance_observation_targets', lambda *a, **k: calls.append(a))
    monkeypatch.setattr(enh, 'stft', lambda *a, **k: calls.append(a))
    act = _activity(['P01', 'P02', 'Noise'])
    for fused in (True, False):
        with pytest.raises(ValueError, match=match):
            enh.enhance_observation_speakers(np.zeros((4, 4096)), act, ids, fused=fused)
    with pytest.raises(ValueError, match='no speaker'):
        enh.enhance_observation_speakers(np.zeros((4, 4096)), _activity(['Noise']))
    assert not calls


def test_contexts_broadcast_to_every_target():
    from pb_chime5_amd import ops
    assert ops.target_contexts(2048, 3) == [2048, 2048, 2048]
    assert ops.target_contexts(np.int64(7), 2) == [7, 7]
    assert ops.target_contexts((1, 2, 3), 3) == [1, 2, 3]
    with pytest.raises(ValueError):
        ops.target_contexts([1, 2], 3)


def test_fused_call_hands_the_targets_over(monkeypatch):
    """The fused path: one ops call with the speakers' class indices, the example's contexts,
    the speaker ids as names; utterances-in-flight 1 around it; dict in the order asked for."""
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import get_enhancer
    enh = get_enhancer(context_samples=2048)
    hints, seen = [], {}

    class FakeCtx:
        def set_utterances_in_flight(self, n):
            hints.append(n)

    def fake(obs, activity, targets, start, end, **kw):
        seen.update(targets=list(targets), start=start, end=end, names=kw['target_names'])
        return np.arange(len(targets))[:, None] * np.ones((1, 5))

    monkeypatch.setattr(enh, '_ctx', lambda: FakeCtx())
    monkeypatch.setattr(ops, 'enhance_observation_targets', fake)
    ex = {'start': {'original': 0}, 'start_orig': {'original': 100},
          'end_orig': {'original': 3900}, 'end': {'original': 4096}}
    act = _activity(['P01', 'P02', 'P03', 'Noise'])
    out = enh.enhance_observation_speakers(np.zeros((4, 4096)), act, ['P03', 'Noise', 'P01'],
                                           ex=ex)
    assert list(out) == ['P03', 'Noise', 'P01']
    assert [float(v[0]) for v in out.values()] == [0.0, 1.0, 2.0]
    assert seen == dict(targets=[2, 3, 0], start=100, end=196, names=['P03', 'Noise', 'P01'])
    assert hints == [1, 0]


def test_block_path_runs_gss_once_and_the_beamformer_per_speaker(monkeypatch):
    """With a block swapped out: one STFT / WPE / GSS, bf_block and the iSTFT per speaker, each
    speaker's output what the one-speaker block path gives (all blocks on the oracle)."""
    from pb_chime5_amd import core, synthetic
    u = synthetic.tiny(num_channels=4, num_samples=6000, num_speakers=2, context=1024)
    enh = core.get_enhancer(wpe=True, wpe_tabs=3, wpe_iterations=1, bss_iterations=2,
                            context_samples=1024)
    counts = {'stft': 0, 'istft': 0, 'wpe': 0, 'gss': 0, 'bf': 0}

    def counted(name, fn):
        def run(*a, **k):
            counts[name] += 1
            return fn(*a, **k)
        return run

    class OracleWPE(core.WPE):
        def __call__(self, Obs, stack=None, debug=False):
            counts['wpe'] += 1
            return oracle.wpe_block(Obs, self.taps, self.delay, self.iterations, self.psd_context)

    class OracleGSS(core.GSS):
        def __call__(self, Obs, acitivity_freq, debug=False):
            counts['gss'] += 1
            return oracle.gss_block(Obs, acitivity_freq, self.iterations, self.iterations_post)

    class OracleBF(core.Beamformer):
        def __call__(self, Obs, target_mask, distortion_mask, debug=False):
            counts['bf'] += 1
            return oracle.beamform_mvdr_souden_from_masks(Obs, target_mask, distortion_mask,
                                                          ban=True)

    w = enh.wpe_block
    enh.wpe_block = OracleWPE(taps=w.taps, delay=w.delay, iterations=w.iterations,
                              psd_context=w.psd_context)
    enh.gss_block = OracleGSS(iterations=enh.gss_block.iterations,
                              iterations_post=enh.gss_block.iterations_post)
    enh.bf_block = OracleBF(type=enh.bf_block.type, postfilter=enh.bf_block.postfilter)
    monkeypatch.setattr(enh, 'stft', counted('stft', lambda x: oracle.stft(x, 1024, 256)))
    monkeypatch.setattr(enh, 'istft', counted('istft', lambda X: oracle.istft(X, 1024, 256)))
    assert not enh._fusable()
    out = enh.enhance_observation_speakers(u.obs, u.activity, ['P02', 'Noise', 'P01'], ex=u.ex)
    assert list(out) == ['P02', 'Noise', 'P01']
    assert counts == {'stft': 1, 'istft': 3, 'wpe': 1, 'gss': 1, 'bf': 3}
    for spk, x in out.items():
        want = enh.enhance_observation(u.obs, u.activity, spk, ex=u.ex)
        assert np.array_equal(x, want), spk


def test_capi_declares_the_targets_entry_points():
    import ctypes
    from pb_chime5_amd import _capi
    for name in ('gss_enhance_observation_targets', 'gss_enhance_observation_targets_pcm16'):
        restype, argtypes = _capi.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == 14
        assert argtypes[9:12] == [ctypes.c_void_p] * 3       # targets, start, end contexts
    restype, argtypes = _capi.SIGNATURES['gss_last_ref_channels']
    assert restype is ctypes.c_int and argtypes[2] is ctypes.c_int
    assert hasattr(_capi.Context, 'last_ref_channels')
    lib = _capi.load_library()
    for name in ('gss_enhance_observation_targets', 'gss_enhance_observation_targets_pcm16',
                 'gss_last_ref_channels'):
        assert hasattr(lib, name)


def test_example_speakers_are_trimmed_like_enhance_example(monkeypatch):
    """enhance_example_speakers trims every output with the class's own _trim_context (the
    CHiME-6 and RTTM subclasses override it)."""
    from pb_chime5_amd import core, core_chime6, core_chime6_rttm
    for cls, ex in (
            (core.Enhancer, {'start_orig': {'observation': {'U01': 110}},
                             'start': {'observation': {'U01': 100}},
                             'num_samples_orig': {'observation': {'U01': 5}}}),
            (core_chime6.Enhancer, {'start_orig': 110, 'start': 100, 'num_samples_orig': 5}),
            (core_chime6_rttm.Enhancer, {'start_orig': 110, 'start': 100,
                                         'num_samples_orig': 5})):
        enh = object.__new__(cls)
        enh.context_samples = 10
        enh.reference_array = 'U01'
        monkeypatch.setattr(enh, '_prepare_example', lambda ex: (None, None, None),
                            raising=False)
        monkeypatch.setattr(
            enh, 'enhance_observation_speakers',
            lambda obs, act, ids, ex=None: {'A': np.arange(40.0), 'B': -np.arange(40.0)},
            raising=False)
        out = enh.enhance_example_speakers(ex)
        assert list(out) == ['A', 'B']
        assert np.array_equal(out['A'], np.arange(10.0, 15.0)), cls
        assert np.array_equal(out['B'], -np.arange(10.0, 15.0)), cls


def test_a_build_without_the_new_entry_points_asks_for_a_rebuild(monkeypatch):
    """The targets entry points came without a new ABI revision: a library that passes the
    revision check but lacks a declared symbol is refused with the rebuild hint, not a bare
    AttributeError."""
    from pb_chime5_amd import _capi
    sigs = dict(_capi.SIGNATURES)
    sigs['gss_enhance_observation_targets_v0'] = sigs['gss_last_ref_channels']
    monkeypatch.setattr(_capi, 'SIGNATURES', sigs)
    with pytest.raises(_capi.GssError, match='gss_enhance_observation_targets_v0.*rebuild'):
        _capi.load_library(_capi.LIB_PATH)
