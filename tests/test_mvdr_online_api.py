"""Online MVDR (gss_mvdr_online, get_enhancer(bf_online=True)): the NumPy reference itself
(tests/online_mvdr_reference.py), the evidence that the online form follows a moving target, the C
surface, and every argument check and front door -- none of it needs a GPU."""
import ctypes
import inspect

import numpy as np
import pytest

import online_mvdr_reference as mr
from conftest import REPO

SYMBOLS = ('gss_mvdr_online_init', 'gss_mvdr_online', 'gss_last_mvdr_online_fallbacks',
           'gss_enhance_observation_bf_online')


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
@pytest.mark.parametrize('cell', mr.CLOSED_FORM_CELLS, ids=str)
def test_reference_recursion_is_its_closed_form(cell):
    D, beta, loading, F, T = cell
    Y, mx, mn, _ = mr.scene(cell, mr.seed_of(cell))
    _, _, st, fallbacks = mr.reference(cell, False, 0, mr.seed_of(cell))
    phi_x, phi_n = mr.closed_form(Y, mx, mn, beta, mr.loading_delta(Y, loading))
    errs = mr.rel_err(st['phi_x'], phi_x), mr.rel_err(st['phi_n'], phi_n)
    assert fallbacks == 0 and max(errs) < mr.CLOSED_FORM_TOL, errs


def test_reference_in_blocks_equals_one_call():
    cell = mr.CHUNK_CELLS[0]
    D, beta, loading, F, T = cell
    Y, mx, mn, _ = mr.scene(cell, mr.seed_of(cell))
    for ban in (False, True):
        X1, W1, st1, _ = mr.reference(cell, ban, D - 1, mr.seed_of(cell))

        def step(Yb, mxb, mnb, state):
            return mr.online_mvdr(Yb, mxb, mnb, beta, D - 1, ban, state=state)[:3]
        X, W, st = mr.in_blocks(Y, mx, mn, beta, D - 1, ban, loading, mr.CHUNKS[T], step)
        assert np.array_equal(X, X1) and np.array_equal(W, W1)
        assert np.array_equal(st['phi_x'], st1['phi_x']) and np.array_equal(st['phi_n'], st1['phi_n'])


def test_reference_zero_target_mask_and_fallbacks():
    cell = mr.CELLS[0]
    D, beta, loading, F, T = cell
    Y, mx, mn, _ = mr.scene(cell)
    for ban in (False, True):
        X, W, _, fallbacks = mr.online_mvdr(Y, np.zeros_like(mx), mn, beta, 0, ban, loading=loading)
        assert np.all(X == 0) and np.all(W == 0) and fallbacks == 0
    Y, mx, mn, st0, beta, count = mr.fallback_case('all')
    X, W, st, fallbacks = mr.online_mvdr(Y, mx, mn, beta, 0, False, state=st0)
    assert fallbacks == count == Y.shape[0] * Y.shape[1] and np.all(X == 0)
    assert np.any(st['phi_x'] != 0) and np.all(st['phi_n'] == 0)     # the update stays
    Y, mx, mn, st0, beta, count = mr.fallback_case('first')
    assert Y.shape[2] == 1
    X, W, st, fallbacks = mr.online_mvdr(Y, mx, mn, beta, 0, False, state=st0)
    assert fallbacks == count == 3 * Y.shape[0]
    assert np.all(X[:, :3] == 0) and np.all(np.isfinite(X)) and np.all(X[:, 3:] != 0)


def test_parity_scenes_are_stable():
    """The rule that keeps a seed: the reference itself moves at least STABILITY_MARGIN x less
    than the bar under a last-bit change of every sample and mask value."""
    for cell in mr.CELLS + mr.LONG_CELLS:
        moved = mr.reference_movement(cell, mr.seed_of(cell))
        assert moved * mr.STABILITY_MARGIN <= mr.TOL, (cell, moved)
    assert max(c[0] for c in mr.CELLS) == 32
    assert mr.LONG_CELLS == [(4, 0.99, 1e-2, 2, 6000), (24, 0.995, 1.0, 1, 3000)]
    for cell in mr.LONG_CELLS:
        assert all(mr.reference(cell, ban, ref, mr.seed_of(cell))[3] == 0 for ban, ref in mr.variants(cell))


def test_the_online_form_follows_a_moving_target():
    """On a scene whose target drifts, the online form's error against the target's image over the
    second half of the frames is below EVIDENCE_BOUND x the whole-window beamformer's (the oracle's
    get_mvdr_vector_souden); the seed is one for which the reference gives <= 0.75."""
    ratio = mr.evidence_ratio()
    print(f'online / whole-window error: {ratio:.3f}')
    assert ratio <= 0.75 < mr.EVIDENCE_BOUND


# ------------------------------------------------------------------ the C surface
def test_the_built_library_exports_the_entry_points():
    from pb_chime5_amd import _capi, build
    assert 'mvdr_online.hip' in build.SOURCES
    lib = _capi.load_library()
    header = (REPO / 'include' / 'gss_hip.h').read_text()
    for name in SYMBOLS:
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
        assert f'int {name}(' in header, name
    assert _capi.GSS_ABI_VERSION == 7 and lib.gss_abi_version() == 7


def test_descriptor_layouts_are_the_header_structs():
    from pb_chime5_amd import _capi, ops
    header = (REPO / 'include' / 'gss_hip.h').read_text()
    for decl in ('gss_cplx *phi_x, *phi_n;', '} gss_mvdr_online_state;', '} gss_bf_online;',
                 'double forget;', 'double loading;', 'int32_t ref_channel;', 'int32_t wpe_online;',
                 'double wpe_alpha;'):
        assert decl in header, decl
    S = _capi.GssMvdrOnlineState
    assert [n for n, _ in S._fields_] == ['phi_x', 'phi_n', 'F', 'D']
    assert [getattr(S, n).offset for n, _ in S._fields_] == [0, 8, 16, 20] and ctypes.sizeof(S) == 24
    C = _capi.GssBfOnline
    assert [n for n, _ in C._fields_] == ['forget', 'loading', 'ref_channel', 'wpe_online', 'wpe_alpha']
    assert [getattr(C, n).offset for n, _ in C._fields_] == [0, 8, 16, 20, 24] and ctypes.sizeof(C) == 32
    assert ops._FUSED_ENTRIES['bf_online'] == ('gss_enhance_observation_bf_online', None,
                                               'online MVDR')
    assert _capi.SIGNATURES['gss_enhance_observation_bf_online'] == \
        _capi._fused(ctypes.POINTER(C))


def test_the_unit_has_one_form_and_no_float_atomics():
    unit = (REPO / 'pb_chime5_amd' / 'csrc' / 'mvdr_online.hip').read_text()
    assert 'getenv' not in unit and 'gss_variant' not in unit
    assert 'rocblas' not in unit.lower() and 'rocsolver' not in unit.lower()
    # the one atomic is the integer count of fallback frames
    assert unit.count('atomicAdd(') == 1 and 'atomicAdd(a.fallbacks, nfall)' in unit


# ------------------------------------------------------------------ argument checks
def test_check_bf_online(no_context):
    from pb_chime5_amd import ops
    assert (ops.BF_ONLINE_FORGET, ops.BF_ONLINE_LOADING) == (0.99, 1e-2)
    assert ops.check_bf_online() == (0.99, 1e-2, 0)
    assert ops.check_bf_online(1, 3, -1, 29) == (1.0, 3.0, -1)
    assert ops.check_bf_online(0.5, 1e-9, 31, 32) == (0.5, 1e-9, 31)
    nan, inf = float('nan'), float('inf')
    for kw, word in ((dict(forget=0.0), 'forget'), (dict(forget=1.0001), 'forget'),
                     (dict(forget=nan), 'forget'), (dict(forget='a'), 'forget'),
                     (dict(forget=True), 'forget'),
                     (dict(loading=0.0), 'loading'), (dict(loading=-1.0), 'loading'),
                     (dict(loading=inf), 'loading'), (dict(loading=nan), 'loading'),
                     (dict(loading=None), 'loading'),
                     (dict(ref_channel=-2), 'ref_channel'), (dict(ref_channel=0.5), 'ref_channel'),
                     (dict(ref_channel=4, num_channels=4), 'ref_channel'),
                     (dict(ref_channel=-1, num_channels=30), 'ref_channel'),
                     (dict(num_channels=0), 'num_channels'), (dict(num_channels=33), 'num_channels'),
                     (dict(num_channels=2.5), 'num_channels')):
        with pytest.raises(ValueError, match=word):
            ops.check_bf_online(**kw)
    sig = inspect.signature(ops.mvdr_souden_online_from_masks).parameters
    assert [sig[k].default for k in ('ban', 'forget', 'loading', 'ref_channel', 'state',
                                     'return_filters', 'return_fallbacks', 'ctx')] == \
        [False, 0.99, 1e-2, 0, None, False, False, None]


def test_stage_argument_errors_before_any_device_work(no_context):
    from pb_chime5_amd import ops
    Y = np.ones((3, 9, 5), complex)
    m = np.ones((9, 5))
    call = ops.mvdr_souden_online_from_masks
    with pytest.raises(ValueError, match='Y'):
        call(Y[0], m, m)
    for kw, word in ((dict(forget=0.0), 'forget'), (dict(loading=0.0), 'loading'),
                     (dict(ref_channel=3), 'ref_channel'), (dict(state=object()), 'state')):
        with pytest.raises(ValueError, match=word):
            call(Y, m, m, **kw)
    with pytest.raises(ValueError, match='num_channels'):
        call(np.ones((33, 9, 5), complex), m, m)
    for bad, word in ((m[:, :4], 'X_mask'), (np.where(np.eye(9, 5) > 0, -1e-9, m), 'X_mask'),
                      (np.where(np.eye(9, 5) > 0, np.nan, m), 'X_mask')):
        with pytest.raises(ValueError, match=word):
            call(Y, bad, m)
        with pytest.raises(ValueError, match='N_mask'):
            call(Y, m, bad)
    for args, kw, word in (((0, 4), {}, 'F'), ((5, 0), {}, 'num_channels'), ((5, 33), {}, 'num_channels'),
                           ((5, 4), dict(loading=0.0), 'loading'),
                           ((5, 4), dict(Y=np.ones((4, 9, 6))), 'Y'),
                           ((5, 4), dict(Y=np.ones((3, 9, 5))), 'Y')):
        with pytest.raises(ValueError, match=word):
            ops.OnlineMVDRState.fresh(*args, **kw)
    for host, word in ((dict(phi_x=np.ones((5, 4, 3)), phi_n=np.ones((5, 4, 3))), 'phi_x'),
                       (dict(phi_x=np.ones((5, 4)), phi_n=np.ones((5, 4))), 'phi_x'),
                       (dict(phi_x=np.ones((5, 4, 4)), phi_n=np.ones((5, 3, 3))), 'phi_n'),
                       (dict(phi_x=np.ones((5, 33, 33)), phi_n=np.ones((5, 33, 33))), 'num_channels')):
        with pytest.raises(ValueError, match=word):
            ops.OnlineMVDRState.from_host(host)
    from pb_chime5_amd.online_mvdr import OnlineMVDR
    for kw, word in ((dict(forget=2.0), 'forget'), (dict(loading=0), 'loading'),
                     (dict(ref_channel=-1), 'ref_channel'), (dict(ref_channel=8), 'ref_channel'),
                     (dict(channel=0), 'num_channels'), (dict(frequency_bins=0), 'frequency_bins')):
        with pytest.raises(ValueError, match=word):
            OnlineMVDR(**kw)


def test_state_shapes_and_a_mismatched_state():
    """The buffers of a state and the rule that a call takes only the state built for it --
    on a context that allocates nothing."""
    from pb_chime5_amd import ops

    class Buf:
        def __init__(self, n):
            self.nbytes, self.ptr = n, 4096

    class Ctx:
        def empty(self, n):
            return Buf(n)
    st = ops.OnlineMVDRState(Ctx(), 5, 3)
    assert st.shapes == {'phi_x': (5, 3, 3), 'phi_n': (5, 3, 3)} and st.key == (5, 3)
    assert {k: b.nbytes for k, b in st.bufs.items()} == {'phi_x': 16 * 45, 'phi_n': 16 * 45}
    s = st.struct()
    assert (s.phi_x, s.phi_n, s.F, s.D) == (4096, 4096, 5, 3)
    m = np.ones((9, 5))
    with pytest.raises(ValueError, match='state'):
        ops.mvdr_souden_online_from_masks(np.ones((4, 9, 5), complex), m, m, state=st)
    with pytest.raises(ValueError, match='state'):
        ops.mvdr_souden_online_from_masks(np.ones((3, 9, 6), complex), np.ones((9, 6)),
                                          np.ones((9, 6)), state=st)
    with pytest.raises(ValueError, match='context'):
        ops.mvdr_souden_online_from_masks(np.ones((3, 9, 5), complex), m, m, state=st, ctx=Ctx())


def test_fused_argument_errors_before_any_device_work(no_context):
    from pb_chime5_amd import ops
    obs, act = np.zeros((4, 4096)), np.ones((3, 4096), bool)
    call = ops.enhance_observation_bf_online
    with pytest.raises(ValueError, match='obs'):
        call(obs[0], act, 0, 0, 0)
    for kw, word in ((dict(forget=0.0), 'forget'), (dict(loading=-1), 'loading'),
                     (dict(ref_channel=4), 'ref_channel'),
                     (dict(wpe_online=True, wpe_alpha=0.0), 'alpha'),
                     (dict(wpe_online=True, wpe=False), 'wpe=False'),
                     (dict(wpe_online=True, wpe_psd_context=1), 'wpe_psd_context'),
                     (dict(wpe_alpha=0.9), 'wpe_alpha')):
        with pytest.raises(ValueError, match=word):
            call(obs, act, 0, 0, 0, **kw)
    for bf in ('gev_ban', 'ch2', 'sum'):
        with pytest.raises(NotImplementedError, match='bf_online'):
            call(obs, act, 0, 0, 0, bf=bf)
    sig = inspect.signature(call).parameters
    assert [sig[k].default for k in ('forget', 'loading', 'ref_channel', 'wpe_online', 'wpe_alpha')] \
        == [0.99, 1e-2, -1, False, 0.9999]


# ------------------------------------------------------------------ the beamformer block
def test_beamformer_block(monkeypatch):
    from pb_chime5_amd import core, ops
    seen = []
    monkeypatch.setattr(ops, 'mvdr_souden_online_from_masks',
                        lambda Y, X_mask, N_mask, **kw: seen.append(kw) or X_mask * 2)
    plain = core.Beamformer('mvdrSouden_ban', None)
    assert (plain.online, plain.forget, plain.loading) == (False, 0.99, 1e-2)
    assert plain.online_settings is None
    assert plain == core.Beamformer('mvdrSouden_ban', None, online=False)
    block = core.Beamformer('mvdrSouden_ban', 'mask_mul', online=True, forget=0.9, loading=0.5)
    assert block.online_settings == dict(forget=0.9, loading=0.5)
    m = np.full((9, 5), 0.5)
    out = block(np.zeros((4, 9, 5), complex), m, m)
    assert seen == [dict(ban=True, ref_channel=-1, forget=0.9, loading=0.5)]
    assert np.all(out == 0.5)                           # the postfilter still applies
    for kw, word in ((dict(type='gev_ban'), 'gev_ban'), (dict(type='ch2'), 'ch2'),
                     (dict(type='wpdSouden_ban'), 'wpdSouden_ban'),
                     (dict(segment_frames=64), 'bf_segment_frames'),
                     (dict(null_interferer=True), 'bf_null_interferer')):
        with pytest.raises(NotImplementedError, match=f'{word}'):
            core.Beamformer(**{**dict(type='mvdrSouden_ban', postfilter=None, online=True), **kw})
    with pytest.raises(ValueError, match='forget'):
        core.Beamformer('mvdrSouden_ban', None, online=True, forget=0.0)
    with pytest.raises(ValueError, match='loading'):
        core.Beamformer('mvdrSouden_ban', None, online=True, loading=0.0)
    for kw, word in ((dict(forget=0.9), 'bf_forget'), (dict(loading=1.0), 'bf_loading')):
        with pytest.raises(NotImplementedError, match=f'{word}.*nobody reads it'):
            core.Beamformer('mvdrSouden_ban', None, **kw)


# ------------------------------------------------------------------ front doors
def test_every_front_door_has_the_keywords_and_carries_them():
    from pb_chime5_amd import core, core_chime6, core_chime6_rttm
    for mod in (core, core_chime6, core_chime6_rttm):
        sig = inspect.signature(mod.get_enhancer).parameters
        assert [sig[k].default for k in ('bf_online', 'bf_forget', 'bf_loading')] == \
            [False, 0.99, 1e-2], mod.__name__
    for mod in (core, core_chime6):
        plain = mod.get_enhancer()
        assert plain._bf_online() is None and not plain.bf_block.online
        enh = mod.get_enhancer(bf_online=True, bf_forget=0.95, bf_loading=0.1, wpe_online=True,
                               wpe_per_array=True, multiarray=True)
        assert enh._bf_online() == dict(forget=0.95, loading=0.1) and enh._fusable()
        assert enh._wpe_online() == 0.9999 and enh.wpe_per_array
        assert mod.get_enhancer(bf_online=True)._bf_online() == dict(forget=0.99, loading=1e-2)
        for kw, word in ((dict(bf='gev_ban'), 'gev_ban.*bf_online'), (dict(bf='ch2'), 'bf_online'),
                         (dict(bf='sum'), 'bf_online'), (dict(bf='wpdSouden_ban'), 'bf_online'),
                         (dict(bf_segment_frames=64), 'bf_online with bf_segment_frames'),
                         (dict(bf_null_interferer=True), 'bf_online with bf_null_interferer'),
                         (dict(channel_keep=3), 'bf_online with channel_keep')):
            with pytest.raises(NotImplementedError, match=word):
                mod.get_enhancer(bf_online=True, **kw)
        for kw, word in ((dict(bf_forget=0.9), 'bf_forget'), (dict(bf_loading=1.0), 'bf_loading')):
            with pytest.raises(NotImplementedError, match=f'{word}.*without bf_online'):
                mod.get_enhancer(**kw)
        with pytest.raises(ValueError, match='forget'):
            mod.get_enhancer(bf_online=True, bf_forget=1.5)
        with pytest.raises(ValueError, match='loading'):
            mod.get_enhancer(bf_online=True, bf_loading=0.0)


def test_rttm_front_door_takes_the_keywords(tmp_path):
    from pb_chime5_amd.core_chime6_rttm import get_enhancer
    from test_rttm_frontdoor import _make_chime6_dir
    root, rttm, _ = _make_chime6_dir(tmp_path)
    kw = dict(database_rttm=[str(rttm)], activity_rttm=[str(rttm)], chime6_dir=root,
              multiarray='outer_array_mics')
    enh = get_enhancer(**kw, bf_online=True, bf_forget=0.98)
    assert enh._bf_online() == dict(forget=0.98, loading=1e-2)
    assert get_enhancer(**kw)._bf_online() is None


def test_command_lines_parse_the_keys(monkeypatch):
    from pb_chime5_amd.scripts import run, kaldi_run, kaldi_run_rttm, enhance_rttm
    cfg = run.main(['print_config', 'with', 'bf_online=True', 'bf_forget=0.95', 'bf_loading=0.1'])
    assert (cfg['bf_online'], cfg['bf_forget'], cfg['bf_loading']) == (True, 0.95, 0.1)
    cfg = run.main(['print_config'])
    assert (cfg['bf_online'], cfg['bf_forget'], cfg['bf_loading']) == (False, 0.99, 1e-2)
    assert kaldi_run.main(['print_config', 'with', 'bf_online=True'])['bf_online'] is True
    assert kaldi_run_rttm.main(['print_config', 'with', 'database_rttm=a.rttm', 'bf_online=True',
                                'bf_forget=0.9'])['bf_forget'] == 0.9

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
        enhance_rttm.main(base + ['--bf-online', '--bf-forget', '0.95', '--bf-loading', '0.5'])
    assert (seen['bf_online'], seen['bf_forget'], seen['bf_loading']) == (True, 0.95, 0.5)
    seen.clear()
    with pytest.raises(Stop):
        enhance_rttm.main(base)
    assert (seen['bf_online'], seen['bf_forget'], seen['bf_loading']) == (False, 0.99, 1e-2)


def test_methods_that_refuse_the_online_beamformer(no_context, tmp_path):
    from pb_chime5_amd.core import get_enhancer
    enh = get_enhancer(bf_online=True)
    obs = np.zeros((4, 4096))
    act = {'P01': np.ones(4096, bool), 'Noise': np.ones(4096, bool)}
    with pytest.raises(NotImplementedError, match='enhance_observation_guided with bf_online'):
        enh.enhance_observation_guided(obs, {'P01': np.ones(19), 'Noise': np.ones(19)}, 'P01')
    with pytest.raises(NotImplementedError, match='enhance_observation_speakers with bf_online'):
        enh.enhance_observation_speakers(obs, act, ['P01'])
    with pytest.raises(NotImplementedError, match='enhance_example_speakers with bf_online'):
        enh.enhance_example_speakers({})
    with pytest.raises(NotImplementedError, match='enhance_observation_activity with bf_online'):
        enh.enhance_observation_activity(obs, act, 'P01')
    with pytest.raises(NotImplementedError, match='enhance_example_activity with bf_online'):
        enh.enhance_example_activity({})
    with pytest.raises(NotImplementedError, match='enhance_observation_blind with bf_online'):
        enh.enhance_observation_blind(obs, 2)
    with pytest.raises(NotImplementedError, match='with bf_online'):
        enh.enhance_recording_blind(obs, 2, window_samples=4096, hop_samples=2048)
    with pytest.raises(NotImplementedError, match='refined_rttm.* with bf_online'):
        enh.enhance_session('S02', tmp_path / 'audio', refined_rttm=True)
    assert not (tmp_path / 'audio').exists()


def test_session_takes_one_utterance_at_a_time(monkeypatch, tmp_path):
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import get_enhancer
    enh = get_enhancer(bf_online=True)
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


def test_fused_call_gets_the_settings(monkeypatch):
    from pb_chime5_amd import core, ops
    seen = {}

    def fake(obs, activity, target, start, end, **kw):
        seen.update(kw, target=target)
        return np.zeros(8)
    monkeypatch.setattr(ops, 'enhance_observation_bf_online', fake)

    def boom(*a, **k):
        raise AssertionError('another fused call')
    monkeypatch.setattr(ops, 'enhance_observation', boom)
    monkeypatch.setattr(ops, 'enhance_observation_wpe_online', boom)

    class Ctx:
        def set_utterances_in_flight(self, n):
            pass
    monkeypatch.setattr(core.Enhancer, '_ctx', lambda self: Ctx())
    act = {'P01': np.ones(4096, bool), 'P02': np.ones(4096, bool), 'Noise': np.ones(4096, bool)}
    enh = core.get_enhancer(bf_online=True, bf_forget=0.9, bf_loading=0.5, bf_drop_context=False)
    enh.enhance_observation(np.zeros((4, 4096)), act, 'P02')
    assert [seen[k] for k in ('forget', 'loading', 'ref_channel', 'wpe_online', 'wpe_alpha',
                              'target')] == [0.9, 0.5, -1, False, 0.9999, 1]
    seen.clear()
    enh = core.get_enhancer(bf_online=True, wpe_online=True, wpe_alpha=0.99, wpe_tabs=4,
                            bf_drop_context=False, multiarray='outer_array_mics',
                            wpe_per_array=True)
    enh.enhance_observation(np.zeros((4, 4096)), act, 'P01')
    assert [seen[k] for k in ('forget', 'loading', 'ref_channel', 'wpe_online', 'wpe_alpha',
                              'wpe_arrays')] == [0.99, 1e-2, -1, True, 0.99, 2]
    assert seen['params'].wpe_taps == 4 and seen['params'].bf == 0
