"""Interferer-nulling LCMV (gss_lcmv_souden, get_enhancer(bf_null_interferer=True)): the C ABI,
the argument checks, the parameter plumbing, the front doors and the NumPy reference itself
(tests/lcmv_reference.py), without a GPU."""
import ctypes
import inspect

import numpy as np
import pytest

import lcmv_reference as lr
from conftest import REPO

SYMBOLS = ('gss_lcmv_souden', 'gss_lcmv_masks_from_posteriors', 'gss_enhance_observation_lcmv',
           'gss_last_lcmv_interferer', 'gss_last_lcmv_fallbacks')


def test_the_built_library_exports_the_lcmv_entry_points():
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
    for decl in ('int32_t interferer;', 'uint32_t candidates;', 'double min_mass;',
                 '} gss_bf_lcmv;'):
        assert decl in header, decl
    S = _capi.GssBfLcmv
    assert [n for n, _ in S._fields_] == ['interferer', 'candidates', 'min_mass']
    assert (S.interferer.offset, S.candidates.offset, S.min_mass.offset) == (0, 4, 8)
    assert ctypes.sizeof(S) == 16


@pytest.fixture
def no_context(monkeypatch):
    """Any attempt to create or fetch a device context fails the test."""
    from pb_chime5_amd import _capi, ops

    def boom(*a, **k):
        raise AssertionError('device work before the argument check')
    monkeypatch.setattr(_capi, 'default_context', boom)
    monkeypatch.setattr(ops, 'default_context', boom)
    monkeypatch.setattr(_capi.Context, '__init__', boom)


# ------------------------------------------------------------------ argument checks
def test_check_bf_lcmv():
    from pb_chime5_amd import ops
    bf = ops.check_bf_lcmv(5, 1, None, None, None, 12)
    assert (bf.interferer, bf.candidates, bf.min_mass) == (-1, 0b11101, 24.0)
    bf = ops.check_bf_lcmv(5, 1, 3, [0, 1, 2], 0.5)
    assert (bf.interferer, bf.candidates, bf.min_mass) == (3, 0b00101, 0.5)   # target bit dropped
    assert ops.check_bf_lcmv(5, 1, None, [], None).candidates == 0
    assert ops.check_bf_lcmv(5, 1, None, None, None).min_mass == 0.0
    assert ops.check_bf_lcmv(19, 18, np.int64(0), (np.int32(17),), 3).candidates == 1 << 17
    for bad, word in ((dict(num_classes=0), 'num_classes'), (dict(num_classes=20), 'num_classes'),
                      (dict(target_index=5), 'target_index'), (dict(target_index=-1), 'target_index'),
                      (dict(interferer=5), 'interferer'), (dict(interferer=-1), 'interferer'),
                      (dict(interferer=1), 'interferer'), (dict(interferer=1.0), 'interferer'),
                      (dict(interferer=True), 'interferer'), (dict(candidates=[5]), 'candidates'),
                      (dict(candidates=[0.5]), 'candidates'), (dict(candidates=3), 'candidates'),
                      (dict(candidates='01'), 'candidates'), (dict(min_mass=-1), 'min_mass'),
                      (dict(min_mass=np.nan), 'min_mass'), (dict(min_mass=np.inf), 'min_mass'),
                      (dict(min_mass='8'), 'min_mass'), (dict(min_mass=True), 'min_mass')):
        kw = {**dict(num_classes=5, target_index=1), **bad}
        with pytest.raises(ValueError, match=word):
            ops.check_bf_lcmv(**kw)


def test_stage_argument_errors_before_any_device_work(no_context):
    from pb_chime5_amd import ops
    Y = np.zeros((4, 130, 3), complex)
    m = np.zeros((130, 3))
    with pytest.raises(ValueError, match='Y'):
        ops.lcmv_souden_from_masks(Y[0], m, m, m)
    with pytest.raises(ValueError, match='X_mask'):
        ops.lcmv_souden_from_masks(Y, m[:-1], m, m)
    with pytest.raises(ValueError, match='I_mask'):
        ops.lcmv_souden_from_masks(Y, m, m.T, m)
    with pytest.raises(ValueError, match='N_mask'):
        ops.lcmv_souden_from_masks(Y, m, m, m[:, :2])
    with pytest.raises(ValueError, match='D=1'):
        ops.lcmv_souden_from_masks(Y[:1], m, m, m)
    with pytest.raises(AssertionError, match='D < 30'):
        ops.lcmv_souden_from_masks(np.zeros((30, 130, 3), complex), m, m, m)
    for ref in (-1, 4, 1.0, True):
        with pytest.raises(ValueError, match='ref_channel'):
            ops.lcmv_souden_from_masks(Y, m, m, m, ref_channel=ref)
    for mass in (-1.0, np.nan, np.inf, '2', None):
        with pytest.raises(ValueError, match='min_mass'):
            ops.lcmv_souden_from_masks(Y, m, m, m, min_mass=mass)
    g = np.zeros((3, 130, 3))
    with pytest.raises(ValueError, match='posterior'):
        ops.lcmv_masks_from_posteriors(g[0], 0)
    with pytest.raises(ValueError, match='target_index'):
        ops.lcmv_masks_from_posteriors(g, 3)
    with pytest.raises(ValueError, match='interferer'):
        ops.lcmv_masks_from_posteriors(g, 1, interferer=1)
    with pytest.raises(ValueError, match='candidates'):
        ops.lcmv_masks_from_posteriors(g, 1, candidates=[3])
    with pytest.raises(ValueError, match='start_context_frames'):
        ops.lcmv_masks_from_posteriors(g, 1, start_context_frames=1.5)
    with pytest.raises(ValueError, match='num_classes'):
        ops.lcmv_masks_from_posteriors(np.zeros((20, 4, 3)), 1)


def test_fused_argument_errors_before_any_device_work(no_context):
    from pb_chime5_amd import ops
    obs, act = np.zeros((4, 4096)), np.ones((3, 4096), bool)
    with pytest.raises(ValueError, match='obs'):
        ops.enhance_observation_lcmv(obs[0], act, 0, 0, 0)
    with pytest.raises(ValueError, match='D=1'):
        ops.enhance_observation_lcmv(obs[:1], act, 0, 0, 0)
    with pytest.raises(ValueError, match='target_index'):
        ops.enhance_observation_lcmv(obs, act, 3, 0, 0)
    with pytest.raises(ValueError, match='interferer'):
        ops.enhance_observation_lcmv(obs, act, 0, 0, 0, interferer=0)
    with pytest.raises(ValueError, match='candidates'):
        ops.enhance_observation_lcmv(obs, act, 0, 0, 0, candidates=[7])
    with pytest.raises(ValueError, match='min_mass'):
        ops.enhance_observation_lcmv(obs, act, 0, 0, 0, min_mass=-2)
    for bf in ('gev_ban', 'ch2', 'sum'):
        with pytest.raises(NotImplementedError, match=bf):
            ops.enhance_observation_lcmv(obs, act, 0, 0, 0, bf=bf)


def test_signatures_and_defaults():
    from pb_chime5_amd import ops
    from pb_chime5_amd.speech_enhancement import beamforming_wrapper
    sig = inspect.signature(ops.lcmv_souden_from_masks).parameters
    assert list(sig)[:5] == ['Y', 'X_mask', 'I_mask', 'N_mask', 'ban']
    assert (sig['ban'].default, sig['min_mass'].default, sig['ref_channel'].default,
            sig['ctx'].default) == (False, 0.0, None, None)
    assert sig['min_mass'].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(beamforming_wrapper.beamform_lcmv_souden_from_masks).parameters
    assert list(sig)[:6] == ['Y', 'X_mask', 'I_mask', 'N_mask', 'ban', 'debug']
    assert (sig['ban'].default, sig['debug'].default, sig['ref_channel'].default) == \
        (False, False, None)
    assert sig['ref_channel'].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig['debug'].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD


def test_wrapper_shape_rules(monkeypatch):
    """2-, 3- and 4-dimensional masks (median over channels), NotImplementedError(shape)
    otherwise, min_mass = 0: what reaches the operator."""
    from pb_chime5_amd import ops
    from pb_chime5_amd.speech_enhancement import beamforming_wrapper as bw
    seen = {}

    def fake(Y, X_mask, I_mask, N_mask, ban=False, **kw):
        seen.update(Y=Y, X=X_mask, I=I_mask, N=N_mask, ban=ban, **kw)
        return 'X_hat'
    monkeypatch.setattr(ops, 'lcmv_souden_from_masks', fake)
    rng = np.random.default_rng(0)
    D, T, F = 3, 7, 2
    Y = rng.standard_normal((D, T, F)) + 1j * rng.standard_normal((D, T, F))
    m3 = rng.uniform(size=(3, D, T, F))
    for masks, Yin in (([np.median(m, axis=0) for m in m3], Y), (list(m3), Y),
                       ([m[None] for m in m3], Y[None])):
        seen.clear()
        assert bw.beamform_lcmv_souden_from_masks(Yin, *masks, ban=True, ref_channel=2) == 'X_hat'
        assert np.array_equal(seen['Y'], Y) and seen['ban'] is True
        for key, m in zip('XIN', m3):
            assert np.array_equal(seen[key], np.median(m, axis=0)), key
        assert seen['min_mass'] == 0.0 and seen['ref_channel'] == 2
    bw.beamform_lcmv_souden_from_masks(Y, *[np.median(m, axis=0) for m in m3])
    assert seen['ban'] is False and seen['ref_channel'] is None
    with pytest.raises(NotImplementedError, match=r'\(7,\)'):
        bw.beamform_lcmv_souden_from_masks(Y, *[np.zeros(7)] * 3)
    with pytest.raises(NotImplementedError):
        bw.beamform_lcmv_souden_from_masks(Y, *[np.zeros((1, 1, D, T, F))] * 3)
    with pytest.raises(AssertionError):
        bw.beamform_lcmv_souden_from_masks(np.zeros((30, T, F), complex), *[np.zeros((T, F))] * 3)


# ------------------------------------------------------------------ blocks and front doors
def test_beamformer_defaults_are_untouched():
    from pb_chime5_amd.core import Beamformer
    bf = Beamformer('mvdrSouden_ban', None)
    assert (bf.null_interferer, bf.null_min_mass) == (False, None)
    assert bf == Beamformer(type='mvdrSouden_ban', postfilter=None)
    assert bf != Beamformer('mvdrSouden_ban', None, null_interferer=True)
    for t in ('gev_ban', 'ch2', 'sum'):
        assert Beamformer(t, 'mask_mul').null_interferer is False
    sig = inspect.signature(Beamformer.__call__).parameters
    assert sig['interferer_mask'].default is None
    assert sig['interferer_mask'].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(sig)[:5] == ['self', 'Obs', 'target_mask', 'distortion_mask', 'debug']


def test_beamformer_with_null_interferer(no_context):
    from pb_chime5_amd.core import Beamformer
    assert Beamformer('mvdrSouden_ban', 'mask_mul', null_interferer=True,
                      null_min_mass=3.5).null_min_mass == 3.5
    for t in ('gev_ban', 'ch2', 'sum', 'nonsense'):
        with pytest.raises(NotImplementedError, match=t):
            Beamformer(type=t, postfilter=None, null_interferer=True)
    with pytest.raises(NotImplementedError, match='segment_frames'):
        Beamformer('mvdrSouden_ban', None, segment_frames=256, null_interferer=True)
    for bad in (0, -1.0, np.nan, np.inf, '4', True):
        with pytest.raises(ValueError, match='null_min_mass'):
            Beamformer('mvdrSouden_ban', None, null_interferer=True, null_min_mass=bad)
    with pytest.raises(ValueError, match='null_min_mass'):
        Beamformer('mvdrSouden_ban', None, null_min_mass=4.0)
    Y, m = np.zeros((4, 130, 3), complex), np.zeros((130, 3))
    with pytest.raises(ValueError, match='interferer_mask'):
        Beamformer('mvdrSouden_ban', None, null_interferer=True)(Y, m, m)
    with pytest.raises(ValueError, match='interferer_mask'):
        Beamformer('mvdrSouden_ban', None)(Y, m, m, interferer_mask=m)


def test_beamformer_call_passes_the_masks_and_the_threshold(monkeypatch):
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import Beamformer
    seen = []

    def fake(Y, X_mask, I_mask, N_mask, ban=False, **kw):
        seen.append(dict(X=X_mask, I=I_mask, N=N_mask, ban=ban, **kw))
        return np.ones((130, 3), complex)
    monkeypatch.setattr(ops, 'lcmv_souden_from_masks', fake)
    rng = np.random.default_rng(1)
    Y = np.zeros((6, 130, 3), complex)
    x, i, n = rng.uniform(size=(3, 130, 3))
    out = Beamformer('mvdrSouden_ban', 'mask_mul', null_interferer=True)(
        Y, x, i + n, interferer_mask=i, noise_mask=n)
    assert np.array_equal(out, x)                                   # the postfilter
    assert seen[-1]['ban'] is True and seen[-1]['min_mass'] == 12   # 2 * channels
    assert seen[-1]['N'] is n and seen[-1]['I'] is i and seen[-1]['X'] is x
    Beamformer('mvdrSouden_ban', None, null_interferer=True, null_min_mass=5)(
        Y, x, i + n, interferer_mask=i)
    assert seen[-1]['min_mass'] == 5 and np.allclose(seen[-1]['N'], n, rtol=0, atol=1e-15)


def test_every_front_door_has_the_option_off_by_default_and_carries_it():
    from pb_chime5_amd import core, core_chime6, core_chime6_rttm
    for mod in (core, core_chime6, core_chime6_rttm):
        sig = inspect.signature(mod.get_enhancer).parameters
        assert (sig['bf_null_interferer'].default, sig['bf_null_min_mass'].default) == \
            (False, None), mod.__name__
    for mod in (core, core_chime6):
        assert mod.get_enhancer().bf_block == core.Beamformer('mvdrSouden_ban', None)
        assert not mod.get_enhancer()._bf_null()
        enh = mod.get_enhancer(bf_null_interferer=True, bf_null_min_mass=7.5, wpe_per_array=True,
                               multiarray=True)
        assert type(enh.bf_block) is core.Beamformer and enh._fusable() and enh._bf_null()
        assert enh.bf_block == core.Beamformer('mvdrSouden_ban', None, null_interferer=True,
                                               null_min_mass=7.5)
        for bf in ('gev_ban', 'ch2', 'sum'):
            with pytest.raises(NotImplementedError, match=bf):
                mod.get_enhancer(bf=bf, bf_null_interferer=True)
        with pytest.raises(NotImplementedError, match='segment_frames'):
            mod.get_enhancer(bf_null_interferer=True, bf_segment_frames=256)
        with pytest.raises(NotImplementedError, match='channel_keep'):
            mod.get_enhancer(bf_null_interferer=True, channel_keep=3)
        with pytest.raises(ValueError, match='null_min_mass'):
            mod.get_enhancer(bf_null_interferer=True, bf_null_min_mass=0)


def test_rttm_front_door_takes_the_option(tmp_path):
    from pb_chime5_amd import core
    from pb_chime5_amd.core_chime6_rttm import get_enhancer
    from test_rttm_frontdoor import _make_chime6_dir
    root, rttm, _ = _make_chime6_dir(tmp_path)
    kw = dict(database_rttm=[str(rttm)], activity_rttm=[str(rttm)], chime6_dir=root,
              multiarray='outer_array_mics')
    enh = get_enhancer(**kw, bf_null_interferer=True)
    assert enh.bf_block == core.Beamformer('mvdrSouden_ban', None, null_interferer=True)
    assert get_enhancer(**kw).bf_block == core.Beamformer('mvdrSouden_ban', None)


def test_command_lines_parse_the_keys(monkeypatch):
    from pb_chime5_amd.scripts import run, kaldi_run, kaldi_run_rttm, enhance_rttm
    cfg = run.main(['print_config', 'with', 'bf_null_interferer=True', 'bf_null_min_mass=6.5'])
    assert (cfg['bf_null_interferer'], cfg['bf_null_min_mass']) == (True, 6.5)
    cfg = run.main(['print_config'])
    assert (cfg['bf_null_interferer'], cfg['bf_null_min_mass']) == (False, None)
    assert kaldi_run.main(['print_config', 'with', 'bf_null_interferer=True'])[
        'bf_null_interferer'] is True
    assert kaldi_run_rttm.main(['print_config', 'with', 'database_rttm=a.rttm',
                                'bf_null_interferer=True'])['bf_null_interferer'] is True

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
        enhance_rttm.main(base + ['--bf-null-interferer'])
    assert seen['bf_null_interferer'] is True
    seen.clear()
    with pytest.raises(Stop):
        enhance_rttm.main(base)
    assert seen['bf_null_interferer'] is False


def test_sessions_guided_and_multi_target_methods_refuse_the_option(no_context, tmp_path):
    from pb_chime5_amd.core import get_enhancer
    enh = get_enhancer(bf_null_interferer=True)
    obs = np.zeros((4, 4096))
    act = {'P01': np.ones(4096, bool), 'Noise': np.ones(4096, bool)}
    with pytest.raises(NotImplementedError, match='enhance_session with bf_null_interferer'):
        enh.enhance_session('S02', tmp_path / 'audio')
    assert not (tmp_path / 'audio').exists()
    with pytest.raises(NotImplementedError, match='bf_null_interferer'):
        enh.enhance_observation_guided(obs, {'P01': np.ones(19), 'Noise': np.ones(19)}, 'P01')
    with pytest.raises(NotImplementedError, match='bf_null_interferer'):
        enh.enhance_observation_speakers(obs, act, ['P01'])
    with pytest.raises(NotImplementedError, match='bf_null_interferer'):
        enh.enhance_example_speakers({})


@pytest.mark.parametrize('garbage_class,noise_keys', [
    (True, ['Noise']), (False, ['Noise']), (None, []), (2, ['Noise0', 'Noise1'])])
def test_candidates_exclude_the_target_and_every_garbage_key(garbage_class, noise_keys):
    from pb_chime5_amd.core import get_enhancer
    enh = get_enhancer(bf_null_interferer=True, activity_garbage_class=garbage_class)
    keys = ['P05', 'P06'] + noise_keys[:1] + ['P07', 'P08'] + noise_keys[1:]
    act = {k: np.ones(8, bool) for k in keys}
    for target in ('P05', 'P07', 'P08'):
        got = enh.interferer_candidates(act, target)
        assert got == [i for i, k in enumerate(keys) if k.startswith('P') and k != target]
    # a speaker that happens to be called like another setting's garbage track stays a candidate
    if garbage_class is None:
        assert enh.interferer_candidates({'P05': 1, 'Noise': 1}, 'P05') == [1]
    if garbage_class == 2:
        assert enh.interferer_candidates({'P05': 1, 'Noise': 1, 'Noise0': 1}, 'P05') == [1]


def test_fused_call_gets_the_candidates_and_the_threshold(monkeypatch):
    from pb_chime5_amd import core, ops
    seen = {}

    class Stop(Exception):
        pass

    def fake(obs, activity, target, start, end, **kw):
        seen.update(target=target, **kw)
        raise Stop

    class Ctx:
        def set_utterances_in_flight(self, n):
            pass
    monkeypatch.setattr(ops, 'enhance_observation_lcmv', fake)
    monkeypatch.setattr(core.Enhancer, '_ctx', lambda self: Ctx())
    enh = core.get_enhancer(bf_null_interferer=True, bf_null_min_mass=9, bf_drop_context=False)
    act = {k: np.ones(4096, bool) for k in ('P05', 'P06', 'P07', 'Noise')}
    with pytest.raises(Stop):
        enh.enhance_observation(np.zeros((4, 4096)), act, 'P06')
    assert (seen['target'], seen['candidates'], seen['min_mass']) == (1, [0, 2], 9)


# ------------------------------------------------------------------ the reference module
_crandn = lr.crandn


def test_reference_reproduces_the_rank_one_identity():
    """On exactly rank-one Phi_X = s_x d d^H, Phi_I = s_i a a^H and any Hermitian positive
    definite Phi_N, column r is the textbook LCMV with C = [d a], g = [conj(d_r), 0]: a null on
    a and the explicit formula, both to 1e-12."""
    rng = np.random.default_rng(0)
    for D in (2, 3, 6, 12):
        d, a, M = _crandn(rng, D), _crandn(rng, D), _crandn(rng, D, D)
        phi_n = M @ M.conj().T + 0.1 * np.eye(D)
        W, g = lr.lcmv_matrix(2.0 * np.outer(d, d.conj()), 3.0 * np.outer(a, a.conj()), phi_n)
        assert g.real > 1e-3 and abs(g.imag) < 1e-9 * g.real
        for r in range(D):
            w = W[:, r]
            assert abs(w.conj() @ a) <= 1e-12 * np.linalg.norm(w) * np.linalg.norm(a)
            assert abs(w.conj() @ d - d[r]) <= 1e-12 * np.linalg.norm(d)     # C^H w = g
            want = lr.explicit_lcmv(d, a, phi_n, r)
            assert np.max(np.abs(w - want)) <= 1e-12 * np.max(np.abs(want)), (D, r)


def test_reference_fallback_branch_is_its_own_mvdr_of_the_merged_mask():
    rng = np.random.default_rng(3)
    D, T, F = 5, 130, 4
    Y, xm, im, nm, _ = lr.scene(rng, D, T, F)
    im[:, 2] = 0.0                                   # the interferer is silent in frequency 2
    for ban in (False, True):
        got, det = lr.lcmv_souden_from_masks(Y, xm, im, nm, ban, min_mass=2 * D)
        assert det['fallbacks'].tolist() == [False, False, True, False]
        mvdr, _ = lr.mvdr_souden_from_masks(Y, xm, im + nm, ban, det['ref_channel'])
        assert np.array_equal(got[:, 2], mvdr[:, 2])
        assert np.max(np.abs(got[:, 1] - mvdr[:, 1])) > 1e-3 * np.max(np.abs(mvdr))
    # min_mass = 0 never falls back: W = 0 there, NaN under ban
    plain, det = lr.lcmv_souden_from_masks(Y, xm, im, nm, False, min_mass=0)
    assert not det['fallbacks'].any() and np.all(plain[:, 2] == 0)
    nan, _ = lr.lcmv_souden_from_masks(Y, xm, im, nm, True, min_mass=0,
                                       ref_channel=det['ref_channel'])
    assert np.all(np.isnan(nan[:, 2])) and np.all(np.isfinite(nan[:, [0, 1, 3]]))


def test_reference_solve_takes_lstsq_on_an_exactly_singular_matrix():
    rng = np.random.default_rng(4)
    M = _crandn(rng, 4, 4)
    A = M @ M.conj().T
    A[2, :] = 0
    A[:, 2] = 0
    B = _crandn(rng, 4, 3)
    X = lr.solve(A, B)
    assert np.all(X[2] == 0)                         # minimum norm: nothing on the dead channel
    keep = [0, 1, 3]
    assert np.allclose(X[keep], np.linalg.solve(A[np.ix_(keep, keep)], B[keep]))


def test_reference_pick_and_masks():
    rng = np.random.default_rng(5)
    K, T, F = 5, 20, 3
    g = rng.uniform(size=(K, T, F)) * np.array([1.0, 0.7, 3.0, 2.0, 0.5])[:, None, None]
    assert lr.pick_interferer(g, 1, [0, 2, 3]) == 2
    assert lr.pick_interferer(g, 1, [0, 3]) == 3          # the largest is no candidate
    assert lr.pick_interferer(g, 2, [0, 1, 2, 3]) == 3    # the target is none either
    assert lr.pick_interferer(g, 1, []) == -1
    assert lr.pick_interferer(np.zeros_like(g), 1, [0, 2]) == -1
    tie = np.ones((3, 4, 2))
    assert lr.pick_interferer(tie, 0, [2, 1]) == 1        # equal masses: the lower index
    # the context decides: class 0 lives in the first frames only
    g2 = g.copy()
    g2[0, :5] = 100.0
    assert lr.pick_interferer(g2, 1, [0, 2]) == 0
    assert lr.pick_interferer(g2, 1, [0, 2], start=5, end=0) == 2
    x, i, n = lr.masks_from_posteriors(g, 1, 3, start=2, end=3)
    z = lr.zero_context(g, 2, 3)
    assert np.all(z[:, :2] == 0) and np.all(z[:, -3:] == 0) and np.array_equal(z[:, 2:-3], g[:, 2:-3])
    assert np.array_equal(x, z[1]) and np.array_equal(i, z[3])
    assert np.array_equal(n, (z[0] + z[2]) + z[4])
    assert np.array_equal(lr.zero_context(g, 2, 0)[:, 2:], g[:, 2:])        # end = 0: no tail
    x, i, n = lr.masks_from_posteriors(g, 1, -1)
    assert np.all(i == 0) and np.array_equal(n, ((g[0] + g[2]) + g[3]) + g[4])
