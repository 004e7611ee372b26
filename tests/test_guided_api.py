"""Weighted and per-frequency guidance of the CACGMM (gss_cacgmm_guided,
gss_enhance_observation_guided): the C ABI, the binding, the host helpers and the dispatch rule
of GSS.__call__, without a GPU."""
import ctypes
import re

import numpy as np
import pytest

import gss_oracle as oracle
from conftest import REPO

HEADER = (REPO / 'include' / 'gss_hip.h').read_text()
ENTRY_POINTS = ('gss_cacgmm_guided', 'gss_enhance_observation_guided')


def test_both_entry_points_in_header_binding_and_library():
    from pb_chime5_amd import _capi
    lib = _capi.load_library()
    for name in ENTRY_POINTS:
        assert re.search(r'\bint\s+' + name + r'\s*\(', HEADER), name
        assert name in _capi.SIGNATURES
        assert hasattr(lib, name)
        # the descriptor goes by pointer, after the observation's shape
        assert ctypes.POINTER(_capi.GssGuidance) in _capi.SIGNATURES[name][1]


def test_abi_revision_stays_7_and_the_header_says_why():
    from pb_chime5_amd import _capi
    assert _capi.GSS_ABI_VERSION == 7
    assert _capi.load_library().gss_abi_version() == 7
    assert '#define GSS_ABI_VERSION 7' in HEADER
    comment = HEADER[HEADER.index('ABI revision of this header'):HEADER.index('#define GSS_ABI_VERSION')]
    for name in ENTRY_POINTS:
        assert name in comment, name


def test_guidance_struct_matches_the_header_layout():
    from pb_chime5_amd import _capi
    body = HEADER[:HEADER.index('} gss_guidance;')].rsplit('typedef struct {', 1)[1]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = re.findall(r'([a-z_0-9]+)\s*;', body)
    assert fields == ['init_dev', 'mask_dev', 'init_f_stride', 'init_k_stride', 'mask_f_stride',
                      'mask_k_stride']
    assert [n for n, _ in _capi.GssGuidance._fields_] == fields
    assert ctypes.sizeof(_capi.GssGuidance) == 2 * ctypes.sizeof(ctypes.c_void_p) + 4 * 8


def test_a_library_without_the_symbols_is_named_in_the_error(tmp_path, monkeypatch):
    """The binding's missing-symbol message covers the two entry points: they came without a
    new ABI revision, so an older build of revision 7 passes the revision check."""
    from pb_chime5_amd import _capi
    present = dict(_capi.SIGNATURES)
    monkeypatch.setitem(_capi.SIGNATURES, 'gss_cacgmm_guided_absent', present['gss_cacgmm_guided'])
    with pytest.raises(_capi.GssError, match='gss_cacgmm_guided_absent'):
        _capi.load_library(_capi.LIB_PATH)


@pytest.mark.parametrize('kind', ['bool', 'uint8', 'float01', 'weighted', 'weighted_ktf'])
def test_guidance_from_activity_equals_the_oracle(kind):
    from pb_chime5_amd import ops
    rng = np.random.default_rng(3)
    act = rng.random((4, 50)) < 0.6
    act[-1] = True
    a = {'bool': act, 'uint8': act.astype(np.uint8), 'float01': act.astype(np.float64),
         'weighted': act * rng.uniform(0.05, 1.0, act.shape),
         'weighted_ktf': act[..., None] * rng.uniform(0.05, 1.0, act.shape + (3,))}[kind]
    init, mask = ops.guidance_from_activity(a)
    want_init, want_mask = oracle.gss_initialization(a)
    assert init.dtype == np.float64 and mask.dtype == bool
    assert np.array_equal(init, want_init) and np.array_equal(mask, want_mask)
    assert np.array_equal(mask, np.asarray(a) != 0)
    if kind.startswith('weighted'):
        # the weights are in the initialisation, not only their support
        assert not np.array_equal(init, oracle.gss_initialization(a != 0)[0])


def test_dispatch_rule_of_the_gss_block():
    """Which inputs of GSS.__call__ take the unweighted call: a (K,T) activity whose non-zero
    values are all 1 and no initialisation.  Everything else must not be binarised."""
    from pb_chime5_amd.ops import activity_is_binary
    act = np.array([[1, 0, 1, 1], [1, 1, 1, 1]])
    for a in (act.astype(bool), act.astype(np.uint8), act.astype(np.int64), act.astype(np.float64),
              act.astype(np.float32), act.astype(bool).tolist()):
        assert activity_is_binary(a)
    assert activity_is_binary(np.zeros((2, 4)))
    w = act * 0.3
    assert not activity_is_binary(w)
    assert not activity_is_binary(act.astype(np.uint8) * 2)
    assert not activity_is_binary(np.where(act == 1, np.nan, 0.0))
    assert not activity_is_binary(np.where(act == 1, -1.0, 0.0))
    assert not activity_is_binary(np.repeat(act[..., None], 3, axis=-1))      # (K,T,F)
    assert not activity_is_binary(act.astype(bool), initialization=np.full((2, 4), 0.5))


def test_gss_block_dispatches_by_that_rule(monkeypatch):
    from pb_chime5_amd import core, ops
    calls = []
    monkeypatch.setattr(ops, 'cacgmm_posteriors',
                        lambda Obs, act, **kw: calls.append(('binary', act, kw)) or 'B')
    monkeypatch.setattr(ops, 'cacgmm_posteriors_guided',
                        lambda Obs, init, mask, **kw: calls.append(('guided', init, mask, kw)) or 'G')
    gss = core.GSS(iterations=7, iterations_post=2)
    act = np.array([[True, False, True], [True, True, True]])
    assert gss(None, act) == 'B'
    assert calls[-1][0] == 'binary' and calls[-1][1] is act
    assert calls[-1][2] == dict(iterations=7, iterations_post=2)
    assert gss(None, act.astype(np.float64)) == 'B'
    w = act * np.array([[0.2, 0.0, 0.7], [1.0, 0.5, 0.9]])
    assert gss(None, w, debug=True) == 'G'
    kind, init, mask, kw = calls[-1]
    assert kind == 'guided' and kw == dict(iterations=7, iterations_post=2)
    assert np.array_equal(init, oracle.gss_initialization(w)[0]) and np.array_equal(mask, act)
    assert np.array_equal(gss.locals['initialization'], init)
    assert np.array_equal(gss.locals['source_active_mask'], act)
    mine = np.full((2, 3), 0.5)
    assert gss(None, act, initialization=mine) == 'G'
    assert calls[-1][1] is mine and np.array_equal(calls[-1][2], act)
    # debug locals of the unweighted call as before
    assert gss(None, act, debug=True) == 'B'
    assert np.array_equal(gss.locals['initialization'], oracle.gss_initialization(act)[0])
    assert np.array_equal(gss.locals['source_active_mask'], act)


def test_guidance_tables_shapes():
    from pb_chime5_amd.ops import guidance_tables
    K, T, F = 3, 10, 4
    rng = np.random.default_rng(0)
    init_kt = rng.random((K, T + 5))
    mask_ktf = rng.random((K, T + 2, F)) < 0.5
    init, mask, k = guidance_tables(init_kt, mask_ktf, T, F)
    assert k == K
    assert init.shape == (K, T) and init.dtype == np.float64 and init.flags.c_contiguous
    assert np.array_equal(init, init_kt[:, :T])                   # cut like the activity
    assert mask.shape == (F, K, T) and mask.dtype == np.uint8 and mask.flags.c_contiguous
    assert np.array_equal(mask, mask_ktf[:, :T].transpose(2, 0, 1))
    # any non-zero value is "active"
    _, mask, _ = guidance_tables(None, np.array([[0.0, 0.25, 2.0, np.nan]]), 4, F)
    assert mask.tolist() == [[0, 1, 1, 1]]
    assert guidance_tables(init_kt, None, T, F)[1] is None
    assert guidance_tables(None, mask_ktf, T, F)[0] is None


@pytest.mark.parametrize('init_shape,mask_shape,match', [
    (None, None, 'both None'),
    ((3, 9), None, 'initialization: 9 frames'),
    (None, (3, 9, 4), 'source_activity_mask: 9 frames'),
    ((3, 10, 5), None, 'initialization: 5 frequencies'),
    ((3, 10), (2, 10), 'source_activity_mask: 2 classes'),
    ((10,), None, r'initialization: shape \(10,\)'),
    (None, (3, 10, 4, 1), 'source_activity_mask: shape'),
])
def test_guidance_tables_value_errors(init_shape, mask_shape, match):
    from pb_chime5_amd import ops
    init = None if init_shape is None else np.ones(init_shape)
    mask = None if mask_shape is None else np.ones(mask_shape, bool)
    with pytest.raises(ValueError, match=match):
        ops.guidance_tables(init, mask, 10, 4)
    # the ops check the shapes before they touch a device
    with pytest.raises(ValueError, match=match):
        ops.cacgmm_posteriors_guided(np.zeros((2, 10, 4), complex), init, mask)


def test_enhancer_guided_rejects_mismatched_speakers():
    from pb_chime5_amd.core import get_enhancer
    enh = get_enhancer()
    guidance = {'P01': np.ones(5), 'P02': np.ones(5)}
    with pytest.raises(ValueError, match='different speakers'):
        enh.enhance_observation_guided(np.zeros((4, 2048)), guidance, 'P01', ex=None,
                                       initialization={'P02': np.ones(5), 'P01': np.ones(5)})
