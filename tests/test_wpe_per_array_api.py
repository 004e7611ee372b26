"""Per-array WPE (gss_params.wpe_arrays, get_enhancer(wpe_per_array=True)): the C ABI, the
parameter plumbing and the front doors, without a GPU."""
import inspect
import re

import numpy as np
import pytest

from conftest import REPO


def _header_struct_fields(name):
    text = (REPO / 'include' / 'gss_hip.h').read_text()
    body = re.search(r'typedef struct \{(.*?)\}\s*' + name + ';', text, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    return re.findall(r'\bint\s+([a-z_0-9]+)\s*;', body)


def test_make_params_wpe_arrays_round_trips_into_the_header_layout():
    import ctypes
    from pb_chime5_amd import ops, _capi
    fields = _header_struct_fields('gss_params')
    assert fields[-1] == 'wpe_arrays'
    assert [n for n, _ in _capi.GssParams._fields_] == fields
    assert ctypes.sizeof(_capi.GssParams) == 4 * len(fields)
    p = ops.make_params(wpe_arrays=6)
    raw = bytes(p)
    assert np.frombuffer(raw, np.int32)[fields.index('wpe_arrays')] == 6
    assert _capi.GssParams.from_buffer_copy(raw).wpe_arrays == 6
    # the default is the joint WPE of the reference, as before the field existed
    assert ops.make_params().wpe_arrays == 0
    assert ops.make_params(wpe_arrays=1).wpe_arrays == 1


def test_abi_revision_7_everywhere():
    from pb_chime5_amd import _capi
    assert _capi.GSS_ABI_VERSION == 7
    assert _capi.load_library().gss_abi_version() == 7
    text = (REPO / 'include' / 'gss_hip.h').read_text()
    assert '#define GSS_ABI_VERSION 7' in text
    assert 'revision 7' in text
    assert 'gss_wpe_arrays' in _capi.SIGNATURES


def test_every_front_door_has_wpe_per_array_off_by_default():
    from pb_chime5_amd import core, core_chime6, core_chime6_rttm
    for mod in (core, core_chime6, core_chime6_rttm):
        param = inspect.signature(mod.get_enhancer).parameters['wpe_per_array']
        assert param.default is False, mod.__name__
    assert core.Enhancer.wpe_per_array is False
    enh = core.get_enhancer(multiarray=True, wpe_per_array=True)
    assert enh.wpe_per_array is True
    assert core.get_enhancer(multiarray=True).wpe_per_array is False
    assert core_chime6.get_enhancer(multiarray='outer_array_mics',
                                    wpe_per_array=True).wpe_per_array is True


def test_rttm_front_door_takes_wpe_per_array(tmp_path):
    from pb_chime5_amd.core_chime6_rttm import get_enhancer
    from test_rttm_frontdoor import _make_chime6_dir
    root, rttm, _ = _make_chime6_dir(tmp_path)
    enh = get_enhancer(database_rttm=[str(rttm)], activity_rttm=[str(rttm)], chime6_dir=root,
                       multiarray='outer_array_mics', wpe_per_array=True)
    assert enh.wpe_per_array is True
    ex = enh.get_dataset('S02')[0]
    # a flat list of channel files: A = D / 2 for the outer microphones of three arrays
    assert len(ex['audio_path']) == 6 and enh.wpe_arrays(ex, 6) == 3


def test_command_line_picks_up_wpe_per_array():
    from pb_chime5_amd.scripts import run, kaldi_run, kaldi_run_rttm
    cfg = run.main(['print_config', 'with', 'multiarray', 'wpe_per_array=True'])
    assert cfg['wpe_per_array'] is True and cfg['multiarray'] is True
    assert run.main(['print_config', 'with', 'multiarray'])['wpe_per_array'] is False
    cfg = kaldi_run.main(['print_config', 'with', 'multiarray=True', 'wpe_per_array=True'])
    assert cfg['wpe_per_array'] is True
    cfg = kaldi_run_rttm.main(['print_config', 'with', 'database_rttm=a.rttm',
                               'wpe_per_array=True'])
    assert cfg['wpe_per_array'] is True


def test_arrays_must_divide_the_channels():
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import get_enhancer
    assert ops.check_wpe_arrays(6, 24) == 6 and ops.check_wpe_arrays(0, 7) == 1
    assert ops.check_wpe_arrays(None, 5) == 1
    for bad in (-1, 2.5, True, '6'):
        with pytest.raises(ValueError):
            ops.check_wpe_arrays(bad, 24)
    with pytest.raises(ValueError, match='does not divide'):
        ops.check_wpe_arrays(5, 24)
    with pytest.raises(ValueError):
        ops.params_for(ops.make_params(wpe_arrays=6), 20)
    with pytest.raises(ValueError):
        ops.params_for(ops.make_params(), 20, wpe_arrays=6)
    assert ops.params_for(ops.make_params(), 24, wpe_arrays=6).wpe_arrays == 6
    # the fused call checks before anything reaches the device
    with pytest.raises(ValueError):
        ops.enhance_observation(np.zeros((10, 4096)), np.ones((2, 4096), bool), 0, 0, 0,
                                wpe_arrays=4)
    enh = get_enhancer(multiarray=True, wpe_per_array=True)
    with pytest.raises(ValueError):
        enh.wpe_arrays(None, 22)
    with pytest.raises(ValueError):
        enh.enhance_observation(np.zeros((24, 4096)), {'P01': np.ones(4096, bool)}, 'P01',
                                ex=None, wpe_arrays=5)


def test_number_of_arrays_comes_from_the_example_and_the_mode():
    from pb_chime5_amd.core import get_enhancer
    ex6 = {'audio_path': {'observation': {f'U0{i}': [f'U0{i}.CH{c}.wav' for c in range(1, 5)]
                                          for i in range(1, 7)}}}
    ex5 = {'audio_path': {'observation': {f'U0{i}': [] for i in range(1, 6)}}}
    for multiarray, C in ((True, 4), ('outer_array_mics', 2), ('first_array_mics', 1)):
        enh = get_enhancer(multiarray=multiarray, wpe_per_array=True)
        assert enh.wpe_arrays(ex6, 6 * C) == 6
        assert enh.wpe_arrays(ex5, 5 * C) == 5
        assert enh.wpe_arrays(None, 6 * C) == 6
        with pytest.raises(ValueError):
            enh.wpe_arrays(ex6, 5 * C)
    # one array, or the option off: one joint WPE
    assert get_enhancer(multiarray=False, wpe_per_array=True).wpe_arrays(ex6, 4) == 1
    assert get_enhancer(multiarray=True).wpe_arrays(ex6, 24) == 1


def test_without_wpe_the_flag_has_no_effect():
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import get_enhancer
    enh = get_enhancer(multiarray=True, wpe=False, wpe_per_array=True)
    assert enh.wpe_block is None
    assert enh.wpe_arrays(None, 24) == 1 and enh.wpe_arrays(None, 22) == 1
    # the C side does not read the field without WPE: no divisibility check either
    assert ops.params_for(ops.make_params(wpe=False, wpe_arrays=6), 22).wpe_arrays == 6
