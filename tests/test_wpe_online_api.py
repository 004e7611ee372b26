"""Online WPE (gss_wpe_online, get_enhancer(wpe_online=True)): the NumPy reference itself
(tests/online_wpe_reference.py: the recursion against the closed form of its least-squares
problem, blocks against one call, the silence rule, the dereverberation evidence), the C ABI, the
argument checks, the parameter plumbing and the front doors, without a GPU."""
import ctypes
import inspect

import numpy as np
import pytest

import online_wpe_reference as wr
from conftest import REPO

SYMBOLS = ('gss_wpe_online_init', 'gss_wpe_online', 'gss_enhance_observation_wpe_online')


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
@pytest.mark.parametrize('cell', [(1, 4, 10, 2, 0.9999, 3, 150), (1, 2, 2, 1, 0.999, 2, 70),
                                  (1, 4, 3, 2, 0.99, 2, 130), (2, 3, 4, 1, 0.995, 2, 60),
                                  (1, 2, 2, 1, 1.0, 3, 70)], ids=str)
def test_reference_is_the_weighted_least_squares_problem(cell):
    """G and P after T frames equal R^-1 B and R^-1 of the exponentially weighted normal
    equations, which share only w, sigma and y with the recursion.  1e-10 relative (measured:
    <= 1.1e-13)."""
    A, C, taps, delay, alpha, F, T = cell
    Y = wr.scene(cell)
    _, st = wr.online_wpe(Y, taps, delay, alpha, A)
    P, G = wr.closed_form(Y, taps, delay, alpha, A)
    errs = wr.rel_err(st['G'], G), wr.rel_err(st['P'], P)
    print(cell, 'G, P vs closed form:', errs)
    assert max(errs) < 1e-10, errs
    # P stays Hermitian to rounding
    assert wr.rel_err(st['P'], st['P'].conj().swapaxes(-1, -2)) < 1e-13


@pytest.mark.parametrize('cell', wr.CHUNK_CELLS, ids=str)
def test_reference_in_blocks_equals_one_call(cell):
    A, C, taps, delay, alpha, F, T = cell
    Y = wr.scene(cell)
    X, st = wr.reference(cell)
    state, out, t0 = None, [], 0
    for n in wr.CHUNKS[T]:
        x, state = wr.online_wpe(Y[:, t0:t0 + n], taps, delay, alpha, A, state)
        out.append(x)
        t0 += n
    assert t0 == T
    assert np.array_equal(np.concatenate(out, axis=1), X)
    for k in ('P', 'G', 'hist'):
        assert np.array_equal(state[k], st[k]), k


def test_reference_silence_rule():
    """A block of zeros in every channel longer than L + 1 frames: finite output, and P and G do
    not move over the frames whose whole buffer is zero (the literal recursion gives NaN)."""
    cell = wr.ONCHIP_CELLS[0]
    A, C, taps, delay, alpha, F, T = cell
    L = taps + delay
    Y = wr.silence_scene(cell, 'block')
    n0, length = T // 2, 2 * (L + 1)
    X, st = wr.online_wpe(Y, taps, delay, alpha, A)
    assert np.all(np.isfinite(X)) and all(np.all(np.isfinite(v)) for v in st.values())
    # frames n0 + L .. n0 + length - 1 see nothing but zeros
    _, before = wr.online_wpe(Y[:, :n0 + L], taps, delay, alpha, A)
    _, after = wr.online_wpe(Y[:, :n0 + length], taps, delay, alpha, A)
    assert np.array_equal(before['P'], after['P']) and np.array_equal(before['G'], after['G'])
    assert np.all(X[:, n0 + L:n0 + length] == 0)
    # ... and the filter goes on afterwards
    _, later = wr.online_wpe(Y[:, :n0 + length + 1], taps, delay, alpha, A)
    assert not np.array_equal(later['P'], after['P'])
    # one silent channel among live ones is no silence
    Xc, stc = wr.online_wpe(wr.silence_scene(cell, 'channel'), taps, delay, alpha, A)
    assert np.all(np.isfinite(Xc)) and np.all(np.isfinite(stc['P'])) and np.all(Xc[:, :, 1] == 0)


@pytest.mark.parametrize('cell', wr.EVIDENCE_CELLS, ids=str)
def test_reference_output_carries_less_energy_than_the_input(cell):
    ratio = wr.evidence_ratio(cell)
    print(cell, 'second-half energy out / in:', ratio)
    assert ratio < 0.9, ratio


def test_parity_scenes_are_stable():
    """The rule that keeps a seed: the reference itself moves at least STABILITY_MARGIN x less
    than the bar under a last-bit change of the input."""
    for cell in wr.CELLS:
        moved = wr.reference_movement(cell, wr.seed_of(cell))
        assert moved * wr.STABILITY_MARGIN <= wr.TOL, (cell, moved)
    assert wr.ONCHIP_CELLS[-1][1] * wr.ONCHIP_CELLS[-1][2] == wr.ONCHIP_MAX_N
    assert wr.MEMORY_CELLS[0][1] * wr.MEMORY_CELLS[0][2] == wr.ONCHIP_MAX_N + 1
    for cell in wr.LONG_CELLS:
        moved = wr.long_reference_movement(cell, wr.long_seed_of(cell))
        assert moved * wr.STABILITY_MARGIN <= wr.TOL, (cell, moved)
    assert [c[1] * c[2] for c in wr.LONG_CELLS] == [40, 120, 12]


def test_long_reference_is_its_closed_form():
    """After thousands of frames the recursion still solves its weighted least-squares problem,
    also with one channel at 1e-7 of the others."""
    for cell in wr.LONG_CELLS:
        st = wr.long_reference(cell, wr.long_seed_of(cell))[1]
        P, G = wr.long_closed_form(cell, wr.long_seed_of(cell))
        errs = wr.rel_err(st['P'], P), wr.rel_err(st['G'], G)
        print(f'{cell}: P, G vs the closed form {errs}')
        assert max(errs) < wr.CLOSED_FORM_TOL, (cell, errs)


# ------------------------------------------------------------------ the C surface
def test_the_built_library_exports_the_online_wpe_entry_points():
    from pb_chime5_amd import _capi, build
    assert 'wpe_online.hip' in build.SOURCES
    lib = _capi.load_library()
    header = (REPO / 'include' / 'gss_hip.h').read_text()
    for name in SYMBOLS:
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
        assert f'int {name}(' in header, name
    # entry points only: the revision is the one the per-array WPE pinned
    assert _capi.GSS_ABI_VERSION == 7 and lib.gss_abi_version() == 7


def test_descriptor_layouts_are_the_header_structs():
    from pb_chime5_amd import _capi
    header = (REPO / 'include' / 'gss_hip.h').read_text()
    for decl in ('gss_cplx *inv_cov_dev;', 'gss_cplx *filter_dev;', 'gss_cplx *history_dev;',
                 '} gss_wpe_online_state;', 'typedef struct { double alpha; } gss_wpe_online_cfg;'):
        assert decl in header, decl
    S = _capi.GssWpeOnlineState
    assert [n for n, _ in S._fields_] == ['inv_cov_dev', 'filter_dev', 'history_dev']
    assert [getattr(S, n).offset for n, _ in S._fields_] == [0, 8, 16] and ctypes.sizeof(S) == 24
    assert [n for n, _ in _capi.GssWpeOnlineCfg._fields_] == ['alpha']
    assert ctypes.sizeof(_capi.GssWpeOnlineCfg) == 8
    # the fused entry is one of the table's, with its descriptor before out_dev
    from pb_chime5_amd import ops
    assert ops._FUSED_ENTRIES['wpe_online'] == ('gss_enhance_observation_wpe_online', None,
                                                'online WPE')
    assert _capi.SIGNATURES['gss_enhance_observation_wpe_online'] == \
        _capi._fused(ctypes.POINTER(_capi.GssWpeOnlineCfg))


def test_the_switch_is_read_in_the_api_unit_and_documented():
    api = (REPO / 'pb_chime5_amd' / 'csrc' / 'gss_api.hip').read_text()
    assert 'gss_variant_set("wpe_online_mem")' in api
    unit = (REPO / 'pb_chime5_amd' / 'csrc' / 'wpe_online.hip').read_text()
    assert 'getenv' not in unit and 'gss_variant' not in unit
    assert 'atomicAdd' not in unit and '__atomic' not in unit and '__hip_atomic' not in unit
    doc = (REPO / 'INTEGRATION.md').read_text()
    assert '`wpe_online_mem`' in doc and 'gss_wpe_online_state' in doc


def test_every_compiled_kernel_of_the_unit_has_a_named_gpu_cell():
    """The kernels of wpe_online.hip in the built library (none of them a template) and the test
    of tests/test_gpu_wpe_online.py that launches each."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, str(REPO / 'tools' / 'kernel_coverage.py'), 'list'],
                         capture_output=True, text=True, check=True).stdout.splitlines()
    reached_by = {
        'wpe_online_sigma_kernel': 'test_onchip_form_against_the_reference',
        'wpe_online_identity_kernel': 'test_onchip_form_against_the_reference',
        'wpe_online_history_kernel': 'test_onchip_form_against_the_reference',
        'wpe_online_onchip_kernel': 'test_onchip_form_against_the_reference',
        'wpe_online_mem_kernel': 'test_memory_form_against_the_reference',
    }
    assert sorted(n for n in out if 'wpe_online' in n) == sorted(reached_by)
    gpu = (REPO / 'tests' / 'test_gpu_wpe_online.py').read_text()
    for test in set(reached_by.values()):
        assert f'def {test}(' in gpu, test


# ------------------------------------------------------------------ argument checks
def test_check_wpe_online(no_context):
    from pb_chime5_amd import ops
    assert ops.check_wpe_online(10, 2, 0.9999, 24, 6) == (6, 4)
    assert ops.check_wpe_online(10, 2, 1.0, 4, 1) == (1, 4)
    assert ops.check_wpe_online(1, 0, 0.5) == (1, None)
    assert ops.check_wpe_online(16, 2, 0.9999, 32, 0) == (1, 32)        # n = 512
    sig = inspect.signature(ops.check_wpe_online).parameters
    assert list(sig) == ['taps', 'delay', 'alpha', 'num_channels', 'arrays']
    assert ops.WPE_ONLINE_ALPHA == 0.9999 == sig['alpha'].default
    for kw, word in ((dict(taps=0), 'taps'), (dict(taps=2.0), 'taps'), (dict(taps=True), 'taps'),
                     (dict(delay=-1), 'delay'), (dict(delay=1.5), 'delay'),
                     (dict(alpha=0.0), 'alpha'), (dict(alpha=1.0001), 'alpha'),
                     (dict(alpha=float('nan')), 'alpha'), (dict(alpha='a'), 'alpha'),
                     (dict(alpha=-0.5), 'alpha'), (dict(num_channels=0), 'num_channels'),
                     (dict(num_channels=4, arrays=3), 'wpe_arrays'),
                     (dict(num_channels=4, arrays=-1), 'wpe_arrays')):
        with pytest.raises(ValueError, match=word):
            ops.check_wpe_online(**{**dict(taps=10, delay=2, alpha=0.9), **kw})
    with pytest.raises(NotImplementedError, match='512'):
        ops.check_wpe_online(22, 2, 0.9, 24)                            # n = 528
    with pytest.raises(NotImplementedError, match='num_channels'):
        ops.check_wpe_online(1, 0, 0.9, 33)


def test_stage_argument_errors_before_any_device_work(no_context):
    from pb_chime5_amd import ops
    Y = np.zeros((4, 30, 3), complex)
    for kw, word in ((dict(taps=0), 'taps'), (dict(delay=-1), 'delay'), (dict(alpha=2.0), 'alpha'),
                     (dict(arrays=3), 'wpe_arrays'), (dict(state='x'), 'state')):
        with pytest.raises(ValueError, match=word):
            ops.wpe_online_dtf(Y, **kw)
    with pytest.raises(ValueError, match='Obs'):
        ops.wpe_online_dtf(Y[0])
    with pytest.raises(ValueError, match='taps'):
        ops.OnlineWPEState.fresh(3, 1, 4, 0, 2)
    with pytest.raises(ValueError, match='F='):
        ops.OnlineWPEState.fresh(0, 1, 4, 10, 2)
    with pytest.raises(NotImplementedError, match='512'):
        ops.OnlineWPEState.fresh(3, 1, 32, 17, 2)
    with pytest.raises(ValueError, match='filter'):
        ops.OnlineWPEState.from_host(dict(filter=np.zeros((2, 3)), taps=1, delay=0))
    from pb_chime5_amd import online_wpe
    with pytest.raises(ValueError, match='alpha'):
        online_wpe.OnlineWPE(10, 2, 0.0, 4, 5)
    with pytest.raises(ValueError, match='frequency_bins'):
        online_wpe.OnlineWPE(10, 2, 0.9, 4, 0)
    sig = inspect.signature(online_wpe.OnlineWPE.__init__).parameters
    assert list(sig)[1:7] == ['taps', 'delay', 'alpha', 'channel', 'frequency_bins', 'arrays']
    sig = inspect.signature(ops.wpe_online_dtf).parameters
    assert [sig[k].default for k in ('taps', 'delay', 'alpha', 'arrays', 'state', 'ctx')] == \
        [10, 2, 0.9999, 1, None, None]


def test_state_shapes_and_a_mismatched_state(monkeypatch):
    """The buffers of a state and the rule that a call takes only the state built for it --
    on a context that allocates nothing."""
    from pb_chime5_amd import ops

    class Buf:
        def __init__(self, n):
            self.nbytes, self.ptr = n, 4096

    class Ctx:
        def empty(self, n):
            return Buf(n)
    st = ops.OnlineWPEState(Ctx(), 5, 2, 3, 4, 1)
    assert st.shapes == {'inv_cov': (5, 2, 12, 12), 'filter': (5, 2, 12, 3), 'history': (5, 2, 5, 3)}
    assert {k: b.nbytes for k, b in st.bufs.items()} == \
        {'inv_cov': 16 * 5 * 2 * 144, 'filter': 16 * 5 * 2 * 36, 'history': 16 * 5 * 2 * 15}
    assert st.key == (5, 2, 3, 4, 1) and (st.n, st.L) == (12, 5)
    s = st.struct()
    assert (s.inv_cov_dev, s.filter_dev, s.history_dev) == (4096, 4096, 4096)
    Obs = np.zeros((6, 9, 5), complex)
    for kw in (dict(taps=4, delay=1, arrays=3), dict(taps=4, delay=2, arrays=2),
               dict(taps=3, delay=1, arrays=2)):
        with pytest.raises(ValueError, match='state'):
            ops.wpe_online_dtf(Obs, alpha=0.9, state=st, **kw)
    with pytest.raises(ValueError, match='state'):
        ops.wpe_online_dtf(Obs[:, :, :4], 4, 1, 0.9, arrays=2, state=st)
    with pytest.raises(ValueError, match='context'):
        ops.wpe_online_dtf(Obs, 4, 1, 0.9, arrays=2, state=st, ctx=Ctx())


def test_fused_argument_errors_before_any_device_work(no_context):
    from pb_chime5_amd import ops
    obs, act = np.zeros((4, 4096)), np.ones((3, 4096), bool)
    with pytest.raises(ValueError, match='obs'):
        ops.enhance_observation_wpe_online(obs[0], act, 0, 0, 0)
    for kw, word in ((dict(alpha=0.0), 'alpha'), (dict(wpe_taps=0), 'taps'),
                     (dict(wpe_delay=-1), 'delay'), (dict(wpe=False), 'wpe=False'),
                     (dict(wpe_psd_context=1), 'wpe_psd_context'), (dict(wpe_arrays=3), 'wpe_arrays')):
        with pytest.raises(ValueError, match=word):
            ops.enhance_observation_wpe_online(obs, act, 0, 0, 0, **kw)
    with pytest.raises(NotImplementedError, match='512'):
        ops.enhance_observation_wpe_online(np.zeros((24, 4096)), act, 0, 0, 0, wpe_taps=22)


# ------------------------------------------------------------------ the WPE block
def test_wpe_block_offline_calls_what_it_called_before(monkeypatch):
    from pb_chime5_amd import core, ops
    seen = []
    monkeypatch.setattr(ops, 'wpe_dtf', lambda Obs, **kw: seen.append(('wpe_dtf', kw)) or Obs)
    monkeypatch.setattr(ops, 'wpe_arrays_dtf',
                        lambda Obs, A, **kw: seen.append(('wpe_arrays_dtf', A, kw)) or Obs)

    def boom(*a, **k):
        raise AssertionError('the online call')
    monkeypatch.setattr(ops, 'wpe_online_dtf', boom)
    block = core.WPE(taps=7, delay=3, iterations=2, psd_context=1)
    assert (block.online, block.alpha) == (False, 0.9999)
    assert block == core.WPE(7, 3, 2, 1, online=False)
    kw = dict(taps=7, delay=3, iterations=2, psd_context=1)
    block(np.zeros((4, 9, 3), complex))
    block(np.zeros((2, 2, 9, 3), complex), stack=True)
    block(np.zeros((2, 2, 9, 3), complex), stack=False)
    assert seen == [('wpe_dtf', kw), ('wpe_dtf', kw), ('wpe_arrays_dtf', 2, kw)]


def test_wpe_block_online(monkeypatch):
    from pb_chime5_amd import core, ops
    seen = []

    def fake(Obs, **kw):
        seen.append((Obs.shape, kw))
        return Obs + 1
    monkeypatch.setattr(ops, 'wpe_online_dtf', fake)

    def boom(*a, **k):
        raise AssertionError('the offline call')
    monkeypatch.setattr(ops, 'wpe_dtf', boom)
    monkeypatch.setattr(ops, 'wpe_arrays_dtf', boom)
    block = core.WPE(taps=7, delay=3, iterations=99, psd_context=0, online=True, alpha=0.99)
    kw = dict(taps=7, delay=3, alpha=0.99)
    assert np.all(block(np.zeros((4, 9, 3), complex)) == 1)
    out = block(np.zeros((2, 3, 9, 5), complex), stack=False)
    assert out.shape == (2, 3, 9, 5) and np.all(out == 1)
    block(np.zeros((2, 3, 9, 5), complex), stack=True)
    assert seen == [((4, 9, 3), kw), ((6, 9, 5), dict(arrays=2, **kw)),
                    ((6, 9, 5), dict(arrays=1, **kw))]
    with pytest.raises(NotImplementedError):
        block(np.zeros((2, 3, 9, 5), complex))
    with pytest.raises(NotImplementedError, match='psd_context'):
        core.WPE(7, 3, 3, 2, online=True)(np.zeros((4, 9, 3), complex))
    with pytest.raises(ValueError, match='alpha'):
        core.WPE(7, 3, 3, 0, online=True, alpha=0.0)
    core.WPE(7, 3, 3, 0, alpha=0.0)             # unread without online


# ------------------------------------------------------------------ front doors
def test_every_front_door_has_the_keywords_and_carries_them():
    from pb_chime5_amd import core, core_chime6, core_chime6_rttm
    for mod in (core, core_chime6, core_chime6_rttm):
        sig = inspect.signature(mod.get_enhancer).parameters
        assert [sig[k].default for k in ('wpe_online', 'wpe_alpha')] == [False, 0.9999], mod.__name__
    for mod in (core, core_chime6):
        plain = mod.get_enhancer()
        assert plain.wpe_block == core.WPE(10, 2, 3, 0) and plain._wpe_online() is None
        enh = mod.get_enhancer(wpe_online=True, wpe_alpha=0.995, wpe_tabs=7, wpe_per_array=True,
                               multiarray=True)
        assert enh.wpe_block == core.WPE(7, 2, 3, 0, online=True, alpha=0.995)
        assert enh._wpe_online() == 0.995 and enh._fusable() and enh.wpe_per_array
        assert mod.get_enhancer(wpe_online=True)._wpe_online() == 0.9999
        for kw, word in ((dict(wpe=False), 'wpe=False'), (dict(wpe_psd_context=2), 'wpe_psd_context'),
                         (dict(bf='wpdSouden_ban'), 'wpdSouden_ban'), (dict(bf='wpdSouden'), 'wpe_online')):
            with pytest.raises(NotImplementedError, match=word):
                mod.get_enhancer(wpe_online=True, **kw)
        with pytest.raises(NotImplementedError, match='wpe_alpha'):
            mod.get_enhancer(wpe_alpha=0.9)
        with pytest.raises(ValueError, match='alpha'):
            mod.get_enhancer(wpe_online=True, wpe_alpha=1.5)
        assert mod.get_enhancer(wpe=False).wpe_block is None


def test_rttm_front_door_takes_the_keywords(tmp_path):
    from pb_chime5_amd import core
    from pb_chime5_amd.core_chime6_rttm import get_enhancer
    from test_rttm_frontdoor import _make_chime6_dir
    root, rttm, _ = _make_chime6_dir(tmp_path)
    kw = dict(database_rttm=[str(rttm)], activity_rttm=[str(rttm)], chime6_dir=root,
              multiarray='outer_array_mics')
    enh = get_enhancer(**kw, wpe_online=True, wpe_alpha=0.999)
    assert enh.wpe_block == core.WPE(10, 2, 3, 0, online=True, alpha=0.999)
    assert get_enhancer(**kw).wpe_block == core.WPE(10, 2, 3, 0)


def test_command_lines_parse_the_keys(monkeypatch):
    from pb_chime5_amd.scripts import run, kaldi_run, kaldi_run_rttm, enhance_rttm
    cfg = run.main(['print_config', 'with', 'wpe_online=True', 'wpe_alpha=0.995'])
    assert (cfg['wpe_online'], cfg['wpe_alpha']) == (True, 0.995)
    cfg = run.main(['print_config'])
    assert (cfg['wpe_online'], cfg['wpe_alpha']) == (False, 0.9999)
    assert kaldi_run.main(['print_config', 'with', 'wpe_online=True'])['wpe_online'] is True
    assert kaldi_run_rttm.main(['print_config', 'with', 'database_rttm=a.rttm', 'wpe_online=True',
                                'wpe_alpha=0.99'])['wpe_alpha'] == 0.99

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
        enhance_rttm.main(base + ['--wpe-online', '--wpe-alpha', '0.995'])
    assert (seen['wpe_online'], seen['wpe_alpha']) == (True, 0.995)
    seen.clear()
    with pytest.raises(Stop):
        enhance_rttm.main(base)
    assert (seen['wpe_online'], seen['wpe_alpha']) == (False, 0.9999)


def test_methods_that_refuse_the_online_wpe(no_context, tmp_path):
    from pb_chime5_amd.core import get_enhancer
    enh = get_enhancer(wpe_online=True)
    obs = np.zeros((4, 4096))
    act = {'P01': np.ones(4096, bool), 'Noise': np.ones(4096, bool)}
    with pytest.raises(NotImplementedError, match='enhance_observation_guided with wpe_online'):
        enh.enhance_observation_guided(obs, {'P01': np.ones(19), 'Noise': np.ones(19)}, 'P01')
    with pytest.raises(NotImplementedError, match='enhance_observation_speakers with wpe_online'):
        enh.enhance_observation_speakers(obs, act, ['P01'])
    with pytest.raises(NotImplementedError, match='enhance_example_speakers with wpe_online'):
        enh.enhance_example_speakers({})
    with pytest.raises(NotImplementedError, match='enhance_observation_activity with wpe_online'):
        enh.enhance_observation_activity(obs, act, 'P01')
    with pytest.raises(NotImplementedError, match='enhance_example_activity with wpe_online'):
        enh.enhance_example_activity({})
    with pytest.raises(NotImplementedError, match='refined_rttm.* with wpe_online'):
        enh.enhance_session('S02', tmp_path / 'audio', refined_rttm=True)
    assert not (tmp_path / 'audio').exists()


def test_fused_call_refuses_a_second_descriptor(monkeypatch):
    from pb_chime5_amd import core

    class Ctx:
        def set_utterances_in_flight(self, n):
            pass
    monkeypatch.setattr(core.Enhancer, '_ctx', lambda self: Ctx())
    obs = np.zeros((4, 4096))
    act = {'P01': np.ones(4096, bool), 'Noise': np.ones(4096, bool)}
    for kw, word in ((dict(bf_segment_frames=64), 'bf_segment_frames'),
                     (dict(bf_null_interferer=True), 'bf_null_interferer'),
                     (dict(channel_keep=3), 'channel_keep')):
        enh = core.get_enhancer(wpe_online=True, bf_drop_context=False, **kw)
        with pytest.raises(NotImplementedError, match=f'wpe_online with {word}'):
            enh.enhance_observation(obs, act, 'P01')


def test_session_takes_one_utterance_at_a_time(monkeypatch, tmp_path):
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import get_enhancer
    enh = get_enhancer(wpe_online=True)
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


def test_fused_call_gets_the_settings_and_the_stage_path_the_block(monkeypatch):
    from pb_chime5_amd import core, ops
    seen = {}

    def fake(obs, activity, target, start, end, **kw):
        seen.update(kw, target=target, start=start, end=end)
        return np.zeros(8)
    monkeypatch.setattr(ops, 'enhance_observation_wpe_online', fake)

    def boom(*a, **k):
        raise AssertionError('the offline fused call')
    monkeypatch.setattr(ops, 'enhance_observation', boom)

    class Ctx:
        def set_utterances_in_flight(self, n):
            pass
    monkeypatch.setattr(core.Enhancer, '_ctx', lambda self: Ctx())
    enh = core.get_enhancer(wpe_online=True, wpe_alpha=0.99, wpe_tabs=4, bf_drop_context=False,
                            multiarray='outer_array_mics', wpe_per_array=True)
    act = {'P01': np.ones(4096, bool), 'P02': np.ones(4096, bool), 'Noise': np.ones(4096, bool)}
    enh.enhance_observation(np.zeros((4, 4096)), act, 'P02')
    assert (seen['alpha'], seen['target'], seen['start'], seen['end'], seen['wpe_arrays']) == \
        (0.99, 1, 0, 0, 2)
    assert seen['params'].wpe_taps == 4 and seen['params'].wpe == 1

    # the stage path: the WPE block is called per array, through ops.wpe_online_dtf
    calls = []
    monkeypatch.setattr(ops, 'wpe_online_dtf',
                        lambda Obs, **kw: calls.append((Obs.shape, kw)) or Obs)
    T, F = 30, 33
    monkeypatch.setattr(core.Enhancer, 'stft', lambda self, x: np.ones((4, T, F), complex))
    out = enh._blocks_wpe(np.ones((4, T, F), complex), False, 2)
    assert out.shape == (4, T, F)
    assert calls == [((4, T, F), dict(taps=4, delay=2, alpha=0.99, arrays=2))]
