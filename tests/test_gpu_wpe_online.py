"""Online WPE on the GPU (gss_wpe_online, gss_enhance_observation_wpe_online) against the NumPy
reference of tests/online_wpe_reference.py: X and the handed-out state in both kernel forms, a
recording fed in blocks, determinism, the closed form on the device's state, digital silence, the
state's triangles, the errors, and the pipeline.  Every device run is made once and shared."""
import ctypes
import functools

import numpy as np
import pytest

import online_wpe_reference as wr
from conftest import rel_err

pytestmark = pytest.mark.gpu

FORMS = ('default', 'mem')
INVALID, UNSUPPORTED = -1, -4


def _set_form(monkeypatch, form):
    if form == 'mem':
        monkeypatch.setenv('GSS_VARIANT', 'wpe_online_mem')
    else:
        monkeypatch.delenv('GSS_VARIANT', raising=False)


def _run(ctx, Y, cell, state=None):
    """Y (F,T,D) -> X (F,T,D) through ops.wpe_online_dtf."""
    from pb_chime5_amd import ops
    A, C, taps, delay, alpha, F, T = cell
    return wr.to_ftd(ops.wpe_online_dtf(wr.to_dtf(Y), taps, delay, alpha, arrays=A, state=state,
                                        ctx=ctx))


_RUNS = {}


def _device(ctx, monkeypatch, cell, form):
    """X and the state after the cell's scene from a fresh state, in the given form; once."""
    from pb_chime5_amd import ops
    key = (cell, form)
    if key not in _RUNS:
        A, C, taps, delay, alpha, F, T = cell
        _set_form(monkeypatch, form)
        state = ops.OnlineWPEState.fresh(F, A, C, taps, delay, ctx=ctx)
        X = _run(ctx, wr.scene(cell, wr.seed_of(cell)), cell, state)
        host = state.to_host()
        for a in (X, host['inv_cov'], host['filter'], host['history']):
            a.setflags(write=False)
        _RUNS[key] = X, host
    return _RUNS[key]


def _parity(cell, X, host, what):
    Xr, st = wr.reference(cell, wr.seed_of(cell))
    errs = dict(X=rel_err(X, Xr), G=rel_err(host['filter'], st['G']),
                P=rel_err(host['inv_cov'], st['P']))
    print(f'{cell} {what}: rel err {errs}')
    assert max(errs.values()) < wr.TOL, (cell, what, errs)
    assert np.array_equal(host['history'], st['hist']), (cell, what)


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize('cell', wr.ONCHIP_CELLS, ids=str)
def test_onchip_form_against_the_reference(gpu_ctx, monkeypatch, cell):
    """wpe_online_onchip_kernel (and sigma, history, identity): n <= 64."""
    assert cell[1] * cell[2] <= wr.ONCHIP_MAX_N
    _parity(cell, *_device(gpu_ctx, monkeypatch, cell, 'default'), 'on-chip')


@pytest.mark.parametrize('cell', wr.MEMORY_CELLS, ids=str)
def test_memory_form_against_the_reference(gpu_ctx, monkeypatch, cell):
    """wpe_online_mem_kernel where n alone selects it: n = 65 ... 512."""
    assert cell[1] * cell[2] > wr.ONCHIP_MAX_N
    _parity(cell, *_device(gpu_ctx, monkeypatch, cell, 'default'), 'memory')


@pytest.mark.parametrize('cell', wr.ONCHIP_CELLS, ids=str)
def test_memory_form_forced_on_the_onchip_cells(gpu_ctx, monkeypatch, cell):
    """GSS_VARIANT=wpe_online_mem: the memory form at small n against the reference and against
    the on-chip form (both within the bar of the reference, so within twice the bar of each
    other; the forms add in different orders)."""
    X, host = _device(gpu_ctx, monkeypatch, cell, 'mem')
    _parity(cell, X, host, 'memory (forced)')
    Xo, hosto = _device(gpu_ctx, monkeypatch, cell, 'default')
    errs = (rel_err(X, Xo), rel_err(host['filter'], hosto['filter']),
            rel_err(host['inv_cov'], hosto['inv_cov']))
    print(f'{cell}: memory vs on-chip {errs}')
    assert max(errs) < 2 * wr.TOL, errs
    assert np.array_equal(host['history'], hosto['history'])


# ------------------------------------------------------------------ long horizons
def _long_device(ctx, cell):
    """X and the state after the long cell's scene in ONE call, in the form n selects; once."""
    from pb_chime5_amd import ops
    key = ('long', cell)
    if key not in _RUNS:
        A, C, taps, delay, alpha, F, T = cell
        state = ops.OnlineWPEState.fresh(F, A, C, taps, delay, ctx=ctx)
        X = _run(ctx, wr.long_scene(cell, wr.long_seed_of(cell)), cell, state)
        host = state.to_host()
        for a in (X, host['inv_cov'], host['filter'], host['history']):
            a.setflags(write=False)
        _RUNS[key] = X, host
    return _RUNS[key]


@pytest.mark.parametrize('cell', wr.LONG_CELLS, ids=str)
def test_long_cells_against_the_reference_and_the_closed_form(gpu_ctx, monkeypatch, cell):
    """Thousands of frames: X, P and G against the reference at TOL, P and G of BOTH sides against
    the weighted least-squares problem at CLOSED_FORM_TOL, the handed-out P exactly Hermitian."""
    monkeypatch.delenv('GSS_VARIANT', raising=False)
    A, C, taps, delay, alpha, F, T = cell
    X, host = _long_device(gpu_ctx, cell)
    Xr, st = wr.long_reference(cell, wr.long_seed_of(cell))
    errs = dict(X=rel_err(X, Xr), G=rel_err(host['filter'], st['G']),
                P=rel_err(host['inv_cov'], st['P']))
    print(f'{cell}: rel err {errs}')
    assert np.all(np.isfinite(X))
    assert max(errs.values()) < wr.TOL, (cell, errs)
    assert np.array_equal(host['history'], st['hist'])
    P, G = wr.long_closed_form(cell, wr.long_seed_of(cell))
    closed = dict(device_G=rel_err(host['filter'], G), device_P=rel_err(host['inv_cov'], P),
                  reference_G=rel_err(st['G'], G), reference_P=rel_err(st['P'], P))
    print(f'{cell}: vs the closed form {closed}')
    assert max(closed.values()) < wr.CLOSED_FORM_TOL, closed
    Pd = host['inv_cov']
    n = Pd.shape[-1]
    assert np.array_equal(Pd, Pd.conj().swapaxes(-1, -2))
    assert np.all(Pd[..., np.arange(n), np.arange(n)].imag == 0)


@pytest.mark.parametrize('cell', wr.LONG_CELLS, ids=str)
def test_long_cells_in_blocks_give_the_bits_of_the_single_call(gpu_ctx, monkeypatch, cell):
    from pb_chime5_amd import ops
    monkeypatch.delenv('GSS_VARIANT', raising=False)
    A, C, taps, delay, alpha, F, T = cell
    X1, host1 = _long_device(gpu_ctx, cell)
    Y = wr.long_scene(cell, wr.long_seed_of(cell))
    state = ops.OnlineWPEState.fresh(F, A, C, taps, delay, ctx=gpu_ctx)
    bounds = np.concatenate([[0], np.cumsum(wr.long_blocks(T))])
    assert bounds[-1] == T
    X = np.concatenate([_run(gpu_ctx, Y[:, a:b], cell, state)
                        for a, b in zip(bounds[:-1], bounds[1:])], axis=1)
    assert np.array_equal(X, X1)
    host = state.to_host()
    for k in ('inv_cov', 'filter', 'history'):
        assert np.array_equal(host[k], host1[k]), k


def test_a_throwaway_state_gives_the_same_output(gpu_ctx, monkeypatch):
    for form in FORMS:
        cell = wr.ONCHIP_CELLS[0]
        _set_form(monkeypatch, form)
        X = _run(gpu_ctx, wr.scene(cell), cell)
        assert np.array_equal(X, _device(gpu_ctx, monkeypatch, cell, form)[0]), form


# ------------------------------------------------------------------ blocks, determinism
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('cell', wr.CHUNK_CELLS, ids=str)
def test_blocks_through_one_state_equal_the_single_call(gpu_ctx, monkeypatch, cell, form):
    """T frames fed as four blocks (the first of one frame, shorter than taps + delay) through one
    state: X and the final state have the bits of the single call; a state saved to the host
    after the second block and restored into a NEW context continues with the same bits."""
    from pb_chime5_amd import ops
    from pb_chime5_amd._capi import Context
    A, C, taps, delay, alpha, F, T = cell
    X1, host1 = _device(gpu_ctx, monkeypatch, cell, form)
    _set_form(monkeypatch, form)
    Y = wr.scene(cell, wr.seed_of(cell))
    state = ops.OnlineWPEState.fresh(F, A, C, taps, delay, ctx=gpu_ctx)
    bounds = np.concatenate([[0], np.cumsum(wr.CHUNKS[T])])
    assert bounds[-1] == T
    out, saved = [], None
    for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        out.append(_run(gpu_ctx, Y[:, a:b], cell, state))
        if i == 1:
            saved = state.to_host()
    X = np.concatenate(out, axis=1)
    host = state.to_host()
    assert np.array_equal(X, X1)
    for k in ('inv_cov', 'filter', 'history'):
        assert np.array_equal(host[k], host1[k]), k
    other = Context(0)
    try:
        restored = ops.OnlineWPEState.from_host(saved, ctx=other)
        tail = [_run(other, Y[:, a:b], cell, restored)
                for a, b in zip(bounds[2:-1], bounds[3:])]
        assert np.array_equal(np.concatenate(tail, axis=1), X1[:, bounds[2]:])
        host2 = restored.to_host()
        for k in ('inv_cov', 'filter', 'history'):
            assert np.array_equal(host2[k], host1[k]), k
        # a copy is independent of its source
        twin = restored.copy()
        _run(other, Y[:, :3], cell, twin)
        assert np.array_equal(restored.to_host()['inv_cov'], host1['inv_cov'])
        assert not np.array_equal(twin.to_host()['inv_cov'], host1['inv_cov'])
        del restored, twin
    finally:
        other.close()


@pytest.mark.parametrize('form', FORMS)
def test_the_same_call_gives_the_same_bits(gpu_ctx, monkeypatch, form):
    from pb_chime5_amd import ops
    cell = wr.ONCHIP_CELLS[4]               # per array
    A, C, taps, delay, alpha, F, T = cell
    X1, host1 = _device(gpu_ctx, monkeypatch, cell, form)
    _set_form(monkeypatch, form)
    state = ops.OnlineWPEState.fresh(F, A, C, taps, delay, ctx=gpu_ctx)
    X2 = _run(gpu_ctx, wr.scene(cell, wr.seed_of(cell)), cell, state)
    host2 = state.to_host()
    assert np.array_equal(X1, X2)
    for k in ('inv_cov', 'filter', 'history'):
        assert np.array_equal(host1[k], host2[k]), k


# ------------------------------------------------------------------ the state
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('cell', wr.CLOSED_FORM_CELLS, ids=str)
def test_device_state_is_the_closed_form(gpu_ctx, monkeypatch, cell, form):
    """The device's own G and P against the weighted least-squares problem, which shares no
    arithmetic with the recursion."""
    A, C, taps, delay, alpha, F, T = cell
    _, host = _device(gpu_ctx, monkeypatch, cell, form)
    P, G = wr.closed_form(wr.scene(cell, wr.seed_of(cell)), taps, delay, alpha, A)
    errs = rel_err(host['filter'], G), rel_err(host['inv_cov'], P)
    print(f'{cell} {form}: device G, P vs closed form {errs}')
    assert max(errs) < wr.CLOSED_FORM_TOL, errs


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('cell', [wr.ONCHIP_CELLS[0], wr.ONCHIP_CELLS[3], wr.MEMORY_CELLS[1]], ids=str)
def test_handed_out_state_is_exactly_hermitian(gpu_ctx, monkeypatch, cell, form):
    _, host = _device(gpu_ctx, monkeypatch, cell, form)
    P = host['inv_cov']
    n = P.shape[-1]
    assert np.array_equal(P, P.conj().swapaxes(-1, -2))
    assert np.all(P[..., np.arange(n), np.arange(n)].imag == 0)


@pytest.mark.parametrize('form', FORMS)
def test_a_reader_takes_the_upper_triangle(gpu_ctx, monkeypatch, form):
    """Garbage below the diagonal and in the imaginary part of the diagonal of a state that is
    handed in changes nothing."""
    from pb_chime5_amd import ops
    cell = wr.ONCHIP_CELLS[1]
    A, C, taps, delay, alpha, F, T = cell
    X1, host1 = _device(gpu_ctx, monkeypatch, cell, form)
    _set_form(monkeypatch, form)
    Y = wr.scene(cell, wr.seed_of(cell))
    state = ops.OnlineWPEState.fresh(F, A, C, taps, delay, ctx=gpu_ctx)
    head = _run(gpu_ctx, Y[:, :30], cell, state)
    mid = state.to_host()
    n = taps * C
    P = mid['inv_cov'].copy()
    lower = np.tril_indices(n, -1)
    P[..., lower[0], lower[1]] = 7.0 - 3.0j
    P[..., np.arange(n), np.arange(n)] += 5.0j
    dirty = ops.OnlineWPEState.from_host({**mid, 'inv_cov': P}, ctx=gpu_ctx)
    tail = _run(gpu_ctx, Y[:, 30:], cell, dirty)
    assert np.array_equal(np.concatenate([head, tail], axis=1), X1)
    assert np.array_equal(dirty.to_host()['inv_cov'], host1['inv_cov'])


# ------------------------------------------------------------------ silence
@pytest.mark.parametrize('form', FORMS)
def test_digital_silence(gpu_ctx, monkeypatch, form):
    from pb_chime5_amd import ops
    cell = wr.ONCHIP_CELLS[0]
    A, C, taps, delay, alpha, F, T = cell
    L = taps + delay
    _set_form(monkeypatch, form)
    # a zero block of 2 (L + 1) frames in every channel, in the middle
    for kind in ('block', 'channel'):
        Y = wr.silence_scene(cell, kind, wr.seed_of(cell))
        Xr, st = wr.online_wpe(Y, taps, delay, alpha, A)
        state = ops.OnlineWPEState.fresh(F, A, C, taps, delay, ctx=gpu_ctx)
        X = _run(gpu_ctx, Y, cell, state)
        host = state.to_host()
        assert np.all(np.isfinite(X)) and all(np.all(np.isfinite(host[k]))
                                              for k in ('inv_cov', 'filter', 'history'))
        errs = rel_err(X, Xr), rel_err(host['filter'], st['G']), rel_err(host['inv_cov'], st['P'])
        print(f'{form} silence {kind}: {errs}')
        assert max(errs) < wr.TOL, (kind, errs)
    # a call whose frames all see an all-zero buffer: P and G keep their bits, the output is zero
    Y = wr.scene(cell, wr.seed_of(cell))[:, :40]
    state = ops.OnlineWPEState.fresh(F, A, C, taps, delay, ctx=gpu_ctx)
    _run(gpu_ctx, np.concatenate([Y, np.zeros((F, L, A * C))], axis=1), cell, state)
    before = state.to_host()
    assert np.all(before['history'] == 0)
    X = _run(gpu_ctx, np.zeros((F, 5, A * C), complex), cell, state)
    after = state.to_host()
    assert np.all(X == 0)
    assert np.array_equal(after['inv_cov'], before['inv_cov'])
    assert np.array_equal(after['filter'], before['filter'])


# ------------------------------------------------------------------ errors
def test_errors_before_any_launch(gpu_ctx, monkeypatch):
    from pb_chime5_amd import _capi, ops
    monkeypatch.delenv('GSS_VARIANT', raising=False)
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    F, T, A, C, taps, delay = 2, 9, 1, 3, 2, 1
    state = ops.OnlineWPEState.fresh(F, A, C, taps, delay, ctx=gpu_ctx)
    before = state.to_host()
    Y = gpu_ctx.to_device(np.ones((F, T, A * C), complex))
    X = gpu_ctx.empty(16 * F * T * A * C)
    used = gpu_ctx.workspace_bytes()

    def call(Yp=Y.ptr, Xp=X.ptr, st=state.struct(), **kw):
        a = {**dict(F=F, T=T, A=A, C=C, taps=taps, delay=delay, alpha=0.99), **kw}
        rc = lib.gss_wpe_online(h, ctypes.c_void_p(Yp), a['F'], a['T'], a['A'], a['C'], a['taps'],
                                a['delay'], a['alpha'],
                                ctypes.byref(st) if st is not None else None, ctypes.c_void_p(Xp))
        return rc, lib.gss_last_error(h).decode()
    S = _capi.GssWpeOnlineState
    p = state.bufs
    cases = [
        (dict(Yp=None), INVALID, 'Y_dev'), (dict(Xp=None), INVALID, 'X_dev'),
        (dict(Xp=Y.ptr), INVALID, 'alias'),
        (dict(st=S(None, p['filter'].ptr, p['history'].ptr)), INVALID, 'inv_cov_dev'),
        (dict(st=S(p['inv_cov'].ptr, None, p['history'].ptr)), INVALID, 'filter_dev'),
        (dict(st=S(p['inv_cov'].ptr, p['filter'].ptr, None)), INVALID, 'history_dev'),
        (dict(F=0), INVALID, 'F'), (dict(T=-1), INVALID, 'T'), (dict(A=0), INVALID, 'A'),
        (dict(C=0), INVALID, 'C'), (dict(taps=0), INVALID, 'taps'), (dict(delay=-1), INVALID, 'delay'),
        (dict(alpha=0.0), INVALID, 'alpha'), (dict(alpha=1.5), INVALID, 'alpha'),
        (dict(alpha=float('nan')), INVALID, 'alpha'),
        (dict(taps=171), UNSUPPORTED, '512'), (dict(A=11), UNSUPPORTED, 'A * C'),
    ]
    for kw, code, word in cases:
        rc, msg = call(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
    rc = lib.gss_wpe_online_init(h, F, A, C, taps, delay, None)
    assert rc == INVALID and 'state' in lib.gss_last_error(h).decode()
    rc = lib.gss_wpe_online_init(h, F, A, C, 0, delay, ctypes.byref(state.struct()))
    assert rc == INVALID and 'taps' in lib.gss_last_error(h).decode()
    rc = lib.gss_wpe_online_init(h, F, A, C, 171, delay, ctypes.byref(state.struct()))
    assert rc == UNSUPPORTED
    # nothing ran: no workspace was taken and the state has its bits; T = 0 is a no-op
    assert call(T=0)[0] == 0
    assert gpu_ctx.workspace_bytes() == used
    after = state.to_host()
    for k in ('inv_cov', 'filter', 'history'):
        assert np.array_equal(after[k], before[k]), k
    with pytest.raises(NotImplementedError):
        ops.wpe_online_dtf(np.zeros((3, 9, 2), complex), taps=171, ctx=gpu_ctx)
    # the fused entry
    u = wr.pipe_scene()
    params = ops.make_params(wpe_taps=2, bss_iterations=1)
    _, utt, _, _ = ops._resident_call(u.obs, u.activity_array, params, None, None, False, gpu_ctx)
    with pytest.raises(ValueError, match='alpha'):
        utt.enqueue(u.target_index, 0, 0, wpe_online=_capi.GssWpeOnlineCfg(alpha=0.0))
    for bad, word in ((dict(wpe=False), 'wpe = 0'), (dict(wpe_psd_context=1), 'wpe_psd_context')):
        pbad = ops.make_params(wpe_taps=2, bss_iterations=1, **bad)
        _, utt, _, _ = ops._resident_call(u.obs, u.activity_array, pbad, None, None, False, gpu_ctx)
        with pytest.raises(ValueError, match=word):
            utt.enqueue(u.target_index, 0, 0, wpe_online=_capi.GssWpeOnlineCfg(alpha=0.9))


def test_online_wpe_object(gpu_ctx, monkeypatch):
    """`online_wpe.OnlineWPE`: blocks and single frames through the object's own state give the
    bits of the single call; reset() starts over."""
    from pb_chime5_amd.online_wpe import OnlineWPE
    monkeypatch.delenv('GSS_VARIANT', raising=False)
    cell = wr.ONCHIP_CELLS[1]
    A, C, taps, delay, alpha, F, T = cell
    X1, host1 = _device(gpu_ctx, monkeypatch, cell, 'default')
    Y = wr.scene(cell, wr.seed_of(cell))
    block = np.ascontiguousarray(Y.transpose(1, 0, 2))          # (T,F,D)
    wpe = OnlineWPE(taps, delay, alpha, channel=A * C, frequency_bins=F, arrays=A, ctx=gpu_ctx)
    out = [wpe.step_frames(block[:40])] + [wpe.step_frame(fr)[None] for fr in block[40:45]]
    out.append(wpe.step_frames(block[45:]))
    got = np.concatenate(out, axis=0).transpose(1, 0, 2)
    assert np.array_equal(got, X1)
    assert np.array_equal(wpe.state.to_host()['inv_cov'], host1['inv_cov'])
    wpe.reset()
    assert np.array_equal(wpe.step_frames(block).transpose(1, 0, 2), X1)
    with pytest.raises(ValueError, match='block'):
        wpe.step_frames(block[:, :1])


# ------------------------------------------------------------------ pipeline
@functools.lru_cache(maxsize=None)
def _pipe_enhancer(arrays):
    from pb_chime5_amd.core import get_enhancer
    p = wr.PIPE
    return get_enhancer(wpe_online=True, wpe_alpha=p['alpha'], wpe_tabs=p['wpe_taps'],
                        wpe_delay=p['wpe_delay'], bss_iterations=p['bss_iterations'],
                        stft_size=p['stft_size'], stft_shift=p['stft_shift'],
                        wpe_per_array=arrays > 1,
                        multiarray='outer_array_mics' if arrays > 1 else False)


@pytest.mark.parametrize('arrays', [1, 2])
def test_pipeline(gpu_ctx, monkeypatch, arrays):
    """The fused call's Obs tap has the bits of ops.wpe_online_dtf(stft(obs)); fused and stage
    path agree as test_block_by_block_path_equals_fused demands of the plain call; |x_hat| is
    within the end-to-end bar of the oracle's stages composed with the reference."""
    from pb_chime5_amd import ops
    monkeypatch.delenv('GSS_VARIANT', raising=False)
    p = wr.PIPE
    u = wr.pipe_scene()
    enh = _pipe_enhancer(arrays)
    assert enh._fusable() and enh._wpe_online() == p['alpha']
    got = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, debug=True,
                                  wpe_arrays=arrays)
    det = enh.enhance_observation_locals['details']
    assert gpu_ctx.last_wpe_zero_pivots() == 0
    Obs = ops.stft(u.obs, p['stft_size'], p['stft_shift'], ctx=gpu_ctx)
    stage = ops.wpe_online_dtf(Obs, p['wpe_taps'], p['wpe_delay'], p['alpha'], arrays=arrays,
                               ctx=gpu_ctx)
    assert np.array_equal(det['Obs'], stage)
    blocks = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, fused=False,
                                     wpe_arrays=arrays)
    print(f'arrays={arrays}: stage path vs fused {rel_err(blocks, got):.1e}')
    assert rel_err(blocks, got) < 1e-10
    want, want_obs = wr.pipe_reference(arrays)
    errs = rel_err(det['Obs'], want_obs), wr.abs_rel_err(got, want)
    print(f'arrays={arrays}: Obs vs reference {errs[0]:.1e}, |x_hat| vs oracle chain {errs[1]:.1e}')
    assert errs[0] < 1e-9 and errs[1] < wr.X_TOL, errs
    # it is another signal than the offline WPE gives
    if arrays == 1:
        from pb_chime5_amd.core import get_enhancer
        plain = get_enhancer(wpe_tabs=p['wpe_taps'], wpe_delay=p['wpe_delay'],
                             bss_iterations=p['bss_iterations'], stft_size=p['stft_size'],
                             stft_shift=p['stft_shift'])
        assert rel_err(plain.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex),
                       got) > 1e-4
