"""Online MVDR on the GPU (gss_mvdr_online, gss_enhance_observation_bf_online) against the NumPy
reference of tests/online_mvdr_reference.py: X, the filters and the handed-out state in every
cell, a recording fed in blocks, determinism, the state's triangles and its closed form, the
loading, edge inputs and the fallback rule, the errors, the evidence, the pipeline, the workspace
hygiene and the untouched default.  Every device run is made once and shared."""
import ctypes
import functools

import numpy as np
import pytest

import online_mvdr_reference as mr
from conftest import rel_err

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -4
PATTERNS = (0x00, 0xFF)


def _run(ctx, Y, mx, mn, cell, ban, ref, state=None, **kw):
    """Y (F,T,D), masks (F,T) -> X (F,T), W (F,T,D) through ops.mvdr_souden_online_from_masks."""
    from pb_chime5_amd import ops
    D, beta, loading, F, T = cell
    X, W = ops.mvdr_souden_online_from_masks(
        mr.to_dtf(Y), mx.T, mn.T, ban, forget=beta, loading=loading, ref_channel=ref, state=state,
        return_filters=True, ctx=ctx, **kw)
    return np.ascontiguousarray(X.T), np.ascontiguousarray(W.transpose(1, 0, 2))


_RUNS = {}


def _device(ctx, cell, ban, ref):
    """X, W and the state after the cell's scene from a fresh state; once."""
    from pb_chime5_amd import ops
    key = (cell, ban, ref)
    if key not in _RUNS:
        D, beta, loading, F, T = cell
        Y, mx, mn, _ = mr.scene(cell, mr.seed_of(cell))
        state = ops.OnlineMVDRState.fresh(F, D, loading, mr.to_dtf(Y), ctx=ctx)
        X, W = _run(ctx, Y, mx, mn, cell, ban, ref, state)
        host = state.to_host()
        for a in (X, W, host['phi_x'], host['phi_n']):
            a.setflags(write=False)
        _RUNS[key] = X, W, host
    return _RUNS[key]


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize('cell', mr.CELLS, ids=str)
def test_against_the_reference(gpu_ctx, cell):
    for ban, ref in mr.variants(cell):
        X, W, host = _device(gpu_ctx, cell, ban, ref)
        Xr, Wr, st, fallbacks = mr.reference(cell, ban, ref, mr.seed_of(cell))
        assert fallbacks == 0
        errs = dict(X=rel_err(X, Xr), W=rel_err(W, Wr), phi_x=rel_err(host['phi_x'], st['phi_x']),
                    phi_n=rel_err(host['phi_n'], st['phi_n']))
        print(f'{cell} ban={ban} ref={ref}: rel err {errs}')
        assert max(errs.values()) < mr.TOL, (cell, ban, ref, errs)


# ------------------------------------------------------------------ long horizons
def _long_device(ctx, cell, ban, ref):
    """X, W, the state and the fallback count after the long cell's scene in ONE call; once."""
    from pb_chime5_amd import ops
    key = ('long', cell, ban, ref)
    if key not in _RUNS:
        D, beta, loading, F, T = cell
        Y, mx, mn, _ = mr.scene(cell, mr.seed_of(cell))
        state = ops.OnlineMVDRState.fresh(F, D, loading, mr.to_dtf(Y), ctx=ctx)
        X, W = _run(ctx, Y, mx, mn, cell, ban, ref, state)
        fallbacks = ctx.last_mvdr_online_fallbacks()
        host = state.to_host()
        for a in (X, W, host['phi_x'], host['phi_n']):
            a.setflags(write=False)
        _RUNS[key] = X, W, host, fallbacks
    return _RUNS[key]


@pytest.mark.parametrize('cell', mr.LONG_CELLS, ids=str)
def test_long_cells_against_the_reference(gpu_ctx, cell):
    """Thousands of frames in one call, every variant: X, W and the state at TOL, no fallback on
    either side, the state exactly Hermitian and its closed form."""
    D, beta, loading, F, T = cell
    Y, mx, mn, _ = mr.scene(cell, mr.seed_of(cell))
    phi_x, phi_n = mr.closed_form(Y, mx, mn, beta, mr.loading_delta(Y, loading))
    for ban, ref in mr.variants(cell):
        X, W, host, fallbacks = _long_device(gpu_ctx, cell, ban, ref)
        Xr, Wr, st, fr = mr.reference(cell, ban, ref, mr.seed_of(cell))
        assert fallbacks == 0 and fr == 0
        errs = dict(X=rel_err(X, Xr), W=rel_err(W, Wr), phi_x=rel_err(host['phi_x'], st['phi_x']),
                    phi_n=rel_err(host['phi_n'], st['phi_n']))
        print(f'{cell} ban={ban} ref={ref}: rel err {errs}')
        assert np.all(np.isfinite(X)) and np.all(np.isfinite(W))
        assert max(errs.values()) < mr.TOL, (cell, ban, ref, errs)
        for k in ('phi_x', 'phi_n'):
            P = host[k]
            assert np.array_equal(P, P.conj().swapaxes(-1, -2)), k
            assert np.all(P[..., np.arange(D), np.arange(D)].imag == 0), k
        closed = rel_err(host['phi_x'], phi_x), rel_err(host['phi_n'], phi_n)
        assert max(closed) < mr.CLOSED_FORM_TOL, closed
    print(f'{cell}: device Phi_X, Phi_N vs closed form {closed}')


@pytest.mark.parametrize('cell', mr.LONG_CELLS, ids=str)
def test_long_cells_in_blocks_give_the_bits_of_the_single_call(gpu_ctx, cell):
    from pb_chime5_amd import ops
    D, beta, loading, F, T = cell
    ban, ref = True, D - 1
    X1, W1, host1, _ = _long_device(gpu_ctx, cell, ban, ref)
    Y, mx, mn, _ = mr.scene(cell, mr.seed_of(cell))
    state = ops.OnlineMVDRState.fresh(F, D, loading, mr.to_dtf(Y), ctx=gpu_ctx)
    bounds = np.concatenate([[0], np.cumsum(mr.long_blocks(T))])
    assert bounds[-1] == T
    outs, total = [], 0
    for a, b in zip(bounds[:-1], bounds[1:]):
        outs.append(_run(gpu_ctx, Y[:, a:b], mx[:, a:b], mn[:, a:b], cell, ban, ref, state))
        total += gpu_ctx.last_mvdr_online_fallbacks()
    assert total == 0
    assert np.array_equal(np.concatenate([o[0] for o in outs], axis=1), X1)
    assert np.array_equal(np.concatenate([o[1] for o in outs], axis=1), W1)
    host = state.to_host()
    for k in ('phi_x', 'phi_n'):
        assert np.array_equal(host[k], host1[k]), k


# ------------------------------------------------------------------ blocks, determinism
@pytest.mark.parametrize('cell', mr.CHUNK_CELLS, ids=str)
def test_blocks_through_one_state_equal_the_single_call(gpu_ctx, cell):
    """T frames fed as four blocks (the first of one frame) through one state: X, W and the final
    state have the bits of the single call; a state saved to the host after the second block and
    restored into a NEW context continues with the same bits; a copy is independent."""
    from pb_chime5_amd import ops
    from pb_chime5_amd._capi import Context
    D, beta, loading, F, T = cell
    ban, ref = True, D - 1
    X1, W1, host1 = _device(gpu_ctx, cell, ban, ref)
    Y, mx, mn, _ = mr.scene(cell, mr.seed_of(cell))
    state = ops.OnlineMVDRState.fresh(F, D, loading, mr.to_dtf(Y), ctx=gpu_ctx)
    bounds = np.concatenate([[0], np.cumsum(mr.CHUNKS[T])])
    assert bounds[-1] == T
    outs, saved = [], None
    for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        outs.append(_run(gpu_ctx, Y[:, a:b], mx[:, a:b], mn[:, a:b], cell, ban, ref, state))
        if i == 1:
            saved = state.to_host()
    assert np.array_equal(np.concatenate([o[0] for o in outs], axis=1), X1)
    assert np.array_equal(np.concatenate([o[1] for o in outs], axis=1), W1)
    host = state.to_host()
    for k in ('phi_x', 'phi_n'):
        assert np.array_equal(host[k], host1[k]), k
    other = Context(0)
    try:
        restored = ops.OnlineMVDRState.from_host(saved, ctx=other)
        tail = [_run(other, Y[:, a:b], mx[:, a:b], mn[:, a:b], cell, ban, ref, restored)
                for a, b in zip(bounds[2:-1], bounds[3:])]
        assert np.array_equal(np.concatenate([o[0] for o in tail], axis=1), X1[:, bounds[2]:])
        assert np.array_equal(np.concatenate([o[1] for o in tail], axis=1), W1[:, bounds[2]:])
        host2 = restored.to_host()
        for k in ('phi_x', 'phi_n'):
            assert np.array_equal(host2[k], host1[k]), k
        twin = restored.copy()
        _run(other, Y[:, :3], mx[:, :3], mn[:, :3], cell, ban, ref, twin)
        assert np.array_equal(restored.to_host()['phi_n'], host1['phi_n'])
        assert not np.array_equal(twin.to_host()['phi_n'], host1['phi_n'])
        del restored, twin
    finally:
        other.close()


def test_a_throwaway_state_and_a_second_call_give_the_same_bits(gpu_ctx):
    from pb_chime5_amd import ops
    for cell in mr.CHUNK_CELLS:
        D, beta, loading, F, T = cell
        ban, ref = True, D - 1
        X1, W1, host1 = _device(gpu_ctx, cell, ban, ref)
        Y, mx, mn, _ = mr.scene(cell, mr.seed_of(cell))
        X, W = _run(gpu_ctx, Y, mx, mn, cell, ban, ref)          # state=None
        assert np.array_equal(X, X1) and np.array_equal(W, W1), cell
        state = ops.OnlineMVDRState.fresh(F, D, loading, mr.to_dtf(Y), ctx=gpu_ctx)
        X, W = _run(gpu_ctx, Y, mx, mn, cell, ban, ref, state)
        host = state.to_host()
        assert np.array_equal(X, X1) and np.array_equal(W, W1), cell
        for k in ('phi_x', 'phi_n'):
            assert np.array_equal(host[k], host1[k]), (cell, k)


# ------------------------------------------------------------------ the state
@pytest.mark.parametrize('cell', [mr.CELLS[0], mr.CELLS[3], mr.CELLS[9], mr.CELLS[11]], ids=str)
def test_handed_out_state_is_exactly_hermitian(gpu_ctx, cell):
    D = cell[0]
    _, _, host = _device(gpu_ctx, cell, False, 0)
    for k in ('phi_x', 'phi_n'):
        P = host[k]
        assert np.array_equal(P, P.conj().swapaxes(-1, -2)), k
        assert np.all(P[..., np.arange(D), np.arange(D)].imag == 0), k


def test_a_reader_takes_the_upper_triangle(gpu_ctx):
    """Garbage below the diagonal and in the imaginary part of the diagonal of a state that is
    handed in changes nothing."""
    from pb_chime5_amd import ops
    cell = mr.CELLS[0]
    D, beta, loading, F, T = cell
    ban, ref = False, 0
    X1, W1, host1 = _device(gpu_ctx, cell, ban, ref)
    Y, mx, mn, _ = mr.scene(cell, mr.seed_of(cell))
    state = ops.OnlineMVDRState.fresh(F, D, loading, mr.to_dtf(Y), ctx=gpu_ctx)
    head = _run(gpu_ctx, Y[:, :30], mx[:, :30], mn[:, :30], cell, ban, ref, state)
    mid = state.to_host()
    lower = np.tril_indices(D, -1)
    dirty = {}
    for k in ('phi_x', 'phi_n'):
        P = mid[k].copy()
        P[..., lower[0], lower[1]] = 7.0 - 3.0j
        P[..., np.arange(D), np.arange(D)] += 5.0j
        dirty[k] = P
    state = ops.OnlineMVDRState.from_host(dirty, ctx=gpu_ctx)
    tail = _run(gpu_ctx, Y[:, 30:], mx[:, 30:], mn[:, 30:], cell, ban, ref, state)
    assert np.array_equal(np.concatenate([head[0], tail[0]], axis=1), X1)
    assert np.array_equal(np.concatenate([head[1], tail[1]], axis=1), W1)
    host = state.to_host()
    for k in ('phi_x', 'phi_n'):
        assert np.array_equal(host[k], host1[k]), k


@pytest.mark.parametrize('cell', mr.CLOSED_FORM_CELLS, ids=str)
def test_device_state_is_the_closed_form(gpu_ctx, cell):
    D, beta, loading, F, T = cell
    _, _, host = _device(gpu_ctx, cell, False, 0)
    Y, mx, mn, _ = mr.scene(cell, mr.seed_of(cell))
    phi_x, phi_n = mr.closed_form(Y, mx, mn, beta, mr.loading_delta(Y, loading))
    errs = rel_err(host['phi_x'], phi_x), rel_err(host['phi_n'], phi_n)
    print(f'{cell}: device Phi_X, Phi_N vs closed form {errs}')
    assert max(errs) < mr.CLOSED_FORM_TOL, errs


def test_loading(gpu_ctx):
    """fresh(..., Y=block): phi_n = loading * mean power * I per frequency; an all-zero bin takes
    p_f = 1; no block: p_f = 1."""
    from pb_chime5_amd import ops
    cell = (5, 0.99, 0.25, 4, 333)
    D, _, loading, F, T = cell
    Y = mr.scene(cell)[0].copy()
    Y[2] = 0
    host = ops.OnlineMVDRState.fresh(F, D, loading, mr.to_dtf(Y), ctx=gpu_ctx).to_host()
    assert np.all(host['phi_x'] == 0)
    want = mr.fresh_state(F, D, loading, Y)['phi_n']
    assert want[2, 0, 0] == loading
    off = ~np.eye(D, dtype=bool)
    assert np.all(host['phi_n'][:, off] == 0) and np.all(host['phi_n'].imag == 0)
    for f in range(F):
        err = rel_err(host['phi_n'][f], want[f])
        print(f'loading, frequency {f}: {err:.1e}')
        assert err < 1e-13, (f, err)
    assert host['phi_n'][2, 0, 0] == loading
    bare = ops.OnlineMVDRState.fresh(F, D, loading, ctx=gpu_ctx).to_host()
    assert np.array_equal(bare['phi_n'], mr.fresh_state(F, D, loading)['phi_n'])


# ------------------------------------------------------------------ edge inputs
def test_digital_silence(gpu_ctx):
    cell = mr.CELLS[0]
    D, beta, loading, F, T = cell
    for kind in ('block', 'channel'):
        Y, mx, mn = mr.edge_scene(cell, kind, mr.seed_of(cell))
        for ban in (False, True):
            Xr, Wr, st, fallbacks = mr.online_mvdr(Y, mx, mn, beta, 0, ban, loading=loading)
            assert fallbacks == 0
            X, W = _run(gpu_ctx, Y, mx, mn, cell, ban, 0)
            errs = rel_err(X, Xr), rel_err(W, Wr)
            print(f'silence {kind} ban={ban}: {errs}')
            assert np.all(np.isfinite(X)) and max(errs) < mr.TOL, (kind, ban, errs)


def test_zero_target_mask_gives_exactly_zero(gpu_ctx):
    cell = mr.CELLS[0]
    Y, mx, mn, _ = mr.scene(cell, mr.seed_of(cell))
    for ban in (False, True):
        X, W = _run(gpu_ctx, Y, np.zeros_like(mx), mn, cell, ban, 0)
        assert np.all(X == 0) and np.all(W == 0), ban


@pytest.mark.parametrize('kind', ['all', 'first'])
def test_fallback_frames(gpu_ctx, kind):
    """A noise matrix with no Cholesky factor: the count equals the reference's, X = 0 on those
    frames and finite elsewhere."""
    from pb_chime5_amd import ops
    Y, mx, mn, st0, beta, count = mr.fallback_case(kind)
    F, T, D = Y.shape
    Xr, Wr, st, fallbacks = mr.online_mvdr(Y, mx, mn, beta, 0, False, state=st0)
    assert fallbacks == count
    state = ops.OnlineMVDRState.from_host(st0, ctx=gpu_ctx)
    X, got = ops.mvdr_souden_online_from_masks(
        mr.to_dtf(Y), mx.T, mn.T, False, forget=beta, ref_channel=0, state=state,
        return_fallbacks=True, ctx=gpu_ctx)
    X = X.T
    assert got == count == gpu_ctx.last_mvdr_online_fallbacks()
    assert np.all(np.isfinite(X))
    if kind == 'all':
        assert np.all(X == 0)
    else:
        assert np.all(X[:, :3] == 0) and np.all(X[:, 3:] != 0)
        assert rel_err(X, Xr) < mr.TOL
    host = state.to_host()
    assert rel_err(host['phi_x'], st['phi_x']) < mr.TOL
    # a later call without fallbacks reads 0
    cell = mr.CELLS[1]
    Y, mx, mn, _ = mr.scene(cell)
    _run(gpu_ctx, Y, mx, mn, cell, False, 0)
    assert gpu_ctx.last_mvdr_online_fallbacks() == 0


# ------------------------------------------------------------------ errors
def test_errors_before_any_launch(gpu_ctx):
    from pb_chime5_amd import _capi, ops
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    F, T, D = 2, 9, 3
    state = ops.OnlineMVDRState.fresh(F, D, 0.5, ctx=gpu_ctx)
    before = state.to_host()
    Y = gpu_ctx.to_device(np.ones((F, T, D), complex))
    mx = gpu_ctx.to_device(np.ones((F, T)))
    mn = gpu_ctx.to_device(np.ones((F, T)))
    pattern = np.full((F, T), 3.0 - 4.0j)
    wpattern = np.full((F, T, D), 3.0 - 4.0j)
    X, W = gpu_ctx.to_device(pattern), gpu_ctx.to_device(wpattern)
    used = gpu_ctx.workspace_bytes()
    S, C = _capi.GssMvdrOnlineState, _capi.GssBfOnline

    def call(Yp=Y.ptr, mxp=mx.ptr, mnp=mn.ptr, Xp=X.ptr, st=state.struct(), cfg=True, **kw):
        a = {**dict(F=F, T=T, D=D, forget=0.9, loading=1.0, ref=0), **kw}
        c = C(forget=a['forget'], loading=a['loading'], ref_channel=a['ref']) if cfg else None
        rc = lib.gss_mvdr_online(
            h, ctypes.c_void_p(Yp), a['F'], a['T'], a['D'], ctypes.c_void_p(mxp),
            ctypes.c_void_p(mnp), 1, ctypes.byref(c) if c is not None else None,
            ctypes.byref(st) if st is not None else None, ctypes.c_void_p(Xp),
            ctypes.c_void_p(W.ptr))
        return rc, lib.gss_last_error(h).decode()
    p = state.bufs
    nan, inf = float('nan'), float('inf')
    cases = [
        (dict(Yp=None), INVALID, 'Y_dev'), (dict(mxp=None), INVALID, 'mask_x_dev'),
        (dict(mnp=None), INVALID, 'mask_n_dev'), (dict(Xp=None), INVALID, 'Xhat_dev'),
        (dict(cfg=False), INVALID, 'cfg'),
        (dict(st=S(None, p['phi_n'].ptr, F, D)), INVALID, 'phi_x'),
        (dict(st=S(p['phi_x'].ptr, None, F, D)), INVALID, 'phi_n'),
        (dict(st=S(p['phi_x'].ptr, p['phi_n'].ptr, F + 1, D)), INVALID, 'state of F'),
        (dict(st=S(p['phi_x'].ptr, p['phi_n'].ptr, F, D + 1)), INVALID, 'state of F'),
        (dict(F=0), INVALID, 'F'), (dict(T=-1), INVALID, 'T'),
        (dict(D=0), UNSUPPORTED, 'D'), (dict(D=33), UNSUPPORTED, 'D'),
        (dict(forget=0.0), INVALID, 'forget'), (dict(forget=1.5), INVALID, 'forget'),
        (dict(forget=nan), INVALID, 'forget'),
        (dict(loading=0.0), INVALID, 'loading'), (dict(loading=-1.0), INVALID, 'loading'),
        (dict(loading=inf), INVALID, 'loading'), (dict(loading=nan), INVALID, 'loading'),
        (dict(ref=-2), INVALID, 'ref_channel'), (dict(ref=D), INVALID, 'ref_channel'),
    ]
    for kw, code, word in cases:
        rc, msg = call(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
    init = lib.gss_mvdr_online_init
    st = state.struct()
    for args, code, word in (
            ((F, D, None, 0, 1.0, None), INVALID, 'state'),
            ((F, D, None, 0, 0.0, ctypes.byref(st)), INVALID, 'loading'),
            ((F, D, None, 0, nan, ctypes.byref(st)), INVALID, 'loading'),
            ((F, D, None, -1, 1.0, ctypes.byref(st)), INVALID, 'T'),
            ((F + 1, D, None, 0, 1.0, ctypes.byref(st)), INVALID, 'state of F'),
            ((F, 33, None, 0, 1.0, ctypes.byref(st)), UNSUPPORTED, 'D')):
        rc = init(h, *args)
        assert rc == code and word in lib.gss_last_error(h).decode(), (args, rc)
    assert lib.gss_last_mvdr_online_fallbacks(h, None) == INVALID
    # nothing ran: no workspace was taken, the state and the outputs have their bits; T = 0 is a no-op
    assert call(T=0)[0] == 0
    assert gpu_ctx.workspace_bytes() == used
    after = state.to_host()
    for k in ('phi_x', 'phi_n'):
        assert np.array_equal(after[k], before[k]), k
    assert np.array_equal(gpu_ctx.to_host(X, (F, T), np.complex128), pattern)
    assert np.array_equal(gpu_ctx.to_host(W, (F, T, D), np.complex128), wpattern)
    # the fused entry
    u = mr.pipe_scene()
    params = ops.make_params(wpe_taps=2, bss_iterations=1)
    _, utt, _, _ = ops._resident_call(u.obs, u.activity_array, params, None, None, False, gpu_ctx)
    for bad, word in ((dict(forget=0.0), 'forget'), (dict(loading=0.0), 'loading'),
                      (dict(ref_channel=4), 'ref_channel'), (dict(wpe_online=1, wpe_alpha=0.0), 'alpha')):
        cfg = C(**{**dict(forget=0.9, loading=1.0, ref_channel=-1, wpe_online=0, wpe_alpha=0.99),
                   **bad})
        with pytest.raises(ValueError, match=word):
            utt.enqueue(u.target_index, 0, 0, bf_online=cfg)
    pbad = ops.make_params(wpe_taps=2, bss_iterations=1, bf='gev_ban')
    _, utt, _, _ = ops._resident_call(u.obs, u.activity_array, pbad, None, None, False, gpu_ctx)
    with pytest.raises(NotImplementedError, match='online'):
        utt.enqueue(u.target_index, 0, 0, bf_online=C(forget=0.9, loading=1.0, ref_channel=-1))


def test_online_mvdr_object(gpu_ctx):
    """`online_mvdr.OnlineMVDR`: blocks and single frames through the object's own state give the
    bits of the single call from the same state; reset() starts over."""
    from pb_chime5_amd import ops
    from pb_chime5_amd.online_mvdr import OnlineMVDR
    cell = mr.CELLS[3]
    D, beta, loading, F, T = cell
    Y, mx, mn, _ = mr.scene(cell)
    state = ops.OnlineMVDRState.fresh(F, D, loading, ctx=gpu_ctx)
    X1, _ = _run(gpu_ctx, Y, mx, mn, cell, True, 1, state)
    block = np.ascontiguousarray(Y.transpose(1, 0, 2))          # (T,F,D)
    bf = OnlineMVDR(beta, loading, channel=D, frequency_bins=F, ref_channel=1, ban=True, ctx=gpu_ctx)
    out = [bf.step_frames(block[:40], mx.T[:40], mn.T[:40])]
    out += [bf.step_frame(block[t], mx[:, t], mn[:, t])[None] for t in range(40, 45)]
    out.append(bf.step_frames(block[45:], mx.T[45:], mn.T[45:]))
    assert np.array_equal(np.concatenate(out, axis=0).T, X1)
    assert np.array_equal(bf.state.to_host()['phi_n'], state.to_host()['phi_n'])
    assert bf.fallbacks == 0
    bf.reset()
    assert np.array_equal(bf.step_frames(block, mx.T, mn.T).T, X1)
    with pytest.raises(ValueError, match='block'):
        bf.step_frames(block[:, :1], mx.T, mn.T)


# ------------------------------------------------------------------ evidence
def test_the_online_form_follows_a_moving_target(gpu_ctx):
    """The device's output on the evidence scene: its error against the target's image over the
    second half of the frames is below EVIDENCE_BOUND x the whole-window beamformer's."""
    cell = mr.EVIDENCE_CELL
    Y, mx, mn, _ = mr.scene(cell, mr.EVIDENCE_SEED)
    X, _ = _run(gpu_ctx, Y, mx, mn, cell, False, 0)
    ratio = mr.evidence_ratio(X)
    print(f'evidence: online / whole-window error {ratio:.3f} (reference {mr.evidence_ratio():.3f})')
    assert ratio < mr.EVIDENCE_BOUND


# ------------------------------------------------------------------ pipeline
@functools.lru_cache(maxsize=None)
def _pipe_enhancer(wpe_online, bf_online=True):
    from pb_chime5_amd.core import get_enhancer
    p = mr.PIPE
    kw = dict(wpe_tabs=p['wpe_taps'], wpe_delay=p['wpe_delay'], bss_iterations=p['bss_iterations'],
              stft_size=p['stft_size'], stft_shift=p['stft_shift'])
    if wpe_online:
        kw.update(wpe_online=True, wpe_alpha=p['wpe_alpha'])
    if bf_online:
        kw.update(bf_online=True, bf_forget=p['forget'], bf_loading=p['loading'])
    return get_enhancer(**kw)


@pytest.mark.parametrize('wpe_online', [False, True])
def test_pipeline(gpu_ctx, wpe_online):
    """The fused call's X_hat has the bits of ops.mvdr_souden_online_from_masks on the call's own
    Obs and mask taps with the window's reference channel; fused and stage path agree as
    test_block_by_block_path_equals_fused demands of the plain call; |x_hat| is within the
    end-to-end bar of the oracle's stages composed with the references."""
    from pb_chime5_amd import ops
    p = mr.PIPE
    u = mr.pipe_scene()
    enh = _pipe_enhancer(wpe_online)
    assert enh._fusable() and enh._bf_online() == dict(forget=p['forget'], loading=p['loading'])
    got = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, debug=True)
    det = enh.enhance_observation_locals['details']
    assert det['bf_online_fallbacks'] == 0
    ref = int(np.ravel(det['ref_channel'])[0])
    tm = np.asarray(det['target_mask']).reshape(det['X_hat'].shape[-2:])
    dm = np.asarray(det['distortion_mask']).reshape(tm.shape)
    assert 0 <= ref < p['num_channels'] and ref == gpu_ctx.last_ref_channel()
    stage = ops.mvdr_souden_online_from_masks(
        det['Obs'], tm, dm, True, forget=p['forget'], loading=p['loading'], ref_channel=ref,
        ctx=gpu_ctx)
    assert np.array_equal(np.asarray(det['X_hat']).reshape(tm.shape), stage)
    # ref_channel = -1 picks that channel on its own
    again = ops.mvdr_souden_online_from_masks(
        det['Obs'], tm, dm, True, forget=p['forget'], loading=p['loading'], ref_channel=-1,
        ctx=gpu_ctx)
    assert gpu_ctx.last_ref_channel() == ref and np.array_equal(again, stage)
    assert np.all(np.isfinite(got))
    blocks = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, fused=False)
    print(f'wpe_online={wpe_online}: stage path vs fused {rel_err(blocks, got):.1e}')
    assert rel_err(blocks, got) < 1e-10
    want = mr.pipe_reference(wpe_online)
    err = mr.abs_rel_err(got, want)
    print(f'wpe_online={wpe_online}: |x_hat| vs oracle chain {err:.1e}')
    assert err < mr.X_TOL, err
    # it is another signal than the whole-window beamformer gives
    plain = _pipe_enhancer(wpe_online, False)
    assert rel_err(plain.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex), got) > 1e-4


def test_bf_online_false_leaves_the_default_bits(gpu_ctx):
    from pb_chime5_amd.core import get_enhancer
    p = mr.PIPE
    u = mr.pipe_scene()
    kw = dict(wpe_tabs=p['wpe_taps'], wpe_delay=p['wpe_delay'], bss_iterations=p['bss_iterations'])
    a = get_enhancer(**kw).enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex)
    b = get_enhancer(bf_online=False, **kw).enhance_observation(u.obs, u.activity, u.speaker_id,
                                                               ex=u.ex)
    assert np.array_equal(a, b)


# ------------------------------------------------------------------ workspace hygiene
# (the few lines of tests/test_gpu_workspace_hygiene.py, restated: importing that module imports
# most of the suite)
@pytest.fixture(scope='module')
def hctx():
    """The module's own context: the session's `gpu_ctx` is never put into the debug mode."""
    from pb_chime5_amd._capi import Context
    ctx = Context(0)
    yield ctx
    ctx.close()


def _bits(value):
    if isinstance(value, np.ndarray):
        return value.dtype.str, value.shape, np.ascontiguousarray(value).tobytes()
    return value


def hygiene(ctx, call, what):
    """No guard violation under either poison pattern, and outputs that do not depend on the
    pattern; returns the outputs of the 0xFF run."""
    outs = {}
    for pattern in PATTERNS:
        ctx.debug_workspace(pattern)
        try:
            out = call(ctx)
            count, text, _ = ctx.debug_workspace_report()
        finally:
            ctx.debug_workspace(None)
        print(f'{what} [0x{pattern:02X}]: {count} guard violations {text}')
        assert count == 0, f'{what} [0x{pattern:02X}]: {text}'
        outs[pattern] = out
    a, b = outs[0x00], outs[0xFF]
    assert sorted(a) == sorted(b)
    differ = [name for name in sorted(a) if _bits(a[name]) != _bits(b[name])]
    assert not differ, f'{what}: {differ} depend on what the workspace held'
    return b


@pytest.mark.parametrize('cell', mr.CHUNK_CELLS, ids=str)
def test_workspace_hygiene_of_the_stage(hctx, cell):
    """From a state the library initialises in a poisoned block and hands back, from a throw-away
    state in the arena, and with the whole-window pass that picks the reference channel."""
    from pb_chime5_amd import ops
    D, beta, loading, F, T = cell
    Y, mx, mn, _ = mr.scene(cell, mr.seed_of(cell))

    def call(ctx):
        out = {}
        state = ops.OnlineMVDRState.fresh(F, D, loading, mr.to_dtf(Y), ctx=ctx)
        out['X'], out['W'] = _run(ctx, Y, mx, mn, cell, True, D - 1, state)
        out.update({f'state {k}': v for k, v in state.to_host().items()})
        out['X thrown away'], out['W thrown away'] = _run(ctx, Y, mx, mn, cell, True, D - 1)
        out['X window ref'], _ = _run(ctx, Y, mx, mn, cell, True, -1)
        out['ref'] = ctx.last_ref_channel()
        return out
    got = hygiene(hctx, call, f'online mvdr {cell}')
    Xr, Wr, st, _ = mr.reference(cell, True, D - 1, mr.seed_of(cell))
    errs = dict(X=rel_err(got['X'], Xr), W=rel_err(got['W'], Wr),
                phi_n=rel_err(got['state phi_n'], st['phi_n']))
    assert max(errs.values()) < mr.TOL, errs
    assert np.array_equal(got['X thrown away'], got['X'])
    assert 0 <= got['ref'] < D


@pytest.mark.parametrize('wpe_online', [False, True])
def test_workspace_hygiene_of_the_fused_entry(hctx, wpe_online):
    from pb_chime5_amd import ops
    p = mr.PIPE
    u = mr.pipe_scene()

    def call(ctx):
        x_hat, det = ops.enhance_observation_bf_online(
            u.obs, u.activity_array, u.target_index, 2048, 2048, forget=p['forget'],
            loading=p['loading'], wpe_online=wpe_online, wpe_alpha=p['wpe_alpha'] if wpe_online
            else ops.WPE_ONLINE_ALPHA, debug=True, ctx=ctx, wpe_taps=p['wpe_taps'],
            wpe_delay=p['wpe_delay'], bss_iterations=p['bss_iterations'],
            stft_size=p['stft_size'], stft_shift=p['stft_shift'])
        return dict(x_hat=x_hat, X_hat=det['X_hat'], fallbacks=det['bf_online_fallbacks'])
    got = hygiene(hctx, call, f'fused online mvdr, wpe_online={wpe_online}')
    assert mr.abs_rel_err(got['x_hat'], mr.pipe_reference(wpe_online)) < mr.X_TOL
