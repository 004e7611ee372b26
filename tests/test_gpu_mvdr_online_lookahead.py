"""The online MVDR's filter look-ahead on the GPU (gss_mvdr_online_lookahead,
gss_mvdr_online_lookahead_targets, gss_mvdr_online_release) against the NumPy reference of
tests/online_mvdr_lookahead_reference.py and against the existing operator: X in every cell, the
filter rows, the sums and the fallback counts to the bit, a recording fed in blocks, the fallback
rule, a zero target mask, the posteriors form, the workspace hygiene and the onset evidence.  Every
device run is made once and shared."""
import numpy as np
import pytest

import online_mvdr_lookahead_reference as lr
import online_mvdr_reference as mr
from conftest import rel_err

pytestmark = pytest.mark.gpu

PATTERNS = (0x00, 0xFF)
_RUNS = {}


def _state(ctx, cell, Y):
    from pb_chime5_amd import ops
    D, beta, loading, F, T = cell[:5]
    return ops.OnlineMVDRState.fresh(F, D, loading, mr.to_dtf(Y), ctx=ctx)


def _call(ctx, Y, mx, mn, cell, ban, ref, state, **kw):
    """Y (F,T,D), masks (F,T) -> X (F,R), W (F,R,D), the fallback count, through
    ops.mvdr_souden_online_from_masks."""
    from pb_chime5_amd import ops
    D, beta, loading = cell[:3]
    X, W, fallbacks = ops.mvdr_souden_online_from_masks(
        mr.to_dtf(Y), mx.T, mn.T, ban, forget=beta, loading=loading, ref_channel=ref, state=state,
        return_filters=True, return_fallbacks=True, ctx=ctx, **kw)
    return np.ascontiguousarray(X.T), np.ascontiguousarray(W.transpose(1, 0, 2)), fallbacks


def _release(hold):
    from pb_chime5_amd import ops
    X, W = ops.mvdr_online_release(hold, return_filters=True)
    return np.ascontiguousarray(X.T), np.ascontiguousarray(W.transpose(1, 0, 2))


def _in_blocks(ctx, Y, mx, mn, cell, ban, ref, blocks):
    """The scene through one state and one line in consecutive blocks, then the release -> X, W,
    the frames every call released, the state and the line on the host, the fallback count."""
    from pb_chime5_amd import ops
    D, beta, loading, F, T, L = cell
    state = _state(ctx, cell, Y)
    hold = ops.OnlineMVDRHold.fresh(F, D, L, ctx=ctx)
    Xs, Ws, counts, total, t0 = [], [], [], 0, 0
    for n in blocks:
        X, W, fallbacks = _call(ctx, Y[:, t0:t0 + n], mx[:, t0:t0 + n], mn[:, t0:t0 + n], cell, ban,
                                ref, state, lookahead=L, hold=hold)
        Xs.append(X)
        Ws.append(W)
        counts.append(X.shape[1])
        total += fallbacks
        t0 += n
    assert t0 == Y.shape[1]
    line = hold.to_host()
    X, W = _release(hold)
    assert hold.held == 0
    return (np.concatenate(Xs + [X], axis=1), np.concatenate(Ws + [W], axis=1), counts,
            state.to_host(), line, total)


def _device(ctx, cell, ban, ref):
    """One call and its release on the cell's scene, and the existing operator on it; once."""
    key = (cell, ban, ref)
    if key not in _RUNS:
        D, beta, loading, F, T, L = cell
        Y, mx, mn, _ = mr.scene(cell[:5], lr.seed_of(cell))
        X, W, counts, host, line, fallbacks = _in_blocks(ctx, Y, mx, mn, cell, ban, ref, (T,))
        state0 = _state(ctx, cell, Y)
        X0, W0, fallbacks0 = _call(ctx, Y, mx, mn, cell, ban, ref, state0)
        host0 = state0.to_host()
        for a in (X, W, X0, W0):
            a.setflags(write=False)
        _RUNS[key] = dict(X=X, W=W, counts=counts, host=host, line=line, fallbacks=fallbacks, X0=X0,
                          W0=W0, host0=host0, fallbacks0=fallbacks0)
    return _RUNS[key]


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize('cell', lr.CELLS, ids=str)
def test_against_the_reference_and_the_existing_operator(gpu_ctx, cell):
    """X at TOL of the reference; the filter rows are rows min(g + L, T - 1) of the existing
    operator's filters, the sums and the fallback counts the existing operator's, to the bit."""
    D, beta, loading, F, T, L = cell
    rows = lr.lookahead_rows(T, L)
    for ban, ref in lr.variants(cell):
        got = _device(gpu_ctx, cell, ban, ref)
        Xr, Wr, st, fallbacks = lr.reference(cell, ban, ref, lr.seed_of(cell))
        err = rel_err(got['X'], Xr)
        print(f'{cell} ban={ban} ref={ref}: X rel err {err:.2e}')
        assert got['X'].shape == (F, T) and got['counts'] == [max(0, T - L)]
        assert err < mr.TOL, (cell, ban, ref, err)
        assert np.array_equal(got['W'], got['W0'][:, rows]), (cell, ban, ref)
        for k in ('phi_x', 'phi_n'):
            assert np.array_equal(got['host'][k], got['host0'][k]), (cell, ban, ref, k)
        assert got['fallbacks'] == got['fallbacks0'] == fallbacks == 0
        assert got['line']['held'] == min(L, T)


def test_the_one_shot_form_is_the_call_plus_the_release(gpu_ctx):
    cell = lr.CELLS[0]
    D, beta, loading, F, T, L = cell
    Y, mx, mn, _ = mr.scene(cell[:5], lr.seed_of(cell))
    got = _device(gpu_ctx, cell, True, D - 1)
    X, W, _ = _call(gpu_ctx, Y, mx, mn, cell, True, D - 1, None, lookahead=L)
    assert np.array_equal(X, got['X']) and np.array_equal(W, got['W'])
    X, W, _ = _call(gpu_ctx, Y, mx, mn, cell, True, D - 1, _state(gpu_ctx, cell, Y), lookahead=L)
    assert np.array_equal(X, got['X']) and np.array_equal(W, got['W'])


# ------------------------------------------------------------------ partitions
@pytest.mark.parametrize('blocks', lr.PARTITIONS, ids=lambda b: f'{len(b)} blocks from {b[:6]}')
def test_partitions_give_the_bits_of_one_call_plus_release(gpu_ctx, blocks):
    cell = lr.PARTITION_CELL
    D, beta, loading, F, T, L = cell
    ban, ref = True, D - 1
    one = _device(gpu_ctx, cell, ban, ref)
    Y, mx, mn, _ = mr.scene(cell[:5], lr.seed_of(cell))
    X, W, counts, host, line, fallbacks = _in_blocks(gpu_ctx, Y, mx, mn, cell, ban, ref, blocks)
    assert counts == lr.released(blocks, L)
    assert np.array_equal(X, one['X']) and np.array_equal(W, one['W'])
    for k in ('phi_x', 'phi_n'):
        assert np.array_equal(host[k], one['host'][k]), k
    for k in ('frames', 'mask', 'filter'):
        assert np.array_equal(line[k], one['line'][k]), k
    assert line['held'] == L and fallbacks == 0
    assert np.array_equal(line['frames'], Y[:, T - L:]) and np.array_equal(line['mask'], mx[:, T - L:])


def test_release_twice_and_before_any_frame(gpu_ctx):
    from pb_chime5_amd import ops
    cell = lr.PARTITION_CELL
    D, beta, loading, F, T, L = cell
    hold = ops.OnlineMVDRHold.fresh(F, D, L, ctx=gpu_ctx)
    X, W = ops.mvdr_online_release(hold, return_filters=True)
    assert X.shape == (0, F) and W.shape == (0, F, D) and hold.held == 0
    Y, mx, mn, _ = mr.scene(cell[:5], lr.seed_of(cell))
    state = _state(gpu_ctx, cell, Y)
    X, _, _ = _call(gpu_ctx, Y[:, :3], mx[:, :3], mn[:, :3], cell, False, 0, state, lookahead=L,
                    hold=hold)
    assert X.shape == (F, 0) and hold.held == 3
    sums = state.to_host()
    assert ops.mvdr_online_release(hold).shape == (3, F) and hold.held == 0
    assert ops.mvdr_online_release(hold).shape == (0, F)
    after = state.to_host()
    assert all(np.array_equal(sums[k], after[k]) for k in sums)     # a release leaves the sums


def test_a_line_saved_to_the_host_continues_with_the_same_bits(gpu_ctx):
    """to_host while frames are held, from_host into a NEW context."""
    from pb_chime5_amd import ops
    from pb_chime5_amd._capi import Context
    cell = lr.PARTITION_CELL
    D, beta, loading, F, T, L = cell
    ban, ref = True, 0
    one = _device(gpu_ctx, cell, ban, ref)
    Y, mx, mn, _ = mr.scene(cell[:5], lr.seed_of(cell))
    state, hold = _state(gpu_ctx, cell, Y), ops.OnlineMVDRHold.fresh(F, D, L, ctx=gpu_ctx)
    a, _, _ = _call(gpu_ctx, Y[:, :70], mx[:, :70], mn[:, :70], cell, ban, ref, state, lookahead=L,
                    hold=hold)
    saved = state.to_host(), hold.to_host()
    other = Context(0)
    try:
        state2 = ops.OnlineMVDRState.from_host(saved[0], ctx=other)
        hold2 = ops.OnlineMVDRHold.from_host(saved[1], ctx=other)
        assert hold2.held == L and hold2.key == (F, D, L)
        b, _, _ = _call(other, Y[:, 70:], mx[:, 70:], mn[:, 70:], cell, ban, ref, state2,
                        lookahead=L, hold=hold2)
        c, _ = _release(hold2)
        assert np.array_equal(np.concatenate([a, b, c], axis=1), one['X'])
        del state2, hold2
    finally:
        other.close()


# ------------------------------------------------------------------ fallbacks, zero mask
def test_fallback_frames(gpu_ctx):
    """'all': every X exactly 0, the count F T.  'first' with L = 2: the filters of frames 0..2 are
    fallbacks, so X[0] (the filter of frame 2) is exactly 0, X[1] (of frame 3) is not and equals
    the reference; the count is 3 F, counted when the frames enter."""
    from pb_chime5_amd import ops
    Y, mx, mn, st0, beta, count = mr.fallback_case('all')
    F, T, D = Y.shape
    cell = (D, beta, 1.0, F, T, 4)
    state = ops.OnlineMVDRState.from_host(st0, ctx=gpu_ctx)
    hold = ops.OnlineMVDRHold.fresh(F, D, 4, ctx=gpu_ctx)
    X, W, fallbacks = _call(gpu_ctx, Y, mx, mn, cell, False, 0, state, lookahead=4, hold=hold)
    tail, _ = _release(hold)
    assert fallbacks == count == F * T and X.shape == (F, T - 4)
    assert np.all(X == 0) and np.all(W == 0) and np.all(tail == 0)

    Y, mx, mn, st0, beta, count = mr.fallback_case('first')
    F, T, D = Y.shape
    cell = (D, beta, 1.0, F, T, 2)
    state = ops.OnlineMVDRState.from_host(st0, ctx=gpu_ctx)
    hold = ops.OnlineMVDRHold.fresh(F, D, 2, ctx=gpu_ctx)
    X, _, fallbacks = _call(gpu_ctx, Y, mx, mn, cell, False, 0, state, lookahead=2, hold=hold)
    X = np.concatenate([X, _release(hold)[0]], axis=1)
    Xr = lr.lookahead_mvdr(Y, mx, mn, beta, 0, False, 2, state=st0)[0]
    assert fallbacks == count == 3 * F
    assert np.all(X[:, 0] == 0) and np.all(X[:, 1] != 0)
    assert rel_err(X, Xr) < mr.TOL


def test_zero_target_mask_gives_exactly_zero(gpu_ctx):
    cell = lr.CELLS[0]
    D, beta, loading, F, T, L = cell
    Y, mx, mn, _ = mr.scene(cell[:5], lr.seed_of(cell))
    for ban in (False, True):
        X, W, fallbacks = _call(gpu_ctx, Y, np.zeros_like(mx), mn, cell, ban, 0, None, lookahead=L)
        assert X.shape == (F, T) and np.all(X == 0) and np.all(W == 0) and fallbacks == 0


# ------------------------------------------------------------------ the posteriors form
def _posteriors(K, T, F, seed=0):
    g = np.random.default_rng([seed, K, T, F]).random((K, T, F)) + 0.05
    return g / g.sum(axis=0)


def _mask_mul(X, mask):
    """re * m, im * m as the library's postfilter, not a complex product."""
    out = np.empty(X.shape, np.complex128)
    out.real, out.imag = X.real * mask, X.imag * mask
    return out


def _targets(ctx, Y, g, targets, cell, postfilter, holds=None, states=None):
    from pb_chime5_amd import ops
    D, beta, loading, F, T, L = cell
    states = states or [_state(ctx, cell, Y) for _ in targets]
    out = ops.mvdr_souden_online_targets(
        mr.to_dtf(Y), g, targets, states=states, forget=beta, ref_channel=D - 1, ban=True,
        postfilter=postfilter, return_filters=True, return_fallbacks=True, lookahead=L, hold=holds)
    return out + (states,)


@pytest.mark.parametrize('postfilter', [None, 'mask_mul'])
def test_posteriors_form_rows_have_the_bits_of_the_masks_form(gpu_ctx, postfilter):
    """S = 3 of K = 4: every row is the masks form on that class's masks; the postfilter multiplies
    by the mask of the OUTPUT frame g (random posteriors: not that of g + L)."""
    from pb_chime5_amd import ops
    cell = (4, 0.99, 1e-2, 3, 150, 4)
    D, beta, loading, F, T, L = cell
    Y = mr.scene(cell[:5])[0]
    g = _posteriors(4, T, F)
    targets = (2, 0, 3)
    X, W, fallbacks, states = _targets(gpu_ctx, Y, g, targets, cell, postfilter)
    assert X.shape == (3, T, F) and W.shape == (3, T, F, D) and fallbacks == [0, 0, 0]
    for s, k in enumerate(targets):
        mx, mn = ops.masks_from_posteriors(g, k, ctx=gpu_ctx)
        st = _state(gpu_ctx, cell, Y)
        Xm, Wm, _ = _call(gpu_ctx, Y, mx.T, mn.T, cell, True, D - 1, st, lookahead=L)
        want = Xm.T
        if postfilter:
            want = _mask_mul(Xm.T, mx)
            assert not np.array_equal(X[s], _mask_mul(Xm.T, mx[lr.lookahead_rows(T, L)]))
        assert np.array_equal(X[s], want), (s, k)
        assert np.array_equal(W[s], Wm.transpose(1, 0, 2)), (s, k)
        for name, a in st.to_host().items():
            assert np.array_equal(states[s].to_host()[name], a), (s, name)


def test_posteriors_form_in_blocks(gpu_ctx):
    """Blocks through S lines, then the release: the bits of the one-shot form, with the
    postfilter on values the lines carried across the calls."""
    from pb_chime5_amd import ops
    cell = (4, 0.99, 1e-2, 3, 150, 4)
    D, beta, loading, F, T, L = cell
    Y = mr.scene(cell[:5])[0]
    g = _posteriors(4, T, F)
    targets = (2, 0, 3)
    X1 = _targets(gpu_ctx, Y, g, targets, cell, 'mask_mul')[0]
    holds = [ops.OnlineMVDRHold.fresh(F, D, L, ctx=gpu_ctx) for _ in targets]
    states = [_state(gpu_ctx, cell, Y) for _ in targets]
    Xs, t0 = [], 0
    for n in (3, 1, 5, 141):
        Xs.append(_targets(gpu_ctx, Y[:, t0:t0 + n], g[:, t0:t0 + n], targets, cell, 'mask_mul',
                           holds, states)[0])
        t0 += n
    Xs.append(ops.mvdr_online_release(holds, postfilter='mask_mul'))
    assert [x.shape[1] for x in Xs] == [0, 0, 5, 141, 4]
    assert np.array_equal(np.concatenate(Xs, axis=1), X1)


@pytest.mark.parametrize('D', [12, 20, 28])
def test_posteriors_form_other_channel_counts(gpu_ctx, D):
    """S = 1 at D = 12, 20 and 28: the other forms NR of the posteriors kernel."""
    from pb_chime5_amd import ops
    cell = (D, 0.99, 1.0, 2, 40, 3)
    beta, loading, F, T, L = cell[1:]
    Y = mr.scene(cell[:5])[0]
    g = _posteriors(3, T, F)
    X, W, fallbacks, _ = _targets(gpu_ctx, Y, g, (1,), cell, None)
    mx, mn = ops.masks_from_posteriors(g, 1, ctx=gpu_ctx)
    Xm, Wm, _ = _call(gpu_ctx, Y, mx.T, mn.T, cell, True, D - 1, _state(gpu_ctx, cell, Y),
                      lookahead=L)
    assert np.array_equal(X[0], Xm.T) and np.array_equal(W[0], Wm.transpose(1, 0, 2))
    assert np.all(np.isfinite(X)) and np.any(X != 0) and fallbacks == [0]


# ------------------------------------------------------------------ workspace hygiene
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


@pytest.mark.parametrize('cell', [lr.CELLS[0], lr.CELLS[5]], ids=str)
def test_workspace_hygiene_of_the_stage_entries(hctx, cell):
    D, beta, loading, F, T, L = cell
    Y, mx, mn, _ = mr.scene(cell[:5], lr.seed_of(cell))
    g = _posteriors(3, T, F)

    def call(ctx):
        out = {}
        out['X'], out['W'], _, host, line, out['fallbacks'] = _in_blocks(
            ctx, Y, mx, mn, cell, True, D - 1, (T // 2, T - T // 2))
        out.update({f'state {k}': v for k, v in host.items()})
        out.update({f'line {k}': v for k, v in line.items()})
        out['X targets'], out['W targets'], out['fallbacks targets'], _ = _targets(
            ctx, Y, g, (2, 0), cell, 'mask_mul')
        return out
    got = hygiene(hctx, call, f'online mvdr look-ahead {cell}')
    Xr = lr.reference(cell, True, D - 1, lr.seed_of(cell))[0]
    assert rel_err(got['X'], Xr) < mr.TOL


# ------------------------------------------------------------------ the evidence
def test_the_lookahead_helps_at_an_onset(gpu_ctx):
    """The device's X on the onset scene: the error over the 16 frames after the onset at L = 4 is
    at most ONSET_BOUND x that at L = 0."""
    D, beta, loading, F, T = lr.ONSET_CELL
    L = lr.ONSET_LOOKAHEAD
    Y, mx, mn, image = lr.onset_scene()
    cell = lr.ONSET_CELL + (L,)
    X0, _, _ = _call(gpu_ctx, Y, mx, mn, cell, False, 0, None)
    X, _, _ = _call(gpu_ctx, Y, mx, mn, cell, False, 0, None, lookahead=L)
    e0, eL = lr.onset_error(X0, image[:, :, 0]), lr.onset_error(X, image[:, :, 0])
    print(f'onset: error {e0:.3f} at L = 0, {eL:.3f} at L = {L}, ratio {eL / e0:.3f}')
    assert eL / e0 <= lr.ONSET_BOUND
