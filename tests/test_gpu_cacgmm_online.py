"""Online CACGMM on the GPU (gss_cacgmm_online, gss_enhance_observation_gss_online) against the
NumPy reference of tests/online_cacgmm_reference.py: the posteriors and the handed-out state in
every cell, a run continued from a fitted model, a recording fed in blocks, determinism, the state's
triangles, the model round trip, edge inputs and the fallback rule, the errors, the evidence, the
pipeline, the workspace hygiene and the untouched default.  Every device run is made once and
shared."""
import ctypes
import functools

import numpy as np
import pytest

import online_cacgmm_reference as cr
from conftest import rel_err

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -4
PATTERNS = (0x00, 0xFF)


def _run(ctx, Y, mask, beta, state=None, prior_mass=1.0, **kw):
    """Y (F,T,D), mask (K,T) / (F,K,T) / None -> gamma (F,K,T) through ops.cacgmm_posteriors_online."""
    from pb_chime5_amd import ops
    if mask is not None and np.ndim(mask) == 3:
        mask = np.transpose(mask, (1, 2, 0))
    out = ops.cacgmm_posteriors_online(cr.to_dtf(Y), mask, forget=beta, prior_mass=prior_mass,
                                       state=state, ctx=ctx, **kw)
    if isinstance(out, tuple):
        return (np.ascontiguousarray(out[0].transpose(2, 0, 1)),) + out[1:]
    return np.ascontiguousarray(out.transpose(2, 0, 1))


_RUNS = {}


def _device(ctx, cell):
    """gamma and the state after the cell's scene from a fresh state; once."""
    from pb_chime5_amd import ops
    if cell not in _RUNS:
        D, K, beta, prior_mass, F, T = cell
        Y, activity = cr.scene(cell, cr.seed_of(cell))
        state = ops.OnlineCACGMMState.fresh(F, K, D, prior_mass, ctx=ctx)
        gamma, fallbacks = _run(ctx, Y, activity, beta, state, return_fallbacks=True)
        host = state.to_host()
        for a in (gamma, host['s'], host['n']):
            a.setflags(write=False)
        _RUNS[cell] = gamma, host, fallbacks
    return _RUNS[cell]


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize('cell', cr.CELLS, ids=str)
def test_against_the_reference(gpu_ctx, cell):
    gamma, host, fallbacks = _device(gpu_ctx, cell)
    gr, st, fr = cr.reference(cell, cr.seed_of(cell))
    assert fallbacks == fr == 0
    errs = dict(gamma=rel_err(gamma, gr), s=rel_err(host['s'], st['s']), n=rel_err(host['n'], st['n']))
    print(f'{cell}: rel err {errs}')
    assert max(errs.values()) < cr.TOL, (cell, errs)


@functools.lru_cache(maxsize=None)
def _fitted_model():
    """A model fitted with cacgmm_fit on the first half of MODEL_CELL's scene."""
    from pb_chime5_amd import ops
    D, K, beta, prior_mass, F, T = cr.MODEL_CELL
    Y, activity = cr.scene(cr.MODEL_CELL)
    half = T // 2
    init, mask = ops.guidance_from_activity(activity[:, :half])
    return ops.cacgmm_fit(cr.to_dtf(Y[:, :half]), init, mask, iterations=5)


def test_an_unguided_run_from_a_fitted_model(gpu_ctx):
    """from_model of a cacgmm_fit model, then the second half without a mask: the state the device
    derives from the model, the posteriors and the final state against the reference started
    from the same model."""
    from pb_chime5_amd import ops
    D, K, beta, prior_mass, F, T = cr.MODEL_CELL
    Y, _ = cr.scene(cr.MODEL_CELL)
    half = T // 2
    model = _fitted_model()
    state = ops.OnlineCACGMMState.from_model(model, mass=cr.MODEL_MASS, ctx=gpu_ctx)
    start = state.to_host()
    want = cr.from_model(model.precision, model.weight, cr.MODEL_MASS)
    errs = rel_err(start['s'], want['s']), rel_err(start['n'], want['n'])
    print(f'from_model: S, n vs np.linalg.inv {errs}')
    assert max(errs) < cr.ROUND_TRIP_TOL, errs
    assert np.array_equal(start['s'], start['s'].conj().swapaxes(-1, -2))
    gamma = _run(gpu_ctx, Y[:, half:], None, beta, state)
    gr, st, fr = cr.online_cacgmm(Y[:, half:], None, beta, start)
    host = state.to_host()
    errs = dict(gamma=rel_err(gamma, gr), s=rel_err(host['s'], st['s']), n=rel_err(host['n'], st['n']))
    print(f'unguided from a model: rel err {errs}')
    assert fr == 0 and max(errs.values()) < cr.TOL, errs
    # the classes are told apart without a mask
    assert np.max(gamma) > 0.9 and np.min(gamma) < 0.1


# ------------------------------------------------------------------ blocks, determinism
@pytest.mark.parametrize('cell', cr.CHUNK_CELLS, ids=str)
def test_blocks_through_one_state_equal_the_single_call(gpu_ctx, cell):
    """T frames fed as four blocks (the first of one frame) through one state: gamma and the final
    state have the bits of the single call; a state saved to the host after the second block and
    restored into a NEW context continues with the same bits; a copy is independent."""
    from pb_chime5_amd import ops
    from pb_chime5_amd._capi import Context
    D, K, beta, prior_mass, F, T = cell
    gamma1, host1, _ = _device(gpu_ctx, cell)
    Y, activity = cr.scene(cell, cr.seed_of(cell))
    state = ops.OnlineCACGMMState.fresh(F, K, D, prior_mass, ctx=gpu_ctx)
    bounds = np.concatenate([[0], np.cumsum(cr.CHUNKS[T])])
    assert bounds[-1] == T
    outs, saved = [], None
    for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        outs.append(_run(gpu_ctx, Y[:, a:b], activity[:, a:b], beta, state))
        if i == 1:
            saved = state.to_host()
    assert np.array_equal(np.concatenate(outs, axis=-1), gamma1)
    host = state.to_host()
    for k in ('s', 'n'):
        assert np.array_equal(host[k], host1[k]), k
    other = Context(0)
    try:
        restored = ops.OnlineCACGMMState.from_host(saved, ctx=other)
        tail = [_run(other, Y[:, a:b], activity[:, a:b], beta, restored)
                for a, b in zip(bounds[2:-1], bounds[3:])]
        assert np.array_equal(np.concatenate(tail, axis=-1), gamma1[:, :, bounds[2]:])
        host2 = restored.to_host()
        for k in ('s', 'n'):
            assert np.array_equal(host2[k], host1[k]), k
        twin = restored.copy()
        _run(other, Y[:, :3], activity[:, :3], beta, twin)
        assert np.array_equal(restored.to_host()['s'], host1['s'])
        assert not np.array_equal(twin.to_host()['s'], host1['s'])
        del restored, twin
    finally:
        other.close()


def test_a_throwaway_state_and_a_second_call_give_the_same_bits(gpu_ctx):
    from pb_chime5_amd import ops
    for cell in cr.CHUNK_CELLS:
        D, K, beta, prior_mass, F, T = cell
        gamma1, host1, _ = _device(gpu_ctx, cell)
        Y, activity = cr.scene(cell, cr.seed_of(cell))
        assert np.array_equal(_run(gpu_ctx, Y, activity, beta, prior_mass=prior_mass), gamma1), cell
        state = ops.OnlineCACGMMState.fresh(F, K, D, prior_mass, ctx=gpu_ctx)
        assert np.array_equal(_run(gpu_ctx, Y, activity, beta, state), gamma1), cell
        host = state.to_host()
        for k in ('s', 'n'):
            assert np.array_equal(host[k], host1[k]), (cell, k)
        # a mask per frequency that says the same thing gives the same bits
        per_f = np.broadcast_to(activity, (F,) + activity.shape)
        assert np.array_equal(_run(gpu_ctx, Y, per_f, beta, prior_mass=prior_mass), gamma1), cell


def test_no_mask_from_a_fresh_state_never_separates(gpu_ctx):
    """(Python refuses the call; the C entry runs it.)  Every class gets the same bits: 1 / K to
    (2 K + 1) half-ulps (test_online_cacgmm_api says why), exactly for K = 2."""
    from pb_chime5_amd import _capi
    for cell in ((4, 3, 0.99, 1.0, 3, 150), (4, 8, 0.9, 1.0, 2, 200), (2, 2, 1.0, 1.0, 2, 70)):
        D, K, beta, prior_mass, F, T = cell
        Y, _ = cr.scene(cell)
        Y_d = gpu_ctx.to_device(Y)
        g_d = gpu_ctx.empty(8 * F * K * T)
        cfg = _capi.GssEmOnline(forget=beta, prior_mass=prior_mass)
        gpu_ctx._check(gpu_ctx.lib.gss_cacgmm_online(
            gpu_ctx.handle, ctypes.c_void_p(Y_d.ptr), F, T, D, None, K, ctypes.byref(cfg), None,
            ctypes.c_void_p(g_d.ptr)), 'gss_cacgmm_online')
        gamma = gpu_ctx.to_host(g_d, (F, K, T), np.float64)
        assert all(np.array_equal(gamma[:, 0], gamma[:, k]) for k in range(K)), cell
        assert np.max(np.abs(gamma * K - 1.0)) <= (2 * K + 1) * np.finfo(float).eps / 2, cell
        if K == 2:
            assert np.all(gamma == 0.5)


# ------------------------------------------------------------------ long horizons
def _long_device(ctx, cell):
    """gamma, the state and the fallback count after the long cell's scene in ONE call; once."""
    from pb_chime5_amd import ops
    key = ('long', cell)
    if key not in _RUNS:
        D, K, beta, prior_mass, F, T = cell
        Y, activity = cr.scene(cell, cr.long_seed_of(cell))
        state = ops.OnlineCACGMMState.fresh(F, K, D, prior_mass, ctx=ctx)
        gamma, fallbacks = _run(ctx, Y, activity, beta, state, return_fallbacks=True)
        host = state.to_host()
        for a in (gamma, host['s'], host['n']):
            a.setflags(write=False)
        _RUNS[key] = gamma, host, fallbacks
    return _RUNS[key]


@pytest.mark.parametrize('cell', cr.LONG_CELLS, ids=str)
def test_long_cells_against_the_reference(gpu_ctx, cell):
    """Thousands of frames in one call: gamma, S and n within the cell's bar (long_tol: TOL, and
    1.1e-10 for the one cell in which no seed allows TOL) of the reference, no fallback
    on either side, gamma finite and summing to 1 over the classes wherever a class is allowed,
    the handed-out S exactly Hermitian and inside the scale band."""
    D, K, beta, prior_mass, F, T = cell
    gamma, host, fallbacks = _long_device(gpu_ctx, cell)
    gr, st, fr = cr.reference(cell, cr.long_seed_of(cell))
    errs = dict(gamma=rel_err(gamma, gr), s=rel_err(host['s'], st['s']), n=rel_err(host['n'], st['n']))
    print(f'{cell}: rel err {errs}, fallbacks {fallbacks} / {fr}, pins {len(cr.long_pins(cell))}')
    assert fallbacks == 0 and fr == 0
    assert max(errs.values()) < cr.long_tol(cell), (cell, errs)
    _, activity = cr.scene(cell, cr.long_seed_of(cell))
    on = activity.any(axis=0)
    assert np.all(np.isfinite(gamma))
    assert np.max(np.abs(gamma.sum(axis=1)[:, on] - 1.0)) <= 1e-12
    S = host['s']
    assert np.array_equal(S, S.conj().swapaxes(-1, -2))
    assert np.all(S[..., np.arange(D), np.arange(D)].imag == 0) and np.all(host['n'] > 0)
    assert np.all(np.abs(cr.scale_exponents(S)) <= cr.SCALE_BAND)
    if cell == cr.PIN_CELL:
        assert len(cr.long_pins(cell)) >= 2


@pytest.mark.parametrize('cell', cr.LONG_CELLS, ids=str)
def test_long_cells_in_blocks_give_the_bits_of_the_single_call(gpu_ctx, cell):
    """Blocks of 625 frames and one ragged partition (online_cacgmm_reference.long_partitions: in
    the cell whose scale pin fires, one rescaling on the last frame of a block and one on the
    first) through one state; in the 625-frame run the state is saved with to_host in the middle
    and restored into a new state that carries on."""
    from pb_chime5_amd import ops
    D, K, beta, prior_mass, F, T = cell
    gamma1, host1, _ = _long_device(gpu_ctx, cell)
    Y, activity = cr.scene(cell, cr.long_seed_of(cell))
    for name, cuts in cr.long_partitions(cell).items():
        bounds = np.concatenate([[0], np.cumsum(cuts)])
        assert bounds[-1] == T
        state = ops.OnlineCACGMMState.fresh(F, K, D, prior_mass, ctx=gpu_ctx)
        outs, total = [], 0
        for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
            if name == 'blocks' and i == len(cuts) // 2:
                state = ops.OnlineCACGMMState.from_host(state.to_host(), ctx=gpu_ctx)
            g, fb = _run(gpu_ctx, Y[:, a:b], activity[:, a:b], beta, state, return_fallbacks=True)
            outs.append(g)
            total += fb
        assert total == 0, name
        assert np.array_equal(np.concatenate(outs, axis=-1), gamma1), name
        host = state.to_host()
        for k in ('s', 'n'):
            assert np.array_equal(host[k], host1[k]), (name, k)


def test_scale_invariance(gpu_ctx):
    """A state handed in with S_k multiplied by 2^e_k, e_k from {-600, -200, 200, 600} and another
    one per class: the gamma of the unscaled run within TOL; after the call every class's
    largest diagonal entry is back inside the band and n is the unscaled run's."""
    from pb_chime5_amd import ops
    cell = cr.CELLS[0]
    D, K, beta, prior_mass, F, T = cell
    assert T == 150
    Y, activity = cr.scene(cell, cr.seed_of(cell))
    state = ops.OnlineCACGMMState.fresh(F, K, D, prior_mass, ctx=gpu_ctx)
    _run(gpu_ctx, Y[:, :20], activity[:, :20], beta, state)
    mid = state.to_host()
    want = _run(gpu_ctx, Y[:, 20:], activity[:, 20:], beta, state)
    n_want = state.to_host()['n']
    scaled = ops.OnlineCACGMMState.from_host(cr.scaled_state(mid), ctx=gpu_ctx)
    assert np.abs(cr.scale_exponents(scaled.to_host()['s'])).min() > 100
    gamma, fallbacks = _run(gpu_ctx, Y[:, 20:], activity[:, 20:], beta, scaled, return_fallbacks=True)
    after = scaled.to_host()
    gr = cr.online_cacgmm(Y[:, 20:], activity[:, 20:], beta, mid)[0]
    errs = rel_err(gamma, want), rel_err(gamma, gr), rel_err(after['n'], n_want)
    print(f'scaled state: gamma vs the unscaled run {errs[0]:.1e}, vs the reference {errs[1]:.1e}, '
          f'n {errs[2]:.1e}; exponents after {cr.scale_exponents(after["s"]).tolist()}')
    assert fallbacks == 0 and max(errs) < cr.TOL, errs
    assert np.all(np.abs(cr.scale_exponents(after['s'])) <= cr.SCALE_BAND)


def _starved_device(ctx):
    """gamma, the state and the fallback count after the starved cell in ONE call; once."""
    from pb_chime5_amd import ops
    if 'starved' not in _RUNS:
        p = cr.STARVED
        Y, activity = cr.starved_scene()
        state = ops.OnlineCACGMMState.fresh(Y.shape[0], p['K'], p['D'], p['prior_mass'], ctx=ctx)
        gamma, fallbacks = _run(ctx, Y, activity, p['beta'], state, return_fallbacks=True)
        host = state.to_host()
        for a in (gamma, host['s'], host['n']):
            a.setflags(write=False)
        _RUNS['starved'] = gamma, host, fallbacks
    return _RUNS['starved']


def test_the_starved_class_keeps_its_factor(gpu_ctx):
    """The starved cell (online_cacgmm_reference.STARVED), the one cell in which the gate of the
    rank guard is not 0: no fallback on the device or in the reference, and -- cond(S_k) x eps is
    1e-5 here, so not at TOL -- the device's gamma within 5 x the float64 reference's own distance
    from the 80-bit referee, plus 1e-9, of that referee.  That bar is mostly its 1e-9; so that an
    error in the device's pivot or gate shows, the device is also held to the reference at 100 x
    the reference's own distance from the referee (two float64 programs of one recursion whose
    exact course the referee gives)."""
    gamma, host, fallbacks = _starved_device(gpu_ctx)
    gr, st, fr, cond = cr.starved_reference()
    referee, failed = cr.starved_referee()
    ref_dist = float(np.max(np.abs(gr - referee)))
    dev_dist = float(np.max(np.abs(gamma - referee)))
    dev_ref = float(np.max(np.abs(gamma - gr)))
    print(f'starved cell: reference vs referee {ref_dist:.1e}, device vs referee {dev_dist:.1e}, '
          f'device vs reference {dev_ref:.1e}; fallbacks {fallbacks} / {fr}, '
          f'cond(S_k) of the reference up to {cond:.1e}')
    assert fallbacks == 0 and fr == 0 and failed == 0
    assert cond <= cr.STARVED_COND and ref_dist <= cr.STARVED_REFEREE_TOL
    assert np.all(np.isfinite(gamma))
    assert dev_dist <= 5 * ref_dist + 1e-9
    assert dev_ref <= 100 * ref_dist
    assert np.array_equal(host['s'], host['s'].conj().swapaxes(-1, -2))
    assert np.max(np.linalg.cond(host['s'])) <= cr.STARVED_COND


def test_the_starved_cell_in_blocks_gives_the_bits_of_the_single_call(gpu_ctx):
    """The rank guard across block borders (test_online_cacgmm_api proves that its gate is above
    0.1 on both sides of the cuts): blocks of 625 frames, with the state saved by to_host and
    restored in the middle, and the ragged partition with a one-frame block among live frames."""
    from pb_chime5_amd import ops
    p = cr.STARVED
    Y, activity = cr.starved_scene()
    F, T, D = Y.shape
    gamma1, host1, _ = _starved_device(gpu_ctx)
    for name, cuts in cr.starved_partitions().items():
        bounds = np.concatenate([[0], np.cumsum(cuts)])
        assert bounds[-1] == T
        state = ops.OnlineCACGMMState.fresh(F, p['K'], D, p['prior_mass'], ctx=gpu_ctx)
        outs, total = [], 0
        for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
            if name == 'blocks' and i == 9:         # the cut at 5 625, where the guard is live
                state = ops.OnlineCACGMMState.from_host(state.to_host(), ctx=gpu_ctx)
            g, fb = _run(gpu_ctx, Y[:, a:b], activity[:, a:b], p['beta'], state, return_fallbacks=True)
            outs.append(g)
            total += fb
        assert total == 0, name
        assert np.array_equal(np.concatenate(outs, axis=-1), gamma1), name
        host = state.to_host()
        for k in ('s', 'n'):
            assert np.array_equal(host[k], host1[k]), (name, k)


# ------------------------------------------------------------------ the state
@pytest.mark.parametrize('cell', [cr.CELLS[0], cr.CELLS[3], cr.CELLS[8], cr.CELLS[10]], ids=str)
def test_handed_out_state_is_exactly_hermitian(gpu_ctx, cell):
    D = cell[0]
    _, host, _ = _device(gpu_ctx, cell)
    S = host['s']
    assert np.array_equal(S, S.conj().swapaxes(-1, -2))
    assert np.all(S[..., np.arange(D), np.arange(D)].imag == 0)
    assert np.all(host['n'] > 0)


def test_a_reader_takes_the_upper_triangle(gpu_ctx):
    """Garbage below the diagonal and in the imaginary part of the diagonal of a state that is
    handed in changes nothing."""
    from pb_chime5_amd import ops
    cell = cr.CELLS[0]
    D, K, beta, prior_mass, F, T = cell
    gamma1, host1, _ = _device(gpu_ctx, cell)
    Y, activity = cr.scene(cell, cr.seed_of(cell))
    state = ops.OnlineCACGMMState.fresh(F, K, D, prior_mass, ctx=gpu_ctx)
    head = _run(gpu_ctx, Y[:, :30], activity[:, :30], beta, state)
    mid = state.to_host()
    lower = np.tril_indices(D, -1)
    S = mid['s'].copy()
    S[..., lower[0], lower[1]] = 7.0 - 3.0j
    S[..., np.arange(D), np.arange(D)] += 5.0j
    state = ops.OnlineCACGMMState.from_host(dict(s=S, n=mid['n']), ctx=gpu_ctx)
    tail = _run(gpu_ctx, Y[:, 30:], activity[:, 30:], beta, state)
    assert np.array_equal(np.concatenate([head, tail], axis=-1), gamma1)
    host = state.to_host()
    for k in ('s', 'n'):
        assert np.array_equal(host[k], host1[k]), k
    # the conversion to a model reads the same way
    assert np.array_equal(ops.OnlineCACGMMState.from_host(dict(s=S, n=mid['n']), ctx=gpu_ctx)
                          .to_model().precision,
                          ops.OnlineCACGMMState.from_host(mid, ctx=gpu_ctx).to_model().precision)


# ------------------------------------------------------------------ the model round trip
@pytest.mark.parametrize('cell', cr.CHUNK_CELLS, ids=str)
def test_model_round_trip(gpu_ctx, cell):
    """to_model() then cacgmm_predict on frame T - 1 is the gamma the online call gives that frame
    when fed next; from_model(to_model(), mass = sum n) gives the state back; the model is the
    reference's."""
    from pb_chime5_amd import ops
    D, K, beta, prior_mass, F, T = cell
    Y, activity = cr.scene(cell, cr.seed_of(cell))
    T = max(T, 2)
    state = ops.OnlineCACGMMState.fresh(F, K, D, prior_mass, ctx=gpu_ctx)
    _run(gpu_ctx, Y[:, :T - 1], activity[:, :T - 1], beta, state)
    before = state.to_host()
    model = state.to_model()
    assert model.shape == (F, K, D)
    P = model.precision
    assert np.array_equal(P, P.conj().swapaxes(-1, -2))
    precision, log_det, weight = cr.to_model(before)
    errs = dict(precision=rel_err(P, precision), log_det=rel_err(model.log_determinant, log_det),
                weight=rel_err(model.weight, weight))
    print(f'{cell}: to_model vs np.linalg {errs}')
    assert max(errs.values()) < cr.ROUND_TRIP_TOL, errs
    last = slice(T - 1, T)
    predicted = ops.cacgmm_predict(model, cr.to_dtf(Y[:, last]), activity[:, last], ctx=gpu_ctx)
    fed = _run(gpu_ctx, Y[:, last], activity[:, last], beta, state.copy())
    err = rel_err(predicted.transpose(2, 0, 1), fed)
    print(f'{cell}: predict(to_model()) vs the next online frame {err:.1e}')
    assert err < cr.TOL, err
    mass = before['n'].sum(axis=1)
    # (every frame adds sum_k g_k, which the clip keeps within [1, 1 + K 1e-10]: the frequencies
    # carry the same mass to that, far inside the round trip's bar)
    assert rel_err(mass, np.full(F, mass[0])) <= K * cr.AFF_EPS
    back = ops.OnlineCACGMMState.from_model(model, mass=float(mass[0]), ctx=gpu_ctx).to_host()
    errs = rel_err(back['s'], before['s']), rel_err(back['n'], before['n'])
    print(f'{cell}: from_model(to_model()) vs the state {errs}')
    assert max(errs) < cr.ROUND_TRIP_TOL, errs
    # the model object's other consumers take it
    perm = np.tile(np.arange(K)[::-1], (F, 1))
    swapped = ops.cacgmm_model_permute(model, perm, ctx=gpu_ctx)
    assert np.array_equal(swapped.weight, model.weight[:, ::-1])
    refit = ops.cacgmm_fit(cr.to_dtf(Y), None, activity, iterations=1, model=model, ctx=gpu_ctx)
    assert np.all(np.isfinite(refit.precision)) and refit.shape == model.shape


def test_a_model_without_a_factor_is_an_error(gpu_ctx):
    from pb_chime5_amd import ops
    from pb_chime5_amd.cacgmm import CACGMM
    model = _fitted_model()
    precision = model.precision.copy()
    precision[1, 2] = -precision[1, 2]
    with pytest.raises(ValueError, match='precision of 1 .* has no Cholesky factor'):
        ops.OnlineCACGMMState.from_model(CACGMM(precision, model.log_determinant, model.weight),
                                         ctx=gpu_ctx)
    ops.OnlineCACGMMState.from_model(model, ctx=gpu_ctx)     # the next call is clean


# ------------------------------------------------------------------ edge inputs
def test_digital_silence(gpu_ctx):
    """Ten frames of zeros in every channel: the state afterwards has the bits of the state before
    and gamma follows the letter (the reference's); one dead channel among live ones matches the
    reference."""
    from pb_chime5_amd import ops
    cell = cr.CELLS[0]
    D, K, beta, prior_mass, F, T = cell
    Y, activity = cr.edge_scene(cell, 'block', cr.seed_of(cell))
    lo = T // 2
    state = ops.OnlineCACGMMState.fresh(F, K, D, prior_mass, ctx=gpu_ctx)
    head = _run(gpu_ctx, Y[:, :lo], activity[:, :lo], beta, state)
    before = state.to_host()
    zeros = _run(gpu_ctx, Y[:, lo:lo + 10], activity[:, lo:lo + 10], beta, state)
    after = state.to_host()
    assert np.all(Y[:, lo:lo + 10] == 0)
    for k in ('s', 'n'):
        assert np.array_equal(after[k], before[k]), k
    tail = _run(gpu_ctx, Y[:, lo + 10:], activity[:, lo + 10:], beta, state)
    gr, st, fr = cr.online_cacgmm(Y, activity, beta, cr.fresh_state(F, K, D, prior_mass))
    gamma = np.concatenate([head, zeros, tail], axis=-1)
    host = state.to_host()
    errs = rel_err(gamma, gr), rel_err(host['s'], st['s']), rel_err(host['n'], st['n'])
    print(f'silence block: {errs}')
    assert fr == 0 and np.all(np.isfinite(gamma)) and max(errs) < cr.TOL, errs
    Y, activity = cr.edge_scene(cell, 'channel', cr.seed_of(cell))
    gr, st, fr = cr.online_cacgmm(Y, activity, beta, cr.fresh_state(F, K, D, prior_mass))
    state = ops.OnlineCACGMMState.fresh(F, K, D, prior_mass, ctx=gpu_ctx)
    gamma, fallbacks = _run(gpu_ctx, Y, activity, beta, state, return_fallbacks=True)
    host = state.to_host()
    errs = rel_err(gamma, gr), rel_err(host['s'], st['s']), rel_err(host['n'], st['n'])
    print(f'dead channel: {errs}')
    assert fallbacks == fr == 0 and max(errs) < cr.TOL, errs


def test_every_class_masked_off_gives_zeros(gpu_ctx):
    cell = cr.CELLS[0]
    D, K, beta, prior_mass, F, T = cell
    Y, activity = cr.edge_scene(cell, 'masked', cr.seed_of(cell))
    gamma = _run(gpu_ctx, Y, activity, beta, prior_mass=prior_mass)
    gr = cr.online_cacgmm(Y, activity, beta, cr.fresh_state(F, K, D, prior_mass))[0]
    assert np.all(gamma[:, :, 5:10] == 0) and np.all(np.isfinite(gamma))
    assert rel_err(gamma, gr) < cr.TOL


@pytest.mark.parametrize('kind', ['first', 'every'])
def test_fallback_classes(gpu_ctx, kind):
    """A state handed in with S_1 = 0 (online_cacgmm_reference.fallback_case says why there are two
    cases): the count equals the reference's, gamma is finite and the reference's."""
    from pb_chime5_amd import ops
    Y, activity, st0, beta, count = cr.fallback_case(kind)
    gr, st, fr = cr.online_cacgmm(Y, activity, beta, st0)
    assert fr == count
    state = ops.OnlineCACGMMState.from_host(st0, ctx=gpu_ctx)
    gamma, got = _run(gpu_ctx, Y, activity, beta, state, return_fallbacks=True)
    assert got == count == gpu_ctx.last_cacgmm_online_fallbacks()
    assert np.all(np.isfinite(gamma))
    host = state.to_host()
    errs = rel_err(gamma, gr), rel_err(host['s'], st['s']), rel_err(host['n'], st['n'])
    print(f'fallback {kind}: {errs}')
    assert max(errs) < cr.TOL, errs
    # a later call without fallbacks reads 0
    cell = cr.CELLS[1]
    Yc, ac = cr.scene(cell)
    _run(gpu_ctx, Yc, ac, cell[2])
    assert gpu_ctx.last_cacgmm_online_fallbacks() == 0


# ------------------------------------------------------------------ errors
def test_errors_before_any_launch(gpu_ctx):
    from pb_chime5_amd import _capi, ops
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    F, T, D, K = 2, 9, 3, 2
    state = ops.OnlineCACGMMState.fresh(F, K, D, 0.5, ctx=gpu_ctx)
    before = state.to_host()
    Y = gpu_ctx.to_device(np.ones((F, T, D), complex))
    mask = gpu_ctx.to_device(np.ones((K, T), np.uint8))
    pattern = np.full((F, K, T), -7.25)
    G = gpu_ctx.to_device(pattern)
    used = gpu_ctx.workspace_bytes()
    S, C, GD = _capi.GssCacgmmOnlineState, _capi.GssEmOnline, _capi.GssGuidance

    def call(Yp=Y.ptr, Gp=G.ptr, st=state.struct(), cfg=True, guide=None, **kw):
        a = {**dict(F=F, T=T, D=D, K=K, forget=0.9, prior_mass=1.0), **kw}
        c = C(forget=a['forget'], prior_mass=a['prior_mass']) if cfg else None
        rc = lib.gss_cacgmm_online(
            h, ctypes.c_void_p(Yp), a['F'], a['T'], a['D'],
            ctypes.byref(guide) if guide is not None else None, a['K'],
            ctypes.byref(c) if c is not None else None,
            ctypes.byref(st) if st is not None else None, ctypes.c_void_p(Gp))
        return rc, lib.gss_last_error(h).decode()
    p = state.bufs
    nan, inf = float('nan'), float('inf')
    cases = [
        (dict(Yp=None), INVALID, 'Y_dev'), (dict(Gp=None), INVALID, 'gamma_dev'),
        (dict(cfg=False), INVALID, 'cfg'),
        (dict(st=S(None, p['n'].ptr, F, K, D)), INVALID, 'state->s'),
        (dict(st=S(p['s'].ptr, None, F, K, D)), INVALID, 'state->n'),
        (dict(st=S(p['s'].ptr, p['n'].ptr, F + 1, K, D)), INVALID, 'state of F'),
        (dict(st=S(p['s'].ptr, p['n'].ptr, F, K + 1, D)), INVALID, 'state of F'),
        (dict(st=S(p['s'].ptr, p['n'].ptr, F, K, D + 1)), INVALID, 'state of F'),
        (dict(F=0), INVALID, 'F'), (dict(T=-1), INVALID, 'T'),
        (dict(D=0), UNSUPPORTED, 'D'), (dict(D=33), UNSUPPORTED, 'D'),
        (dict(K=0), UNSUPPORTED, 'K'), (dict(K=9), UNSUPPORTED, 'K'), (dict(K=19), UNSUPPORTED, 'K'),
        (dict(forget=0.0), INVALID, 'forget'), (dict(forget=1.5), INVALID, 'forget'),
        (dict(forget=nan), INVALID, 'forget'), (dict(forget=inf), INVALID, 'forget'),
        (dict(prior_mass=0.0), INVALID, 'prior_mass'), (dict(prior_mass=-1.0), INVALID, 'prior_mass'),
        (dict(prior_mass=inf), INVALID, 'prior_mass'), (dict(prior_mass=nan), INVALID, 'prior_mass'),
        (dict(guide=GD(None, mask.ptr, 0, 0, 0, T - 1)), INVALID, 'mask_k_stride'),
        (dict(guide=GD(None, mask.ptr, 0, 0, T, T)), INVALID, 'mask_f_stride'),
    ]
    for kw, code, word in cases:
        rc, msg = call(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
    init = lib.gss_cacgmm_online_init
    st = state.struct()
    dev = ops.DeviceModel(gpu_ctx, F, K, D)
    M = _capi.GssCacgmmModel
    for args, code, word in (
            ((F, K, D, 1.0, None, 0.0, None), INVALID, 'state'),
            ((F, K, D, 0.0, None, 1.0, ctypes.byref(st)), INVALID, 'prior_mass'),
            ((F, K, D, nan, None, 1.0, ctypes.byref(st)), INVALID, 'prior_mass'),
            ((F, K, D, 1.0, ctypes.byref(dev.struct), 0.0, ctypes.byref(st)), INVALID, 'model_mass'),
            ((F, K, D, 1.0, ctypes.byref(dev.struct), inf, ctypes.byref(st)), INVALID, 'model_mass'),
            ((F, K, D, 1.0, ctypes.byref(M(None, dev.log_det_d.ptr, dev.weight_d.ptr)), 1.0,
              ctypes.byref(st)), INVALID, 'precision_dev'),
            ((F, K, D, 1.0, ctypes.byref(M(dev.precision_d.ptr, dev.log_det_d.ptr, None)), 1.0,
              ctypes.byref(st)), INVALID, 'weight_dev'),
            ((F + 1, K, D, 1.0, None, 1.0, ctypes.byref(st)), INVALID, 'state of F'),
            ((0, K, D, 1.0, None, 1.0, ctypes.byref(st)), INVALID, 'F'),
            ((F, 9, D, 1.0, None, 1.0, ctypes.byref(st)), UNSUPPORTED, 'K'),
            ((F, K, 33, 1.0, None, 1.0, ctypes.byref(st)), UNSUPPORTED, 'D')):
        rc = init(h, *args)
        assert rc == code and word in lib.gss_last_error(h).decode(), (args, rc)
    to_model = lib.gss_cacgmm_online_model
    for args, code, word in (
            ((None, ctypes.byref(dev.struct)), INVALID, 'state'),
            ((ctypes.byref(st), None), INVALID, 'model_out'),
            ((ctypes.byref(S(None, p['n'].ptr, F, K, D)), ctypes.byref(dev.struct)), INVALID, 'state->s'),
            ((ctypes.byref(st), ctypes.byref(M(dev.precision_d.ptr, None, dev.weight_d.ptr))), INVALID,
             'log_det_dev'),
            ((ctypes.byref(st), ctypes.byref(M(p['s'].ptr, dev.log_det_d.ptr, dev.weight_d.ptr))),
             INVALID, 'shares a buffer'),
            ((ctypes.byref(S(p['s'].ptr, p['n'].ptr, F, 9, D)), ctypes.byref(dev.struct)), UNSUPPORTED, 'K')):
        rc = to_model(h, *args)
        assert rc == code and word in lib.gss_last_error(h).decode(), (args, rc)
    assert lib.gss_last_cacgmm_online_fallbacks(h, None) == INVALID
    # nothing ran: no workspace was taken, the state and the output have their bits; T = 0 is a no-op
    assert call(T=0)[0] == 0
    assert gpu_ctx.workspace_bytes() == used
    after = state.to_host()
    for k in ('s', 'n'):
        assert np.array_equal(after[k], before[k]), k
    assert np.array_equal(gpu_ctx.to_host(G, (F, K, T), np.float64), pattern)
    # the fused entry
    u = cr.pipe_scene()
    params = ops.make_params(wpe_taps=2, bss_iterations=1)
    _, utt, _, _ = ops._resident_call(u.obs, u.activity_array, params, None, None, False, gpu_ctx)
    B = _capi.GssBfOnline
    good_bf = dict(forget=0.9, loading=1.0, ref_channel=-1, wpe_online=0, wpe_alpha=0.99)
    for em, bf, word in ((dict(forget=0.0), None, 'forget'), (dict(prior_mass=0.0), None, 'prior_mass'),
                         ({}, dict(loading=0.0), 'loading'), ({}, dict(ref_channel=4), 'ref_channel'),
                         ({}, dict(wpe_online=1, wpe_alpha=0.0), 'alpha')):
        cfg = C(**{**dict(forget=0.9, prior_mass=1.0), **em})
        with pytest.raises(ValueError, match=word):
            utt.enqueue(u.target_index, 0, 0,
                        gss_online=(cfg, B(**{**good_bf, **bf}) if bf is not None else None))
    pbad = ops.make_params(wpe_taps=2, bss_iterations=1, bf='gev_ban')
    _, utt, _, _ = ops._resident_call(u.obs, u.activity_array, pbad, None, None, False, gpu_ctx)
    with pytest.raises(NotImplementedError, match='online'):
        utt.enqueue(u.target_index, 0, 0, gss_online=(C(forget=0.9, prior_mass=1.0), B(**good_bf)))


def test_online_cacgmm_object(gpu_ctx):
    """`online_cacgmm.OnlineCACGMM`: blocks and single frames through the object's own state give
    the bits of the single call; reset() starts over; a stream built from a model needs no mask."""
    from pb_chime5_amd.online_cacgmm import OnlineCACGMM
    cell = cr.CELLS[3]
    D, K, beta, prior_mass, F, T = cell
    Y, activity = cr.scene(cell, cr.seed_of(cell))
    gamma1, host1, _ = _device(gpu_ctx, cell)
    want = cr.to_ktf(gamma1)
    block = np.ascontiguousarray(Y.transpose(1, 0, 2))          # (T,F,D)
    em = OnlineCACGMM(beta, prior_mass, num_classes=K, channel=D, frequency_bins=F, ctx=gpu_ctx)
    out = [em.step_frames(block[:40], activity[:, :40])]
    out += [em.step_frame(block[t], activity[:, t])[:, None] for t in range(40, 45)]
    out.append(em.step_frames(block[45:], activity[:, 45:]))
    assert np.array_equal(np.concatenate(out, axis=1), want)
    assert np.array_equal(em.state.to_host()['s'], host1['s']) and em.fallbacks == 0
    em.reset()
    assert np.array_equal(em.step_frames(block, activity), want)
    model = _fitted_model()
    D, K, beta, prior_mass, F, T = cr.MODEL_CELL
    Y, _ = cr.scene(cr.MODEL_CELL)
    em = OnlineCACGMM(beta, cr.MODEL_MASS, model=model, ctx=gpu_ctx)
    assert (em.frequency_bins, em.num_classes, em.channel) == (F, K, D)
    gamma = em.step_frames(np.ascontiguousarray(Y[:, T // 2:].transpose(1, 0, 2)))
    assert gamma.shape == (K, T - T // 2, F) and np.max(gamma) > 0.9


# ------------------------------------------------------------------ evidence
def test_the_continued_model_follows_a_moving_speaker(gpu_ctx):
    """The device on the evidence scene: guided for 200 stationary frames, then no mask while
    speaker 0 moves.  The state that keeps learning classifies the frames from 400 on with less
    than EVIDENCE_BOUND x the error of the SAME state frozen at frame 200 (to_model +
    cacgmm_predict)."""
    from pb_chime5_amd import ops
    e = cr.EVIDENCE
    Y, activity = cr.evidence_scene()
    g = e['guided']
    state = ops.OnlineCACGMMState.fresh(e['F'], e['K'], e['D'], e['prior_mass'], ctx=gpu_ctx)
    _run(gpu_ctx, Y[:, :g], activity[:, :g], e['beta'], state)
    frozen = ops.cacgmm_predict(state.to_model(), cr.to_dtf(Y[:, g:]), ctx=gpu_ctx).transpose(2, 0, 1)
    moving = _run(gpu_ctx, Y[:, g:], None, e['beta'], state)
    ratio = cr.evidence_error(moving, activity) / cr.evidence_error(frozen, activity)
    print(f'evidence: continued / frozen error {ratio:.3f} (reference {cr.evidence_ratio():.3f})')
    assert ratio < cr.EVIDENCE_BOUND


# ------------------------------------------------------------------ pipeline
@functools.lru_cache(maxsize=None)
def _pipe_enhancer(gss_online, bf_online, wpe_online):
    from pb_chime5_amd.core import get_enhancer
    p = cr.PIPE
    kw = dict(wpe_tabs=p['wpe_taps'], wpe_delay=p['wpe_delay'], bss_iterations=3,
              stft_size=p['stft_size'], stft_shift=p['stft_shift'])
    if gss_online:
        kw.update(gss_online=True, gss_forget=p['forget'], gss_prior_mass=p['prior_mass'])
    if wpe_online:
        kw.update(wpe_online=True, wpe_alpha=p['wpe_alpha'])
    if bf_online:
        kw.update(bf_online=True, bf_forget=p['bf_forget'], bf_loading=p['bf_loading'])
    return get_enhancer(**kw)


@pytest.mark.parametrize('bf_online,wpe_online', [(False, False), (True, False), (True, True)],
                         ids=['alone', 'bf_online', 'bf_online+wpe_online'])
def test_pipeline(gpu_ctx, bf_online, wpe_online):
    """The fused call's posteriors have the bits of ops.cacgmm_posteriors_online on the call's own
    Obs and frame activity, and its masks and X_hat the bits of the existing mask and beamformer
    ops on them (the stage path); |x_hat| is within the end-to-end bar of the oracle's stages
    composed with the NumPy references."""
    from pb_chime5_amd import ops
    p = cr.PIPE
    u = cr.pipe_scene()
    enh = _pipe_enhancer(True, bf_online, wpe_online)
    assert enh._fusable() and enh._gss_online() == dict(forget=p['forget'], prior_mass=p['prior_mass'])
    got = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, debug=True)
    loc = enh.enhance_observation_locals
    det = loc['details']
    assert det['gss_online_fallbacks'] == 0
    stage = ops.cacgmm_posteriors_online(det['Obs'], np.asarray(det['acitivity_freq']) != 0,
                                         forget=p['forget'], prior_mass=p['prior_mass'], ctx=gpu_ctx)
    assert np.array_equal(det['posterior'], stage)
    target = tuple(u.activity.keys()).index(u.speaker_id)
    masks = loc['masks']
    tm = np.asarray(det['target_mask']).reshape(masks.shape[1:])
    dm = np.asarray(det['distortion_mask']).reshape(tm.shape)
    assert np.array_equal(tm, masks[target])
    assert rel_err(dm, np.sum(np.delete(masks, target, axis=0), axis=0)) < 1e-14
    ref = int(np.ravel(det['ref_channel'])[0])
    if bf_online:
        X = ops.mvdr_souden_online_from_masks(det['Obs'], tm, dm, True, forget=p['bf_forget'],
                                              loading=p['bf_loading'], ref_channel=ref, ctx=gpu_ctx)
    else:
        X = ops.mvdr_souden_from_masks(det['Obs'], tm, dm, ban=True, ctx=gpu_ctx)
    assert np.array_equal(np.asarray(det['X_hat']).reshape(tm.shape), X)
    assert np.all(np.isfinite(got))
    blocks = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, fused=False)
    print(f'bf_online={bf_online} wpe_online={wpe_online}: stage path vs fused '
          f'{rel_err(blocks, got):.1e}')
    assert rel_err(blocks, got) < 1e-10
    want = cr.pipe_reference(bf_online, wpe_online)
    err = cr.abs_rel_err(got, want)
    print(f'bf_online={bf_online} wpe_online={wpe_online}: |x_hat| vs oracle chain {err:.1e}')
    assert err < cr.X_TOL, err
    # it is another signal than the iterated mixture model gives
    plain = _pipe_enhancer(False, bf_online, wpe_online)
    assert rel_err(plain.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex), got) > 1e-4


def test_gss_online_false_leaves_the_default_bits(gpu_ctx):
    from pb_chime5_amd.core import get_enhancer
    p = cr.PIPE
    u = cr.pipe_scene()
    kw = dict(wpe_tabs=p['wpe_taps'], wpe_delay=p['wpe_delay'], bss_iterations=3)
    a = get_enhancer(**kw).enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex)
    b = get_enhancer(gss_online=False, **kw).enhance_observation(u.obs, u.activity, u.speaker_id,
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


@pytest.mark.parametrize('cell', cr.CHUNK_CELLS, ids=str)
def test_workspace_hygiene_of_the_stage(hctx, cell):
    """From a state the library initialises in a poisoned block and hands back, from a throw-away
    state in the arena, and through both conversions of the model."""
    from pb_chime5_amd import ops
    D, K, beta, prior_mass, F, T = cell
    Y, activity = cr.scene(cell, cr.seed_of(cell))

    def call(ctx):
        out = {}
        state = ops.OnlineCACGMMState.fresh(F, K, D, prior_mass, ctx=ctx)
        out['gamma'] = _run(ctx, Y, activity, beta, state)
        out.update({f'state {k}': v for k, v in state.to_host().items()})
        out['gamma thrown away'] = _run(ctx, Y, activity, beta, prior_mass=prior_mass)
        model = state.to_model()
        out.update(precision=model.precision, log_det=model.log_determinant, weight=model.weight)
        out.update({f'back {k}': v for k, v in
                    ops.OnlineCACGMMState.from_model(model, mass=3.0, ctx=ctx).to_host().items()})
        return out
    got = hygiene(hctx, call, f'online cacgmm {cell}')
    gr, st, _ = cr.reference(cell, cr.seed_of(cell))
    errs = dict(gamma=rel_err(got['gamma'], gr), s=rel_err(got['state s'], st['s']),
                n=rel_err(got['state n'], st['n']))
    assert max(errs.values()) < cr.TOL, errs
    assert np.array_equal(got['gamma thrown away'], got['gamma'])


@pytest.mark.parametrize('bf_online,wpe_online', [(False, False), (True, True)],
                         ids=['alone', 'bf_online+wpe_online'])
def test_workspace_hygiene_of_the_fused_entry(hctx, bf_online, wpe_online):
    from pb_chime5_amd import ops
    p = cr.PIPE
    u = cr.pipe_scene()

    def call(ctx):
        x_hat, det = ops.enhance_observation_gss_online(
            u.obs, u.activity_array, u.target_index, 2048, 2048, forget=p['forget'],
            prior_mass=p['prior_mass'], bf_online=bf_online, bf_forget=p['bf_forget'],
            bf_loading=p['bf_loading'], wpe_online=wpe_online,
            wpe_alpha=p['wpe_alpha'] if wpe_online else ops.WPE_ONLINE_ALPHA, debug=True, ctx=ctx,
            wpe_taps=p['wpe_taps'], wpe_delay=p['wpe_delay'], stft_size=p['stft_size'],
            stft_shift=p['stft_shift'])
        return dict(x_hat=x_hat, X_hat=det['X_hat'], posterior=det['posterior'],
                    fallbacks=det['gss_online_fallbacks'])
    got = hygiene(hctx, call, f'fused online cacgmm, bf_online={bf_online}, wpe_online={wpe_online}')
    assert cr.abs_rel_err(got['x_hat'], cr.pipe_reference(bf_online, wpe_online)) < cr.X_TOL
