"""Permutation alignment on the GPU (gss_cacgmm_align, gss_cacgmm_model_permute,
gss_last_align_moved; ops.align_posteriors / cacgmm_model_permute / cacgmm_fit_blind,
method='aligned' of the annotation-free front doors).

The reference for every number is tests/align_reference.py.  The mapping is asked to EQUAL the
reference's on the same input bits: every parity scene has a margin (best minus second-best
total, over all passes and frequencies) of at least 1e-9, four orders above what two float64
summation orders of unit-norm rows differ by (seed 0 passed in all eleven cells, margins
2.5e-6 ... 1.6).  The activity is held to 1e-10, the bar of the project's other fixed-order
float64 reductions; predict under a gathered model to the 1e-7 of tests/test_gpu_cacgmm_model.py."""
import ctypes
import functools

import numpy as np
import pytest

import align_reference as ar
import shared_prior_reference as spr

pytestmark = pytest.mark.gpu

c_void_p = ctypes.c_void_p


def _ptr(buf):
    return c_void_p(buf.ptr if buf is not None else None)


def _align_status(ctx, g_d, F, K, T, plan, m_d, a_d, act_d):
    """gss_cacgmm_align as the C ABI has it -> status; `plan` a ops.DeviceAlignPlan or None."""
    return ctx.lib.gss_cacgmm_align(ctx.handle, _ptr(g_d), F, K, T,
                                    ctypes.byref(plan.struct) if plan is not None else None,
                                    _ptr(m_d), _ptr(a_d), _ptr(act_d))


def _align(ctx, gamma, plan, aligned=True, activity=True):
    """gamma (F,K,T) -> dict(mapping (F,K) int32, aligned (F,K,T), activity (K,T), moved)."""
    from pb_chime5_amd import ops
    F, K, T = gamma.shape
    g_d = ctx.to_device(np.ascontiguousarray(gamma, dtype=np.float64))
    m_d = ctx.empty(4 * F * K)
    a_d = ctx.empty(8 * F * K * T) if aligned else None
    act_d = ctx.empty(8 * K * T) if activity else None
    dplan = ops.DeviceAlignPlan(ops.check_alignment_plan(plan, F))
    ctx._check(_align_status(ctx, g_d, F, K, T, dplan, m_d, a_d, act_d), 'gss_cacgmm_align')
    out = dict(mapping=ctx.to_host(m_d, (F, K), np.int32), moved=ctx.last_align_moved())
    if aligned:
        out['aligned'] = ctx.to_host(a_d, (F, K, T), np.float64)
    if activity:
        out['activity'] = ctx.to_host(act_d, (K, T), np.float64)
    return out


# ------------------------------------------------------------------ parity with the reference
@pytest.mark.parametrize('plan_index', (0, 1), ids=('whole', 'widening'))
@pytest.mark.parametrize('cell', ar.CELLS, ids=lambda c: '-'.join(map(str, c)))
def test_mapping_equals_the_reference(gpu_ctx, cell, plan_index):
    D, T, F, K = cell
    seed = ar.seed_of(cell)
    gamma = ar.parity_input(cell, seed)
    plan = ar.plans(F)[plan_index]
    want, margin, passes = ar.parity_reference(cell, seed, plan_index)
    assert ar.cell_margin(cell, seed) >= ar.MIN_MARGIN
    got = _align(gpu_ctx, gamma, plan)
    want_aligned = ar.gather(gamma, want)
    err = float(np.max(np.abs(got['activity'] - ar.activity(want_aligned))))
    print(f'align {cell} plan {plan_index}: margin {margin:.1e}, {passes} passes, '
          f'{ar.moved(want)} of {F} rows moved (GPU {got["moved"]}), '
          f'{int(np.sum(np.any(got["mapping"] != want, axis=1)))} rows differ, activity {err:.2e}')
    assert ar.is_permutation_rows(got['mapping'])
    np.testing.assert_array_equal(got['mapping'], want)
    np.testing.assert_array_equal(got['aligned'], want_aligned)
    assert err < ar.ACTIVITY_TOL
    assert got['moved'] == ar.moved(want)
    # the same call gives the same bits; the outputs a caller does not take change nothing
    again = _align(gpu_ctx, gamma, plan)
    for name in ('mapping', 'aligned', 'activity'):
        assert got[name].tobytes() == again[name].tobytes(), name
    only_activity = _align(gpu_ctx, gamma, plan, aligned=False)
    assert only_activity['activity'].tobytes() == got['activity'].tobytes()
    neither = _align(gpu_ctx, gamma, plan, aligned=False, activity=False)
    np.testing.assert_array_equal(neither['mapping'], want)


def test_rows_outside_the_plan_stay_the_identity(gpu_ctx):
    cell = (7, 200, 33, 4)
    gamma = ar.parity_input(cell, ar.seed_of(cell))
    F, K, T = gamma.shape
    plan = [(3, 5, 20), (2, 9, 28)]
    want, margin, _ = ar.align(gamma, plan)
    assert margin >= ar.MIN_MARGIN
    got = _align(gpu_ctx, gamma, plan)
    np.testing.assert_array_equal(got['mapping'], want)
    outside = [f for f in range(F) if not 5 <= f < 28]
    np.testing.assert_array_equal(got['mapping'][outside], np.tile(np.arange(K), (len(outside), 1)))
    assert 0 < got['moved'] == ar.moved(want)
    np.testing.assert_array_equal(got['aligned'], ar.gather(gamma, want))


def test_operator_layouts(gpu_ctx):
    """ops.align_posteriors: (K,T,F) in and out, the default plan, the optional results."""
    from pb_chime5_amd import ops
    cell = (6, 135, 16, 5)
    gamma = ar.parity_input(cell, ar.seed_of(cell))
    F = gamma.shape[0]
    posterior = np.ascontiguousarray(gamma.transpose(1, 2, 0))
    want, mapping, activity, margin = ar.align_ktf(posterior, ops.alignment_plan(F))
    assert margin >= ar.MIN_MARGIN
    got, got_mapping, got_activity = ops.align_posteriors(posterior, return_mapping=True,
                                                          return_activity=True, ctx=gpu_ctx)
    np.testing.assert_array_equal(got_mapping, mapping)
    np.testing.assert_array_equal(got, want)
    assert float(np.max(np.abs(got_activity - activity))) < ar.ACTIVITY_TOL
    np.testing.assert_array_equal(ops.align_posteriors(posterior, ctx=gpu_ctx), want)


# ------------------------------------------------------------------ the model
def _random_model(F, K, D, seed):
    from pb_chime5_amd.cacgmm import CACGMM
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((F, K, D, D)) + 1j * rng.standard_normal((F, K, D, D))
    return CACGMM(A @ A.conj().swapaxes(-1, -2), rng.standard_normal((F, K)),
                  rng.uniform(size=(F, K)))


@pytest.mark.parametrize('shape', [(5, 3, 4), (2, 19, 32), (70, 8, 17), (1, 1, 2)],
                         ids=lambda s: '-'.join(map(str, s)))
def test_model_gather_gives_the_bits_of_the_host_gather(gpu_ctx, shape):
    from pb_chime5_amd import ops
    F, K, D = shape
    model = _random_model(F, K, D, 5)
    rng = np.random.default_rng(6)
    mapping = np.stack([rng.permutation(K) for _ in range(F)]).astype(np.int32)
    want = model.permuted(mapping)
    got = ops.cacgmm_model_permute(model, mapping, ctx=gpu_ctx)
    for name in ('precision', 'log_determinant', 'weight'):
        assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), name


def test_model_gather_writes_nan_for_an_entry_out_of_range(gpu_ctx):
    """The C ABI does not ask for a permutation: an entry outside [0, K) gives NaN for that class
    and reads nothing; the other classes are gathered."""
    from pb_chime5_amd import ops
    ctx = gpu_ctx
    F, K, D = 3, 4, 5
    model = _random_model(F, K, D, 7)
    mapping = np.tile(np.arange(K, dtype=np.int32), (F, 1))[:, ::-1].copy()
    mapping[1, 2], mapping[2, 0] = K, -1
    src, dst = ops.DeviceModel(ctx, F, K, D, model), ops.DeviceModel(ctx, F, K, D)
    m_d = ctx.to_device(mapping)
    ctx._check(ctx.lib.gss_cacgmm_model_permute(ctx.handle, ctypes.byref(src.struct), F, K, D,
                                                _ptr(m_d), ctypes.byref(dst.struct)), 'permute')
    got = dst.to_host(ctx)
    for f in range(F):
        for k in range(K):
            j = mapping[f, k]
            if 0 <= j < K:
                assert got.precision[f, k].tobytes() == model.precision[f, j].tobytes()
                assert got.weight[f, k] == model.weight[f, j]
            else:
                assert np.all(np.isnan(got.precision[f, k].real))
                assert np.all(np.isnan(got.precision[f, k].imag))
                assert np.isnan(got.log_determinant[f, k]) and np.isnan(got.weight[f, k])


def test_predict_under_the_gathered_model(gpu_ctx):
    from pb_chime5_amd import ops
    D, T, F, K = cell = (6, 135, 16, 5)
    Y, _ = spr.parity_scene(D, T, F, K, ar.seed_of(cell))
    start = np.random.default_rng([0, 7]).uniform(0.01, 1.0, size=(K, T, F))
    model = ops.cacgmm_fit(Y, start / start.sum(axis=0, keepdims=True), None, 5, ctx=gpu_ctx)
    posterior = ops.cacgmm_predict(model, Y, ctx=gpu_ctx)
    _, mapping = ops.align_posteriors(posterior, [(4, 0, F)], return_mapping=True, ctx=gpu_ctx)
    assert ar.moved(mapping) > 0
    got = ops.cacgmm_predict(ops.cacgmm_model_permute(model, mapping, ctx=gpu_ctx), Y, ctx=gpu_ctx)
    want = ar.gather(posterior.transpose(2, 0, 1), mapping).transpose(1, 2, 0)
    err = float(np.max(np.abs(got - want)))
    print(f'predict(permuted model) vs permuted predict(model): {err:.2e}')
    assert err < ar.POSTERIOR_TOL


# ------------------------------------------------------------------ what the method is for
@functools.lru_cache(maxsize=None)
def _table_posteriors(seed, D, start):
    from pb_chime5_amd import ops
    Obs, truth, starts = ar.table_starts(seed, D)
    return truth, ops.cacgmm_posteriors_guided(Obs, starts[start], None, spr.TABLE_ITERATIONS, 1)


@pytest.mark.parametrize('start', ('random', 'blind'))
@pytest.mark.parametrize('run', ar.TABLE_RUNS, ids=lambda r: f's{r[0]}-D{r[1]}')
def test_alignment_makes_the_bins_consistent(gpu_ctx, run, start):
    """The table scenes (F = 129, T = 1003, K = 3, 20 EM iterations), the GPU's own per-frequency
    posteriors: at most 0.6 of the bins consistent before the alignment, at least 0.95 after it,
    and the GPU's mapping is the reference aligner's on the same posteriors."""
    from pb_chime5_amd import ops
    truth, posterior = _table_posteriors(*run, start)
    K, T, F = posterior.shape
    before, _, _ = spr.bins_consistent(posterior, np.mean(posterior, axis=-1), truth)
    aligned, mapping, activity = ops.align_posteriors(posterior, return_mapping=True,
                                                      return_activity=True, ctx=gpu_ctx)
    after, gap, corr = spr.bins_consistent(aligned, activity, truth)
    _, want, _, margin = ar.align_ktf(posterior, ops.alignment_plan(F))
    print(f'table run {run} {start} start: bins consistent {before:.3f} -> {after:.3f}, '
          f'corr {corr[0]:.2f} {corr[1]:.2f}, margin {margin:.1e}, '
          f'{gpu_ctx.last_align_moved()} rows moved')
    assert before <= 0.6
    assert after >= 0.95
    np.testing.assert_array_equal(mapping, want)


def test_fit_blind_gives_a_model_that_keeps_the_speakers(gpu_ctx):
    """ops.cacgmm_fit_blind on the first 500 frames of the table scene (s = 0, D = 4): predict on
    the fitted frames is the aligned posteriors, and on the other 503 frames each speaker stays in
    the class it has on the fitted stretch (the class whose row mean over f correlates best with
    the speaker's true activity)."""
    from pb_chime5_amd import ops
    Obs, truth = spr.table_scene(0, 4)
    split = 500
    fitted, rest = Obs[:, :split], Obs[:, split:]
    model, aligned = ops.cacgmm_fit_blind(fitted, spr.TABLE_K, spr.TABLE_ITERATIONS, seed=0,
                                          return_posterior=True, ctx=gpu_ctx)
    again = model.predict(fitted, ctx=gpu_ctx)
    err = float(np.max(np.abs(again - aligned)))
    new = model.predict(rest, ctx=gpu_ctx)
    winners = []
    for s in range(truth.shape[0]):
        c_fit = spr._corr_rows(np.mean(aligned, axis=-1), truth[s, :split].astype(np.float64))
        c_new = spr._corr_rows(np.mean(new, axis=-1), truth[s, split:].astype(np.float64))
        winners.append((int(np.argmax(c_fit)), int(np.argmax(c_new))))
        print(f'fit_blind speaker {s}: corr on the fitted stretch {np.round(c_fit, 3)}, on the '
              f'other {np.round(c_new, 3)}')
    print(f'fit_blind: predict(model) vs aligned posteriors {err:.2e}')
    assert err < ar.POSTERIOR_TOL
    assert all(a == b for a, b in winners), winners
    assert winners[0][0] != winners[1][0]


# ------------------------------------------------------------------ the front doors
def test_front_door_aligned_is_the_composition_of_the_stages(gpu_ctx):
    from pb_chime5_amd import core, ops
    from pb_chime5_amd.speech_enhancement.beamforming_wrapper import (
        beamform_mvdr_souden_from_masks)
    b = spr.BLIND
    u = spr.blind_scene()
    K = b['num_speakers'] + 1
    enh = core.get_enhancer(wpe_tabs=b['wpe_taps'], wpe_delay=b['wpe_delay'],
                            wpe_iterations=b['wpe_iterations'], bss_iterations=b['iterations'],
                            stft_size=b['stft_size'], stft_shift=b['stft_shift'])
    out = enh.enhance_observation_blind(u.obs, b['num_speakers'], ex=u.ex, method='aligned')
    size, shift = b['stft_size'], b['stft_shift']
    Obs = ops.stft(u.obs, size=size, shift=shift, fading=True, ctx=gpu_ctx)
    Obs = ops.wpe_dtf(Obs, taps=b['wpe_taps'], delay=b['wpe_delay'],
                      iterations=b['wpe_iterations'], psd_context=0, ctx=gpu_ctx)
    init = ops.blind_initialization(K, Obs.shape[1], 0)
    posterior = ops.cacgmm_posteriors_guided(Obs, init, None, b['iterations'], 1, ctx=gpu_ctx)
    masks, activity = ops.align_posteriors(posterior, return_activity=True, ctx=gpu_ctx)
    sf, ef = core.start_end_context_frames(u.ex, stft_size=size, stft_shift=shift,
                                           stft_fading=True)
    masks = masks.copy()
    masks[:, :sf, :] = 0
    if ef > 0:
        masks[:, -ef:, :] = 0
    want = np.stack([ops.istft(beamform_mvdr_souden_from_masks(
        Y=Obs, X_mask=masks[k], N_mask=np.sum(np.delete(masks, k, axis=0), axis=0), ban=True),
        size=size, shift=shift, fading=True, ctx=gpu_ctx) for k in range(K)])
    err = float(np.max(np.abs(out.x_hat - want)))
    perr = float(np.max(np.abs(out.prior - activity)))
    print(f'enhance_observation_blind(method=aligned) vs the stages: x_hat {err:.2e}, '
          f'prior {perr:.2e}')
    assert out.x_hat.shape == want.shape and out.prior.shape == (K, Obs.shape[1])
    assert err <= 1e-12 and perr <= 1e-12
    # the default is the shared prior, bit for bit what it was
    default = enh.enhance_observation_blind(u.obs, b['num_speakers'], ex=u.ex)
    named = enh.enhance_observation_blind(u.obs, b['num_speakers'], ex=u.ex, method='shared_prior')
    assert default.x_hat.tobytes() == named.x_hat.tobytes()
    assert default.prior.tobytes() == named.prior.tobytes()
    posterior, prior = ops.cacgmm_posteriors_blind(Obs, K, b['iterations'], seed=0,
                                                   return_prior=True, ctx=gpu_ctx)
    assert prior.tobytes() == default.prior.tobytes()
    want, want_prior = ops.cacgmm_posteriors_shared_prior(Obs, init, None, b['iterations'], 1,
                                                          return_prior=True, ctx=gpu_ctx)
    assert posterior.tobytes() == want.tobytes() and prior.tobytes() == want_prior.tobytes()
    # the operator's aligned method is the two operators
    got, got_activity = ops.cacgmm_posteriors_blind(Obs, K, b['iterations'], seed=0,
                                                    return_prior=True, method='aligned',
                                                    ctx=gpu_ctx)
    full = ops.align_posteriors(ops.cacgmm_posteriors_guided(Obs, init, None, b['iterations'], 1,
                                                             ctx=gpu_ctx), ctx=gpu_ctx)
    assert got.tobytes() == full.tobytes() and got_activity.tobytes() == activity.tobytes()


# ------------------------------------------------------------------ hygiene
@pytest.fixture
def fresh_ctx():
    from pb_chime5_amd import _capi
    ctx = _capi.Context(0)
    yield ctx
    ctx.close()


def test_poisoned_workspace_changes_nothing(fresh_ctx):
    """One parity cell and the model gather under gss_debug_workspace(ctx, 0xFF): no guard is
    touched and the results are those of the plain run."""
    from pb_chime5_amd import ops
    ctx = fresh_ctx
    cell = (7, 200, 33, 4)
    gamma = ar.parity_input(cell, ar.seed_of(cell))
    plan = ar.plans(cell[2])[1]
    model = _random_model(9, 5, 6, 8)
    mapping = np.stack([np.random.default_rng(f).permutation(5) for f in range(9)]).astype(np.int32)
    plain = _align(ctx, gamma, plan)
    plain_only = _align(ctx, gamma, plan, aligned=False)
    plain_model = ops.cacgmm_model_permute(model, mapping, ctx=ctx)
    ctx.debug_workspace(0xFF)
    try:
        got = _align(ctx, gamma, plan)
        got_only = _align(ctx, gamma, plan, aligned=False)
        got_model = ops.cacgmm_model_permute(model, mapping, ctx=ctx)
        count, text, _ = ctx.debug_workspace_report()
    finally:
        ctx.debug_workspace(None)
    assert count == 0, text
    for name in ('mapping', 'aligned', 'activity'):
        assert got[name].tobytes() == plain[name].tobytes(), name
    assert got['moved'] == plain['moved']
    assert got_only['activity'].tobytes() == plain_only['activity'].tobytes()
    assert got_model.precision.tobytes() == plain_model.precision.tobytes()
    np.testing.assert_array_equal(got['mapping'], ar.parity_reference(cell, ar.seed_of(cell), 1)[0])


@pytest.mark.parametrize('T', (100, 1163, 2172))
def test_fresh_context_reserves_enough(T):
    """F = 513 on a context that has never grown its workspace: the reserve's own term must
    cover the call (a NOMEM here is a sizing formula that is too small), with and without an
    aligned table of the caller's."""
    from pb_chime5_amd import _capi, ops
    F, K = 513, 5
    rng = np.random.default_rng(T)
    gamma = rng.uniform(0.01, 1.0, size=(F, K, T))
    plan = ops.alignment_plan(F, main_iterations=2, sub_iterations=1)
    for aligned in (False, True):
        ctx = _capi.Context(0)
        try:
            assert ctx.workspace_bytes() == 0
            out = _align(ctx, gamma, plan, aligned=aligned)
            assert ar.is_permutation_rows(out['mapping'])
            assert ctx.workspace_bytes() > 0
        finally:
            ctx.close()


# ------------------------------------------------------------------ errors
def test_align_errors_come_back_before_any_launch(gpu_ctx):
    from pb_chime5_amd import _capi, ops
    ctx = gpu_ctx
    cell = (4, 70, 5, 2)
    gamma = ar.parity_input(cell, ar.seed_of(cell))
    F, K, T = gamma.shape
    g_d = ctx.to_device(gamma)
    m_d, a_d, act_d = ctx.empty(4 * F * 9), ctx.empty(8 * F * K * T), ctx.empty(8 * K * T)
    sentinel = np.full((F, K), -7, np.int32)

    def plan_of(rows, **kw):
        p = ops.DeviceAlignPlan(rows)
        for name, value in kw.items():
            setattr(p.struct, name, value)
        return p
    good = plan_of([(2, 0, F)])

    def call(g=g_d, F_=F, K_=K, T_=T, plan=good, m=m_d, a=a_d, act=act_d):
        return _align_status(ctx, g, F_, K_, T_, plan, m, a, act)
    cases = [
        (dict(g=None), 'gamma_dev is NULL'), (dict(m=None), 'mapping_dev is NULL'),
        (dict(plan=None), 'plan is NULL'),
        (dict(plan=plan_of([(2, 0, F)], iterations=None)), 'an array'),
        (dict(plan=plan_of([(2, 0, F)], start=None)), 'an array'),
        (dict(plan=plan_of([(2, 0, F)], end=None)), 'an array'),
        (dict(plan=plan_of([(2, 0, F)], entries=0)), 'entries=0'),
        (dict(plan=plan_of([(2, 0, F), (0, 0, F)])), 'entry 1: iterations=0'),
        (dict(plan=plan_of([(2, -1, F)])), 'entry 0: not 0 <= start=-1'),
        (dict(plan=plan_of([(2, 3, 3)])), 'entry 0: not 0 <= start=3 < end=3'),
        (dict(plan=plan_of([(2, 0, F + 1)])), f'end={F + 1} <= F={F}'),
        (dict(F_=0), 'F=0'), (dict(T_=0), 'T=0'), (dict(K_=0), 'K=0'),
        (dict(a=g_d), 'aligned_dev is gamma_dev'),
    ]
    for kw, match in cases:
        ctx.upload(m_d, sentinel)
        status = call(**kw)
        assert status == _capi.GSS_ERR_INVALID, match
        with pytest.raises(ValueError, match=match):
            ctx._check(status, 'gss_cacgmm_align')
        if kw.get('m', m_d) is not None:
            np.testing.assert_array_equal(ctx.to_host(m_d, (F, K), np.int32), sentinel)
    ctx.upload(m_d, sentinel)
    status = call(K_=9)
    assert status == _capi.GSS_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError, match='K=9 is larger than 8'):
        ctx._check(status, 'gss_cacgmm_align')
    np.testing.assert_array_equal(ctx.to_host(m_d, (F, K), np.int32), sentinel)
    # and the good call still works
    ctx._check(call(), 'gss_cacgmm_align')
    np.testing.assert_array_equal(ctx.to_host(m_d, (F, K), np.int32), ar.align(gamma, [(2, 0, F)])[0])
    with pytest.raises(ValueError, match='gss_last_align_moved: NULL'):
        ctx._check(ctx.lib.gss_last_align_moved(ctx.handle, None), 'moved')


def test_model_permute_errors(gpu_ctx):
    from pb_chime5_amd import _capi, ops
    ctx = gpu_ctx
    F, K, D = 3, 4, 5
    model = _random_model(F, K, D, 9)
    src, dst = ops.DeviceModel(ctx, F, K, D, model), ops.DeviceModel(ctx, F, K, D)
    m_d = ctx.to_device(np.tile(np.arange(K, dtype=np.int32), (F, 1)))

    def struct(base, **kw):
        fields = dict(precision_dev=base.precision_d.ptr, log_det_dev=base.log_det_d.ptr,
                      weight_dev=base.weight_d.ptr)
        return _capi.GssCacgmmModel(**{**fields, **kw})

    def call(a=struct(src), b=struct(dst), F_=F, K_=K, D_=D, m=m_d):
        return ctx.lib.gss_cacgmm_model_permute(
            ctx.handle, ctypes.byref(a) if a is not None else None, F_, K_, D_, _ptr(m),
            ctypes.byref(b) if b is not None else None)
    invalid = [
        (dict(a=None), 'model is NULL'), (dict(b=None), 'model_out is NULL'),
        (dict(a=struct(src, precision_dev=None)), 'model: precision_dev is NULL'),
        (dict(a=struct(src, log_det_dev=None)), 'model: log_det_dev is NULL'),
        (dict(b=struct(dst, weight_dev=None)), 'model_out: weight_dev is NULL'),
        (dict(m=None), 'mapping_dev is NULL'),
        (dict(F_=0), 'F=0'), (dict(K_=0), 'K=0'), (dict(D_=0), 'D=0'),
        (dict(b=struct(src)), 'shares a buffer'),
        (dict(b=struct(dst, weight_dev=src.log_det_d.ptr)), 'shares a buffer'),
        (dict(b=struct(dst, precision_dev=src.precision_d.ptr)), 'shares a buffer'),
    ]
    for kw, match in invalid:
        status = call(**kw)
        assert status == _capi.GSS_ERR_INVALID, match
        with pytest.raises(ValueError, match=match):
            ctx._check(status, 'gss_cacgmm_model_permute')
    for kw, match in ((dict(K_=20), 'K=20 is larger than 19'), (dict(D_=33), 'D=33 is larger than 32')):
        status = call(**kw)
        assert status == _capi.GSS_ERR_UNSUPPORTED, match
        with pytest.raises(NotImplementedError, match=match):
            ctx._check(status, 'gss_cacgmm_model_permute')
    ctx._check(call(), 'gss_cacgmm_model_permute')
    assert dst.to_host(ctx).precision.tobytes() == model.precision.tobytes()


def test_moved_count_is_zero_before_any_alignment():
    from pb_chime5_amd import _capi
    ctx = _capi.Context(0)
    try:
        assert ctx.last_align_moved() == 0
    finally:
        ctx.close()
