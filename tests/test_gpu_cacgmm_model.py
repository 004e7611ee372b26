"""The mixture model as an object on the GPU: gss_cacgmm_fit / gss_cacgmm_predict,
ops.cacgmm_fit / cacgmm_predict / cacgmm_log_likelihood, cacgmm.CACGMM / CACGMMTrainer and
GSS.__call__(debug=True)['learned'].

References: the closed call (ops.cacgmm_posteriors_guided) for the compositions, the untouched
oracle (CACGMMTrainer.fit(initialization=CACGMM), CACGMM.predict) for everything else, through
tests/cacgmm_model_reference.py.

The model a fit hands out is at the scale the EM left it (include/gss_hip.h, "Scale"): it is
compared with the oracle's, which pb_bss normalises to a largest eigenvalue of 1, after
``CACGMM.normalized()``.  On these scenes that step costs at most 6e-12 (precision) and 1.5e-10
(ln det) when the oracle's own model is scaled by a random factor, rounded and normalised back."""
import ctypes

import numpy as np
import pytest

import cacgmm_model_reference as ref
from test_gpu_guided import _oracle_guided

pytestmark = pytest.mark.gpu

# Bars of the model test: 10 x the worst distance of the GPU's head model from the oracle's over
# ref.NONFLOORED as measured on an MI355X (precision 2.7e-11 at 12 channels,
# ln det 1.6e-10 at 24, weights 4.3e-13 at 12), all below the caps 1e-8 / 1e-8 / 1e-10.  The
# oracle's own last-bit movement is 1.5e-11, 3.2e-11 and 2.9e-13.  Part of what the precision and
# ln det figures measure is NumPy, not the GPU: normalized() scales by the smallest eigenvalue
# `eigvalsh` finds for the precision, which is known only to eps * cond(B_k) (module docstring).
# The test prints every figure before it asserts.
BAR_PRECISION = 2.7e-10   # relative Frobenius norm per (f, k)
BAR_LOG_DET = 1.6e-9
BAR_WEIGHT = 4.3e-12


def _rel_fro(a, b):
    return np.linalg.norm(a - b, axis=(-1, -2)) / np.linalg.norm(b, axis=(-1, -2))


_HEAD = {}


def _head_model(gpu_ctx, sc):
    """ops.cacgmm_fit on the head of the scene, once per session."""
    from pb_chime5_amd import ops
    if sc not in _HEAD:
        D, T, F, K, iters = sc
        Y, act = ref.scene(D, T, F, K)
        n = ref.head_frames(T)
        _HEAD[sc] = ops.cacgmm_fit(Y[:, :n], None, act[:, :n], iters, ctx=gpu_ctx)
    return _HEAD[sc]


def _oracle_predict(model, Y, mask=None):
    """oracle.CACGMM.predict -> (K,T,F)."""
    return model.predict(ref.to_ftd(Y), source_activity_mask=mask).transpose(1, 2, 0)


# ------------------------------------------------------------------ 1. compositions
def _composition(ctx, Y, act, iters, post):
    from pb_chime5_amd import ops
    model = ops.cacgmm_fit(Y, None, act, iters, ctx=ctx)
    if post == 0:
        return ops.cacgmm_predict(model, Y, act, ctx=ctx)
    if post > 1:
        model = ops.cacgmm_fit(Y, iterations=post - 1, model=model, ctx=ctx)
    return ops.cacgmm_predict(model, Y, ctx=ctx)


@pytest.mark.parametrize('D,T,F,K,iters', [(6, 200, 3, 3, 5), (7, 200, 4, 4, 5), (12, 333, 3, 5, 4),
                                           (24, 400, 3, 5, 6), (6, 129, 3, 9, 3)])
@pytest.mark.parametrize('post', [0, 1, 2])
def test_fit_and_predict_compose_to_the_closed_call_bit_for_bit(gpu_ctx, D, T, F, K, iters, post):
    """fit(I) + predict(mask) / fit(I) + predict() / fit(I) + fit(model, post - 1) + predict()
    enqueue the launches of gss_cacgmm_guided(I, post) and convert the model losslessly."""
    from pb_chime5_amd import ops
    Y, act = ref.scene(D, T, F, K)
    want = ops.cacgmm_posteriors_guided(Y, None, act, iters, post, ctx=gpu_ctx)
    got = _composition(gpu_ctx, Y, act, iters, post)
    assert got.shape == want.shape == (K, T, F)
    assert np.array_equal(got, want)


@pytest.mark.parametrize('D,T,F,K,iters', [(4, 330, 3, 3, 5), (4, 700, 2, 5, 4)])
@pytest.mark.parametrize('post', [0, 1, 2])
def test_one_array_compositions_match_the_oracle(gpu_ctx, D, T, F, K, iters, post):
    """One array: the closed call runs em_onchip4_kernel, the model calls the multi-launch path;
    both are held to the oracle (1e-7, the bar of test_cacgmm_matches_oracle)."""
    from pb_chime5_amd import ops
    Y, act = ref.scene(D, T, F, K)
    init, mask = ops.guidance_from_activity(act)
    want = _oracle_guided(Y, init[None], mask[None], iters, post)
    got = _composition(gpu_ctx, Y, act, iters, post)
    closed = ops.cacgmm_posteriors_guided(Y, None, act, iters, post, ctx=gpu_ctx)
    err = np.max(np.abs(got - want))
    print(f'D={D} T={T} K={K} post={post}: composition vs oracle {err:.1e}, vs the closed call '
          f'{np.max(np.abs(got - closed)):.1e}, bit-equal: {np.array_equal(got, closed)}')
    assert err < 1e-7


# ------------------------------------------------------------------ 2. the model itself
@pytest.mark.parametrize('sc', ref.NONFLOORED, ids=str)
def test_head_model_against_the_oracles(gpu_ctx, sc):
    D, T, F, K, iters = sc
    want = ref.oracle_fit(*sc, frames=ref.head_frames(T))
    assert ref.floored_eigenvalues(want) == 0
    precision, log_det, weight = ref.dense(want)
    raw = _head_model(gpu_ctx, sc)
    assert raw.precision.shape == (F, K, D, D)
    # both triangles are stored and agree exactly; the diagonal is real
    assert np.array_equal(raw.precision, raw.precision.conj().swapaxes(-1, -2))
    got = raw.normalized()
    e_p = np.max(_rel_fro(got.precision, precision))
    e_l = np.max(np.abs(got.log_determinant - log_det))
    e_w = np.max(np.abs(got.weight - weight))
    scale = np.max(np.abs(np.log(np.linalg.eigvalsh(raw.precision)[..., 0])))
    print(f'{sc}: precision {e_p:.1e} log_det {e_l:.1e} weight {e_w:.1e}; '
          f'max |ln scale| of the model as fitted {scale:.2f}')
    assert e_p <= BAR_PRECISION
    assert e_l <= BAR_LOG_DET
    assert e_w <= BAR_WEIGHT


# ------------------------------------------------------------------ 3. held-out predict
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('sc', ref.NONFLOORED, ids=str)
def test_predict_on_frames_the_model_never_saw(gpu_ctx, sc, masked):
    from pb_chime5_amd import ops
    D, T, F, K, iters = sc
    Y, act = ref.scene(D, T, F, K)
    model = ref.oracle_fit(*sc, frames=ref.head_frames(T))
    mask = ref.mask_fkt(act, F) if masked else None
    want = _oracle_predict(model, Y, mask)
    got = ops.cacgmm_predict(_head_model(gpu_ctx, sc), Y, act if masked else None, ctx=gpu_ctx)
    whole = _oracle_predict(ref.oracle_fit(*sc), Y, mask)
    err, gap = np.max(np.abs(got - want)), np.max(np.abs(got - whole))
    print(f'{sc} masked={masked}: held-out predict vs oracle {err:.1e}; vs a whole-window fit {gap:.1e}')
    assert got.shape == (K, T, F)
    assert err < 1e-7
    # a predict that quietly refits on the frames it is given cannot pass
    assert gap > 1e-3
    if masked:
        assert np.all(got[~act] == 0)


# ------------------------------------------------------------------ 4. import on its own
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('sc', ref.NONFLOORED + [ref.FLOORED], ids=str)
def test_predict_from_the_oracles_model(gpu_ctx, sc, masked):
    """Dense precision, ln det and weights built from the ORACLE's model.  The floored scene's
    precision has entries near 4e9."""
    from pb_chime5_amd import ops
    from pb_chime5_amd.cacgmm import CACGMM
    D, T, F, K, iters = sc
    Y, act = ref.scene(D, T, F, K)
    model = ref.oracle_fit(*sc, frames=ref.head_frames(T))
    if sc == ref.FLOORED:
        assert ref.floored_eigenvalues(model) > 0
    want = _oracle_predict(model, Y, ref.mask_fkt(act, F) if masked else None)
    got = ops.cacgmm_predict(CACGMM(*ref.dense(model)), Y, act if masked else None, ctx=gpu_ctx)
    err = np.max(np.abs(got - want))
    print(f'{sc} masked={masked}: predict from the oracle\'s model {err:.1e}')
    assert err < 1e-7


# ------------------------------------------------------------------ 5. refit
def _models_equal(a, b):
    return (np.array_equal(a.precision, b.precision) and
            np.array_equal(a.log_determinant, b.log_determinant) and np.array_equal(a.weight, b.weight))


@pytest.mark.parametrize('sc', ref.NONFLOORED + [ref.FLOORED], ids=str)
def test_refit_continues_the_fit(gpu_ctx, sc):
    """fit(model, 2, mask) after fit(I, it) is fit(I, it + 2): bit for bit from 6 channels on
    (the oracle agrees with itself exactly here), within the bars of the model test below."""
    from pb_chime5_amd import ops
    D, T, F, K, iters = sc
    Y, act = ref.scene(D, T, F, K)
    first = ops.cacgmm_fit(Y, None, act, iters, ctx=gpu_ctx)
    got = ops.cacgmm_fit(Y, None, act, 2, model=first, ctx=gpu_ctx)
    want = ops.cacgmm_fit(Y, None, act, iters + 2, ctx=gpu_ctx)
    same = _models_equal(got, want)
    e_p = np.max(_rel_fro(got.precision, want.precision))
    e_l = np.max(np.abs(got.log_determinant - want.log_determinant))
    e_w = np.max(np.abs(got.weight - want.weight))
    print(f'{sc}: refit bit-equal {same}; precision {e_p:.1e} log_det {e_l:.1e} weight {e_w:.1e}')
    if D >= 6:
        assert same
    assert e_p <= BAR_PRECISION and e_l <= BAR_LOG_DET and e_w <= BAR_WEIGHT
    assert not _models_equal(first, want)
    # the trainer spells the same two calls
    from pb_chime5_amd.cacgmm import CACGMMTrainer
    init, mask = ops.guidance_from_activity(act)
    again = CACGMMTrainer().fit(Y, first, 2, source_activity_mask=mask, ctx=gpu_ctx)
    assert _models_equal(again, got)
    # zero iterations: the model's bits
    assert _models_equal(ops.cacgmm_fit(Y, iterations=0, model=first, ctx=gpu_ctx), first)


def _guidance(ctx, T, K, mask=None, mask_strides=None, init=None, init_strides=None):
    """gss_guidance over flat host tables with explicit (f, k) strides; returns (struct, buffers)."""
    from pb_chime5_amd import _capi
    init_d = ctx.to_device(np.ascontiguousarray(init, np.float64)) if init is not None else None
    mask_d = ctx.to_device(np.ascontiguousarray(mask, np.uint8)) if mask is not None else None
    ms = mask_strides or (0, T)
    ins = init_strides or (0, T)
    g = _capi.GssGuidance(init_dev=init_d.ptr if init_d else None,
                          mask_dev=mask_d.ptr if mask_d else None,
                          init_f_stride=ins[0], init_k_stride=ins[1],
                          mask_f_stride=ms[0], mask_k_stride=ms[1])
    return g, (init_d, mask_d)


def _raw_fit(ctx, Y_d, F, T, D, K, iterations, guidance, start, out):
    byref = lambda s: ctypes.byref(s) if s is not None else None     # noqa: E731
    return ctx.lib.gss_cacgmm_fit(ctx.handle, ctypes.c_void_p(Y_d.ptr), F, T, D, byref(guidance), K,
                                  iterations, byref(start), byref(out))


def _raw_predict(ctx, Y_d, F, T, D, K, model, guidance, gamma_d, loglik_d):
    byref = lambda s: ctypes.byref(s) if s is not None else None     # noqa: E731
    return ctx.lib.gss_cacgmm_predict(
        ctx.handle, ctypes.c_void_p(Y_d.ptr), F, T, D, byref(model), K, byref(guidance),
        ctypes.c_void_p(gamma_d.ptr if gamma_d else None),
        ctypes.c_void_p(loglik_d.ptr if loglik_d else None))


@pytest.mark.parametrize('sc', [(4, 330, 3, 3, 5), (12, 333, 3, 5, 8), (7, 200, 4, 4, 5)], ids=str)
def test_refit_in_place(gpu_ctx, sc):
    """model_out == init_model gives the result of separate buffers."""
    from pb_chime5_amd import ops
    D, T, F, K, iters = sc
    ctx = gpu_ctx
    Y, act = ref.scene(D, T, F, K)
    first = ops.cacgmm_fit(Y, None, act, iters, ctx=ctx)
    want = ops.cacgmm_fit(Y, None, act, 2, model=first, ctx=ctx)
    Y_d, _ = ops._obs_to_device_ftd(ctx, Y)
    g, keep = _guidance(ctx, T, K, mask=act)
    dev = ops.DeviceModel(ctx, F, K, D, first)
    ctx._check(_raw_fit(ctx, Y_d, F, T, D, K, 2, g, dev.struct, dev.struct), 'gss_cacgmm_fit')
    assert _models_equal(dev.to_host(ctx), want)


# ------------------------------------------------------------------ 6. log-likelihood
@pytest.mark.parametrize('sc', ref.NONFLOORED, ids=str)
def test_log_likelihood(gpu_ctx, sc):
    from pb_chime5_amd import ops
    D, T, F, K, iters = sc
    Y, act = ref.scene(D, T, F, K)
    oracle_model = ref.oracle_fit(*sc, frames=ref.head_frames(T))
    model = _head_model(gpu_ctx, sc)
    off = act.copy()
    off[:, [5, T - 1]] = False            # two frames with every class masked off
    for name, mask in (('unmasked', None), ('masked', act), ('frames off', off)):
        want = ref.log_likelihood(oracle_model, Y, None if mask is None else ref.mask_fkt(mask, F))
        got = model.log_likelihood(Y, mask, ctx=gpu_ctx)
        assert got.shape == want.shape == (T, F)
        assert np.array_equal(np.isneginf(got), np.isneginf(want))
        fin = np.isfinite(want)
        assert np.all(np.isfinite(got[fin]))
        err = np.max(np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin])))
        print(f'{sc} {name}: log-likelihood vs NumPy {err:.1e} (|ll| up to {np.max(np.abs(want[fin])):.0f})')
        assert err <= 1e-7
        if name == 'frames off':
            assert np.all(np.isneginf(got[[5, T - 1]])) and np.sum(np.isneginf(got)) == 2 * F
        else:
            assert not np.any(np.isneginf(got))
        # with the posteriors from the same call, and once more: the same bits
        posterior, both = ops.cacgmm_predict(model, Y, mask, log_likelihood=True, ctx=gpu_ctx)
        assert np.array_equal(both, got)
        assert np.array_equal(posterior, ops.cacgmm_predict(model, Y, mask, ctx=gpu_ctx))
        assert np.array_equal(model.log_likelihood(Y, mask, ctx=gpu_ctx), got)


def test_log_likelihood_shifts_over_the_active_classes_only(gpu_ctx):
    """A class the mask turns off may outweigh every active one by more than exp() spans (here
    ln det lowered by 2000, as floored eigenvalues at 24 channels can do): the shift of the
    log-sum-exp is the maximum of the ACTIVE terms, so the frame keeps the value it has without
    that class -- the same bits, since the class enters nothing else."""
    from pb_chime5_amd.cacgmm import CACGMM
    sc = (6, 200, 3, 3, 5)
    D, T, F, K, iters = sc
    Y, act = ref.scene(D, T, F, K)
    oracle_model = ref.oracle_fit(*sc, frames=ref.head_frames(T))
    precision, log_det, weight = ref.dense(oracle_model)
    mask = act.copy()
    mask[0] = False
    mask[1:, ::7] = True                  # some frames keep more than one active class
    heavy = log_det.copy()
    heavy[:, 0] -= 2000.0
    want = ref.log_likelihood(oracle_model, Y, ref.mask_fkt(mask, F))
    plain = CACGMM(precision, log_det, weight).log_likelihood(Y, mask, ctx=gpu_ctx)
    got = CACGMM(precision, heavy, weight).log_likelihood(Y, mask, ctx=gpu_ctx)
    fin = np.isfinite(want)
    assert np.sum(fin) > T * F // 2
    assert np.array_equal(np.isneginf(got), np.isneginf(want))
    err = np.max(np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin])))
    print(f'{sc}: log-likelihood with a masked-off class 2000 nats above vs NumPy {err:.1e}')
    assert err <= 1e-7
    assert np.array_equal(got, plain)


# ------------------------------------------------------------------ 7. strided per-frequency mask
@pytest.mark.parametrize('D,T,F,K', [(4, 300, 5, 3), (24, 200, 4, 5), (7, 130, 4, 4)])
def test_strided_per_frequency_mask_through_fit_and_predict(gpu_ctx, D, T, F, K):
    from pb_chime5_amd import ops
    ctx = gpu_ctx
    Y, act = ref.scene(D, T, F, K)
    mask = ref.mask_fkt(act, F).astype(np.uint8)
    mask[F // 2:, 0, :T // 3] = 0
    Y_d, _ = ops._obs_to_device_ftd(ctx, Y)
    ks, fs = T + 13, K * (T + 13) + 7
    rows = np.ones((F, K, ks), np.uint8)        # the padding holds what must not be read
    rows[..., :T] = mask
    padded = np.ones((F, fs), np.uint8)
    padded[:, :K * ks] = rows.reshape(F, -1)

    def run(table, strides):
        g, keep = _guidance(ctx, T, K, mask=table, mask_strides=strides)
        first, out = ops.DeviceModel(ctx, F, K, D), ops.DeviceModel(ctx, F, K, D)
        ctx._check(_raw_fit(ctx, Y_d, F, T, D, K, 3, g, None, first.struct), 'gss_cacgmm_fit')
        ctx._check(_raw_fit(ctx, Y_d, F, T, D, K, 2, g, first.struct, out.struct), 'gss_cacgmm_fit')
        g_d, ll_d = ctx.empty(8 * F * K * T), ctx.empty(8 * F * T)
        ctx._check(_raw_predict(ctx, Y_d, F, T, D, K, out.struct, g, g_d, ll_d), 'gss_cacgmm_predict')
        return (out.to_host(ctx), ctx.to_host(g_d, (F, K, T), np.float64),
                ctx.to_host(ll_d, (F, T), np.float64))
    m0, g0, l0 = run(mask, (K * T, T))
    m1, g1, l1 = run(padded, (fs, ks))
    assert _models_equal(m0, m1) and np.array_equal(g0, g1) and np.array_equal(l0, l1)
    assert np.all(g0[mask == 0] == 0)
    # the mask of the first frequency for all of them (f stride 0) is another model
    m2, g2, _ = run(mask[0], (0, T))
    assert not np.array_equal(g2, g0)
    assert np.array_equal(g2[0], g0[0]) and np.array_equal(m2.precision[0], m0.precision[0])


# ------------------------------------------------------------------ 8. fresh context, growing frames
@pytest.mark.parametrize('D,K', [(4, 3), (24, 5)])
def test_fresh_context_fit_short_then_predict_longer(D, K):
    """Each call sizes the arena for its own (F, T, D, K): a predict with more frames than any
    earlier call of a new context must not run out of workspace.  The fit sees 128 frames from
    the middle of the scene (where its sources are active), predict its first 200, 700 and all."""
    from pb_chime5_amd import _capi, ops
    T, F, iters, n, start = 2700, 2, 4, 128, 1286
    Y, act = ref.scene(D, T, F, K)
    want_model = ref.oracle_fit(D, T, F, K, iters, frames=n, start=start)
    ctx = _capi.Context(0)
    try:
        model = ops.cacgmm_fit(Y[:, start:start + n], None, act[:, start:start + n], iters, ctx=ctx)
        for frames in (200, 700, 2700):
            got, ll = ops.cacgmm_predict(model, Y[:, :frames], act[:, :frames], log_likelihood=True,
                                         ctx=ctx)
            assert got.shape == (K, frames, F) and ll.shape == (frames, F)
            assert np.all(np.isfinite(got)) and np.all(np.isfinite(ll))
            if frames < T:
                want = _oracle_predict(want_model, Y[:, :frames], ref.mask_fkt(act[:, :frames], F))
                err = np.max(np.abs(got - want))
                print(f'D={D}: fit on {n}, predict {frames} frames vs oracle {err:.1e}')
                assert err < 1e-7
    finally:
        ctx.close()


# ------------------------------------------------------------------ 9. errors
def test_errors_name_the_argument_and_leave_the_context_usable(gpu_ctx):
    from pb_chime5_amd import _capi, ops
    from pb_chime5_amd.cacgmm import CACGMM
    ctx = gpu_ctx
    D, T, F, K, iters = 6, 200, 3, 3, 3
    Y, act = ref.scene(D, T, F, K)
    Y_d, _ = ops._obs_to_device_ftd(ctx, Y)
    good, keep = _guidance(ctx, T, K, mask=act)
    first, out = ops.DeviceModel(ctx, F, K, D), ops.DeviceModel(ctx, F, K, D)
    g_d, ll_d = ctx.empty(8 * F * K * T), ctx.empty(8 * F * T)

    def model(**kw):
        fields = dict(precision_dev=out.precision_d.ptr, log_det_dev=out.log_det_d.ptr,
                      weight_dev=out.weight_d.ptr)
        return _capi.GssCacgmmModel(**{**fields, **kw})

    def fit(iterations=iters, guidance=good, start=None, dst=out.struct):
        return _raw_fit(ctx, Y_d, F, T, D, K, iterations, guidance, start, dst)

    def predict(m=first.struct, guidance=good, gamma=g_d, loglik=ll_d, k=K, d=D):
        return _raw_predict(ctx, Y_d, F, T, d, k, m, guidance, gamma, loglik)

    def normal_calls():
        ctx._check(fit(dst=first.struct), 'gss_cacgmm_fit')
        ctx._check(predict(), 'gss_cacgmm_predict')
        return ctx.to_host(g_d, (F, K, T), np.float64)
    want = normal_calls()
    bad_k, _ = _guidance(ctx, T, K, mask=act, mask_strides=(0, T - 1))
    bad_f, _ = _guidance(ctx, T, K, mask=ref.mask_fkt(act, F), mask_strides=(K * T - 1, T))
    no_tables = _capi.GssGuidance()
    cases = [
        (lambda: fit(dst=None), 'model_out is NULL'),
        (lambda: fit(dst=model(precision_dev=None)), 'model_out: precision_dev'),
        (lambda: fit(dst=model(log_det_dev=None)), 'model_out: log_det_dev'),
        (lambda: fit(dst=model(weight_dev=None)), 'model_out: weight_dev'),
        (lambda: fit(start=model(weight_dev=None)), 'init_model: weight_dev'),
        (lambda: fit(iterations=-1), 'iterations=-1'),
        (lambda: fit(iterations=-1, start=first.struct), 'iterations=-1'),
        (lambda: fit(iterations=0), 'iterations=0'),
        (lambda: fit(guidance=None), 'guidance is NULL'),
        (lambda: fit(guidance=no_tables), 'init_dev and mask_dev are both NULL'),
        (lambda: fit(guidance=bad_k), 'mask_k_stride'),
        (lambda: fit(guidance=bad_f), 'mask_f_stride'),
        (lambda: fit(guidance=bad_k, start=first.struct), 'mask_k_stride'),
        (lambda: predict(m=None), 'model is NULL'),
        (lambda: predict(m=model(precision_dev=None)), 'model: precision_dev'),
        (lambda: predict(m=model(log_det_dev=None)), 'model: log_det_dev'),
        (lambda: predict(gamma=None, loglik=None), 'gamma_dev and loglik_dev are both NULL'),
        (lambda: predict(guidance=bad_k), 'mask_k_stride'),
        (lambda: predict(guidance=bad_f), 'mask_f_stride'),
    ]
    for call, match in cases:
        status = call()
        assert status == _capi.GSS_ERR_INVALID, match
        with pytest.raises(ValueError, match=match):
            ctx._check(status, 'model call')
        assert np.array_equal(normal_calls(), want), match
    # the limits of D and K and their messages are gss_cacgmm's
    with pytest.raises(AssertionError, match='K < 20'):
        ctx._check(predict(k=20), 'gss_cacgmm_predict')
    with pytest.raises(NotImplementedError, match='D=1 outside'):
        ctx._check(predict(d=1), 'gss_cacgmm_predict')
    # a guidance without a mask, or none, is an unmasked predict / refit
    ctx._check(predict(guidance=None), 'gss_cacgmm_predict')
    unmasked = ctx.to_host(g_d, (F, K, T), np.float64)
    ctx._check(predict(guidance=no_tables), 'gss_cacgmm_predict')
    assert np.array_equal(ctx.to_host(g_d, (F, K, T), np.float64), unmasked)
    assert np.max(np.abs(unmasked.sum(axis=1) - 1)) < 1e-12 and not np.array_equal(unmasked, want)
    ctx._check(fit(guidance=None, start=first.struct), 'gss_cacgmm_fit')

    # Python: shapes are checked before any device work (a context that cannot be used)
    fitted = first.to_host(ctx)

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError(f'device touched: {name}')
    for call, match in [
            (lambda: ops.cacgmm_predict(fitted, Y[:D - 1], ctx=NoDevice()), 'D = 5'),
            (lambda: ops.cacgmm_predict(fitted, Y[..., :F - 1], ctx=NoDevice()), 'F = 2'),
            (lambda: ops.cacgmm_predict(fitted, Y, act[:, :T - 1], ctx=NoDevice()), 'frames'),
            (lambda: ops.cacgmm_predict(fitted, Y, act[:K - 1], ctx=NoDevice()), 'classes'),
            (lambda: ops.cacgmm_fit(Y, None, act[:, :T - 1], 2, model=fitted, ctx=NoDevice()), 'frames'),
            (lambda: ops.cacgmm_fit(Y[:D - 1], None, act, 2, model=fitted, ctx=NoDevice()), 'D = 5'),
            (lambda: ops.cacgmm_fit(Y, None, None, 2, ctx=NoDevice()), 'both None'),
            (lambda: ops.cacgmm_fit(Y, act, act, 2, model=fitted, ctx=NoDevice()), 'initialization'),
            (lambda: ops.cacgmm_log_likelihood(fitted, Y[0], ctx=NoDevice()), r'not \(D,T,F\)'),
            (lambda: ops.cacgmm_predict((fitted.precision,), Y, ctx=NoDevice()), 'CACGMM')]:
        with pytest.raises(ValueError, match=match):
            call()
    assert np.array_equal(ops.cacgmm_predict(fitted, Y, act, ctx=ctx).transpose(2, 0, 1), want)
    assert isinstance(fitted, CACGMM)


# ------------------------------------------------------------------ 10. GSS.__call__(debug=True)
@pytest.mark.parametrize('D,T,F,K,iters', [(7, 200, 4, 4, 5), (4, 330, 3, 3, 5)])
@pytest.mark.parametrize('post', [0, 1, 2])
@pytest.mark.parametrize('weighted', [False, True])
def test_gss_block_keeps_the_learned_model(gpu_ctx, D, T, F, K, iters, post, weighted):
    from pb_chime5_amd.cacgmm import CACGMM
    from pb_chime5_amd.core import GSS
    Y, act = ref.scene(D, T, F, K)
    activity = act * np.random.default_rng(K).uniform(0.05, 1.0, size=act.shape) if weighted else act
    block = GSS(iterations=iters, iterations_post=post)
    plain = block(Y, activity)
    assert not hasattr(block, 'locals')
    got = block(Y, activity, debug=True)
    assert np.array_equal(got, plain)
    learned = block.locals['learned']
    assert isinstance(learned, CACGMM) and learned.shape == (F, K, D)
    again = learned.predict(Y, act if post == 0 else None)
    if D == 4:
        assert np.max(np.abs(again - got)) < 1e-7
    else:
        assert np.array_equal(again, got)


# ------------------------------------------------------------------ 11. the log-form fall-back
@pytest.mark.parametrize('D', [24, 4])
def test_predict_takes_the_log_form_where_the_ratio_form_underflows(gpu_ctx, D):
    """The register-form E-step takes the posterior as (q_min / q_k)^D pi_k exp(ln det_min -
    ln det_k) and falls back to the log form where the sum of those terms is below 1e-280
    (posterior_ratio, csrc/cacgmm_estep.h).  A hand-made model -- the entry checks pointers only,
    precision and ln det need not be consistent -- whose classes are 330 decades apart both ways:
    precision_1 ~ I against precision_2 ~ 10^(330 / D) I and ln det_2 = -330 ln 10 + ln 3, so that
    in the ratio form BOTH terms of every frame underflow to zero (0 / tiny = 0 for both classes)
    while the log form gives posteriors near (3 pi_1, pi_2) / (3 pi_1 + pi_2), moved per frame
    by the diagonals.  Frequency 1 carries an ordinary, consistent model instead, so one launch
    runs both branches.  Reference: the log form in NumPy; bar: 1e-7, what this module holds
    cacgmm_predict to (the rounding of ln q and of the 760-nat terms is below 1e-12)."""
    from pb_chime5_amd import ops
    from pb_chime5_amd.cacgmm import CACGMM
    K, F, T = 2, 3, 70
    rng = np.random.default_rng(D)
    Y = rng.standard_normal((D, T, F)) + 1j * rng.standard_normal((D, T, F))
    scale = 10.0 ** (330.0 / D)
    precision = np.zeros((F, K, D, D), complex)
    log_det = np.zeros((F, K))
    for f in (0, 2):
        precision[f, 0] = np.diag(rng.uniform(0.9, 1.1, D))
        precision[f, 1] = scale * np.diag(rng.uniform(0.9, 1.1, D))
        log_det[f] = 0.0, -330.0 * np.log(10.0) + np.log(3.0)
    for k in range(K):
        A = rng.standard_normal((D, D)) + 1j * rng.standard_normal((D, D))
        precision[1, k] = A @ A.conj().T + np.eye(D)
        log_det[1, k] = -np.linalg.slogdet(precision[1, k])[1]
    weight = np.tile([0.4, 0.6], (F, 1))

    yn = Y / np.linalg.norm(Y, axis=0, keepdims=True)
    q = np.abs(np.einsum('dtf,fkde,etf->fkt', yn.conj(), precision, yn))           # (F,K,T)
    with np.errstate(under='ignore'):
        ratio = ((q.min(axis=1, keepdims=True) / q) ** D
                 * (weight * np.exp(log_det.min(axis=1, keepdims=True) - log_det))[:, :, None])
    assert np.all(ratio[[0, 2]].sum(axis=1) < 1e-280)       # every frame there takes the branch
    assert np.all(ratio[1].sum(axis=0) >= 1e-280)           # and no frame here
    lp = -D * np.log(q) - log_det[:, :, None]
    want = weight[:, :, None] * np.exp(lp - lp.max(axis=1, keepdims=True))
    want = (want / want.sum(axis=1, keepdims=True)).transpose(1, 2, 0)              # (K,T,F)
    assert 0.05 < want[:, :, [0, 2]].min() and want[:, :, [0, 2]].max() < 0.95

    got = ops.cacgmm_predict(CACGMM(precision, log_det, weight), Y, ctx=gpu_ctx)
    err = np.max(np.abs(got - want), axis=(0, 1))
    print(f'D={D}: predict vs the NumPy log form, per frequency {err}')
    assert got.shape == (K, T, F)
    assert np.max(err) < 1e-7
