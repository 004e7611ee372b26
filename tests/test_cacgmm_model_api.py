"""The host side of the model calls (no GPU): cacgmm.CACGMM, the shape rules of ops.cacgmm_fit /
cacgmm_predict, the C declarations, GSS.__call__(debug=...) and the NumPy log-likelihood helper
the GPU tests compare against."""
import re

import numpy as np
import pytest

import cacgmm_model_reference as ref
import gss_oracle as oracle
from conftest import REPO

SCENE = (6, 200, 3, 3, 5)


class NoDevice:
    """A context that fails the test when anything reaches for the device."""

    def __getattr__(self, name):
        raise AssertionError(f'device touched: {name}')


def _oracle_model():
    from pb_chime5_amd.cacgmm import CACGMM
    return CACGMM(*ref.dense(ref.oracle_fit(*SCENE)))


def test_model_fields_and_constructor_checks():
    from pb_chime5_amd.cacgmm import CACGMM
    D, T, F, K, _ = SCENE
    m = _oracle_model()
    assert m.shape == (F, K, D)
    assert m.precision.shape == (F, K, D, D) and m.precision.dtype == np.complex128
    assert m.log_determinant.shape == m.weight.shape == (F, K)
    assert m.precision.flags.c_contiguous
    for args, match in [
            ((m.precision[0], m.log_determinant, m.weight), 'precision'),
            ((m.precision[..., :-1], m.log_determinant, m.weight), 'precision'),
            ((m.precision.real, m.log_determinant, m.weight), 'complex'),
            ((m.precision, m.log_determinant[:, :-1], m.weight), 'log_determinant'),
            ((m.precision, m.log_determinant, m.weight[:1]), 'weight'),
            ((m.precision, m.log_determinant, m.weight.astype(complex)), 'weight')]:
        with pytest.raises(ValueError, match=match):
            CACGMM(*args)


def test_save_and_load_round_trip_without_pickle(tmp_path):
    from pb_chime5_amd.cacgmm import CACGMM
    m = _oracle_model()
    path = tmp_path / 'model.npz'
    m.save(path)
    with np.load(path, allow_pickle=False) as data:
        assert sorted(data.files) == ['log_determinant', 'precision', 'weight']
    back = CACGMM.load(path)
    assert np.array_equal(back.precision, m.precision)
    assert np.array_equal(back.log_determinant, m.log_determinant)
    assert np.array_equal(back.weight, m.weight)
    assert back.precision.dtype == np.complex128 and back.weight.dtype == np.float64


def test_normalized_undoes_any_scale():
    """normalized(): largest eigenvalue of B_k = 1, ln det moved along; the oracle's model, which
    is normalised, is a fixed point."""
    from pb_chime5_amd.cacgmm import CACGMM
    D = SCENE[0]
    m = _oracle_model()
    c = np.random.default_rng(0).uniform(0.01, 100.0, size=m.weight.shape)
    scaled = CACGMM(m.precision / c[..., None, None], m.log_determinant + D * np.log(c), m.weight)
    for model in (m, scaled):
        n = model.normalized()
        assert np.max(np.abs(np.linalg.eigvalsh(n.precision)[..., 0] - 1)) < 1e-12
        rel = np.linalg.norm(n.precision - m.precision, axis=(-1, -2)) / \
            np.linalg.norm(m.precision, axis=(-1, -2))
        assert np.max(rel) < 1e-10
        assert np.max(np.abs(n.log_determinant - m.log_determinant)) < 1e-9
        assert np.array_equal(n.weight, m.weight)


def test_shapes_are_checked_before_any_device_work():
    from pb_chime5_amd import ops
    from pb_chime5_amd.cacgmm import CACGMMTrainer
    D, T, F, K, _ = SCENE
    Y, act = ref.scene(D, T, F, K)
    m = _oracle_model()
    dev = NoDevice()
    cases = [
        (lambda: ops.cacgmm_predict(m, Y[:D - 1], ctx=dev), 'D = 5'),
        (lambda: ops.cacgmm_predict(m, Y[..., :F - 1], ctx=dev), 'F = 2'),
        (lambda: ops.cacgmm_predict(m, Y[0], ctx=dev), r'not \(D,T,F\)'),
        (lambda: ops.cacgmm_predict(m, Y, act[:, :T - 1], ctx=dev), 'frames'),
        (lambda: ops.cacgmm_predict(m, Y, act[:K - 1], ctx=dev), 'classes'),
        (lambda: ops.cacgmm_predict(m, Y, np.repeat(act[..., None], F + 1, axis=-1), ctx=dev),
         'frequencies'),
        (lambda: ops.cacgmm_log_likelihood(m, Y, act[0], ctx=dev), 'source_activity_mask'),
        (lambda: ops.cacgmm_predict(ref.oracle_fit(*SCENE), Y, ctx=dev), 'CACGMM'),
        (lambda: m.predict(Y[:D - 1], ctx=dev), 'D = 5'),
        (lambda: m.log_likelihood(Y, act[:, :T - 1], ctx=dev), 'frames'),
        (lambda: ops.cacgmm_fit(Y, None, None, 3, ctx=dev), 'both None'),
        (lambda: ops.cacgmm_fit(Y[0], None, act, 3, ctx=dev), r'not \(D,T,F\)'),
        (lambda: ops.cacgmm_fit(Y, None, act, 2.5, ctx=dev), 'iterations'),
        (lambda: ops.cacgmm_fit(Y, act[:, :T - 1], act, 3, ctx=dev), 'frames'),
        (lambda: ops.cacgmm_fit(Y, None, act[:, :T - 1], 3, model=m, ctx=dev), 'frames'),
        (lambda: ops.cacgmm_fit(Y[:D - 1], None, act, 3, model=m, ctx=dev), 'D = 5'),
        (lambda: ops.cacgmm_fit(Y, act, act, 3, model=m, ctx=dev), 'initialization'),
        (lambda: CACGMMTrainer().fit(Y, None, 3, act, ctx=dev), 'initialization'),
        (lambda: CACGMMTrainer().fit(Y[..., :F - 1], m, 3, act, ctx=dev), 'F = 2'),
    ]
    for call, match in cases:
        with pytest.raises(ValueError, match=match):
            call()


def test_header_and_binding_name_the_same_model_symbols():
    from pb_chime5_amd import _capi, build
    text = (REPO / 'include' / 'gss_hip.h').read_text()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in ('gss_cacgmm_fit', 'gss_cacgmm_predict'):
        assert re.search(rf'\bint {name}\s*\(', code), name
        assert name in _capi.SIGNATURES
    # the struct: the same fields in the same order, all pointers
    body = re.search(r'typedef struct \{([^}]*)\} gss_cacgmm_model;', code).group(1)
    fields = re.findall(r'\*\s*([a-z_]+_dev)\s*;', body)
    assert fields == [name for name, _ in _capi.GssCacgmmModel._fields_] == \
        ['precision_dev', 'log_det_dev', 'weight_dev']
    fit, predict = _capi.SIGNATURES['gss_cacgmm_fit'], _capi.SIGNATURES['gss_cacgmm_predict']
    assert len(fit[1]) == 10 and len(predict[1]) == 10
    # entry points only: the revision stays, and the new translation unit is part of the build
    assert '#define GSS_ABI_VERSION 7' in text and _capi.GSS_ABI_VERSION == 7
    assert 'cacgmm_model.hip' in build.SOURCES
    assert 'normalising constant' in text      # the header says what the log-likelihood leaves out


def test_gss_block_fits_the_learned_model_only_when_it_is_read(monkeypatch):
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import GSS
    D, T, F, K, _ = SCENE
    Y, act = ref.scene(D, T, F, K)
    calls = []
    posterior = np.zeros((K, T, F))
    monkeypatch.setattr(ops, 'cacgmm_posteriors', lambda *a, **k: posterior)
    monkeypatch.setattr(ops, 'cacgmm_posteriors_guided', lambda *a, **k: posterior)

    def fit(Obs, initialization=None, source_activity_mask=None, iterations=100, *, model=None,
            ctx=None):
        calls.append((initialization is not None, source_activity_mask is not None, iterations, model))
        return f'model {len(calls)}'
    monkeypatch.setattr(ops, 'cacgmm_fit', fit)
    block = GSS(iterations=7, iterations_post=3)
    assert block(Y, act) is posterior and calls == []
    assert block(Y, act, debug=True) is posterior
    # ... and even then only once somebody reads the key
    assert calls == [] and block.locals['initialization'].shape == (K, T)
    # `in` knows the key without fitting; iteration shows it once it has been read
    assert 'learned' in block.locals and 'nothing' not in block.locals and calls == []
    assert 'learned' not in list(block.locals) and block.locals.get('nothing', 3) == 3
    assert block.locals.get('learned') == 'model 2' and len(calls) == 2
    assert 'learned' in list(block.locals) and dict(block.locals)['learned'] == 'model 2'
    assert block.locals['learned'] == 'model 2' and len(calls) == 2
    # a 0/1 activity: the mask alone, then fit(initialization=model, post - 1) without a mask
    assert calls == [(False, True, 7, None), (False, False, 2, 'model 1')]
    assert block.locals['learned'] == 'model 2'
    del calls[:]
    block = GSS(iterations=4, iterations_post=1)
    block(Y, act * 0.5, debug=True)
    assert block.locals['learned'] == 'model 1'
    assert calls == [(True, True, 4, None)] and block.locals['learned'] == 'model 1'
    assert np.array_equal(block.locals['source_active_mask'], act)


def test_reference_log_likelihood_is_the_normaliser_of_the_posteriors():
    """The helper the GPU is compared with: exp(log_pdf + ln(pi m) - ll) are the oracle's
    posteriors, and a frame with every class off is -inf."""
    D, T, F, K, _ = SCENE
    Y, act = ref.scene(D, T, F, K)
    model = ref.oracle_fit(*SCENE)
    y = oracle.normalize_observation(ref.to_ftd(Y))
    log_pdf, _ = model._log_pdf(y)
    for mask in (None, ref.mask_fkt(act, F)):
        ll = ref.log_likelihood(model, Y, mask)
        assert ll.shape == (T, F) and np.all(np.isfinite(ll))
        w = model.weight if mask is None else model.weight * mask
        post = np.exp(log_pdf - ll.T[:, None, :]) * w
        want = model.predict(ref.to_ftd(Y), source_activity_mask=mask)
        assert np.max(np.abs(post - want)) < 1e-12
    off = ref.mask_fkt(act, F).copy()
    off[:, :, 7] = False
    ll = ref.log_likelihood(model, Y, off)
    assert np.all(np.isneginf(ll[7])) and np.sum(np.isneginf(ll)) == F
    # the scale of B_k cancels: -D ln(c q) - (ln det - D ln c)
    scaled = oracle.CACGMM(model.weight, model.covariance_eigenvectors,
                           model.covariance_eigenvalues * 3.0)
    assert np.max(np.abs(ref.log_likelihood(scaled, Y) - ref.log_likelihood(model, Y))) < 1e-9
