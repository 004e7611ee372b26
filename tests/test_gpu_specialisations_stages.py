"""The kernel specialisations of the stages that tests/test_gpu_specialisations.py does not
name: the shared-prior E-step, the model's log-likelihood, posterior activity, channel selection
and the int16 STFT.  One cell per instantiation that a traced run of the GPU suite left
unlaunched (tools/kernel_coverage.py, tests/KERNEL_COVERAGE.md), each the smallest case that
launches it, compared with the CPU reference of its stage at the bar the stage's own tests use:
no bar is new here.

Scenes follow the rule of that module: the reference's own output moves at least 100 x less
than the bar when every input sample moves in its last bit.  Measured on the CPU:
 - shared prior: tests/shared_prior_reference.py (`python tests/shared_prior_reference.py`
   re-derives the seeds; seed 0 passed in every cell, the reference moves by at most 1.3e-11);
 - log-likelihood: at most 6.1e-14 at 7 channels and 1.9e-12 at 17, relative to max(1, |ll|),
   against the bar of 1e-7; no model has an eigenvalue at the floor
   (`test_log_likelihood_scenes_are_stable_for_the_reference` re-checks a sample);
 - posterior activity and channel selection: their bars are derived, not measured (see the
   stages' test modules), and the selection cells assert the MARGIN of their own scene;
 - int16 STFT: the oracle's x_hat moves by 5.9e-12 (window 400) and 1.0e-7 (window 2048)
   relative, against the bar of 1e-4.
"""
import functools

import numpy as np
import pytest

import cacgmm_model_reference as cmr
import channel_select_reference as csr
import gss_oracle as oracle
import shared_prior_reference as spr
from conftest import rel_err

gpu = pytest.mark.gpu

STABILITY_MARGIN = 100.0


def _cell_id(cell):
    return f'D{cell[0]}-K{cell[3]}'


# ================================================================== shared-prior E-step, LDS form
@gpu
@pytest.mark.parametrize('cell', spr.LDS_CELLS, ids=_cell_id)
def test_shared_prior_lds_form_estep_at_every_class_count(gpu_ctx, cell):
    """em_estep_prior_kernel<K, first | fit | predict> for K = 1..19 at D = 7 and D = 17 (no
    register form at either): two iterations run first and fit, the unmasked predict the third
    mode.  Weakly guided (a masked fit), against the reference at EM_TOL.  K = 1 launches its
    three instantiations but cannot fail on values: the posterior of a single class is 1."""
    from test_gpu_shared_prior import _run
    want, want_prior = spr.reference(cell, 'weak', spr.seed_of(cell, 'weak'))
    got, prior = _run(gpu_ctx, cell, 'weak')
    assert got.shape == want.shape and prior.shape == want_prior.shape
    err, perr = float(np.max(np.abs(got - want))), float(np.max(np.abs(prior - want_prior)))
    print(f'shared prior, LDS form {cell} weak: posteriors {err:.2e}, prior {perr:.2e}')
    assert err < spr.EM_TOL and perr < spr.EM_TOL


@gpu
@pytest.mark.parametrize('cell', spr.LDS_BLIND_CELLS, ids=_cell_id)
def test_shared_prior_lds_form_estep_from_an_unguided_start(gpu_ctx, cell):
    """The same instantiations with no mask at all: the (K,T) start of the annotation-free
    separation."""
    from test_gpu_shared_prior import _run
    want, want_prior = spr.reference(cell, 'blind', spr.seed_of(cell, 'blind'))
    got, prior = _run(gpu_ctx, cell, 'blind')
    err, perr = float(np.max(np.abs(got - want))), float(np.max(np.abs(prior - want_prior)))
    print(f'shared prior, LDS form {cell} blind: posteriors {err:.2e}, prior {perr:.2e}')
    assert err < spr.EM_TOL and perr < spr.EM_TOL


# ================================================================== log-likelihood
LOGLIK_TOL = 1e-7           # relative to max(1, |ll|): test_gpu_cacgmm_model.py::test_log_likelihood
LOGLIK_ITERATIONS = 3
# (D, T, F, K, iterations): every class count at one D <= 12, and one D in 13..32
LOGLIK_CELLS = ([(7, spr.lds_frames(7, K), 2, K, LOGLIK_ITERATIONS) for K in range(1, 20)] +
                [(17, spr.lds_frames(17, 13), 2, 13, LOGLIK_ITERATIONS)])


def _loglik_masks(act):
    off = act.copy()
    off[:, [5, act.shape[1] - 1]] = False     # two frames with every class masked off
    return (('unmasked', None), ('masked', act), ('frames off', off))


def _loglik_err(got, want):
    fin = np.isfinite(want)
    return float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))))


@functools.lru_cache(maxsize=None)
def _loglik_reference(sc):
    """The oracle's model of the whole window and its log-likelihood under the three masks."""
    D, T, F, K, _ = sc
    Y, act = cmr.scene(D, T, F, K)
    model = cmr.oracle_fit(*sc)
    want = {name: cmr.log_likelihood(model, Y, None if mask is None else cmr.mask_fkt(mask, F))
            for name, mask in _loglik_masks(act)}
    return model, want


@gpu
@pytest.mark.parametrize('sc', LOGLIK_CELLS, ids=lambda sc: f'D{sc[0]}-K{sc[3]}')
def test_log_likelihood_at_every_class_count(gpu_ctx, sc):
    """cacgmm_loglik_kernel<K>, K = 1..19.  The model is the ORACLE's, handed over in the dense
    form, so the cell tests this kernel (and the import) and not the fit."""
    from pb_chime5_amd.cacgmm import CACGMM
    D, T, F, K, _ = sc
    Y, act = cmr.scene(D, T, F, K)
    oracle_model, wants = _loglik_reference(sc)
    model = CACGMM(*cmr.dense(oracle_model))
    for name, mask in _loglik_masks(act):
        want = wants[name]
        got = model.log_likelihood(Y, mask, ctx=gpu_ctx)
        assert got.shape == want.shape == (T, F)
        assert np.array_equal(np.isneginf(got), np.isneginf(want))
        fin = np.isfinite(want)
        assert np.all(np.isfinite(got[fin]))
        err = _loglik_err(got, want)
        print(f'{sc} {name}: log-likelihood vs NumPy {err:.1e} '
              f'(|ll| up to {np.max(np.abs(want[fin])):.0f})')
        assert err <= LOGLIK_TOL
        if name == 'frames off':
            assert np.all(np.isneginf(got[[5, T - 1]])) and np.sum(np.isneginf(got)) == 2 * F
        else:
            assert not np.any(np.isneginf(got))


@pytest.mark.parametrize('sc', [LOGLIK_CELLS[0], LOGLIK_CELLS[7], LOGLIK_CELLS[18],
                                LOGLIK_CELLS[19]], ids=lambda sc: f'D{sc[0]}-K{sc[3]}')
def test_log_likelihood_scenes_are_stable_for_the_reference(sc):
    """Host only: the reference moves at least 100 x less than the bar under a last-bit change of
    the observation, and the model has no eigenvalue at the floor."""
    D, T, F, K, _ = sc
    Y, act = cmr.scene(D, T, F, K)
    model, wants = _loglik_reference(sc)
    assert cmr.floored_eigenvalues(model) == 0
    moved = spr.last_bit(Y, np.random.default_rng(12345))
    for name, mask in _loglik_masks(act):
        other = cmr.log_likelihood(model, moved, None if mask is None else cmr.mask_fkt(mask, F))
        assert np.array_equal(np.isneginf(other), np.isneginf(wants[name]))
        assert _loglik_err(other, wants[name]) * STABILITY_MARGIN <= LOGLIK_TOL


# ================================================================== posterior activity
# (D, T, F, K): pact_sums_kernel<12> serves K = 6..12 -- both its ends, one past it and its middle
PACT_SHAPES = [(5, 65, 3, 6), (12, 130, 2, 12), (4, 70, 2, 13), (7, 63, 2, 9)]


@gpu
@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('D,T,F,K', PACT_SHAPES)
def test_posterior_activity_at_the_class_count_buckets(gpu_ctx, D, T, F, K, weighted):
    from pb_chime5_amd import ops
    from test_gpu_posterior_activity import _case, _within
    _, _, Obs, post, w, scores, power = _case(D, T, F, K, weighted)
    got, gotp = ops.posterior_activity(Obs, post, w, return_power=True, ctx=gpu_ctx)
    _within(got, scores, F, D, f'{(D, T, F, K)} scores')
    _within(gotp, power, F, D, f'{(D, T, F, K)} power')


# ================================================================== channel selection
# chsel_bands_kernel<8 | 16 | 32 | 48 | 64>: both sides of every bucket edge and the last band
# count (65 is refused: test_gpu_channel_select.py::test_abi_errors_name_the_field).  F = B + 2
# is the smallest table in which `random_bank` gives every band a centre bin of its own
# (its centres are the B inner points of linspace(0, F - 1, B + 2)).
CHSEL_BANDS = [8, 9, 16, 17, 32, 33, 48, 49, 64]
CHSEL_D, CHSEL_T = 4, 100


@functools.lru_cache(maxsize=None)
def _chsel_case(B):
    """Scene (F,T,D), its (D,T,F) view, the bank, the reference's scores and variances."""
    F = B + 2
    Y = csr.scene(CHSEL_D, CHSEL_T, F)
    W = csr.random_bank(np.random.default_rng(100 * B + F), B, F)
    scores, V = csr.channel_scores(Y, W)
    Obs = np.ascontiguousarray(Y.transpose(2, 1, 0))
    for a in (Y, W, scores, V, Obs):
        a.setflags(write=False)
    return Obs, W, scores, V


@gpu
@pytest.mark.parametrize('B', CHSEL_BANDS)
def test_channel_selection_at_the_band_count_buckets(gpu_ctx, B):
    from pb_chime5_amd import ops
    from test_gpu_channel_select import BAR, MARGIN, _keeps, _rel
    Obs, W, scores, V = _chsel_case(B)
    D = CHSEL_D
    got, gotV = ops.channel_scores(Obs, bank=W, return_band_variances=True, ctx=gpu_ctx)
    assert got.shape == (D,) and gotV.shape == (B, D)
    es, ev = _rel(got, scores), _rel(gotV, V)
    print(f'B={B}: scores {es:.1e}, band variances {ev:.1e}')
    assert es <= BAR and ev <= BAR
    for keep in _keeps(D):
        gap = csr.boundary_gap(scores, keep)
        assert gap > MARGIN, (keep, gap)        # (a scene that comes close is to be changed)
        sel, channels = ops.select_channels(Obs, keep, bank=W, ctx=gpu_ctx)
        assert np.array_equal(channels, csr.pick(scores, keep)), (keep, channels)
        assert np.array_equal(sel, Obs[channels]), keep


@pytest.mark.parametrize('B', CHSEL_BANDS)
def test_channel_selection_scenes_keep_the_margin(B):
    """Host only: no selection boundary of these scenes comes near a tie."""
    from test_gpu_channel_select import MARGIN, _keeps
    scores = _chsel_case(B)[2]
    assert min(csr.boundary_gap(scores, keep) for keep in _keeps(CHSEL_D)) > MARGIN


# ================================================================== online CACGMM: state <-> model
# cacgmm_online_convert_kernel<NR> holds an NR x NR block per lane: NR = ceil(D / 8).  The stage's
# own round trip runs at D = 4 and 24 (NR = 1, 3); these are the parity cells of
# tests/online_cacgmm_reference.py either side of every edge, 8 | 9, 16 | 17, 24 | 29 and 32.
# Their states have cond(S) <= 3.7e3; np.linalg's model of them moves by at most 7.1e-14
# (precision), 3.5e-15 (ln det) and 3.2e-16 (weight) under a last-bit change of the state, against
# the bar of 1e-9.
ONLINE_CONVERT_D = (8, 9, 16, 17, 24, 29, 32)


def _online_convert_cells():
    import online_cacgmm_reference as cr
    return [next(c for c in cr.CELLS if c[0] == D and c[5] > 1) for D in ONLINE_CONVERT_D]


@gpu
@pytest.mark.parametrize('cell', _online_convert_cells(), ids=lambda c: f'D{c[0]}-K{c[1]}')
def test_online_state_to_model_and_back_at_every_block_width(gpu_ctx, cell):
    """to_model() of the REFERENCE's state after the cell's scene against np.linalg, and
    from_model() of np.linalg's model against that state: both directions of the conversion
    kernel alone, at the bar of test_gpu_cacgmm_online.py::test_model_round_trip."""
    import online_cacgmm_reference as cr
    from pb_chime5_amd import ops
    from pb_chime5_amd.cacgmm import CACGMM
    D, K, beta, prior_mass, F, T = cell
    _, st, _ = cr.reference(cell, cr.seed_of(cell))
    precision, log_det, weight = cr.to_model(st)
    model = ops.OnlineCACGMMState.from_host(st, ctx=gpu_ctx).to_model()
    assert model.shape == (F, K, D)
    P = model.precision
    assert np.array_equal(P, P.conj().swapaxes(-1, -2))
    errs = dict(precision=cr.rel_err(P, precision),
                log_det=cr.rel_err(model.log_determinant, log_det),
                weight=cr.rel_err(model.weight, weight))
    print(f'{cell}: to_model vs np.linalg {errs}')
    assert max(errs.values()) < cr.ROUND_TRIP_TOL, errs
    mass = st['n'].sum(axis=1)
    assert cr.rel_err(mass, np.full(F, mass[0])) <= K * cr.AFF_EPS
    back = ops.OnlineCACGMMState.from_model(CACGMM(precision, log_det, weight),
                                            mass=float(mass[0]), ctx=gpu_ctx).to_host()
    errs = cr.rel_err(back['s'], st['s']), cr.rel_err(back['n'], st['n'])
    print(f'{cell}: from_model vs the state {errs}')
    assert max(errs) < cr.ROUND_TRIP_TOL, errs


# ================================================================== int16 STFT
X_TOL = 1e-4                # x_hat against the oracle (tests/test_gpu_pipeline.py: TOL_STFT_MAG)
PCM_PARAMS = dict(wpe_taps=2, wpe_iterations=2, bss_iterations=3)


@functools.lru_cache(maxsize=None)
def _pcm_scene():
    from pb_chime5_amd import synthetic
    u = synthetic.tiny(seed=0, num_channels=4, num_samples=12000)
    pcm = np.clip(np.rint(u.obs / np.abs(u.obs).max() * 20000), -32768, 32767).astype(np.int16)
    return u, pcm, pcm.astype(np.float64) / 2 ** 15


@gpu
@pytest.mark.parametrize('stft_size,stft_shift', [(400, 100), (2048, 512)])
def test_pcm16_input_is_bit_identical_to_float64_at_other_windows(gpu_ctx, stft_size, stft_shift):
    """The assertion of test_gpu_pipeline.py::test_pcm16_input_is_bit_identical_to_float64 where
    int16 samples take stft_dft_kernel<short> (a window that is no power of two) and
    stft_kernel<1, short> (a window above 1024); the float64 call against the oracle."""
    from pb_chime5_amd import ops
    u, pcm, as_float = _pcm_scene()
    cs = u.ex['start_orig']['original'] - u.ex['start']['original']
    ce = u.ex['end']['original'] - u.ex['end_orig']['original']
    params = ops.make_params(stft_size=stft_size, stft_shift=stft_shift, **PCM_PARAMS)
    want = ops.enhance_observation(as_float, u.activity_array, u.target_index, cs, ce,
                                   params=params, ctx=gpu_ctx)
    pipe = ops.UtterancePipeline(params, depth=2, first_ctx=gpu_ctx)
    try:
        pipe.enqueue('pcm', pcm, u.activity_array, u.target_index, cs, ce)
        pipe.enqueue('f64', as_float, u.activity_array, u.target_index, cs, ce)
        got = dict(pipe.pop() for _ in range(2))
    finally:
        pipe.close()
    assert np.array_equal(got['f64'], want)
    assert np.array_equal(got['pcm'], want)
    ref = oracle.enhance_observation(as_float, u.activity_array, u.target_index, u.ex,
                                     stft_size=stft_size, stft_shift=stft_shift,
                                     gss_fn=oracle.gss_block_batched, **PCM_PARAMS)
    assert want.shape == ref.shape
    err = rel_err(want, ref)
    print(f'window {stft_size}/{stft_shift}: float64 call vs the oracle {err:.1e}')
    assert err < X_TOL
