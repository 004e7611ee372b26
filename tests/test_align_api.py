"""Permutation alignment without a GPU: the NumPy reference's own properties, the plan, every
argument error of the Python layer (a ValueError before any device work), the host-side model
gather and the binding's table."""
import ctypes

import numpy as np
import pytest

import align_reference as ar
import shared_prior_reference as spr


# ------------------------------------------------------------------ the reference's properties
def test_reference_recovers_a_scrambled_aligned_posterior():
    """The shared-prior posteriors of the table scene (classes aligned by construction), scrambled
    with a random permutation per bin, come back in every bin up to ONE global permutation; the
    mapping's rows are permutations; a second run on the aligned output is the identity."""
    from pb_chime5_amd import ops
    _, truth, _, posterior, prior = spr.table_run(0, 4)
    K, T, F = posterior.shape
    scrambled, perm = ar.scramble(posterior, 0)
    assert ar.moved(perm) > F // 2                       # the scramble is one
    plan = ops.alignment_plan(F)
    aligned, mapping, activity, margin = ar.align_ktf(scrambled, plan)
    assert mapping.shape == (F, K) and mapping.dtype == np.int32
    assert ar.is_permutation_rows(mapping)
    assert margin > 0
    # aligned[k,:,f] = posterior[perm[f, mapping[f,k]],:,f]: one q for all f
    composed = perm[np.arange(F)[:, None], mapping]
    q = ar.global_permutation(composed, np.tile(np.arange(K, dtype=np.int32), (F, 1)))
    assert q is not None, 'some bin was not recovered'
    np.testing.assert_array_equal(aligned, posterior[q])
    np.testing.assert_allclose(activity, np.mean(posterior[q], axis=-1), rtol=0, atol=1e-12)
    share, _, _ = spr.bins_consistent(aligned, activity, truth)
    share0, _, _ = spr.bins_consistent(posterior, prior, truth)
    assert share == share0
    again, mapping2, _, _ = ar.align_ktf(aligned, plan)
    np.testing.assert_array_equal(mapping2, np.tile(np.arange(K), (F, 1)))
    np.testing.assert_array_equal(again, aligned)


def test_reference_edge_cases():
    rng = np.random.default_rng(3)
    # K = 1: the identity, no margin
    mapping, margin, _ = ar.align(rng.uniform(size=(4, 1, 9)), [(3, 0, 4)])
    assert mapping.tolist() == [[0]] * 4 and margin == np.inf
    # entries that do not cover all of F leave the other rows alone
    gamma = rng.uniform(size=(6, 3, 20))
    gamma[2:5] = gamma[2:5][:, [2, 0, 1]] * np.array([1.0, 5.0, 9.0])[None, :, None]
    mapping, _, _ = ar.align(gamma, [(3, 2, 5)])
    assert mapping[[0, 1, 5]].tolist() == [[0, 1, 2]] * 3
    assert ar.is_permutation_rows(mapping)
    # a zero row has zero features; exact ties take the lexicographically smallest permutation
    gamma = np.zeros((2, 3, 5))
    mapping, margin, passes = ar.align(gamma, [(4, 0, 2)])
    assert mapping.tolist() == [[0, 1, 2]] * 2 and margin == 0.0 and passes == 1
    assert np.all(ar.features(gamma) == 0)


def test_parity_cells_follow_the_margin_rule():
    assert len(ar.CELLS) == 11 and (4, 70, 513, 3) in ar.CELLS
    assert any(T < 64 for _, T, _, _ in ar.CELLS) and any(K == 1 for *_, K in ar.CELLS)
    for cell in ar.CELLS:
        if cell[2] > 100:
            continue                                     # (the GPU test checks its own cells)
        seed = ar.seed_of(cell)
        assert ar.cell_margin(cell, seed) >= ar.MIN_MARGIN, cell
        for i in range(2):
            assert ar.is_permutation_rows(ar.parity_reference(cell, seed, i)[0])


# ------------------------------------------------------------------ the plan
def test_alignment_plan_values():
    from pb_chime5_amd import ops
    assert ops.alignment_plan(257) == [(20, 70, 170), (2, 50, 190), (2, 30, 210), (2, 10, 230),
                                       (2, 0, 250), (2, 0, 257)]
    assert ops.alignment_plan(129) == [(20, 35, 85), (2, 25, 95), (2, 15, 105), (2, 5, 115),
                                       (2, 0, 125), (2, 0, 129)]
    assert ops.alignment_plan(513) == [(20, 139, 338), (2, 100, 377), (2, 61, 416), (2, 22, 455),
                                       (2, 0, 494), (2, 0, 513)]
    assert ops.alignment_plan(1) == [(20, 0, 1)]
    assert ops.alignment_plan(2) == [(20, 0, 1), (2, 0, 2)]
    assert ops.alignment_plan(9, segment_start=3, segment_width=3, segment_shift=1,
                              main_iterations=6, sub_iterations=2) == \
        [(6, 3, 6), (2, 2, 7), (2, 1, 8), (2, 0, 9)]
    assert ops.alignment_plan(5, segment_start=99, segment_width=0) == \
        [(20, 4, 5), (2, 3, 5), (2, 2, 5), (2, 1, 5), (2, 0, 5)]
    for F in (1, 2, 3, 7, 129, 257, 513, 1000):
        plan = ops.alignment_plan(F)
        assert ops.check_alignment_plan(plan, F) == plan
        assert plan[-1][1:] == (0, F)
    for kw in (dict(num_frequencies=0), dict(num_frequencies=2.0), dict(num_frequencies=True),
               dict(num_frequencies=9, segment_start=-1), dict(num_frequencies=9, segment_width=-1),
               dict(num_frequencies=9, segment_shift=0), dict(num_frequencies=9, segment_shift=1.5),
               dict(num_frequencies=9, main_iterations=0), dict(num_frequencies=9, sub_iterations=0),
               dict(num_frequencies=9, sub_iterations=None)):
        with pytest.raises(ValueError):
            ops.alignment_plan(**kw)


def test_check_alignment_plan_rejects():
    from pb_chime5_amd import ops
    assert ops.check_alignment_plan([(np.int64(2), 0, np.int32(4))], 4) == [(2, 0, 4)]
    for bad, match in (([], 'no entries'), (None, 'not a sequence'), ('abc', 'not a sequence'),
                       (3, 'not a sequence'), ([(1, 0)], 'entry 0'), ([(1, 0, 4, 5)], 'entry 0'),
                       ([(1, 0, 2), (1.0, 0, 4)], 'entry 1'), ([(True, 0, 4)], 'entry 0'),
                       ([(0, 0, 4)], 'iterations'), ([(-1, 0, 4)], 'iterations'),
                       ([(1, -1, 4)], 'start'), ([(1, 2, 2)], 'start'), ([(1, 3, 2)], 'start'),
                       ([(1, 0, 5)], 'end'), ([5], 'entry 0')):
        with pytest.raises(ValueError, match=match):
            ops.check_alignment_plan(bad, 4)


# ------------------------------------------------------------------ argument errors, no device
def test_align_posteriors_argument_errors():
    from pb_chime5_amd import ops
    good = np.full((3, 10, 4), 1 / 3)
    for posterior, plan, match in (
            (np.zeros((3, 10)), None, r'not \(K,T,F\)'),
            (np.zeros((3, 10, 4), complex), None, 'not real'),
            (np.zeros((3, 0, 4)), None, 'no frames'),
            (np.zeros((3, 10, 0)), None, 'no frames'),
            (np.zeros((9, 10, 4)), None, r'9 classes outside \[1, 8\]'),
            (np.zeros((0, 10, 4)), None, r'0 classes outside'),
            (good, [], 'no entries'),
            (good, [(1, 0, 5)], 'plan entry 0'),
            (good, [(0, 0, 4)], 'iterations')):
        with pytest.raises(ValueError, match=match):
            ops.align_posteriors(posterior, plan)


def test_blind_calls_argument_errors():
    from pb_chime5_amd import ops
    Obs = np.ones((4, 10, 3), complex)
    with pytest.raises(ValueError, match='method'):
        ops.cacgmm_posteriors_blind(Obs, 3, method='hungarian')
    with pytest.raises(ValueError, match='method'):
        ops.check_blind_method(None)
    assert ops.check_blind_method('aligned') == 'aligned'
    with pytest.raises(ValueError, match='plan'):
        ops.cacgmm_posteriors_blind(Obs, 3, plan=[(1, 0, 3)])
    for fn in (lambda **kw: ops.cacgmm_posteriors_blind(Obs, method='aligned', **kw),
               lambda **kw: ops.cacgmm_fit_blind(Obs, **kw)):
        with pytest.raises(ValueError, match=r'9 classes outside \[1, 8\]'):
            fn(num_classes=9)
        with pytest.raises(ValueError, match='num_classes'):
            fn(num_classes=0)
        with pytest.raises(ValueError, match='iterations'):
            fn(num_classes=3, iterations=0)
        with pytest.raises(ValueError, match='seed'):
            fn(num_classes=3, seed=-1)
        with pytest.raises(ValueError, match='plan entry 0'):
            fn(num_classes=3, plan=[(1, 0, 4)])
    with pytest.raises(ValueError, match='not complex'):
        ops.cacgmm_fit_blind(np.ones((4, 10, 3)), 3)
    with pytest.raises(ValueError, match=r'not \(D,T,F\)'):
        ops.cacgmm_fit_blind(np.ones((4, 10), complex), 3)


def _model(F=3, K=4, D=2, seed=0):
    from pb_chime5_amd.cacgmm import CACGMM
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((F, K, D, D)) + 1j * rng.standard_normal((F, K, D, D))
    return CACGMM(A @ A.conj().swapaxes(-1, -2), rng.standard_normal((F, K)),
                  rng.uniform(size=(F, K)))


def test_model_permuted_is_fancy_indexing():
    model = _model()
    F, K, D = model.shape
    rng = np.random.default_rng(1)
    mapping = np.stack([rng.permutation(K) for _ in range(F)])
    out = model.permuted(mapping)
    for f in range(F):
        for k in range(K):
            j = mapping[f, k]
            np.testing.assert_array_equal(out.precision[f, k], model.precision[f, j])
            assert out.log_determinant[f, k] == model.log_determinant[f, j]
            assert out.weight[f, k] == model.weight[f, j]
    same = model.permuted(np.tile(np.arange(K), (F, 1)))
    np.testing.assert_array_equal(same.precision, model.precision)
    # the inverse permutation undoes it
    back = out.permuted(np.argsort(mapping, axis=1))
    np.testing.assert_array_equal(back.precision, model.precision)
    np.testing.assert_array_equal(back.weight, model.weight)


def test_mapping_argument_errors():
    from pb_chime5_amd import ops
    model = _model()
    F, K, _ = model.shape
    ident = np.tile(np.arange(K), (F, 1))
    bad_row = ident.copy()
    bad_row[1] = [0, 0, 2, 3]
    out_of_range = ident.copy()
    out_of_range[2, 3] = K
    negative = ident.copy()
    negative[0, 0] = -1
    for mapping, match in ((ident[:, :3], 'shape'), (ident[:2], 'shape'), (ident.ravel(), 'shape'),
                           (ident.astype(float), 'integer'), (bad_row, 'row 1'),
                           (out_of_range, 'row 2'), (negative, 'row 0')):
        with pytest.raises(ValueError, match=match):
            model.permuted(mapping)
        with pytest.raises(ValueError, match=match):
            ops.cacgmm_model_permute(model, mapping)
    with pytest.raises(ValueError, match='CACGMM'):
        ops.cacgmm_model_permute(None, ident)
    assert ops.check_mapping(ident, F, K).dtype == np.int32


def test_front_door_rejects_unknown_methods():
    from pb_chime5_amd import core
    enhancer = core.get_enhancer(wpe=False, bss_iterations=2, stft_size=64, stft_shift=16)
    obs = np.zeros((4, 640))
    with pytest.raises(ValueError, match='method'):
        enhancer.enhance_observation_blind(obs, 2, method='pb_bss')
    with pytest.raises(ValueError, match='num_speakers'):
        enhancer.enhance_observation_blind(obs, 8, method='aligned')


# ------------------------------------------------------------------ the binding
def test_binding_declares_the_three_symbols():
    from pb_chime5_amd import _capi, build
    for name in ('gss_cacgmm_align', 'gss_cacgmm_model_permute', 'gss_last_align_moved'):
        assert name in _capi.SIGNATURES
    assert len(_capi.SIGNATURES['gss_cacgmm_align'][1]) == 9
    assert len(_capi.SIGNATURES['gss_cacgmm_model_permute'][1]) == 7
    plan = _capi.GssAlignPlan
    assert [n for n, _ in plan._fields_] == ['iterations', 'start', 'end', 'entries']
    assert ctypes.sizeof(plan) == 3 * ctypes.sizeof(ctypes.c_void_p) + 8     # int32 + padding
    assert 'cacgmm_align.hip' in build.SOURCES
    from pb_chime5_amd import ops
    d = ops.DeviceAlignPlan([(3, 1, 4), (2, 0, 5)])
    assert d.struct.entries == 2
    assert [a.tolist() for a in d.arrays] == [[3, 2], [1, 0], [4, 5]]
    assert all(a.dtype == np.int32 for a in d.arrays)
    build.build(verbose=False)
    lib = _capi.load_library()
    assert hasattr(lib, 'gss_cacgmm_align') and hasattr(lib, 'gss_last_align_moved')
