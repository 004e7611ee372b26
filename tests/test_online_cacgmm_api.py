"""Online CACGMM (gss_cacgmm_online, get_enhancer(gss_online=True)): the NumPy reference itself
(tests/online_cacgmm_reference.py), the evidence that the continued model follows a moving speaker
where the frozen one does not, the C surface, and every argument check and front door -- none of it
needs a GPU."""
import ctypes
import inspect

import numpy as np
import pytest

import online_cacgmm_reference as cr
from conftest import REPO

SYMBOLS = ('gss_cacgmm_online_init', 'gss_cacgmm_online', 'gss_cacgmm_online_model',
           'gss_last_cacgmm_online_fallbacks', 'gss_enhance_observation_gss_online')


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
def test_reference_in_blocks_equals_one_call():
    for cell in cr.CHUNK_CELLS:
        D, K, beta, prior_mass, F, T = cell
        Y, activity = cr.scene(cell, cr.seed_of(cell))
        gamma1, st1, _ = cr.reference(cell, cr.seed_of(cell))

        def step(Yb, ab, state):
            return cr.online_cacgmm(Yb, ab, beta, state)[:2]
        gamma, st = cr.in_blocks(Y, activity, cr.fresh_state(F, K, D, prior_mass), cr.CHUNKS[T], step)
        assert np.array_equal(gamma, gamma1)
        assert np.array_equal(st['s'], st1['s']) and np.array_equal(st['n'], st1['n'])


@pytest.mark.parametrize('cell', cr.CLOSED_FORM_CELLS, ids=str)
def test_reference_recursion_is_its_closed_form(cell):
    """With every g and q known, n_k = beta^T n0 + sum beta^(T-1-t) g_kt and S_k likewise."""
    D, K, beta, prior_mass, F, T = cell
    Y, activity = cr.scene(cell, cr.seed_of(cell))
    gamma, st, fallbacks, g, q, live = cr.online_cacgmm(
        Y, activity, beta, cr.fresh_state(F, K, D, prior_mass), record=True)
    assert fallbacks == 0 and live.all()
    assert np.array_equal(g, np.clip(gamma, cr.AFF_EPS, 1 - cr.AFF_EPS))
    S, n = cr.closed_form(Y, g, q, beta, prior_mass)
    errs = cr.rel_err(st['s'], S), cr.rel_err(st['n'], n)
    assert max(errs) < cr.CLOSED_FORM_TOL, errs
    assert np.all(n > 0)


def test_no_mask_from_a_fresh_state_gives_exactly_one_over_k():
    """Identical classes stay identical: every class gets the very same bits at every frame, so
    the state never separates.  The value is 1 / K exactly for K = 2 (n + n and e + e are exact);
    for other K the two sums of K equal terms carry up to K - 1 roundings each and three more
    operations follow, so it is 1 / K to (2 K + 1) half-ulps."""
    for cell in ((4, 3, 0.99, 1.0, 3, 150), (3, 3, 0.95, 1.0, 2, 90), (4, 8, 0.9, 1.0, 2, 200),
                 (2, 2, 1.0, 1.0, 2, 70), (24, 5, 0.995, 1.0, 2, 120)):
        D, K, beta, prior_mass, F, T = cell
        Y, _ = cr.scene(cell)
        gamma, st, _ = cr.online_cacgmm(Y, None, beta, cr.fresh_state(F, K, D, prior_mass))
        assert all(np.array_equal(gamma[:, 0], gamma[:, k]) for k in range(K)), cell
        assert np.max(np.abs(gamma * K - 1.0)) <= (2 * K + 1) * np.finfo(float).eps / 2, cell
        if K == 2:
            assert np.all(gamma == 0.5), cell
        assert all(np.array_equal(st['s'][:, 0], st['s'][:, k]) for k in range(K))
        assert all(np.array_equal(st['n'][:, 0], st['n'][:, k]) for k in range(K))


def test_a_zero_frame_leaves_the_state_bit_identical():
    cell = cr.CELLS[0]
    D, K, beta, prior_mass, F, T = cell
    Y, activity = cr.scene(cell)
    _, st, _ = cr.online_cacgmm(Y[:, :40], activity[:, :40], beta, cr.fresh_state(F, K, D, prior_mass))
    zeros = np.zeros((F, 10, D), complex)
    gamma, st2, fallbacks = cr.online_cacgmm(zeros, activity[:, 40:50], beta, st)
    assert np.array_equal(st2['s'], st['s']) and np.array_equal(st2['n'], st['n'])
    assert fallbacks == 0 and np.all(np.isfinite(gamma))
    # the letter: z = 0, q = tiny for every class, so only ln det B_k, pi_k and the mask decide
    assert np.array_equal(gamma, cr.predict(zeros, st, activity[:, 40:50]))
    # the edge scene is the same thing inside a call
    Ye, act = cr.edge_scene(cell, 'block')
    lo = T // 2
    _, before, _ = cr.online_cacgmm(Ye[:, :lo], act[:, :lo], beta, cr.fresh_state(F, K, D, prior_mass))
    _, after, _ = cr.online_cacgmm(Ye[:, lo:lo + 10], act[:, lo:lo + 10], beta, before)
    assert np.array_equal(after['s'], before['s']) and np.array_equal(after['n'], before['n'])


def test_one_class_gets_everything_and_a_masked_frame_nothing():
    cell = (4, 1, 0.99, 1.0, 2, 20)
    gamma, st, _ = cr.reference(cell)
    assert np.all(gamma == 1.0) and np.all(st['n'] > 0)
    cell = cr.CELLS[0]
    D, K, beta, prior_mass, F, T = cell
    Y, activity = cr.edge_scene(cell, 'masked')
    gamma, _, _ = cr.online_cacgmm(Y, activity, beta, cr.fresh_state(F, K, D, prior_mass))
    assert np.all(gamma[:, :, 5:10] == 0) and np.all(np.isfinite(gamma))
    on = activity.any(axis=0)
    assert np.allclose(gamma.sum(axis=1)[:, on], 1.0, atol=1e-12)


def test_reference_fallback_cases():
    for kind in ('first', 'every'):
        Y, activity, st0, beta, count = cr.fallback_case(kind)
        gamma, st, fallbacks = cr.online_cacgmm(Y, activity, beta, st0)
        assert fallbacks == count == Y.shape[0] * Y.shape[1], kind
        assert np.all(np.isfinite(gamma)) and np.any(st['s'][:, 1] != 0)     # the update stays


def test_reference_model_round_trip():
    cell = cr.CELLS[0]
    D, K, beta, prior_mass, F, T = cell
    Y, activity = cr.scene(cell)
    _, st, _ = cr.reference(cell)
    precision, log_det, weight = cr.to_model(st)
    back = cr.from_model(precision, weight, float(st['n'].sum(axis=1)[0]))
    # (the clip keeps every frame's sum_k g_k within [1, 1 + K 1e-10])
    assert np.allclose(st['n'].sum(axis=1), st['n'].sum(axis=1)[0], rtol=K * cr.AFF_EPS, atol=0)
    assert cr.rel_err(back['s'], st['s']) < cr.ROUND_TRIP_TOL
    assert cr.rel_err(back['n'], st['n']) < cr.ROUND_TRIP_TOL
    # the oracle's own predict on that model is the frozen posterior
    import gss_oracle as oracle
    lam, vec = np.linalg.eigh(np.linalg.inv(precision))
    # (CACGMM takes the eigendecomposition of B_k; ln det B_k = sum ln lambda)
    model = oracle.CACGMM(weight[..., None], vec, lam)
    assert np.allclose(model.log_determinant, log_det, rtol=0, atol=1e-9)
    want = model.predict(Y[:, :7])
    assert cr.rel_err(cr.predict(Y[:, :7], st), want) < 1e-9


def test_parity_scenes_are_stable():
    """The rule that keeps a seed: the reference itself moves at least STABILITY_MARGIN x less
    than the bar under a last-bit change of every sample."""
    for cell in cr.CELLS:
        moved = cr.reference_movement(cell, cr.seed_of(cell))
        assert moved * cr.STABILITY_MARGIN <= cr.TOL, (cell, moved)
        assert cr.reference(cell, cr.seed_of(cell))[2] == 0
    assert max(c[0] for c in cr.CELLS) == 32 and max(c[1] for c in cr.CELLS) == 8
    assert cr.CELLS[:2] == [(4, 3, 0.99, 1.0, 3, 150), (1, 2, 0.9, 1.0, 1, 5)] and len(cr.CELLS) == 16
    for cell in cr.LONG_CELLS:
        moved = cr.reference_movement(cell, cr.long_seed_of(cell))
        print(f'{cell}: seed {cr.long_seed_of(cell)} moves {moved:.1e}')
        assert moved * cr.STABILITY_MARGIN <= cr.long_tol(cell), (cell, moved)
        assert cr.TOL <= cr.long_tol(cell) <= cr.LONG_BAR_CAP
        assert cr.reference(cell, cr.long_seed_of(cell))[2] == 0
    assert cr.LONG_CELLS == [(4, 4, 0.99, 1.0, 2, 6000), (12, 4, 0.99, 1.0, 1, 5000),
                             (24, 5, 0.99, 1.0, 1, 4000), (4, 3, 0.95, 1.0, 2, 4000)]


# ------------------------------------------------------------------ long horizons
def test_long_reference_in_blocks_equals_one_call_and_the_pin_fires_on_a_border():
    """The cell whose scale drifts: the reference rescales a class at least twice, the ragged
    partition puts one rescaling on the last frame of a block and one on the first, and both
    partitions give the bits of the single call."""
    cell = cr.PIN_CELL
    assert cell in cr.LONG_CELLS
    D, K, beta, prior_mass, F, T = cell
    Y, activity = cr.scene(cell, cr.long_seed_of(cell))
    gamma1, st1, _ = cr.reference(cell, cr.long_seed_of(cell))
    frames = sorted({t for t, _, _ in cr.long_pins(cell)})
    parts = cr.long_partitions(cell)
    ends = np.cumsum(parts['ragged'])
    assert len(frames) >= 2 and frames[0] + 1 in ends and frames[1] in ends
    inner = np.cumsum(parts['blocks'])
    assert not any(t in inner or t + 1 in inner for t in frames)      # inside the 625-blocks
    assert np.all(np.abs(cr.scale_exponents(st1['s'])) <= cr.SCALE_BAND)

    def step(Yb, ab, state):
        return cr.online_cacgmm(Yb, ab, beta, state)[:2]
    for name, cuts in parts.items():
        gamma, st = cr.in_blocks(Y, activity, cr.fresh_state(F, K, D, prior_mass), cuts, step)
        assert np.array_equal(gamma, gamma1), name
        assert np.array_equal(st['s'], st1['s']) and np.array_equal(st['n'], st1['n']), name
    # without the pin the same cell leaves the band (and float64's normal range is 1022 wide)
    lo = [0]

    def watch(t, S, n):
        lo[0] = min(lo[0], int(cr.scale_exponents(S).min()))
    cr.online_cacgmm(Y, activity, beta, cr.fresh_state(F, K, D, prior_mass), watch=watch, band=10 ** 6)
    print(f'{cell}: the exponent reaches {lo[0]} without the pin')
    assert lo[0] < -cr.SCALE_BAND


def test_the_band_is_never_reached_by_the_short_cells():
    """The extremes that justify SCALE_BAND: with the pin off, the exponent of the largest
    diagonal entry, watched after every frame, stays inside +-40 on every parity cell, every
    64-point stream cell and the pipeline scene -- so the pin changes no existing cell."""
    import gss_oracle as oracle
    import stream_reference as sr
    ext = {}

    def run(what, Y, activity, beta, state):
        def watch(t, S, n):
            e = cr.scale_exponents(S)
            lo, hi = ext.get(what, (0, 0))
            ext[what] = min(lo, int(e.min())), max(hi, int(e.max()))
        cr.online_cacgmm(Y, activity, beta, state, watch=watch, watch_every=1, band=10 ** 6)
    for cell in cr.CELLS:
        D, K, beta, prior_mass, F, T = cell
        Y, activity = cr.scene(cell, cr.seed_of(cell))
        run('CELLS', Y, activity, beta, cr.fresh_state(F, K, D, prior_mass))
    for name, c in sr.CELLS.items():
        if c[0] > 64:
            continue
        x, activity = sr.scene(name, sr.seed_of(name))
        Obs = sr.reference(name, sr.seed_of(name))[1]['Obs']
        actf = oracle.activity_time_to_frequency(activity, c[0], c[1], True)[:, :Obs.shape[1]]
        run('stream', Obs, actf, sr.SETTINGS['gss_forget'], sr.fresh_states(name)['em'])
    # the pipeline scene: the oracle's stages up to the mixture model, whose frames go through `run`
    pp, u = cr.PIPE, cr.pipe_scene()

    def gss_fn(Obs, acitivity_freq, iterations, iterations_post):
        Y = cr.to_ftd(Obs)
        act = np.asarray(acitivity_freq)[:, :Y.shape[1]]
        state = cr.fresh_state(Y.shape[0], act.shape[0], Y.shape[2], pp['prior_mass'])
        run('pipeline', Y, act, pp['forget'], state)
        return cr.to_ktf(cr.online_cacgmm(Y, act, pp['forget'], state)[0])
    oracle.enhance_observation(u.obs, u.activity_array, u.target_index, u.ex, wpe_taps=pp['wpe_taps'],
                               wpe_delay=pp['wpe_delay'], stft_size=pp['stft_size'],
                               stft_shift=pp['stft_shift'], gss_fn=gss_fn)
    print(f'exponents without the pin: {ext}')
    assert sorted(ext) == ['CELLS', 'pipeline', 'stream']
    for what, (lo, hi) in ext.items():
        assert -40 <= lo and hi <= 40, (what, lo, hi)


def test_reference_is_scale_invariant():
    """S_k handed in multiplied by 2^e_k, another e_k per class: the same gamma within TOL, and
    every class back inside the band after the call."""
    cell = cr.CELLS[0]
    D, K, beta, prior_mass, F, T = cell
    Y, activity = cr.scene(cell, cr.seed_of(cell))
    _, mid, _ = cr.online_cacgmm(Y[:, :20], activity[:, :20], beta, cr.fresh_state(F, K, D, prior_mass))
    want, _, _ = cr.online_cacgmm(Y[:, 20:], activity[:, 20:], beta, mid)
    scaled = cr.scaled_state(mid)
    assert np.abs(cr.scale_exponents(scaled['s'])).min() > 100
    gamma, st, fallbacks = cr.online_cacgmm(Y[:, 20:], activity[:, 20:], beta, scaled)
    err = cr.rel_err(gamma, want)
    print(f'scaled state: gamma moves {err:.1e}')
    assert fallbacks == 0 and err < cr.TOL
    assert np.all(np.abs(cr.scale_exponents(st['s'])) <= cr.SCALE_BAND)
    assert np.array_equal(st['n'].shape, mid['n'].shape) and cr.rel_err(st['n'], cr.online_cacgmm(
        Y[:, 20:], activity[:, 20:], beta, mid)[1]['n']) < cr.TOL


# ------------------------------------------------------------------ the starved class
def test_the_starved_cell_breaks_the_plain_recursion_and_not_the_guarded_one():
    """Plain (the recursion without guard and pin): within 8 000 frames cond(S_k) passes 1e15 and
    np.linalg.cholesky fails.  Guarded: no fallback, cond(S_k) sampled every 100 frames stays
    at or below STARVED_COND, and the float64 reference lies within STARVED_REFEREE_TOL of the
    80-bit referee -- the condition under which the device may be held to the referee."""
    import ext_precision as xp
    p = cr.STARVED
    Y, activity = cr.starved_scene()
    assert Y.shape == (2, 7500, p['D']) and Y.shape[1] <= 8000
    _, st, fallbacks, cond = cr.starved_reference(plain=True)
    print(f'plain: {fallbacks} fallbacks, cond(S_k) up to {cond:.1e}, n {np.round(st["n"], 3).tolist()}')
    assert fallbacks >= 1 and cond > 1e15
    gamma, st, fallbacks, cond = cr.starved_reference()
    print(f'guarded: {fallbacks} fallbacks, cond(S_k) up to {cond:.1e}')
    assert fallbacks == 0 and cond <= cr.STARVED_COND
    assert st['n'].min() < 0.5 < p['D']                 # a class whose mass is far below D
    on = activity.any(axis=0)
    assert np.all(np.isfinite(gamma)) and np.allclose(gamma.sum(axis=1)[:, on], 1.0, atol=1e-12)
    referee, failed = cr.starved_referee()
    dist = float(np.max(np.abs(gamma - referee)))
    print(f'guarded float64 reference vs the 80-bit referee: {dist:.1e}')
    assert failed == 0 and dist <= cr.STARVED_REFEREE_TOL


def test_the_continued_model_follows_a_moving_speaker():
    """From frame 200 on nobody guides the model and speaker 0 moves: the state that keeps
    learning classifies the frames from 400 on with less than EVIDENCE_BOUND x the error of the
    SAME state frozen at frame 200; the seed is one for which the reference gives <= 0.75."""
    ratio = cr.evidence_ratio()
    print(f'continued / frozen error: {ratio:.3f}')
    assert ratio <= 0.75 < cr.EVIDENCE_BOUND


def test_the_starved_reference_in_blocks_equals_one_call_with_the_guard_live_on_the_cuts():
    """The rank guard across block borders: in the starved cell the gate phi is above 0.1 on the
    frame before and the frame after the later 625-frame cuts and around both cuts of the ragged
    partition's one-frame block, and both partitions give the bits of the single call."""
    p = cr.STARVED
    Y, activity = cr.starved_scene()
    F, T, D = Y.shape
    gamma1, st1, _, _ = cr.starved_reference()
    gates = cr.starved_gates()
    parts = cr.starved_partitions()
    cuts = np.cumsum(parts['blocks'])[:-1]
    alive = [int(c) for c in cuts if gates[c - 1] > 0.1 and gates[c] > 0.1]
    print(f'starved cell: phi up to {gates.max():.2f}, above 0 on {int((gates > 0).sum())} frames; '
          f'625-frame cuts with phi > 0.1 on both sides: {alive}; ragged {parts["ragged"]}')
    assert len(alive) >= 3
    a, b = np.cumsum(parts['ragged'])[1:3]
    assert b == a + 1 and min(gates[a - 1], gates[a], gates[b]) > 0.1

    def step(Yb, ab, state):
        return cr.online_cacgmm(Yb, ab, p['beta'], state)[:2]
    for name, cut in parts.items():
        gamma, st = cr.in_blocks(Y, activity, cr.fresh_state(F, p['K'], D, p['prior_mass']), cut, step)
        assert np.array_equal(gamma, gamma1), name
        assert np.array_equal(st['s'], st1['s']) and np.array_equal(st['n'], st1['n']), name


def test_the_long_stream_scene_breaks_the_plain_recursion_and_not_the_guarded_one():
    """The frames of stream_reference.long_scene (no WPE in front): the recursion without the
    guard loses factors, the guarded one loses none."""
    import gss_oracle as oracle
    import stream_reference as sr
    p = sr.LONG
    x, act = sr.long_scene()
    Y = oracle.stft(x, p['W'], p['H'], fading=True)
    actf = oracle.activity_time_to_frequency(act, p['W'], p['H'], True)[:, :Y.shape[1]] != 0
    Y = cr.to_ftd(Y)
    F, T, D = Y.shape
    assert 8000 <= T <= 8200
    counts = [cr.online_cacgmm(Y, actf, sr.SETTINGS['gss_forget'],
                               cr.fresh_state(F, p['K'], D, sr.SETTINGS['gss_prior_mass']), plain=plain)[2]
              for plain in (True, False)]
    print(f'long stream scene: fallbacks plain {counts[0]}, guarded {counts[1]}')
    assert counts[0] >= 1 and counts[1] == 0


# ------------------------------------------------------------------ the C surface
def test_the_built_library_exports_the_entry_points():
    from pb_chime5_amd import _capi, build
    assert 'cacgmm_online.hip' in build.SOURCES
    lib = _capi.load_library()
    header = (REPO / 'include' / 'gss_hip.h').read_text()
    for name in SYMBOLS:
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
        assert f'int {name}(' in header, name
    assert _capi.GSS_ABI_VERSION == 7 and lib.gss_abi_version() == 7


def test_descriptor_layouts_are_the_header_structs():
    from pb_chime5_amd import _capi, ops
    header = (REPO / 'include' / 'gss_hip.h').read_text()
    for decl in ('gss_cplx *s;', 'double *n;', 'int32_t F, K, D;', '} gss_cacgmm_online_state;',
                 '} gss_em_online;', 'double forget;', 'double prior_mass;',
                 '#define GSS_CACGMM_ONLINE_MAX_CLASSES 8'):
        assert decl in header, decl
    S = _capi.GssCacgmmOnlineState
    assert [n for n, _ in S._fields_] == ['s', 'n', 'F', 'K', 'D']
    assert [getattr(S, n).offset for n, _ in S._fields_] == [0, 8, 16, 20, 24] and ctypes.sizeof(S) == 32
    C = _capi.GssEmOnline
    assert [n for n, _ in C._fields_] == ['forget', 'prior_mass']
    assert [getattr(C, n).offset for n, _ in C._fields_] == [0, 8] and ctypes.sizeof(C) == 16
    assert ops._FUSED_ENTRIES['gss_online'] == ('gss_enhance_observation_gss_online', None,
                                                'online CACGMM')
    assert _capi.SIGNATURES['gss_enhance_observation_gss_online'] == \
        _capi._fused(ctypes.POINTER(C), ctypes.POINTER(_capi.GssBfOnline))
    assert ops._ONLINE_MAX_CLASSES == 8


def test_the_unit_has_one_form_and_no_float_atomics():
    unit = (REPO / 'pb_chime5_amd' / 'csrc' / 'cacgmm_online.hip').read_text()
    assert 'getenv' not in unit and 'gss_variant' not in unit
    assert 'rocblas' not in unit.lower() and 'rocsolver' not in unit.lower()
    # the atomics are integer counts: the fallbacks of a frequency, the failed pivots of a conversion
    assert unit.count('atomicAdd(') == 2
    assert 'atomicAdd(a.fallbacks, total)' in unit and 'atomicAdd(a.failed, 1)' in unit
    assert 'chol_inverse_sweep<8, NR, true>' in unit and 'c_outer(' in unit


def test_the_host_side_inverts_nothing():
    """from_model and to_model convert on the device: the package's host code has no np.linalg
    call on their path."""
    from pb_chime5_amd import ops
    for fn in (ops.OnlineCACGMMState.from_model.__func__, ops.OnlineCACGMMState.to_model,
               ops.cacgmm_posteriors_online):
        assert 'linalg' not in inspect.getsource(fn), fn


# ------------------------------------------------------------------ argument checks
def test_check_gss_online(no_context):
    from pb_chime5_amd import ops
    assert (ops.GSS_ONLINE_FORGET, ops.GSS_ONLINE_PRIOR_MASS) == (0.99, 1.0)
    assert ops.check_gss_online() == (0.99, 1.0)
    assert ops.check_gss_online(1, 3, 8, 32) == (1.0, 3.0)
    assert ops.check_gss_online(0.5, 1e-9, 1, 1) == (0.5, 1e-9)
    nan, inf = float('nan'), float('inf')
    for kw, word in ((dict(forget=0.0), 'forget'), (dict(forget=1.0001), 'forget'),
                     (dict(forget=nan), 'forget'), (dict(forget='a'), 'forget'),
                     (dict(forget=True), 'forget'),
                     (dict(prior_mass=0.0), 'prior_mass'), (dict(prior_mass=-1.0), 'prior_mass'),
                     (dict(prior_mass=inf), 'prior_mass'), (dict(prior_mass=nan), 'prior_mass'),
                     (dict(prior_mass=None), 'prior_mass'),
                     (dict(num_classes=0), 'num_classes'), (dict(num_classes=9), 'num_classes'),
                     (dict(num_classes=2.5), 'num_classes'),
                     (dict(num_channels=0), 'num_channels'), (dict(num_channels=33), 'num_channels'),
                     (dict(num_channels=2.5), 'num_channels')):
        with pytest.raises(ValueError, match=word):
            ops.check_gss_online(**kw)
    sig = inspect.signature(ops.cacgmm_posteriors_online).parameters
    assert [sig[k].default for k in ('source_activity_mask', 'num_classes', 'forget', 'prior_mass',
                                     'state', 'return_fallbacks', 'ctx')] == \
        [None, None, 0.99, 1.0, None, False, None]


def test_stage_argument_errors_before_any_device_work(no_context):
    from pb_chime5_amd import ops
    from pb_chime5_amd.cacgmm import CACGMM
    Y = np.ones((3, 9, 5), complex)
    m = np.ones((2, 9), bool)
    call = ops.cacgmm_posteriors_online
    with pytest.raises(ValueError, match='Obs'):
        call(Y[0], m)
    with pytest.raises(ValueError, match='start from a model'):
        call(Y)
    with pytest.raises(ValueError, match='start from a model'):
        call(Y, num_classes=3)
    for kw, word in ((dict(forget=0.0), 'forget'), (dict(prior_mass=0.0), 'prior_mass'),
                     (dict(state=object()), 'state'), (dict(num_classes=3), 'num_classes')):
        with pytest.raises(ValueError, match=word):
            call(Y, m, **kw)
    with pytest.raises(ValueError, match='num_channels'):
        call(np.ones((33, 9, 5), complex), m)
    with pytest.raises(ValueError, match='num_classes'):
        call(Y, np.ones((9, 9), bool))
    for bad, word in ((np.ones((2, 8), bool), 'frames'), (np.ones((2, 9, 4), bool), 'frequencies'),
                      (np.ones(9, bool), 'source_activity_mask')):
        with pytest.raises(ValueError, match=word):
            call(Y, bad)
    for args, kw, word in (((0, 2, 4), {}, 'F'), ((5, 0, 4), {}, 'num_classes'),
                           ((5, 9, 4), {}, 'num_classes'), ((5, 2, 0), {}, 'num_channels'),
                           ((5, 2, 33), {}, 'num_channels'),
                           ((5, 2, 4), dict(prior_mass=0.0), 'prior_mass')):
        with pytest.raises(ValueError, match=word):
            ops.OnlineCACGMMState.fresh(*args, **kw)
    for host, word in ((dict(s=np.ones((5, 2, 4, 3)), n=np.ones((5, 2))), "s: shape"),
                       (dict(s=np.ones((5, 4, 4)), n=np.ones((5, 2))), "s: shape"),
                       (dict(s=np.ones((5, 2, 4, 4)), n=np.ones((5, 3))), 'n: shape'),
                       (dict(s=np.ones((5, 9, 4, 4)), n=np.ones((5, 9))), 'num_classes'),
                       (dict(s=np.ones((5, 2, 33, 33)), n=np.ones((5, 2))), 'num_channels')):
        with pytest.raises(ValueError, match=word):
            ops.OnlineCACGMMState.from_host(host)
    model = CACGMM(np.ones((5, 2, 4, 4), complex), np.zeros((5, 2)), np.full((5, 2), 0.5))
    with pytest.raises(ValueError, match='model'):
        ops.OnlineCACGMMState.from_model(object())
    for mass in (0.0, float('nan'), -1.0):
        with pytest.raises(ValueError, match='prior_mass'):
            ops.OnlineCACGMMState.from_model(model, mass=mass)
    big = CACGMM(np.ones((5, 9, 4, 4), complex), np.zeros((5, 9)), np.full((5, 9), 1 / 9))
    with pytest.raises(ValueError, match='num_classes'):
        ops.OnlineCACGMMState.from_model(big)
    from pb_chime5_amd.online_cacgmm import OnlineCACGMM
    for kw, word in ((dict(forget=2.0), 'forget'), (dict(prior_mass=0), 'prior_mass'),
                     (dict(num_classes=9), 'num_classes'), (dict(channel=0), 'num_channels'),
                     (dict(frequency_bins=0), 'frequency_bins'), (dict(model=object()), 'model')):
        with pytest.raises(ValueError, match=word):
            OnlineCACGMM(**kw)


def test_state_shapes_and_a_mismatched_state():
    """The buffers of a state and the rule that a call takes only the state built for it --
    on a context that allocates nothing."""
    from pb_chime5_amd import ops

    class Buf:
        def __init__(self, n):
            self.nbytes, self.ptr = n, 4096

    class Ctx:
        def empty(self, n):
            return Buf(n)
    st = ops.OnlineCACGMMState(Ctx(), 5, 2, 3)
    assert st.shapes == {'s': (5, 2, 3, 3), 'n': (5, 2)} and st.key == (5, 2, 3)
    assert {k: b.nbytes for k, b in st.bufs.items()} == {'s': 16 * 90, 'n': 8 * 10}
    s = st.struct()
    assert (s.s, s.n, s.F, s.K, s.D) == (4096, 4096, 5, 2, 3)
    m = np.ones((2, 9), bool)
    for Y, mask in ((np.ones((4, 9, 5), complex), m), (np.ones((3, 9, 6), complex), m),
                    (np.ones((3, 9, 5), complex), np.ones((3, 9), bool))):
        with pytest.raises(ValueError, match='state'):
            ops.cacgmm_posteriors_online(Y, mask, state=st)
    with pytest.raises(ValueError, match='context'):
        ops.cacgmm_posteriors_online(np.ones((3, 9, 5), complex), m, state=st, ctx=Ctx())


def test_the_stream_object(monkeypatch):
    from pb_chime5_amd import ops
    from pb_chime5_amd.online_cacgmm import OnlineCACGMM
    made, seen = [], []
    monkeypatch.setattr(ops.OnlineCACGMMState, 'fresh',
                        classmethod(lambda cls, F, K, D, prior_mass, ctx=None:
                                    made.append((F, K, D, prior_mass)) or 'state'))

    def fake(Obs, mask, **kw):
        seen.append((Obs.shape, None if mask is None else np.shape(mask), kw))
        return np.zeros((3, Obs.shape[1], Obs.shape[2])), 2
    monkeypatch.setattr(ops, 'cacgmm_posteriors_online', fake)
    em = OnlineCACGMM(forget=0.9, prior_mass=0.5, num_classes=3, channel=4, frequency_bins=5)
    assert made == [(5, 3, 4, 0.5)] and em.state == 'state' and em.fallbacks == 0
    out = em.step_frames(np.zeros((7, 5, 4), complex), np.ones((3, 7), bool))
    assert out.shape == (3, 7, 5) and em.fallbacks == 2
    assert seen[-1] == ((4, 7, 5), (3, 7), dict(forget=0.9, prior_mass=0.5, state='state',
                                                return_fallbacks=True))
    out = em.step_frame(np.zeros((5, 4), complex), np.ones(3, bool))
    assert out.shape == (3, 5) and seen[-1][:2] == ((4, 1, 5), (3, 1)) and em.fallbacks == 4
    with pytest.raises(ValueError, match='block'):
        em.step_frames(np.zeros((7, 4, 5), complex), np.ones((3, 7), bool))
    with pytest.raises(ValueError, match='frame'):
        em.step_frame(np.zeros((4, 5), complex), np.ones(3, bool))
    with pytest.raises(ValueError, match='model'):
        em.step_frames(np.zeros((7, 5, 4), complex))
    em.reset()
    assert len(made) == 2 and em.fallbacks == 0


def test_fused_argument_errors_before_any_device_work(no_context):
    from pb_chime5_amd import ops
    obs, act = np.zeros((4, 4096)), np.ones((3, 4096), bool)
    call = ops.enhance_observation_gss_online
    with pytest.raises(ValueError, match='obs'):
        call(obs[0], act, 0, 0, 0)
    for kw, word in ((dict(forget=0.0), 'forget'), (dict(prior_mass=-1), 'prior_mass'),
                     (dict(bf_online=True, bf_forget=0.0), 'forget'),
                     (dict(bf_online=True, bf_loading=0.0), 'loading'),
                     (dict(bf_online=True, ref_channel=4), 'ref_channel'),
                     (dict(bf_online=True, wpe_online=True, wpe_alpha=0.0), 'alpha'),
                     (dict(bf_online=True, wpe_online=True, wpe=False), 'wpe=False'),
                     (dict(wpe_online=True), 'without bf_online')):
        with pytest.raises(ValueError, match=word):
            call(obs, act, 0, 0, 0, **kw)
    with pytest.raises(ValueError, match='num_classes'):
        call(obs, np.ones((9, 4096), bool), 0, 0, 0)
    with pytest.raises(NotImplementedError, match='bf_online'):
        call(obs, act, 0, 0, 0, bf_online=True, bf='gev_ban')
    sig = inspect.signature(call).parameters
    assert [sig[k].default for k in ('forget', 'prior_mass', 'bf_online', 'bf_forget', 'bf_loading',
                                     'ref_channel', 'wpe_online', 'wpe_alpha')] \
        == [0.99, 1.0, False, 0.99, 1e-2, -1, False, 0.9999]


# ------------------------------------------------------------------ the mixture-model block
def test_gss_block(monkeypatch):
    from pb_chime5_amd import core, ops
    seen = []

    def fake(Obs, mask, **kw):
        seen.append((mask.dtype, mask.shape, kw))
        return np.full((mask.shape[0],) + Obs.shape[1:], 0.25), 0
    monkeypatch.setattr(ops, 'cacgmm_posteriors_online', fake)

    def boom(*a, **k):
        raise AssertionError('the iterated EM')
    monkeypatch.setattr(ops, 'cacgmm_posteriors', boom)
    monkeypatch.setattr(ops, 'cacgmm_posteriors_guided', boom)
    plain = core.GSS(20, 1)
    assert (plain.online, plain.forget, plain.prior_mass) == (False, 0.99, 1.0)
    assert plain.online_settings is None and plain == core.GSS(20, 1, online=False)
    block = core.GSS(20, 1, online=True, forget=0.9, prior_mass=0.5)
    assert block.online_settings == dict(forget=0.9, prior_mass=0.5)
    out = block(np.zeros((4, 9, 5), complex), np.array([[1] * 12, [0] * 12, [0.3] * 12]))
    assert out.shape == (3, 9, 5)
    assert seen == [(np.dtype(bool), (3, 12), dict(forget=0.9, prior_mass=0.5, return_fallbacks=True))]
    with pytest.raises(NotImplementedError, match='gss_online with an initialization'):
        block(np.zeros((4, 9, 5), complex), np.ones((3, 12)), initialization=np.ones((3, 12)))
    with pytest.raises(NotImplementedError, match='gss_online with shared_prior'):
        core.GSS(20, 1, online=True, shared_prior=True)
    with pytest.raises(ValueError, match='forget'):
        core.GSS(20, 1, online=True, forget=0.0)
    with pytest.raises(ValueError, match='prior_mass'):
        core.GSS(20, 1, online=True, prior_mass=0.0)
    for kw, word in ((dict(forget=0.9), 'gss_forget'), (dict(prior_mass=2.0), 'gss_prior_mass')):
        with pytest.raises(NotImplementedError, match=f'{word}.*nobody reads it'):
            core.GSS(20, 1, **kw)


# ------------------------------------------------------------------ front doors
def test_every_front_door_has_the_keywords_and_carries_them():
    from pb_chime5_amd import core, core_chime6, core_chime6_rttm
    for mod in (core, core_chime6, core_chime6_rttm):
        sig = inspect.signature(mod.get_enhancer).parameters
        assert [sig[k].default for k in ('gss_online', 'gss_forget', 'gss_prior_mass')] == \
            [False, 0.99, 1.0], mod.__name__
    for mod in (core, core_chime6):
        plain = mod.get_enhancer()
        assert plain._gss_online() is None and not plain.gss_block.online
        assert plain.gss_block == mod.get_enhancer(gss_online=False).gss_block
        enh = mod.get_enhancer(gss_online=True, gss_forget=0.95, gss_prior_mass=0.1, bf_online=True,
                               wpe_online=True, wpe_per_array=True, multiarray=True)
        assert enh._gss_online() == dict(forget=0.95, prior_mass=0.1) and enh._fusable()
        assert enh._wpe_online() == 0.9999 and enh._bf_online() == dict(forget=0.99, loading=1e-2)
        assert mod.get_enhancer(gss_online=True)._gss_online() == dict(forget=0.99, prior_mass=1.0)
        for kw, word in ((dict(bf='wpdSouden_ban'), "gss_online with bf='wpdSouden_ban'"),
                         (dict(bf='wpdSouden'), "gss_online with bf='wpdSouden'"),
                         (dict(bf_segment_frames=64), 'gss_online with bf_segment_frames'),
                         (dict(bf_null_interferer=True), 'gss_online with bf_null_interferer'),
                         (dict(channel_keep=3), 'gss_online with channel_keep')):
            with pytest.raises(NotImplementedError, match=word):
                mod.get_enhancer(gss_online=True, **kw)
        for kw, word in ((dict(gss_forget=0.9), 'gss_forget'),
                         (dict(gss_prior_mass=2.0), 'gss_prior_mass')):
            with pytest.raises(NotImplementedError, match=f'{word}.*without gss_online'):
                mod.get_enhancer(**kw)
        with pytest.raises(ValueError, match='forget'):
            mod.get_enhancer(gss_online=True, gss_forget=1.5)
        with pytest.raises(ValueError, match='prior_mass'):
            mod.get_enhancer(gss_online=True, gss_prior_mass=0.0)


def test_rttm_front_door_takes_the_keywords(tmp_path):
    from pb_chime5_amd.core_chime6_rttm import get_enhancer
    from test_rttm_frontdoor import _make_chime6_dir
    root, rttm, _ = _make_chime6_dir(tmp_path)
    kw = dict(database_rttm=[str(rttm)], activity_rttm=[str(rttm)], chime6_dir=root,
              multiarray='outer_array_mics')
    enh = get_enhancer(**kw, gss_online=True, gss_forget=0.98)
    assert enh._gss_online() == dict(forget=0.98, prior_mass=1.0)
    assert get_enhancer(**kw)._gss_online() is None


def test_command_lines_parse_the_keys(monkeypatch):
    from pb_chime5_amd.scripts import run, kaldi_run, kaldi_run_rttm, enhance_rttm
    cfg = run.main(['print_config', 'with', 'gss_online=True', 'gss_forget=0.95',
                    'gss_prior_mass=0.1'])
    assert (cfg['gss_online'], cfg['gss_forget'], cfg['gss_prior_mass']) == (True, 0.95, 0.1)
    cfg = run.main(['print_config'])
    assert (cfg['gss_online'], cfg['gss_forget'], cfg['gss_prior_mass']) == (False, 0.99, 1.0)
    assert kaldi_run.main(['print_config', 'with', 'gss_online=True'])['gss_online'] is True
    assert kaldi_run_rttm.main(['print_config', 'with', 'database_rttm=a.rttm', 'gss_online=True',
                                'gss_forget=0.9'])['gss_forget'] == 0.9

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
        enhance_rttm.main(base + ['--gss-online', '--gss-forget', '0.95', '--gss-prior-mass', '0.5'])
    assert (seen['gss_online'], seen['gss_forget'], seen['gss_prior_mass']) == (True, 0.95, 0.5)
    seen.clear()
    with pytest.raises(Stop):
        enhance_rttm.main(base)
    assert (seen['gss_online'], seen['gss_forget'], seen['gss_prior_mass']) == (False, 0.99, 1.0)


def test_methods_that_refuse_the_online_mixture_model(no_context, tmp_path):
    from pb_chime5_amd.core import get_enhancer
    enh = get_enhancer(gss_online=True)
    obs = np.zeros((4, 4096))
    act = {'P01': np.ones(4096, bool), 'Noise': np.ones(4096, bool)}
    with pytest.raises(NotImplementedError, match='enhance_observation_guided with gss_online'):
        enh.enhance_observation_guided(obs, {'P01': np.ones(19), 'Noise': np.ones(19)}, 'P01')
    with pytest.raises(NotImplementedError, match='enhance_observation_speakers with gss_online'):
        enh.enhance_observation_speakers(obs, act, ['P01'])
    with pytest.raises(NotImplementedError, match='enhance_example_speakers with gss_online'):
        enh.enhance_example_speakers({})
    with pytest.raises(NotImplementedError, match='enhance_observation_activity with gss_online'):
        enh.enhance_observation_activity(obs, act, 'P01')
    with pytest.raises(NotImplementedError, match='enhance_example_activity with gss_online'):
        enh.enhance_example_activity({})
    with pytest.raises(NotImplementedError, match='enhance_observation_blind with gss_online'):
        enh.enhance_observation_blind(obs, 2)
    with pytest.raises(NotImplementedError, match='with gss_online'):
        enh.enhance_recording_blind(obs, 2, window_samples=4096, hop_samples=2048)
    with pytest.raises(NotImplementedError, match='refined_rttm.* with gss_online'):
        enh.enhance_session('S02', tmp_path / 'audio', refined_rttm=True)
    assert not (tmp_path / 'audio').exists()


def test_session_takes_one_utterance_at_a_time(monkeypatch, tmp_path):
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import get_enhancer
    enh = get_enhancer(gss_online=True)
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


def test_fused_call_gets_the_settings(monkeypatch):
    from pb_chime5_amd import core, ops
    seen = {}

    def fake(obs, activity, target, start, end, **kw):
        seen.update(kw, target=target)
        return np.zeros(8)
    monkeypatch.setattr(ops, 'enhance_observation_gss_online', fake)

    def boom(*a, **k):
        raise AssertionError('another fused call')
    for name in ('enhance_observation', 'enhance_observation_wpe_online',
                 'enhance_observation_bf_online'):
        monkeypatch.setattr(ops, name, boom)

    class Ctx:
        def set_utterances_in_flight(self, n):
            pass
    monkeypatch.setattr(core.Enhancer, '_ctx', lambda self: Ctx())
    act = {'P01': np.ones(4096, bool), 'P02': np.ones(4096, bool), 'Noise': np.ones(4096, bool)}
    enh = core.get_enhancer(gss_online=True, gss_forget=0.9, gss_prior_mass=0.5,
                            bf_drop_context=False)
    enh.enhance_observation(np.zeros((4, 4096)), act, 'P02')
    assert [seen[k] for k in ('forget', 'prior_mass', 'target')] == [0.9, 0.5, 1]
    assert 'bf_online' not in seen and 'wpe_online' not in seen
    seen.clear()
    enh = core.get_enhancer(gss_online=True, bf_online=True, bf_forget=0.97, wpe_online=True,
                            wpe_alpha=0.99, wpe_tabs=4, bf_drop_context=False,
                            multiarray='outer_array_mics', wpe_per_array=True)
    enh.enhance_observation(np.zeros((4, 4096)), act, 'P01')
    assert [seen[k] for k in ('forget', 'prior_mass', 'bf_online', 'bf_forget', 'bf_loading',
                              'ref_channel', 'wpe_online', 'wpe_alpha', 'wpe_arrays')] == \
        [0.99, 1.0, True, 0.97, 1e-2, -1, True, 0.99, 2]
    assert seen['params'].wpe_taps == 4 and seen['params'].bf == 0
    enh = core.get_enhancer(gss_online=True, wpe_online=True, bf_drop_context=False)
    with pytest.raises(NotImplementedError, match='gss_online with wpe_online.*fused=False'):
        enh.enhance_observation(np.zeros((4, 4096)), act, 'P01')


def test_off_is_the_call_without_the_argument(monkeypatch):
    """get_enhancer(gss_online=False) routes as get_enhancer() does: the plain fused call, with the
    same parameter block."""
    from pb_chime5_amd import core, ops
    calls = []

    def fake(obs, activity, target, start, end, **kw):
        calls.append(bytes(kw['params']))
        return np.zeros(8)
    monkeypatch.setattr(ops, 'enhance_observation', fake)

    class Ctx:
        def set_utterances_in_flight(self, n):
            pass
    monkeypatch.setattr(core.Enhancer, '_ctx', lambda self: Ctx())
    act = {'P01': np.ones(4096, bool), 'Noise': np.ones(4096, bool)}
    for enh in (core.get_enhancer(bf_drop_context=False),
                core.get_enhancer(gss_online=False, bf_drop_context=False)):
        enh.enhance_observation(np.zeros((4, 4096)), act, 'P01')
    assert len(calls) == 2 and calls[0] == calls[1]
