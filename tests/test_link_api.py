"""Cross-window linking and the recording driver without a GPU: the NumPy reference's own
properties, the window plan, the start table and the cross-fade of `pb_chime5_amd.recording`
against the independent forms of tests/link_reference.py, what the periodic scene shows, every
argument error of the new front doors (before any device work) and the binding's table."""
import itertools

import numpy as np
import pytest

import link_reference as lr


@pytest.fixture
def no_context(monkeypatch):
    """Any attempt to create or fetch a device context fails the test."""
    from pb_chime5_amd import _capi, ops

    def boom(*a, **k):
        raise AssertionError('device work before the argument check')
    monkeypatch.setattr(_capi, 'default_context', boom)
    monkeypatch.setattr(ops, 'default_context', boom)
    monkeypatch.setattr(_capi.Context, '__init__', boom)


# ------------------------------------------------------------------ the reference's properties
@pytest.mark.parametrize('K', (2, 3, 5, 8))
def test_reference_recovers_a_known_permutation(K):
    rng = np.random.default_rng(K)
    F, T = 6, 80
    prev = rng.uniform(size=(F, K, T)) ** 3
    prev /= prev.sum(axis=1, keepdims=True)
    hidden = rng.permutation(K)
    cur = np.empty_like(prev)
    cur[:, hidden, :] = prev + 0.05 * rng.uniform(size=prev.shape)      # cur[hidden[a]] ~ prev[a]
    mapping, S, margin = lr.link(prev, cur)
    assert mapping.dtype == np.int32 and sorted(mapping.tolist()) == list(range(K))
    np.testing.assert_array_equal(mapping, hidden)
    assert margin > 0.01
    assert np.all(S >= 0) and np.all(S <= 1 + 1e-12)
    # the linked table continues prev: linking it again is the identity
    again, _, _ = lr.link(prev, cur[:, mapping, :])
    np.testing.assert_array_equal(again, np.arange(K))
    # frame ranges: the same frames somewhere else in longer tables
    prev_long = np.concatenate([rng.uniform(size=(F, K, 7)), prev], axis=2)
    cur_long = np.concatenate([rng.uniform(size=(F, K, 3)), cur, rng.uniform(size=(F, K, 4))], axis=2)
    m2, S2, _ = lr.link(prev_long, cur_long, 7, 3, T)
    np.testing.assert_array_equal(m2, hidden)
    assert S2.tobytes() == S.tobytes()


def test_reference_tie_rule_and_zero_rows():
    rng = np.random.default_rng(1)
    prev = rng.uniform(size=(3, 3, 20))
    cur = rng.uniform(size=(3, 3, 20))
    cur[:, 2, :] = cur[:, 0, :]                         # classes 0 and 2 of cur are one row
    S = lr.scores(prev, cur)
    assert S[:, 0].tobytes() == S[:, 2].tobytes()       # identical rows, identical bits
    mapping, best, second = lr.best_permutation(S)
    assert best == second                               # an exact tie ...
    twin = mapping.copy()
    i0, i2 = int(np.where(mapping == 0)[0][0]), int(np.where(mapping == 2)[0][0])
    twin[i0], twin[i2] = 2, 0
    assert mapping.tolist() < twin.tolist()             # ... takes the lexicographically smaller
    # all zero: every total is 0, the identity is the first candidate
    mapping, best, second = lr.best_permutation(np.zeros((4, 4)))
    assert mapping.tolist() == [0, 1, 2, 3] and best == second == 0.0
    # a zero row scores 0 against everything and takes what the others leave
    cur = rng.uniform(size=(3, 3, 20))
    prev = cur[:, [1, 2, 0], :].copy()
    prev[:, 1, :] = 0.0
    mapping, S, _ = lr.link(prev, cur)
    assert np.all(S[1] == 0.0) and mapping.tolist() == [1, 2, 0]
    # K = 1
    mapping, S, margin = lr.link(rng.uniform(size=(2, 1, 5)), rng.uniform(size=(2, 1, 5)))
    assert mapping.tolist() == [0] and margin == np.inf and S.shape == (1, 1)


def test_parity_cells_follow_the_margin_rule():
    kinds = [c[-1] for c in lr.CELLS]
    assert 'tie' in kinds and 'zero_row' in kinds
    assert {c[1] for c in lr.CELLS} == set(range(1, 9))
    for cell in lr.CELLS:
        F, K, T_prev, T_cur, L, pb, cb, kind = cell
        assert pb + L <= T_prev and cb + L <= T_cur
        mapping, S, margin = lr.parity_reference(cell)
        prev, cur, hidden = lr.parity_input(cell)
        if kind == 'one_frame':
            assert np.all(S == 1.0) and margin == 0.0 and mapping.tolist() == list(range(K))
        elif kind == 'tie':
            assert margin == 0.0
            totals = sorted({sum(S[a, p[a]] for a in range(K))
                             for p in itertools.permutations(range(K))})
            assert totals[-1] - totals[-2] >= lr.PARITY_MIN_MARGIN
        elif K > 1:
            assert margin >= lr.PARITY_MIN_MARGIN, cell
        if kind == 'plain':
            np.testing.assert_array_equal(mapping, hidden)


# ------------------------------------------------------------------ plan, start table, cross-fade
@pytest.mark.parametrize('N,want', [
    (50, [(0, 50)]), (99, [(0, 99)]), (100, [(0, 100)]), (159, [(0, 159)]),
    (160, [(0, 100), (60, 160)]), (161, [(0, 100), (60, 161)]), (219, [(0, 100), (60, 219)]),
    (220, [(0, 100), (60, 160), (120, 220)]), (250, [(0, 100), (60, 160), (120, 250)])])
def test_window_plan(N, want):
    from pb_chime5_amd import recording
    assert recording.window_plan(N, 100, 60) == want == lr.window_plan(N, 100, 60)
    for (s, e) in want[:-1]:
        assert e - s == 100
    assert want[-1][1] == N and (N < 100 or 100 <= want[-1][1] - want[-1][0] < 160)


def test_recording_plan_frames():
    from pb_chime5_amd import ops, recording
    plan = recording.check_recording(160000, 2, 64000, 32000, 256, 64)
    assert list(plan.windows) == lr.window_plan(160000, 64000, 32000)
    T = ops.stft_frames(64000, 256, 64, True)
    assert (plan.hop_frames, plan.shared_frames, plan.edge_frames) == (500, T - 500, 3)
    assert plan.overlap_samples == 32000
    assert plan.link_frames == ((503, T - 3), (3, T - 503))
    # frame t of window w + 1 has the sample support of frame t + H of window w
    one = recording.check_recording(5000, 2, 64000, 32000, 256, 64)
    assert list(one.windows) == [(0, 5000)] and one.shared_frames == 0


def test_stitch_weights_sum_to_one_and_keep_a_constant():
    from pb_chime5_amd import recording
    r = recording.fade_weights(8)
    np.testing.assert_array_equal(r, (np.arange(8) + 0.5) / 8)
    np.testing.assert_allclose(r + r[::-1], 1.0, rtol=0, atol=1e-16)
    windows = lr.window_plan(250, 100, 60)
    pieces = [np.full((2, e - s), 3.25) for s, e in windows]
    offsets = [s for s, _ in windows]
    out = recording.stitch(pieces, offsets, 250)
    assert out.shape == (2, 250)
    np.testing.assert_allclose(out, 3.25, rtol=0, atol=1e-15)
    rng = np.random.default_rng(0)
    pieces = [rng.standard_normal((2, e - s)) for s, e in windows]
    out = recording.stitch(pieces, offsets, 250)
    np.testing.assert_allclose(out, lr.stitch(pieces, offsets, 250), rtol=0, atol=1e-15)
    np.testing.assert_array_equal(out, lr.stitch_by_blend(pieces, offsets, 250))
    # outside the overlaps the one window's samples are taken unchanged
    np.testing.assert_array_equal(out[:, :60], pieces[0][:, :60])
    np.testing.assert_array_equal(out[:, 100:120], pieces[1][:, 40:60])
    np.testing.assert_array_equal(out[:, 160:], pieces[2][:, 40:])
    np.testing.assert_array_equal(recording.stitch([pieces[0]], [0], 100), pieces[0])
    with pytest.raises(ValueError):
        recording.stitch(pieces, offsets, 251)
    with pytest.raises(ValueError):
        recording.stitch([np.zeros(100), np.zeros(50)], [0, 10], 60)    # an end that does not ascend
    # frames of the STFT's padding that three windows hold: a fade window by window, weights 1
    frames = recording.stitch([np.full(1003, 2.5)] * 4, [0, 500, 1000, 1500], 2503)
    np.testing.assert_allclose(frames, 2.5, rtol=0, atol=1e-15)
    rnd = [rng.standard_normal((3, 1003)) for _ in range(4)]
    np.testing.assert_array_equal(recording.stitch(rnd, [0, 500, 1000, 1500], 2503),
                                  lr.stitch_by_blend(rnd, [0, 500, 1000, 1500], 2503))


def test_start_table():
    from pb_chime5_amd import ops, recording
    K, T, H, L = 3, 40, 25, 15
    for w in (0, 1, 4):
        fresh = recording.start_table(K, T, 7, w, 'fresh')
        assert fresh.tobytes() == ops.blind_initialization(K, T, 7 + w).tobytes()
    assert (recording.start_table(K, T, 7, 0, 'carry').tobytes()
            == ops.blind_initialization(K, T, 7).tobytes())
    prior = np.random.default_rng(2).uniform(size=(K, 40))
    prior /= prior.sum(axis=0) * 1.01                    # (a prior's columns sum to about 1)
    table = recording.start_table(K, T, 7, 2, 'carry', prior, H, L)
    np.testing.assert_allclose(table.sum(axis=0), 1.0, rtol=0, atol=1e-15)
    np.testing.assert_allclose(table[:, :L], prior[:, H:] / prior[:, H:].sum(axis=0), atol=1e-15)
    # (every column is divided by its sum again: the untouched ones move in the last bit at most)
    np.testing.assert_allclose(table[:, L:], ops.blind_initialization(K, T, 9)[:, L:], rtol=0,
                               atol=1e-15)
    np.testing.assert_allclose(table, lr.start_table(K, T, 7, 2, 'carry', prior, H, L), atol=1e-15)
    with pytest.raises(ValueError):
        recording.start_table(K, T, 7, 1, 'warm')
    with pytest.raises(ValueError):
        recording.start_table(K, T, 7, 1, 'carry', prior[:2], H, L)


# ------------------------------------------------------------------ what the method is for
@pytest.mark.parametrize('seed', lr.SCENE_SEEDS)
def test_periodic_scene_needs_the_link_and_the_link_holds(seed):
    """Conditions on the inputs, shown by the reference alone: with window starts of their own
    the classes are renumbered in some window, after linking each speaker keeps one class
    through all windows, and every link is decided by a margin of at least 0.1."""
    obs, acts = lr.periodic_scene(seed)
    assert obs.shape == (4, 160000) and acts.shape == (2, 160000)
    truth = lr.frame_truth(acts)
    fresh = lr.recording_reference(seed, 'fresh')
    carry = lr.recording_reference(seed, 'carry')
    n, K = fresh['mappings'].shape
    assert (n, K) == (4, 3) and fresh['windows'] == [(0, 64000), (32000, 96000), (64000, 128000),
                                                    (96000, 160000)]
    print(f'seed {seed}: fresh mappings {fresh["mappings"].tolist()} margins '
          f'{np.round(fresh["margins"][1:], 3).tolist()}; carry mappings '
          f'{carry["mappings"].tolist()} margins {np.round(carry["margins"][1:], 3).tolist()}')
    assert np.any(fresh['mappings'] != np.arange(K))
    for run in (fresh, carry):
        assert min(run['margins'][1:]) >= lr.MIN_MARGIN
        whole = lr.best_classes(run['prior'], truth)
        assert whole[0][0] != whole[1][0]
        for w, prior in enumerate(run['priors']):
            span = slice(w * run['H'], w * run['H'] + run['frames'][w])
            mine = lr.best_classes(prior, truth[:, span])
            assert [k for k, _ in mine] == [k for k, _ in whole], (w, mine, whole)
    np.testing.assert_array_equal(carry['mappings'], np.tile(np.arange(K), (n, 1)))


def test_golden_file_is_the_reference():
    """tests/golden/link_periodic.npz (what the GPU tests compare with) against a fresh run."""
    from conftest import GOLDEN
    golden = np.load(GOLDEN / 'link_periodic.npz')
    fresh = lr.golden_arrays()
    assert sorted(golden.files) == sorted(fresh)
    for name, want in fresh.items():
        if want.dtype.kind == 'f':
            np.testing.assert_allclose(golden[name], want, rtol=0, atol=1e-9, err_msg=name)
        else:
            np.testing.assert_array_equal(golden[name], want, err_msg=name)


def test_scene_seed_follows_the_stability_rule():
    for start in ('fresh', 'carry'):
        moved = lr.reference_movement(lr.SCENE_SEED, start)
        print(f'periodic scene seed {lr.SCENE_SEED} {start}: the reference scores move {moved:.1e}')
        assert moved * lr.STABILITY_MARGIN <= lr.MIN_MARGIN


# ------------------------------------------------------------------ argument errors
def _tables(K=3, T=20, F=5):
    rng = np.random.default_rng(0)
    return rng.uniform(size=(K, T, F)), rng.uniform(size=(K, T + 4, F))


@pytest.mark.parametrize('change,match', [
    (dict(prev=np.zeros((3, 20))), r'\(K,T,F\)'),
    (dict(cur=np.zeros((3, 20, 5), complex)), 'not real'),
    (dict(cur=np.zeros((4, 24, 5))), 'classes'),
    (dict(cur=np.zeros((3, 24, 6))), 'frequencies'),
    (dict(prev=np.zeros((9, 20, 5)), cur=np.zeros((9, 24, 5))), 'outside'),
    (dict(), 'covers 20 frames, cur_frames 24'),
    (dict(prev_frames=(0, 21), cur_frames=(0, 21)), 'prev_frames'),
    (dict(prev_frames=(5, 5), cur_frames=(0, 1)), 'prev_frames'),
    (dict(prev_frames=(0, 10), cur_frames=(-1, 9)), 'cur_frames'),
    (dict(prev_frames=(0, 10), cur_frames=(20, 30)), 'cur_frames'),
    (dict(prev_frames=(0.0, 10), cur_frames=(0, 10)), 'pair of integers'),
    (dict(prev_frames=3, cur_frames=(0, 10)), 'pair of integers'),
    (dict(prev_frames=(0, 10, 2), cur_frames=(0, 10)), 'pair of integers'),
])
def test_link_posteriors_refuses_before_any_device_work(no_context, change, match):
    from pb_chime5_amd import ops
    prev, cur = _tables()
    kw = dict(prev=prev, cur=cur, prev_frames=None, cur_frames=None)
    kw.update(change)
    with pytest.raises(ValueError, match=match):
        ops.link_posteriors(kw.pop('prev'), kw.pop('cur'), **kw)


@pytest.mark.parametrize('obs,init,match', [
    (np.zeros(4000), np.ones((3, 19)), r'\(D,N\)'),
    (np.zeros((4, 4000), complex), np.ones((3, 19)), r'\(D,N\)'),
    (np.zeros((1, 4000)), np.ones((3, 19)), 'channels'),
    (np.zeros((33, 4000)), np.ones((3, 19)), 'channels'),
    (np.zeros((4, 0)), np.ones((3, 19)), 'no samples'),
    (np.zeros((4, 4000)), np.ones(19), r'\(K,T\)'),
    (np.zeros((4, 4000)), np.ones((20, 19)), 'classes'),
    (np.zeros((4, 4000)), np.ones((3, 18)), 'frames'),
])
def test_separate_observation_refuses_before_any_device_work(no_context, obs, init, match):
    from pb_chime5_amd import ops
    assert ops.stft_frames(4000, 1024, 256, True) == 19
    with pytest.raises(ValueError, match=match):
        ops.separate_observation(obs, init)


REFUSED = [('bf_segment_frames', dict(bf_segment_frames=64)),
           ('bf_null_interferer', dict(bf_null_interferer=True)),
           ('channel_keep', dict(channel_keep=3)),
           ('wpdSouden', dict(bf='wpdSouden_ban')),
           ('wpe_per_array', dict(wpe_per_array=True, multiarray=True)),
           ('wpe_online', dict(wpe_online=True))]


@pytest.mark.parametrize('option,kw', REFUSED, ids=[str(k) for _, k in REFUSED])
def test_fused_front_doors_refuse_the_options_they_are_not_built_for(no_context, option, kw):
    from pb_chime5_amd import core
    enh = core.get_enhancer(**kw)
    with pytest.raises(NotImplementedError, match=option):
        enh.enhance_observation_blind(np.zeros((4, 4000)), 2, fused=True)
    with pytest.raises(NotImplementedError, match=option):
        enh.enhance_recording_blind(np.zeros((4, 40000)), 2, window_samples=16384,
                                    hop_samples=8192)


def test_fused_window_refuses_the_aligned_method_and_context_frames(no_context):
    from pb_chime5_amd import core
    enh = core.get_enhancer()
    with pytest.raises(NotImplementedError, match='aligned'):
        enh.enhance_observation_blind(np.zeros((4, 4000)), 2, fused=True, method='aligned')
    ex = {'start': {'original': 0}, 'start_orig': {'original': 500},
          'end_orig': {'original': 3500}, 'end': {'original': 4000}}
    with pytest.raises(NotImplementedError, match='context frames'):
        enh.enhance_observation_blind(np.zeros((4, 4000)), 2, ex=ex, fused=True)
    with pytest.raises(ValueError):
        enh.enhance_observation_blind(np.zeros((4, 4000)), 0, fused=True)
    with pytest.raises(ValueError, match=r'\(D,N\)'):
        enh.enhance_observation_blind(np.zeros(4000), 2, fused=True)


@pytest.mark.parametrize('kw,match', [
    (dict(num_speakers=0), 'num_speakers'), (dict(num_speakers=8), 'num_speakers'),
    (dict(num_speakers=2.0), 'num_speakers'), (dict(num_speakers=True), 'num_speakers'),
    (dict(window_samples=16000), 'multiple of stft_shift'),
    (dict(hop_samples=8000), 'multiple of stft_shift'),
    (dict(window_samples=8192, hop_samples=8192), 'hop_samples = 8192 < window_samples'),
    (dict(window_samples=16640, hop_samples=8192), '<= 2 hop_samples'),
    (dict(window_samples=8448, hop_samples=8192), 'nothing to link'),
    (dict(window_samples=0), 'window_samples'), (dict(hop_samples=-256), 'hop_samples'),
    (dict(window_samples=16384.0), 'window_samples'),
    (dict(start='warm'), 'start'), (dict(seed=-1), 'seed'), (dict(seed=0.5), 'seed'),
])
def test_recording_driver_refuses_before_any_device_work(no_context, kw, match):
    from pb_chime5_amd import core
    args = dict(num_speakers=2, window_samples=16384, hop_samples=8192)
    args.update(kw)
    enh = core.get_enhancer()
    with pytest.raises(ValueError, match=match):
        enh.enhance_recording_blind(np.zeros((4, 40000)), args.pop('num_speakers'), **args)
    with pytest.raises(ValueError, match=r'\(D,N\)'):
        enh.enhance_recording_blind(np.zeros(40000), 2, window_samples=16384, hop_samples=8192)
    with pytest.raises(ValueError, match='channels'):
        enh.enhance_recording_blind(np.zeros((1, 40000)), 2, window_samples=16384,
                                    hop_samples=8192)


def test_binding_declares_the_new_entries():
    from pb_chime5_amd import _capi, ops
    for name, nargs in (('gss_cacgmm_link', 12), ('gss_cacgmm_link_gather', 7),
                        ('gss_separate_observation', 12)):
        assert len(_capi.SIGNATURES[name][1]) == nargs
    # the fused window call is no one-target entry: not in the table of those
    assert all('separate' not in str(v) for v in ops._FUSED_ENTRIES.values())
    assert _capi.GSS_ABI_VERSION == 7
