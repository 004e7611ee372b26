"""Several targets of one stream on the GPU (gss_mvdr_online_targets, gss_istft_stream_targets,
gss_stream_block_targets, `StreamingEnhancer(targets=)`) against the single-target stream and
tests/stream_targets_reference.py: the bits of every row against the stream of that target,
partition invariance, the fused block against the single-target stage operators, parity with the
composed NumPy references, the operators alone, the edges, the C-ABI errors and the workspace
hygiene.  Every device run is made once and shared."""
import ctypes

import numpy as np
import pytest

import online_mvdr_reference as mref
import stream_reference as sr
import stream_targets_reference as tr

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -4
PATTERNS = (0x00, 0xFF)
PER_TARGET = ('target_mask', 'distortion_mask', 'X_hat')
_AXIS = dict(Obs=1, posterior=1, target_mask=1, distortion_mask=1, X_hat=1, acitivity_freq=1)
_AXIS_ONE = dict(Obs=1, posterior=1, target_mask=0, distortion_mask=0, X_hat=0, acitivity_freq=1)
ALL = sorted(tr.CELLS)


def enhancer(name, ctx, **kw):
    from pb_chime5_amd.streaming import StreamingEnhancer
    W, H, D, A, taps, delay, K, N, wpe = tr.CELLS[name]
    s = tr.SETTINGS
    args = dict(ref_channel=s['ref_channel'], stft_size=W, stft_shift=H, wpe=wpe, wpe_taps=taps,
                wpe_delay=delay, wpe_alpha=s['wpe_alpha'], wpe_arrays=A, gss_forget=s['gss_forget'],
                gss_prior_mass=s['gss_prior_mass'], bf_forget=s['bf_forget'],
                bf_loading=s['bf_loading'], ctx=ctx)
    args.update(kw)
    if 'target' not in args:
        args.setdefault('targets', tr.TARGETS[name])
    return StreamingEnhancer(D, K, **args)


def states_of(enh):
    """{'wpe.inv_cov': array, ..., 'bf.phi_x': (S,F,D,D), 'tails': (S, W - H)}."""
    host = enh.to_host()
    out = {}
    for stage in ('stream', 'wpe', 'em', 'bf'):
        for k, v in (host[stage] or {}).items():
            out[f'{stage}.{k}'] = np.asarray(v)
    if 'tails' in host:
        out['tails'] = host['tails']
    return out


def feed(enh, x, activity, cuts, after_block=None):
    """x in blocks of ``cuts`` and the flush through ``enh`` -> samples, the taps over all frames,
    the final states, the fallback counts."""
    axis = _AXIS if enh.targets is not None else _AXIS_ONE
    outs, taps = [], []
    for i, (a, b) in enumerate(sr.blocks_of(x.shape[1], cuts)):
        y, d = enh.process(x[:, a:b], activity[:, a:b], debug=True)
        outs.append(y)
        if d is not None:
            taps.append(d)
        if after_block is not None:
            after_block(i, enh)
    y, d = enh.flush(debug=True)
    outs.append(y)
    if d is not None:
        taps.append(d)
    res = {k: np.concatenate([t[k] for t in taps], axis=axis[k]) for k in axis if k in taps[0]}
    res['x_hat'] = np.concatenate(outs, axis=-1)
    res['fallbacks'] = {k: (tuple(v) if isinstance(v, list) else v) for k, v in enh.fallbacks.items()}
    res['states'] = states_of(enh)
    assert enh.samples_out == enh.samples_in == x.shape[1] and enh.latency_samples == 0
    assert res['x_hat'].shape[-1] == x.shape[1]
    return res


_RUNS = {}


def run(ctx, name, part='one', **kw):
    """The cell's scene through a stream of its targets (``target=``: of that one target)."""
    key = (name, part, tuple(sorted(kw.items())))
    if key not in _RUNS:
        x, activity = tr.scene(name, tr.seed_of(name))
        _RUNS[key] = feed(enhancer(name, ctx, **kw), x, activity, tr.partitions(name)[part])
    return _RUNS[key]


def same_bits(a, b, what):
    assert sorted(a) == sorted(b), (what, sorted(a), sorted(b))
    for k in a:
        if isinstance(a[k], dict):
            same_bits(a[k], b[k], f'{what} {k}')
        elif isinstance(a[k], np.ndarray):
            assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k)
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


def row_is_the_single_stream(multi, s, one, what):
    """Row s of a run of several targets against the run of that target alone."""
    assert np.array_equal(multi['x_hat'][s], one['x_hat']), (what, 'x_hat')
    for k in PER_TARGET:
        assert multi[k].shape[1:] == one[k].shape and np.array_equal(multi[k][s], one[k]), (what, k)
    for k in ('Obs', 'posterior', 'acitivity_freq'):
        assert np.array_equal(multi[k], one[k]), (what, k)
    for k, v in one['states'].items():
        if k.startswith('bf.'):
            assert np.array_equal(multi['states'][k][s], v), (what, k)
        elif k == 'stream.ola_tail':      # (the tails of the targets live in a buffer of their own)
            assert np.array_equal(multi['states']['tails'][s], v), (what, k)
            assert not np.any(multi['states'][k]), (what, k)
        else:
            assert np.array_equal(multi['states'][k], v), (what, k)
    assert multi['fallbacks']['mvdr_targets'][s] == one['fallbacks']['mvdr'], what
    assert multi['fallbacks']['cacgmm'] == one['fallbacks']['cacgmm'], what


# ------------------------------------------------------------------ 1. bits against single targets
@pytest.mark.parametrize('name', ALL)
def test_row_s_has_the_bits_of_the_single_target_stream(gpu_ctx, name):
    multi = run(gpu_ctx, name)
    S = len(tr.TARGETS[name])
    assert multi['x_hat'].shape == (S, tr.CELLS[name][7])
    for s, target in enumerate(tr.TARGETS[name]):
        row_is_the_single_stream(multi, s, run(gpu_ctx, name, target=target), (name, target))
    assert multi['fallbacks']['mvdr'] == sum(multi['fallbacks']['mvdr_targets'])


# ------------------------------------------------------------------ 2. partition invariance
@pytest.mark.parametrize('name,part', [(n, p) for n in ('a', 'f', 'm') for p in tr.partitions(n)
                                       if p != 'one'])
def test_every_partition_has_the_bits_of_the_single_block(gpu_ctx, name, part):
    same_bits(run(gpu_ctx, name, part), run(gpu_ctx, name), f'{name} {part}')


# ------------------------------------------------------------------ 3. fused against the stages
@pytest.mark.parametrize('name', ['a', 'f', 'n'])
@pytest.mark.parametrize('postfilter', [None, 'mask_mul'])
def test_the_fused_block_has_the_bits_of_the_single_target_operators(gpu_ctx, name, postfilter):
    fused = run(gpu_ctx, name, 'borders', postfilter=postfilter)
    stages = run(gpu_ctx, name, 'borders', postfilter=postfilter, fused=False)
    same_bits(fused, stages, f'{name} {postfilter} fused vs stages')
    if postfilter:
        plain = run(gpu_ctx, name, 'borders', postfilter=None)
        assert not np.array_equal(fused['X_hat'], plain['X_hat'])
        for k, v in plain['states'].items():      # the postfilter touches the output alone
            assert np.array_equal(fused['states'][k], v) == (k != 'tails'), k


# ------------------------------------------------------------------ 4. parity with NumPy
_STATE_NAMES = {'wpe.P': 'wpe.inv_cov', 'wpe.G': 'wpe.filter', 'wpe.hist': 'wpe.history',
                'em.s': 'em.s', 'em.n': 'em.n', 'bf.phi_x': 'bf.phi_x', 'bf.phi_n': 'bf.phi_n'}


@pytest.mark.parametrize('name', ALL)
def test_parity_with_the_composed_references(gpu_ctx, name):
    got = run(gpu_ctx, name)
    x_hat, taps, states = tr.reference(name, tr.seed_of(name))
    S = len(tr.TARGETS[name])
    errs = {'gamma': sr.rel_err(got['posterior'].transpose(2, 0, 1), taps['gamma'])}
    x_errs = []
    for s in range(S):
        errs[f'X_hat[{s}]'] = sr.rel_err(got['X_hat'][s], taps['X_hat'][s])
        x_errs.append(tr.abs_rel_err(got['x_hat'][s], x_hat[s]))
    for k, v in tr.state_arrays(states).items():
        if k.startswith('bf.'):
            for s in range(S):
                errs[f'{k}[{s}]'] = sr.rel_err(got['states'][_STATE_NAMES[k]][s], v[s])
        else:
            errs[k] = sr.rel_err(got['states'][_STATE_NAMES[k]], v)
    print(f'{name}: rel err {errs}, |x_hat| {x_errs}')
    assert got['fallbacks'] == {'mvdr': 0, 'cacgmm': 0, 'mvdr_targets': (0,) * S}
    assert taps['fallbacks'] == ((0,) * S, 0)
    assert max(errs.values()) < tr.TOL, (name, errs)
    assert max(x_errs) < tr.X_TOL


# ------------------------------------------------------------------ 5. ordering and S = 1
def test_one_target_in_a_list_is_the_single_target_stream(gpu_ctx):
    multi, one = run(gpu_ctx, 'a', targets=(1,)), run(gpu_ctx, 'a', target=1)
    assert multi['x_hat'].shape == (1, tr.CELLS['a'][7])
    row_is_the_single_stream(multi, 0, one, 'S = 1')


@pytest.mark.parametrize('part', ['hops', 'borders'])
def test_one_target_in_a_list_is_the_single_target_stream_whatever_the_cuts(gpu_ctx, part):
    """In blocks of one hop and in uneven ones: samples, X_hat, masks and the beamformer sums of
    a ``targets=(t,)`` stream are those of the ``target=t`` stream, its tails[0] that one's
    ola_tail (both are the S = 1 form of one block path)."""
    multi, one = run(gpu_ctx, 'a', part, targets=(1,)), run(gpu_ctx, 'a', part, target=1)
    row_is_the_single_stream(multi, 0, one, f'S = 1, {part}')


def test_the_rows_follow_the_order_of_the_targets(gpu_ctx):
    a, b = run(gpu_ctx, 'a', targets=(2, 0)), run(gpu_ctx, 'a', targets=(0, 2))
    for k in PER_TARGET + ('x_hat',):
        assert np.array_equal(a[k], b[k][::-1]), k
    for k, v in a['states'].items():
        swapped = k.startswith('bf.') or k == 'tails'
        assert np.array_equal(v, b['states'][k][::-1] if swapped else b['states'][k]), k
    assert not np.array_equal(a['x_hat'][0], a['x_hat'][1])


# ------------------------------------------------------------------ 6. the operators alone
@pytest.mark.parametrize('D', [4, 12, 24, 32])
def test_mvdr_online_targets_has_the_bits_of_the_single_target_operator(gpu_ctx, D):
    """Random posteriors of three classes, blocks of unequal length through carried states, with
    the filters, with and without the postfilter: every NR form of the kernel."""
    from pb_chime5_amd import ops
    F, T, K, targets, blocks = 5, 37, 3, (2, 0), (1, 20, 16)
    rng = np.random.default_rng([D, F, T])
    Y = mref.crandn(rng, D, T, F)
    gamma = rng.random((K, T, F)) + 0.05
    gamma /= gamma.sum(axis=0)
    kw = dict(forget=0.97, ref_channel=D - 1, ban=True)
    for postfilter in (None, 'mask_mul'):
        states = [ops.OnlineMVDRState.fresh(F, D, 1e-2, ctx=gpu_ctx) for _ in targets]
        singles = [ops.OnlineMVDRState.fresh(F, D, 1e-2, ctx=gpu_ctx) for _ in targets]
        for a, b in sr.blocks_of(T, blocks):
            X, W, fallbacks = ops.mvdr_souden_online_targets(
                Y[:, a:b], gamma[:, a:b], targets, states=states, postfilter=postfilter,
                return_filters=True, return_fallbacks=True, **kw)
            assert X.shape == (2, b - a, F) and W.shape == (2, b - a, F, D) and fallbacks == [0, 0]
            for s, target in enumerate(targets):
                mx, mn = ops.masks_from_posteriors(gamma[:, a:b], target, ctx=gpu_ctx)
                X1, W1 = ops.mvdr_souden_online_from_masks(Y[:, a:b], mx, mn, state=singles[s],
                                                           return_filters=True, **kw)
                if postfilter:
                    X1 = (X1.view(np.float64).reshape(X1.shape + (2,))
                          * mx[..., None]).reshape(X1.shape[0], -1).view(np.complex128)
                assert np.array_equal(X[s], X1), (D, postfilter, a, s)
                assert np.array_equal(W[s], W1), (D, postfilter, a, s)
        for state, single in zip(states, singles):
            same_bits(state.to_host(), single.to_host(), (D, postfilter))
        assert not np.array_equal(X[0], X[1])


def test_mvdr_online_targets_in_more_than_one_round_of_waves(gpu_ctx):
    """F = 513, S = 4, D = 24: the 2 052 waves of cell r, on random posteriors of five classes
    that tell every target apart, two blocks through carried states."""
    from pb_chime5_amd import ops
    F, T, D, K, targets = 513, 6, 24, 5, (3, 0, 4, 1)
    rng = np.random.default_rng([F, D, K])
    Y = mref.crandn(rng, D, T, F)
    gamma = rng.random((K, T, F)) + 0.05
    gamma /= gamma.sum(axis=0)
    kw = dict(forget=0.97, ref_channel=0, ban=True)
    states = [ops.OnlineMVDRState.fresh(F, D, 1e-2, ctx=gpu_ctx) for _ in targets]
    singles = [ops.OnlineMVDRState.fresh(F, D, 1e-2, ctx=gpu_ctx) for _ in targets]
    rows = []
    for a, b in ((0, 4), (4, T)):
        X, fallbacks = ops.mvdr_souden_online_targets(Y[:, a:b], gamma[:, a:b], targets,
                                                      states=states, return_fallbacks=True, **kw)
        assert X.shape == (4, b - a, F) and fallbacks == [0] * 4
        for s, target in enumerate(targets):
            mx, mn = ops.masks_from_posteriors(gamma[:, a:b], target, ctx=gpu_ctx)
            X1 = ops.mvdr_souden_online_from_masks(Y[:, a:b], mx, mn, state=singles[s], **kw)
            assert np.array_equal(X[s], X1), (a, s)
        rows.append(X)
    for state, single in zip(states, singles):
        same_bits(state.to_host(), single.to_host(), 'two rounds of waves')
    X = np.concatenate(rows, axis=1)
    for s in range(4):
        for r in range(s):
            assert not np.array_equal(X[s], X[r]), (s, r)
            assert not np.array_equal(states[s].to_host()['phi_x'], states[r].to_host()['phi_x'])


def test_one_target_falls_back_and_another_does_not(gpu_ctx):
    from pb_chime5_amd import ops
    Y, gamma, state, beta, targets, counts = tr.fallback_scene()
    Obs, posterior = mref.to_dtf(Y), np.ascontiguousarray(gamma.transpose(1, 2, 0))
    states = [ops.OnlineMVDRState.from_host(state, ctx=gpu_ctx) for _ in targets]
    X, fallbacks = ops.mvdr_souden_online_targets(Obs, posterior, targets, states=states, forget=beta,
                                                  ban=True, return_fallbacks=True)
    assert tuple(fallbacks) == counts and counts[0] == 0 < counts[1]
    assert gpu_ctx.last_mvdr_online_fallbacks() == sum(counts)
    for s, target in enumerate(targets):
        mx, mn = tr.masks(gamma, target)
        want, _, after, count = mref.online_mvdr(Y, mx, mn, beta, 0, True, state=state)
        assert count == counts[s]
        assert sr.rel_err(X[s], want.T) < tr.TOL
        assert sr.rel_err(states[s].to_host()['phi_n'], after['phi_n']) < tr.TOL
    assert not np.any(X[1][:3]) and np.all(X[1][3:] != 0) and np.all(X[0][3:] != 0)


@pytest.mark.parametrize('name', ['a', 'r'])
def test_istft_stream_targets_has_the_bits_of_istft_stream(gpu_ctx, name):
    """Whatever the cuts; cell r: the power-of-two transform at 1024."""
    from pb_chime5_amd import ops
    W, H = tr.CELLS[name][:2]
    X = tr.reference(name, tr.seed_of(name))[1]['X_hat'][:3, :24]
    S, T, F = X.shape
    X = X + 1j * np.arange(1, S + 1)[:, None, None] * X        # (three different signals)
    outs = {}
    for part, cuts in (('one', (T,)), ('borders', (1, 2, 1, 0, 3, T - 7)),
                       ('random', sr.random_cuts(T, 5)), ('frames', (1,) * T)):
        state = ops.StreamState.fresh(1, 0, W, H, ctx=gpu_ctx)
        tails = ops.StreamTails.fresh(S, W, H, ctx=gpu_ctx)
        ops.stft_stream(np.zeros((1, T * H)), None, state=state)    # (the analysis side leads)
        outs[part] = np.concatenate([ops.istft_stream_targets(X[:, a:b], state=state, tails=tails)
                                     for a, b in sr.blocks_of(T, cuts)], axis=1)
        assert state.frames_out == T and not np.any(state.to_host()['ola_tail'])
        outs[part + ' tails'] = tails.to_host()['tails']
    assert outs['one'].shape == (S, T * H - (W - H))
    for s in range(S):
        state = ops.StreamState.fresh(1, 0, W, H, ctx=gpu_ctx)
        ops.stft_stream(np.zeros((1, T * H)), None, state=state)
        assert np.array_equal(ops.istft_stream(X[s], state=state), outs['one'][s]), s
        assert np.array_equal(state.to_host()['ola_tail'], outs['one tails'][s]), s
    for part in ('borders', 'random', 'frames'):
        assert np.array_equal(outs[part], outs['one']), (name, part)
        assert np.array_equal(outs[part + ' tails'], outs['one tails']), (name, part)


# ------------------------------------------------------------------ 7. carried-over behaviours
def test_a_pcm16_stream_is_the_float64_stream_of_the_same_values(gpu_ctx):
    x, activity = tr.scene('a')
    pcm = np.round(x / np.max(np.abs(x)) * 20000).astype(np.int16)
    a = feed(enhancer('a', gpu_ctx), pcm, activity, tr.partitions('a')['borders'])
    b = feed(enhancer('a', gpu_ctx), pcm / 32768, activity, (x.shape[1],))
    same_bits(a, b, 'pcm16')


@pytest.mark.parametrize('fused', [True, False])
def test_a_checkpoint_continues_in_a_new_context(gpu_ctx, fused):
    from pb_chime5_amd._capi import Context
    x, activity = tr.scene('a')
    cuts = tr.partitions('a')['random']
    saved = {}

    def after(i, enh):
        if i == 2:
            saved.update(enh.to_host())
    first = feed(enhancer('a', gpu_ctx, fused=fused), x, activity, cuts, after)
    same_bits(first, run(gpu_ctx, 'a'), 'the run that was saved')
    other = Context(0)
    try:
        with pytest.raises(ValueError, match='targets'):
            enhancer('a', other, targets=(0, 1)).from_host(saved)
        enh = enhancer('a', other, fused=fused).from_host(saved)
        blocks = sr.blocks_of(x.shape[1], cuts)[3:]
        outs = [enh.process(x[:, a:b], activity[:, a:b]) for a, b in blocks] + [enh.flush()]
        done = int(saved['samples_out'])
        assert np.array_equal(np.concatenate(outs, axis=1), first['x_hat'][:, done:])
        same_bits(states_of(enh), first['states'], 'checkpoint')
        assert enh.fallbacks == {k: list(v) if isinstance(v, tuple) else v
                                 for k, v in first['fallbacks'].items()}
        del enh
    finally:
        other.close()


def test_reset_gives_the_first_run_again(gpu_ctx):
    x, activity = tr.scene('a')
    cuts = tr.partitions('a')['borders']
    enh = enhancer('a', gpu_ctx)
    first = feed(enh, x, activity, cuts)
    with pytest.raises(RuntimeError, match='flush'):
        enh.process(x[:, :10], activity[:, :10])
    enh.reset()
    same_bits(feed(enh, x, activity, cuts), first, 'reset')
    same_bits(first, run(gpu_ctx, 'a'), 'reset vs the shared run')


def test_an_empty_block_is_a_no_op(gpu_ctx):
    x, activity = tr.scene('a')
    enh = enhancer('a', gpu_ctx)
    enh.process(x[:, :100], activity[:, :100])
    before = states_of(enh)
    out = enh.process(x[:, :0], activity[:, :0])
    assert out.shape == (3, 0)
    same_bits(states_of(enh), before, 'n = 0')


def test_a_stream_shorter_than_one_hop(gpu_ctx):
    W, H, D = tr.CELLS['a'][:3]
    x, activity = tr.scene('a')
    enh = enhancer('a', gpu_ctx)
    assert enh.process(x[:, :H - 3], activity[:, :H - 3]).shape == (3, 0)
    assert enh.latency_samples == H - 3
    out = enh.flush()
    want = tr.compose_whole('a', x[:, :H - 3], activity[:, :H - 3], tr.TARGETS['a'])[0]
    assert out.shape == (3, H - 3)
    for s in range(3):
        assert tr.abs_rel_err(out[s], want[s]) < tr.X_TOL, s


# ------------------------------------------------------------------ 8. C-ABI errors
def test_errors_before_any_launch(gpu_ctx):
    from pb_chime5_amd import _capi, ops
    W, H, D, A, taps, delay, K, N, wpe = tr.CELLS['a']
    F, n, S = W // 2 + 1, 200, 2
    ctx, lib = gpu_ctx, gpu_ctx.lib
    x, activity = tr.scene('a')
    ops._prepare_windows(ctx, W, H)
    st = ops.StreamState.fresh(D, K, W, H, ctx=ctx)
    ws = ops.OnlineWPEState.fresh(F, A, D // A, taps, delay, ctx=ctx)
    em = ops.OnlineCACGMMState.fresh(F, K, D, 1.0, ctx=ctx)
    bfs = [ops.OnlineMVDRState.fresh(F, D, 1e-2, ctx=ctx) for _ in range(S)]
    tails = ops.StreamTails.from_host({'tails': np.full((S, W - H), 3.0)}, ctx=ctx)
    x_d = ctx.to_device(x[:, :n])
    a_d = ctx.to_device(activity[:, :n].astype(np.uint8))
    m = ops.stream_num_samples_out(0, n, W, H)
    o_d = ctx.to_device(np.full((S, m), 7.0))

    def snapshot():
        out = {f'{i}.{k}': v for i, s in enumerate([st, ws, em, tails] + bfs)
               for k, v in s.to_host().items()}
        out['out'] = ctx.to_host(o_d, (S, m), np.float64)
        return out
    before = snapshot()
    table = lambda states: (_capi.GssMvdrOnlineState * len(states))(*(s.struct() for s in states))
    other = lambda **kw: ops.OnlineMVDRState.fresh(kw.get('F', F), kw.get('D', D), 1e-2, ctx=ctx)
    shared = _capi.GssMvdrOnlineState(phi_x=bfs[0].bufs['phi_n'].ptr, phi_n=bfs[1].bufs['phi_n'].ptr,
                                      F=F, D=D)

    def call(params=None, cfg=None, stream=st, wpe_state=ws, em_state=em, bf=table(bfs),
             tails_p=tails.ptr, x_p=x_d.ptr, act_p=a_d.ptr, count=n, out_p=o_d.ptr, targets=(0, 2),
             num=None, **cfg_kw):
        p = params if params is not None else ops.make_params(
            stft_size=W, stft_shift=H, wpe_taps=taps, wpe_delay=delay)
        c = dict(wpe_alpha=0.999, em_forget=0.99, bf_forget=0.99, ref_channel=0)
        c.update(cfg_kw)
        ref = ctypes.byref
        return lib.gss_stream_block_targets(
            ctx.handle, ref(p) if p is not False else None,
            ref(_capi.GssStreamCfg(**c)) if cfg is not False else None,
            ref(stream.struct()) if stream is not None else None,
            ref(wpe_state.struct()) if wpe_state is not None else None,
            ref(em_state.struct()) if em_state is not None else None, bf,
            ctypes.c_void_p(tails_p), ctypes.c_void_p(x_p), 0, ctypes.c_void_p(act_p), count,
            (ctypes.c_int32 * len(targets))(*targets) if targets is not None else None,
            len(targets) if num is None else num, ctypes.c_void_p(out_p), None)
    mk = lambda **kw: ops.make_params(stft_size=W, stft_shift=H, wpe_taps=taps, wpe_delay=delay, **kw)
    cases = {
        'S = 0': (dict(num=0), INVALID),
        'S = 9': (dict(targets=tuple(range(9)), bf=table((bfs * 5)[:9])), INVALID),
        'targets NULL': (dict(targets=None, num=2), INVALID),
        'states NULL': (dict(bf=None), INVALID),
        'tails NULL': (dict(tails_p=None), INVALID),
        'the tails are the stream state\'s own': (dict(tails_p=st.bufs['ola_tail'].ptr), INVALID),
        'target = K': (dict(targets=(0, K)), INVALID),
        'target < 0': (dict(targets=(-1, 0)), INVALID),
        'the same target twice': (dict(targets=(1, 1)), INVALID),
        'the same state twice': (dict(bf=table([bfs[0], bfs[0]])), INVALID),
        'two states sharing a buffer': (
            dict(bf=(_capi.GssMvdrOnlineState * 2)(bfs[1].struct(), shared)), INVALID),
        'D of a state': (dict(bf=table([bfs[0], other(D=D + 1)])), INVALID),
        'F of a state': (dict(bf=table([other(F=F + 1), bfs[1]])), INVALID),
        # what gss_stream_block refuses keeps its code
        'params NULL': (dict(params=False), INVALID),
        'cfg NULL': (dict(cfg=False), INVALID),
        'stream state NULL': (dict(stream=None), INVALID),
        'em state NULL': (dict(em_state=None), INVALID),
        'x NULL': (dict(x_p=None), INVALID),
        'out NULL': (dict(out_p=None), INVALID),
        'activity NULL for a guided stream': (dict(act_p=None), INVALID),
        'K of the CACGMM state': (dict(em_state=ops.OnlineCACGMMState.fresh(F, K + 1, D, 1.0, ctx=ctx)),
                                  INVALID),
        'ref_channel < 0': (dict(ref_channel=-1), INVALID),
        'ref_channel = D': (dict(ref_channel=D), INVALID),
        'bf_forget > 1': (dict(bf_forget=1.5), INVALID),
        'wpe_alpha NaN': (dict(wpe_alpha=float('nan')), INVALID),
        'stft_fading = 0': (dict(params=mk(stft_fading=False)), UNSUPPORTED),
        'bf != 0': (dict(params=mk(bf='sum')), UNSUPPORTED),
        'a WPE state with wpe = 0': (dict(params=mk(wpe=False)), INVALID),
        'no WPE state with wpe = 1': (dict(wpe_state=None), INVALID),
        'n < 0': (dict(count=-1), INVALID),
    }
    for what, (kw, status) in cases.items():
        got = call(**kw)
        assert got == status, (what, got, lib.gss_last_error(ctx.handle))
        assert st.received == 0 and st.frames_out == 0, what
    same_bits(snapshot(), before, 'after the refused calls')
    # the two stages on their own
    ref = ctypes.byref
    Y_d, g_d = ctx.empty(16 * F * D * 8), ctx.empty(8 * F * K * 8)
    X_d = ctx.empty(16 * S * F * 8)
    cfg = _capi.GssBfOnline(forget=0.99, loading=1.0, ref_channel=0, wpe_online=0, wpe_alpha=1.0)

    def mvdr(targets=(0, 2), states=table(bfs), gamma_p=g_d.ptr, c=cfg, num=None, classes=K):
        return lib.gss_mvdr_online_targets(
            ctx.handle, ctypes.c_void_p(Y_d.ptr), F, 8, D, ctypes.c_void_p(gamma_p), classes,
            (ctypes.c_int32 * len(targets))(*targets), len(targets) if num is None else num, 1,
            ref(c) if c is not None else None, states, 0, None, None, ctypes.c_void_p(X_d.ptr), None)
    window = _capi.GssBfOnline(forget=0.99, loading=1.0, ref_channel=-1, wpe_online=0, wpe_alpha=1.0)
    for what, kw, status in (('S = 0', dict(num=0), INVALID), ('target = K', dict(targets=(K, 0)), INVALID),
                             ('twice', dict(targets=(2, 2)), INVALID), ('states NULL', dict(states=None), INVALID),
                             ('gamma NULL', dict(gamma_p=None), INVALID), ('cfg NULL', dict(c=None), INVALID),
                             ('ref_channel = -1', dict(c=window), INVALID),
                             ('aliased', dict(states=table([bfs[1], bfs[1]])), INVALID),
                             ('K = 9', dict(classes=9), UNSUPPORTED)):
        got = mvdr(**kw)
        assert got == status, (what, got, lib.gss_last_error(ctx.handle))
    o2 = ctypes.c_void_p(o_d.ptr)
    assert lib.gss_istft_stream_targets(ctx.handle, ctypes.c_void_p(X_d.ptr), 1, S, ref(st.struct()),
                                        ctypes.c_void_p(tails.ptr), o2) == INVALID    # (no frame analysed yet)
    assert lib.gss_istft_stream_targets(ctx.handle, ctypes.c_void_p(X_d.ptr), 0, 0, ref(st.struct()),
                                        ctypes.c_void_p(tails.ptr), o2) == INVALID
    assert lib.gss_istft_stream_targets(ctx.handle, ctypes.c_void_p(X_d.ptr), 0, S, ref(st.struct()),
                                        None, o2) == INVALID
    counts = (ctypes.c_int64 * 8)()
    assert lib.gss_last_mvdr_online_fallbacks_targets(ctx.handle, None, 1) == INVALID
    assert lib.gss_last_mvdr_online_fallbacks_targets(ctx.handle, counts, 0) == INVALID
    same_bits(snapshot(), before, 'after the refused stage calls')
    # and the same arguments, unrefused, run
    assert call() == 0
    assert st.received == n and st.frames_out == n // H
    assert lib.gss_last_mvdr_online_fallbacks_targets(ctx.handle, counts, S) == 0
    assert lib.gss_last_mvdr_online_fallbacks_targets(ctx.handle, counts, S + 1) == INVALID
    after = snapshot()
    assert not np.array_equal(after['out'], before['out']) and np.all(np.isfinite(after['out']))
    assert not np.array_equal(after['3.tails'], before['3.tails'])


# ------------------------------------------------------------------ 9. workspace hygiene
@pytest.fixture(scope='module')
def hctx():
    """The module's own context: the session's `gpu_ctx` is never put into the debug mode."""
    from pb_chime5_amd._capi import Context
    ctx = Context(0)
    yield ctx
    ctx.close()


def _flat(res):
    out = {k: v for k, v in res.items() if k not in ('states', 'fallbacks')}
    out.update({f'state {k}': v for k, v in res['states'].items()})
    out.update({f'fallbacks {k}': v for k, v in res['fallbacks'].items()})
    return out


def _bits(value):
    if isinstance(value, np.ndarray):
        return value.dtype.str, value.shape, np.ascontiguousarray(value).tobytes()
    return value


@pytest.mark.parametrize('name', ['a', 'f'])
def test_workspace_hygiene(hctx, gpu_ctx, name):
    """No guard violation under either poison pattern and the bits of the plain run."""
    x, activity = tr.scene(name, tr.seed_of(name))
    cuts = tr.partitions(name)['borders']
    plain = _flat(run(gpu_ctx, name))
    for pattern in PATTERNS:
        hctx.debug_workspace(pattern)
        try:
            got = _flat(feed(enhancer(name, hctx), x, activity, cuts))
            count, text, _ = hctx.debug_workspace_report()
        finally:
            hctx.debug_workspace(None)
        print(f'stream targets {name} [0x{pattern:02X}]: {count} guard violations {text}')
        assert count == 0, f'stream targets {name} [0x{pattern:02X}]: {text}'
        differ = [k for k in sorted(plain) if _bits(got[k]) != _bits(plain[k])]
        assert sorted(got) == sorted(plain) and not differ, (name, hex(pattern), differ)
