"""The sample-block stream on the GPU (gss_stft_stream, gss_istft_stream, gss_stream_block,
`StreamingEnhancer`) against tests/stream_reference.py: the two ends against `ops.stft` and
`oracle.istft`, partition invariance of the whole stream, the fused block against the stage
operators and against the operators on the whole signal, parity with the composed NumPy
references, the edges, the C-ABI errors and the workspace hygiene.  Every device run is made once
and shared."""
import ctypes

import numpy as np
import pytest

import gss_oracle as oracle
import stream_reference as sr

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -4
PATTERNS = (0x00, 0xFF)
TAPS = ('Obs', 'posterior', 'target_mask', 'distortion_mask', 'X_hat')
_AXIS = dict(Obs=1, posterior=1, target_mask=0, distortion_mask=0, X_hat=0, acitivity_freq=1)
ALL = sorted(sr.CELLS)


def enhancer(name, ctx, **kw):
    from pb_chime5_amd.streaming import StreamingEnhancer
    W, H, D, A, taps, delay, K, N, wpe = sr.CELLS[name]
    s = sr.SETTINGS
    args = dict(target=s['target'], ref_channel=s['ref_channel'], stft_size=W, stft_shift=H, wpe=wpe,
                wpe_taps=taps, wpe_delay=delay, wpe_alpha=s['wpe_alpha'], wpe_arrays=A,
                gss_forget=s['gss_forget'], gss_prior_mass=s['gss_prior_mass'],
                bf_forget=s['bf_forget'], bf_loading=s['bf_loading'], ctx=ctx)
    args.update(kw)
    if 'model' in args:
        return StreamingEnhancer(**args)
    return StreamingEnhancer(D, K, **args)


def states_of(enh):
    """{'wpe.inv_cov': array, ...} and the counters of the stream state."""
    host = enh.to_host()
    out = {}
    for stage in ('stream', 'wpe', 'em', 'bf'):
        for k, v in (host[stage] or {}).items():
            out[f'{stage}.{k}'] = np.asarray(v)
    return out


def feed(enh, x, activity, cuts, after_block=None):
    """x in blocks of ``cuts`` and the flush through ``enh`` -> samples, the taps over all frames,
    the final states, the fallback counts."""
    outs, taps = [], []
    for i, (a, b) in enumerate(sr.blocks_of(x.shape[1], cuts)):
        y, d = enh.process(x[:, a:b], None if activity is None else activity[:, a:b], debug=True)
        outs.append(y)
        if d is not None:
            taps.append(d)
        if after_block is not None:
            after_block(i, enh)
    y, d = enh.flush(debug=True)
    outs.append(y)
    if d is not None:
        taps.append(d)
    keys = [k for k in _AXIS if k in taps[0]]
    res = {k: np.concatenate([t[k] for t in taps], axis=_AXIS[k]) for k in keys}
    res['x_hat'] = np.concatenate(outs)
    res['fallbacks'] = (enh.fallbacks['mvdr'], enh.fallbacks['cacgmm'])
    res['states'] = states_of(enh)
    assert enh.samples_out == enh.samples_in == x.shape[1] and enh.latency_samples == 0
    return res


_RUNS = {}


def run(ctx, name, part, fused=True):
    key = (name, part, fused)
    if key not in _RUNS:
        x, activity = sr.scene(name, sr.seed_of(name))
        _RUNS[key] = feed(enhancer(name, ctx, fused=fused), x, activity, sr.partitions(name)[part])
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


# ------------------------------------------------------------------ 1. the stage operators
@pytest.mark.parametrize('name', ['a', 'b', 'e', 'g'])
def test_stft_stream_has_the_bits_of_stft(gpu_ctx, name):
    """float64 and int16 blocks: the frames over all blocks are `ops.stft` on the whole signal,
    the frame activity is `ops.activity_time_to_frequency_device` on the whole track."""
    from pb_chime5_amd import ops
    W, H, D, A, taps, delay, K, N, wpe = sr.CELLS[name]
    x, activity = sr.scene(name)
    pcm = np.round(x / np.max(np.abs(x)) * 20000).astype(np.int16)
    for signal in (x, pcm):
        whole = ops.stft(signal / 32768 if signal.dtype == np.int16 else signal, W, H, fading=True,
                         ctx=gpu_ctx)
        actf = ops.activity_time_to_frequency_device(activity, W, H, True, ctx=gpu_ctx)
        for part, cuts in sr.partitions(name).items():
            if part == 'hops' and signal is pcm:
                continue
            state = ops.StreamState.fresh(D, K, W, H, ctx=gpu_ctx)
            Ys, As = [], []
            blocks = [(signal[:, a:b], activity[:, a:b]) for a, b in sr.blocks_of(N, cuts)]
            n_flush = ops.stream_flush_samples(N, W, H)
            blocks.append((np.zeros((D, n_flush), signal.dtype), np.zeros((K, n_flush), bool)))
            for blk, act in blocks:
                Y, f = ops.stft_stream(blk, act, state=state)
                Ys.append(Y), As.append(f)
            assert state.received == N + n_flush
            Y = np.concatenate(Ys, axis=1)
            assert Y.shape == whole.shape and np.array_equal(Y, whole), (name, part, signal.dtype)
            assert np.array_equal(np.concatenate(As, axis=1), actf[:, :Y.shape[1]]), (name, part)


@pytest.mark.parametrize('name', ['a', 'e', 'g'])
def test_istft_stream_matches_the_oracle_whatever_the_cuts(gpu_ctx, name):
    from pb_chime5_amd import ops
    W, H, D, A, taps, delay, K, N, wpe = sr.CELLS[name]
    X = sr.reference(name)[1]['X_hat']
    T = X.shape[0]
    want = oracle.istft(X, W, H, fading=True)
    outs = {}
    for part, cuts in (('one', (T,)), ('borders', (1, 2, 1, 0, 3, T - 7)),
                       ('random', sr.random_cuts(T, 5)), ('frames', (1,) * T)):
        state = ops.StreamState.fresh(1, 0, W, H, ctx=gpu_ctx)
        ops.stft_stream(np.zeros((1, T * H)), None, state=state)    # (the analysis side leads)
        outs[part] = np.concatenate([ops.istft_stream(X[a:b], state=state)
                                     for a, b in sr.blocks_of(T, cuts)])
        assert state.frames_out == T
    err = sr.rel_err(outs['one'], want[:len(outs['one'])])
    print(f'{name}: istft_stream vs oracle.istft {err:.2e}')
    assert len(outs['one']) == T * H - (W - H) and err < sr.ISTFT_TOL
    for part, out in outs.items():
        assert np.array_equal(out, outs['one']), (name, part)


# ------------------------------------------------------------------ 2. partition invariance
@pytest.mark.parametrize('name,part', [(n, p) for n in ALL for p in sr.partitions(n) if p != 'one'])
def test_every_partition_has_the_bits_of_the_single_block(gpu_ctx, name, part):
    one, cut = run(gpu_ctx, name, 'one'), run(gpu_ctx, name, part)
    same_bits(cut, one, f'{name} {part}')


# ------------------------------------------------------------------ 3. the stream is the composition
_WHOLE = {}


def whole_operators(ctx, name):
    """The stage operators once on the whole signal, from the fresh states of a stream."""
    from pb_chime5_amd import ops
    if name not in _WHOLE:
        W, H, D, A, taps, delay, K, N, wpe = sr.CELLS[name]
        s, F = sr.SETTINGS, W // 2 + 1
        x, activity = sr.scene(name, sr.seed_of(name))
        Obs = ops.stft(x, W, H, fading=True, ctx=ctx)
        if wpe:
            Obs = ops.wpe_online_dtf(Obs, taps, delay, s['wpe_alpha'], arrays=A,
                                     state=ops.OnlineWPEState.fresh(F, A, D // A, taps, delay, ctx=ctx))
        actf = ops.activity_time_to_frequency_device(activity, W, H, True, ctx=ctx)[:, :Obs.shape[1]]
        posterior = ops.cacgmm_posteriors_online(
            Obs, actf, forget=s['gss_forget'],
            state=ops.OnlineCACGMMState.fresh(F, K, D, s['gss_prior_mass'], ctx=ctx))
        mx, mn = ops.masks_from_posteriors(posterior, s['target'], ctx=ctx)
        X_hat = ops.mvdr_souden_online_from_masks(
            Obs, mx, mn, ban=True, forget=s['bf_forget'], ref_channel=s['ref_channel'],
            state=ops.OnlineMVDRState.fresh(F, D, s['bf_loading'], ctx=ctx))
        _WHOLE[name] = dict(Obs=Obs, posterior=posterior, target_mask=mx, distortion_mask=mn,
                            X_hat=X_hat)
    return _WHOLE[name]


@pytest.mark.parametrize('name', ALL)
def test_the_fused_block_is_the_composition_of_the_operators(gpu_ctx, name):
    W, H, D, A, taps, delay, K, N, wpe = sr.CELLS[name]
    fused, stages = run(gpu_ctx, name, 'borders'), run(gpu_ctx, name, 'borders', fused=False)
    same_bits(fused, stages, f'{name} fused vs stages')
    whole = whole_operators(gpu_ctx, name)
    for k in TAPS:
        assert np.array_equal(fused[k], whole[k]), (name, k)
    want = oracle.istft(whole['X_hat'], W, H, fading=True)[:N]
    err = sr.rel_err(fused['x_hat'], want)
    print(f'{name}: stream samples vs oracle.istft of the operators\' X_hat {err:.2e}')
    assert err < sr.ISTFT_TOL


# ------------------------------------------------------------------ 4. parity with NumPy
_STATE_NAMES = {'wpe.P': 'wpe.inv_cov', 'wpe.G': 'wpe.filter', 'wpe.hist': 'wpe.history',
                'em.s': 'em.s', 'em.n': 'em.n', 'bf.phi_x': 'bf.phi_x', 'bf.phi_n': 'bf.phi_n'}


@pytest.mark.parametrize('name', ALL)
def test_parity_with_the_composed_references(gpu_ctx, name):
    got = run(gpu_ctx, name, 'one')
    x_hat, taps, states = sr.reference(name, sr.seed_of(name))
    errs = {'gamma': sr.rel_err(got['posterior'].transpose(2, 0, 1), taps['gamma']),
            'X_hat': sr.rel_err(got['X_hat'], taps['X_hat'])}
    for k, v in sr.state_arrays(states).items():
        errs[k] = sr.rel_err(got['states'][_STATE_NAMES[k]], v)
    x_err = sr.abs_rel_err(got['x_hat'], x_hat)
    print(f'{name}: rel err {errs}, |x_hat| {x_err:.2e}')
    assert got['fallbacks'] == taps['fallbacks'] == (0, 0)
    assert max(errs.values()) < sr.TOL, (name, errs)
    assert x_err < sr.X_TOL


def test_a_long_stream_keeps_every_factor(gpu_ctx):
    """8 128 frames of the starved-class scene (stream_reference.long_scene) in blocks of 10 000
    samples: no stage falls back, the output is finite, and the fused block has the bits of the
    stage operators."""
    from pb_chime5_amd.streaming import StreamingEnhancer
    p, s = sr.LONG, sr.SETTINGS
    x, activity = sr.long_scene()
    N = x.shape[1]
    cuts = (p['block'],) * (N // p['block'])
    assert sum(cuts) == N
    res = {}
    for fused in (True, False):
        enh = StreamingEnhancer(p['D'], p['K'], target=s['target'], ref_channel=s['ref_channel'],
                                stft_size=p['W'], stft_shift=p['H'], wpe=True, wpe_taps=p['taps'],
                                wpe_delay=p['delay'], wpe_alpha=s['wpe_alpha'], wpe_arrays=1,
                                gss_forget=s['gss_forget'], gss_prior_mass=s['gss_prior_mass'],
                                bf_forget=s['bf_forget'], bf_loading=s['bf_loading'], fused=fused,
                                ctx=gpu_ctx)
        outs = [enh.process(x[:, a:b], activity[:, a:b]) for a, b in sr.blocks_of(N, cuts)]
        outs.append(enh.flush())
        res[fused] = dict(x_hat=np.concatenate(outs), states=states_of(enh),
                          fallbacks=dict(enh.fallbacks))
        assert enh.samples_out == enh.samples_in == N
        assert all(v == 0 for v in enh.fallbacks.values()), (fused, enh.fallbacks)
    x_hat = res[True]['x_hat']
    assert x_hat.shape == (N,) and np.all(np.isfinite(x_hat)) and np.any(x_hat != 0)
    assert all(np.all(np.isfinite(v)) for v in res[True]['states'].values()
               if v.dtype.kind in 'fc')
    S = res[True]['states']['em.s']
    print(f'long stream: {oracle.stft_frames(N, p["W"], p["H"], fading=True)} frames, fallbacks {res[True]["fallbacks"]}, '
          f'cond(S_k) at the end up to {np.max(np.linalg.cond(S)):.1e}, n_k down to '
          f'{res[True]["states"]["em.n"].min():.3f}')
    same_bits(res[True], res[False], 'long stream fused vs stages')


# ------------------------------------------------------------------ 5. edges
def test_an_empty_block_is_a_no_op(gpu_ctx):
    x, activity = sr.scene('a')
    enh = enhancer('a', gpu_ctx)
    enh.process(x[:, :100], activity[:, :100])
    before = states_of(enh)
    out = enh.process(x[:, :0], activity[:, :0])
    assert out.shape == (0,)
    same_bits(states_of(enh), before, 'n = 0')


def test_a_stream_shorter_than_one_hop(gpu_ctx):
    W, H, D = sr.CELLS['a'][:3]
    x, activity = sr.scene('a')
    enh = enhancer('a', gpu_ctx)
    assert enh.process(x[:, :H - 3], activity[:, :H - 3]).shape == (0,)
    assert enh.latency_samples == H - 3
    out = enh.flush()
    want = sr.compose_whole('a', x[:, :H - 3], activity[:, :H - 3])[0]
    assert out.shape == (H - 3,) and sr.abs_rel_err(out, want) < sr.X_TOL


def test_digital_silence_mid_stream(gpu_ctx):
    """2 W zeros in the middle: the WPE and CACGMM states keep their bits over the frames that see
    nothing but zeros, and the stream equals the composition."""
    W, H, D, A, taps, delay, K, N, wpe = sr.CELLS['a']
    x, activity = sr.scene('a')
    x = np.array(x)
    lo = 640
    x[:, lo:lo + 2 * W] = 0.0
    # a block whose frames, and the taps + delay frames before them that the WPE's buffer still
    # holds, cover zeros only: frame t covers [t H - (W - H), t H + H)
    quiet = (lo + W - H + (taps + delay) * H, lo + 2 * W)
    assert quiet[0] % H == 0 and quiet[1] % H == 0 and quiet[0] < quiet[1]
    cuts = (quiet[0], quiet[1] - quiet[0], N - quiet[1])
    seen = {}

    def after(i, enh):
        seen[i] = states_of(enh)
    cut = feed(enhancer('a', gpu_ctx), x, activity, cuts, after)
    for k in seen[0]:
        if k.startswith(('wpe.inv_cov', 'wpe.filter', 'em.')):
            assert np.array_equal(seen[0][k], seen[1][k]), k
    one = feed(enhancer('a', gpu_ctx), x, activity, (N,))
    same_bits(cut, one, 'silence')
    stages = feed(enhancer('a', gpu_ctx, fused=False), x, activity, cuts)
    same_bits(cut, stages, 'silence, stages')


def test_a_pcm16_stream_is_the_float64_stream_of_the_same_values(gpu_ctx):
    x, activity = sr.scene('a')
    N = x.shape[1]
    pcm = np.round(x / np.max(np.abs(x)) * 20000).astype(np.int16)
    cuts = sr.partitions('a')['borders']
    a = feed(enhancer('a', gpu_ctx), pcm, activity, cuts)
    b = feed(enhancer('a', gpu_ctx), pcm / 32768, activity, (N,))
    same_bits(a, b, 'pcm16')


def test_a_checkpoint_continues_in_a_new_context(gpu_ctx):
    from pb_chime5_amd._capi import Context
    x, activity = sr.scene('a')
    cuts = sr.partitions('a')['random']
    saved = {}

    def after(i, enh):
        if i == 2:
            saved.update(enh.to_host())
    first = feed(enhancer('a', gpu_ctx), x, activity, cuts, after)
    other = Context(0)
    try:
        enh = enhancer('a', other).from_host(saved)
        blocks = sr.blocks_of(x.shape[1], cuts)[3:]
        outs = [enh.process(x[:, a:b], activity[:, a:b]) for a, b in blocks] + [enh.flush()]
        done = int(saved['samples_out'])
        assert np.array_equal(np.concatenate(outs), first['x_hat'][done:])
        same_bits(states_of(enh), first['states'], 'checkpoint')
        del enh
    finally:
        other.close()


def test_a_model_stream_without_activity(gpu_ctx):
    """The second half of cell a from a model fitted on the first half: no activity, equal to the
    stage operators."""
    from pb_chime5_amd import ops
    W, H, D, A, taps, delay, K, N, wpe = sr.CELLS['a']
    x, activity = sr.scene('a')
    half = N // 2
    Obs = ops.stft(x[:, :half], W, H, fading=True, ctx=gpu_ctx)
    actf = ops.activity_time_to_frequency_device(activity[:, :half], W, H, True, ctx=gpu_ctx)
    init, mask = ops.guidance_from_activity(actf[:, :Obs.shape[1]])
    model = ops.cacgmm_fit(Obs, init, mask, iterations=5, ctx=gpu_ctx)
    cuts = sr.random_cuts(N - half, 9)
    fused = feed(enhancer('a', gpu_ctx, model=model, gss_prior_mass=50.0), x[:, half:], None, cuts)
    stages = feed(enhancer('a', gpu_ctx, model=model, gss_prior_mass=50.0, fused=False),
                  x[:, half:], None, cuts)
    same_bits(fused, stages, 'model stream')
    assert np.max(fused['posterior']) > 0.9 and np.min(fused['posterior']) < 0.1
    with pytest.raises(ValueError, match='activity'):
        enhancer('a', gpu_ctx, model=model).process(x[:, :10], activity[:, :10])


def test_reset_gives_the_first_run_again(gpu_ctx):
    x, activity = sr.scene('a')
    cuts = sr.partitions('a')['borders']
    enh = enhancer('a', gpu_ctx)
    first = feed(enh, x, activity, cuts)
    with pytest.raises(RuntimeError, match='flush'):
        enh.process(x[:, :10], activity[:, :10])
    enh.reset()
    same_bits(feed(enh, x, activity, cuts), first, 'reset')
    same_bits(first, run(gpu_ctx, 'a', 'one'), 'reset vs the shared run')


# ------------------------------------------------------------------ 6. C-ABI errors
def test_errors_before_any_launch(gpu_ctx):
    from pb_chime5_amd import _capi, ops
    W, H, D, A, taps, delay, K, N, wpe = sr.CELLS['a']
    F, n = W // 2 + 1, 200
    ctx, lib = gpu_ctx, gpu_ctx.lib
    x, activity = sr.scene('a')
    ops._prepare_windows(ctx, W, H)
    st = ops.StreamState.fresh(D, K, W, H, ctx=ctx)
    ws = ops.OnlineWPEState.fresh(F, A, D // A, taps, delay, ctx=ctx)
    em = ops.OnlineCACGMMState.fresh(F, K, D, 1.0, ctx=ctx)
    bf = ops.OnlineMVDRState.fresh(F, D, 1e-2, ctx=ctx)
    x_d = ctx.to_device(x[:, :n])
    a_d = ctx.to_device(activity[:, :n].astype(np.uint8))
    o_d = ctx.to_device(np.full(n, 7.0))

    def snapshot():
        out = {f'{i}.{k}': v for i, s in enumerate((st, ws, em, bf)) for k, v in s.to_host().items()}
        out['out'] = ctx.to_host(o_d, (n,), np.float64)
        return out
    before = snapshot()

    def call(params=None, cfg=None, stream=st, wpe_state=ws, em_state=em, bf_state=bf, x_p=x_d.ptr,
             act_p=a_d.ptr, count=n, out_p=o_d.ptr, target=0, **cfg_kw):
        p = params if params is not None else ops.make_params(
            stft_size=W, stft_shift=H, wpe_taps=taps, wpe_delay=delay)
        c = dict(wpe_alpha=0.999, em_forget=0.99, bf_forget=0.99, ref_channel=0)
        c.update(cfg_kw)
        ref = ctypes.byref
        return lib.gss_stream_block(
            ctx.handle, ref(p) if p is not False else None,
            ref(_capi.GssStreamCfg(**c)) if cfg is not False else None,
            ref(stream.struct()) if stream is not None else None,
            ref(wpe_state.struct()) if wpe_state is not None else None,
            ref(em_state.struct()) if em_state is not None else None,
            ref(bf_state.struct()) if bf_state is not None else None,
            ctypes.c_void_p(x_p), 0, ctypes.c_void_p(act_p), count, target, ctypes.c_void_p(out_p),
            None)
    mk = lambda **kw: ops.make_params(stft_size=W, stft_shift=H, wpe_taps=taps, wpe_delay=delay, **kw)
    cases = {
        'params NULL': (dict(params=False), INVALID),
        'cfg NULL': (dict(cfg=False), INVALID),
        'stream state NULL': (dict(stream=None), INVALID),
        'em state NULL': (dict(em_state=None), INVALID),
        'bf state NULL': (dict(bf_state=None), INVALID),
        'x NULL': (dict(x_p=None), INVALID),
        'out NULL': (dict(out_p=None), INVALID),
        'activity NULL for a guided stream': (dict(act_p=None), INVALID),
        'D of the MVDR state': (dict(bf_state=ops.OnlineMVDRState.fresh(F, D + 1, 1e-2, ctx=ctx)),
                                INVALID),
        'D of the CACGMM state': (dict(em_state=ops.OnlineCACGMMState.fresh(F, K, D + 1, 1.0, ctx=ctx)),
                                  INVALID),
        'K of the CACGMM state': (dict(em_state=ops.OnlineCACGMMState.fresh(F, K + 1, D, 1.0, ctx=ctx)),
                                  INVALID),
        'ref_channel < 0': (dict(ref_channel=-1), INVALID),
        'ref_channel = D': (dict(ref_channel=D), INVALID),
        'target = K': (dict(target=K), INVALID),
        'em_forget = 0': (dict(em_forget=0.0), INVALID),
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
    # the two ends on their own
    Y_d = ctx.empty(16 * F * D * 64)
    ref = ctypes.byref
    assert lib.gss_stft_stream(ctx.handle, None, 0, ctypes.c_void_p(a_d.ptr), n, ref(st.struct()),
                               ctypes.c_void_p(Y_d.ptr), ctypes.c_void_p(Y_d.ptr)) == INVALID
    assert lib.gss_stft_stream(ctx.handle, ctypes.c_void_p(x_d.ptr), 2, ctypes.c_void_p(a_d.ptr), n,
                               ref(st.struct()), ctypes.c_void_p(Y_d.ptr),
                               ctypes.c_void_p(Y_d.ptr)) == INVALID
    assert lib.gss_istft_stream(ctx.handle, ctypes.c_void_p(Y_d.ptr), 1, ref(st.struct()),
                                ctypes.c_void_p(o_d.ptr)) == INVALID     # (no frame analysed yet)
    assert lib.gss_stream_init(ctx.handle, None) == INVALID
    same_bits(snapshot(), before, 'after the refused stage calls')
    # and the same arguments, unrefused, run
    assert call() == 0
    assert st.received == n and st.frames_out == n // H


# ------------------------------------------------------------------ 7. workspace hygiene
@pytest.fixture(scope='module')
def hctx():
    """The module's own context: the session's `gpu_ctx` is never put into the debug mode."""
    from pb_chime5_amd._capi import Context
    ctx = Context(0)
    yield ctx
    ctx.close()


def _flat(res):
    out = {k: v for k, v in res.items() if k != 'states'}
    out.update({f'state {k}': v for k, v in res['states'].items()})
    return out


def _bits(value):
    if isinstance(value, np.ndarray):
        return value.dtype.str, value.shape, np.ascontiguousarray(value).tobytes()
    return value


@pytest.mark.parametrize('name', ['a', 'f'])
def test_workspace_hygiene(hctx, gpu_ctx, name):
    """No guard violation under either poison pattern and the bits of the plain run."""
    x, activity = sr.scene(name, sr.seed_of(name))
    cuts = sr.partitions(name)['borders']
    plain = _flat(run(gpu_ctx, name, 'one'))
    for pattern in PATTERNS:
        hctx.debug_workspace(pattern)
        try:
            got = _flat(feed(enhancer(name, hctx), x, activity, cuts))
            count, text, _ = hctx.debug_workspace_report()
        finally:
            hctx.debug_workspace(None)
        print(f'stream {name} [0x{pattern:02X}]: {count} guard violations {text}')
        assert count == 0, f'stream {name} [0x{pattern:02X}]: {text}'
        differ = [k for k in sorted(plain) if _bits(got[k]) != _bits(plain[k])]
        assert sorted(got) == sorted(plain) and not differ, (name, hex(pattern), differ)
