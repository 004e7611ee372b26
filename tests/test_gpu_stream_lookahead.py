"""The sample-block stream with a filter look-ahead on the GPU (StreamingEnhancer(lookahead=),
gss_stream_block_lookahead): on the sizes and scenes of tests/stream_reference.py with L = 3, with
and without WPE -- every partition against the single block, the fused call against the stage
operators, the composed NumPy reference with the look-ahead beamformer in its place, several
targets, a checkpoint taken while frames are held, lookahead=0 against an enhancer built without
the argument, and the workspace hygiene.  Every device run is made once and shared."""
import numpy as np
import pytest

import online_mvdr_lookahead_reference as lr
import online_mvdr_reference as mr
import stream_reference as sr
from test_gpu_stream import _AXIS, _STATE_NAMES, enhancer, same_bits

pytestmark = pytest.mark.gpu

L = 3
NAMES = ['a', 'h']           # with and without WPE
PATTERNS = (0x00, 0xFF)


def states_of(enh):
    """{'wpe.inv_cov': array, ...}, the counters of the stream state, the delay lines and tails."""
    host = enh.to_host()
    out = {}
    for stage in ('stream', 'wpe', 'em', 'bf'):
        for k, v in (host[stage] or {}).items():
            out[f'{stage}.{k}'] = np.asarray(v)
    for s, hold in enumerate(host.get('holds', ())):
        for k, v in hold.items():
            out[f'hold{s}.{k}'] = np.asarray(v)
    if 'tails' in host:
        out['tails'] = np.asarray(host['tails'])
    return out


def feed(enh, x, activity, cuts, after_block=None):
    """x in blocks of ``cuts`` and the flush through ``enh`` -> samples, the taps over all frames,
    the samples every call returned, the final states, the fallback counts."""
    outs, taps = [], []
    for i, (a, b) in enumerate(sr.blocks_of(x.shape[1], cuts)):
        y, d = enh.process(x[:, a:b], None if activity is None else activity[:, a:b], debug=True)
        outs.append(y)
        if d is not None:
            taps.append(d)
        if after_block is not None:
            enh = after_block(i, enh) or enh
    y, d = enh.flush(debug=True)
    outs.append(y)
    if d is not None:
        taps.append(d)
    res = {k: np.concatenate([t[k] for t in taps if k in t], axis=_AXIS[k] + (enh.targets is not None
                                                                              and k in PER_TARGET))
           for k in _AXIS if any(k in t for t in taps)}
    res['x_hat'] = np.concatenate(outs, axis=-1)
    res['counts'] = [y.shape[-1] for y in outs]
    res['fallbacks'] = (enh.fallbacks['mvdr'], enh.fallbacks['cacgmm'])
    res['states'] = states_of(enh)
    assert enh.samples_out == enh.samples_in == x.shape[1] and enh.latency_samples == 0
    return res


PER_TARGET = ('target_mask', 'distortion_mask', 'X_hat')
_RUNS = {}


def run(ctx, name, part, fused=True, **kw):
    key = (name, part, fused, tuple(sorted(kw.items())))
    if key not in _RUNS:
        x, activity = sr.scene(name, sr.seed_of(name))
        enh = enhancer(name, ctx, fused=fused, lookahead=L, **kw)
        _RUNS[key] = feed(enh, x, activity, sr.partitions(name)[part])
    return _RUNS[key]


def without_counts(res):
    return {k: v for k, v in res.items() if k != 'counts'}


# ------------------------------------------------------------------ partitions, fused and stages
@pytest.mark.parametrize('name,part', [(n, p) for n in NAMES for p in sr.partitions(n) if p != 'one'])
def test_every_partition_has_the_bits_of_the_single_block(gpu_ctx, name, part):
    """Samples, taps and all final states, the delay lines included."""
    same_bits(without_counts(run(gpu_ctx, name, part)), without_counts(run(gpu_ctx, name, 'one')),
              f'{name} {part}')


@pytest.mark.parametrize('name', NAMES)
def test_sample_accounting(gpu_ctx, name):
    """A block returns the samples of the frames it releases: the stream's count, L hops late."""
    W, H, D, A, taps, delay, K, N, wpe = sr.CELLS[name]
    cuts = sr.partitions(name)['random']
    got = run(gpu_ctx, name, 'random')
    received, frames, want = 0, 0, []
    for n in cuts:
        Tn = sr.num_frames(received, n, W, H)
        released = max(0, min(L, frames) + Tn - L)
        out_before = frames - min(L, frames)
        want.append(sr.emitted((out_before + released) * H, W, H) - sr.emitted(out_before * H, W, H))
        received, frames = received + n, frames + Tn
    assert got['counts'][:-1] == want and sum(got['counts']) == N


@pytest.mark.parametrize('name', NAMES)
def test_fused_equals_the_stage_operators(gpu_ctx, name):
    for part in ('one', 'random'):
        same_bits(without_counts(run(gpu_ctx, name, part, fused=False)),
                  without_counts(run(gpu_ctx, name, 'one')), f'{name} {part} stages')


@pytest.mark.parametrize('name', NAMES)
def test_fused_equals_the_stage_operators_with_the_postfilter(gpu_ctx, name):
    """postfilter='mask_mul' through the fused entry: the mask of the OUTPUT frame, carried by the
    line across the blocks and into the release, against the stage operators, for one target and
    for two; and not the result without the postfilter."""
    x, activity = sr.scene(name, sr.seed_of(name))
    cuts = sr.partitions(name)['random']
    for kw in (dict(), dict(target=0, targets=(0, 2))):
        fused = feed(enhancer(name, gpu_ctx, lookahead=L, postfilter='mask_mul', **kw), x,
                     activity, cuts)
        stages = feed(enhancer(name, gpu_ctx, lookahead=L, postfilter='mask_mul', fused=False,
                               **kw), x, activity, (x.shape[1],))
        same_bits(without_counts(fused), without_counts(stages), f'{name} {kw} postfilter')
        if not kw:
            plain = run(gpu_ctx, name, 'one')
            assert not np.array_equal(fused['X_hat'], plain['X_hat'])
            want = np.empty_like(plain['X_hat'])
            want.real = plain['X_hat'].real * fused['target_mask']
            want.imag = plain['X_hat'].imag * fused['target_mask']
            assert np.array_equal(fused['X_hat'], want)


# ------------------------------------------------------------------ the composed reference
def composed(name):
    """`sr.reference` with the look-ahead beamformer in the place of the online MVDR: X_hat from
    the filters of the same recursion, then the oracle's synthesis."""
    import gss_oracle as oracle
    W, H, D, A, taps, delay, K, N, wpe = sr.CELLS[name]
    s = sr.SETTINGS
    _, t, states = sr.reference(name, sr.seed_of(name))
    _, Wf, _, fallbacks = mr.online_mvdr(t['Obs'], t['target_mask'], t['distortion_mask'],
                                         s['bf_forget'], s['ref_channel'], True,
                                         state=sr.fresh_states(name)['bf'])
    X = lr.one_shot(t['Obs'], Wf, L)[0]
    return oracle.istft(X.T, W, H, fading=True)[:N], np.ascontiguousarray(X.T), t, states


@pytest.mark.parametrize('name', NAMES)
def test_parity_with_the_composed_reference(gpu_ctx, name):
    got = run(gpu_ctx, name, 'one')
    x_hat, X_hat, taps, states = composed(name)
    errs = {'gamma': sr.rel_err(got['posterior'].transpose(2, 0, 1), taps['gamma']),
            'X_hat': sr.rel_err(got['X_hat'], X_hat)}
    for k, v in sr.state_arrays(states).items():
        errs[k] = sr.rel_err(got['states'][_STATE_NAMES[k]], v)
    x_err = sr.abs_rel_err(got['x_hat'], x_hat)
    print(f'{name}: rel err {errs}, |x_hat| {x_err:.2e}')
    assert got['fallbacks'] == (0, 0)
    assert max(errs.values()) < sr.TOL, (name, errs)
    assert x_err < sr.X_TOL


# ------------------------------------------------------------------ targets, checkpoint, L = 0
def test_target_rows_equal_the_one_target_streams(gpu_ctx):
    name = 'a'
    x, activity = sr.scene(name, sr.seed_of(name))
    both = feed(enhancer(name, gpu_ctx, lookahead=L, target=0, targets=(0, 2)), x, activity,
                sr.partitions(name)['random'])
    assert both['x_hat'].shape == (2, x.shape[1])
    for s, k in enumerate((0, 2)):
        one = (run(gpu_ctx, name, 'one') if k == 0 else
               feed(enhancer(name, gpu_ctx, lookahead=L, target=k), x, activity, (x.shape[1],)))
        assert np.array_equal(both['x_hat'][s], one['x_hat']), k
        assert np.array_equal(both['X_hat'][s], one['X_hat']), k
        for key in ('frames', 'mask', 'filter', 'held'):
            assert np.array_equal(both['states'][f'hold{s}.{key}'], one['states'][f'hold0.{key}'])


@pytest.mark.parametrize('name', NAMES)
def test_a_checkpoint_with_frames_held_continues_in_a_new_context(gpu_ctx, name):
    from pb_chime5_amd._capi import Context
    x, activity = sr.scene(name, sr.seed_of(name))
    other = Context(0)
    seen = {}

    def swap(i, enh):
        if i != 2:
            return None
        host = enh.to_host()
        seen['held'] = [h['held'] for h in host['holds']]
        return enhancer(name, other, lookahead=L).from_host(host)
    try:
        got = feed(enhancer(name, gpu_ctx, lookahead=L), x, activity,
                   sr.partitions(name)['random'], swap)
        assert seen['held'] == [L]
        want = run(gpu_ctx, name, 'one')
        assert np.array_equal(got['x_hat'], want['x_hat'])
        same_bits(got['states'], want['states'], f'{name} checkpoint')
        host = _host(gpu_ctx, name)
        with pytest.raises(ValueError, match='lookahead'):
            enhancer(name, other, lookahead=L + 1).from_host(host)
        with pytest.raises(ValueError, match='lookahead'):
            enhancer(name, other).from_host(host)
    finally:
        other.close()


def _host(ctx, name):
    x, activity = sr.scene(name, sr.seed_of(name))
    enh = enhancer(name, ctx, lookahead=L)
    enh.process(x[:, :200], activity[:, :200])
    return enh.to_host()


def test_lookahead_zero_is_the_enhancer_built_without_the_argument(gpu_ctx):
    """The bits, the shapes and the key sets, of the taps and of the checkpoint."""
    from test_gpu_stream import feed as feed0
    name = 'a'
    x, activity = sr.scene(name, sr.seed_of(name))
    cuts = sr.partitions(name)['random']
    for kw in (dict(), dict(fused=False), dict(target=0, targets=(0, 2))):
        a, b = enhancer(name, gpu_ctx, lookahead=0, **kw), enhancer(name, gpu_ctx, **kw)
        if 'targets' in kw:
            ya = [a.process(x[:, :700], activity[:, :700], debug=True), a.flush(debug=True)]
            yb = [b.process(x[:, :700], activity[:, :700], debug=True), b.flush(debug=True)]
            for (sa, da), (sb, db) in zip(ya, yb):
                assert np.array_equal(sa, sb)
                same_bits(da, db, 'targets taps')
        else:
            same_bits(feed0(a, x, activity, cuts), feed0(b, x, activity, cuts), str(kw))
        ha, hb = a.to_host(), b.to_host()
        assert sorted(ha) == sorted(hb) and 'holds' not in ha and 'lookahead' not in ha


# ------------------------------------------------------------------ workspace hygiene
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


@pytest.mark.parametrize('name', NAMES)
def test_workspace_hygiene_of_the_fused_entry(hctx, gpu_ctx, name):
    x, activity = sr.scene(name, sr.seed_of(name))
    outs = {}
    for pattern in PATTERNS:
        hctx.debug_workspace(pattern)
        try:
            outs[pattern] = _flat(feed(enhancer(name, hctx, lookahead=L), x, activity,
                                       sr.partitions(name)['random']))
            count, text, _ = hctx.debug_workspace_report()
        finally:
            hctx.debug_workspace(None)
        print(f'{name} [0x{pattern:02X}]: {count} guard violations {text}')
        assert count == 0, text
    a, b = outs[0x00], outs[0xFF]
    differ = [k for k in sorted(a) if _bits(a[k]) != _bits(b[k])]
    assert not differ, f'{name}: {differ} depend on what the workspace held'
    want = _flat(run(gpu_ctx, name, 'one'))
    assert all(_bits(b[k]) == _bits(want[k]) for k in want if k != 'counts')
