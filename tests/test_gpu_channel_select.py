"""Envelope-variance channel selection on the GPU (chsel_bands / chsel_scores / chsel_pick /
chsel_gather behind gss_channel_scores, gss_select_channels and
gss_enhance_observation_select) against tests/channel_select_reference.py.

The reference on these scenes (measured on a CPU, float64 against 80-bit arithmetic): scores
move by at most 2.3e-15 relative, band variances by 1.0e-14; the smallest relative gap between
neighbouring sorted scores is 2.2e-4 (D = 32) and the smallest gap at a selection boundary that
a test uses 4.3e-2.  The bar of 1e-10 lies four orders of magnitude above the reference's own
movement and six below the smallest gap."""
import ctypes
import functools
import math

import numpy as np
import pytest

import channel_select_reference as ref
from conftest import rel_err

pytestmark = pytest.mark.gpu

# (D, T, F, B): a ragged and a sub-tile T, odd D, D = 32, one band, the real bank; one, two,
# three and eight frequency shares of chsel_bands
SHAPES = [(4, 100, 6, 3), (5, 37, 4, 2), (7, 200, 17, 5), (12, 333, 33, 8), (24, 941, 65, 12),
          (29, 150, 9, 4), (32, 130, 9, 4), (24, 130, 513, 40), (3, 64, 5, 1)]
BAR = 1e-10
MARGIN = 1e-6


def _bank(B, F):
    if (B, F) == (40, 513):
        return ref.mel_bank(40, 1024)
    return ref.random_bank(np.random.default_rng(100 * B + F), B, F)


@functools.lru_cache(maxsize=None)
def _case(D, T, F, B):
    """Scene (F,T,D), its (D,T,F) view for `ops`, the bank, the reference scores and variances;
    computed once and shared (read-only)."""
    Y, W = ref.scene(D, T, F), _bank(B, F)
    scores, V = ref.channel_scores(Y, W)
    Obs = np.ascontiguousarray(Y.transpose(2, 1, 0))
    for a in (Y, W, scores, V, Obs):
        a.setflags(write=False)
    return Y, Obs, W, scores, V


def _keeps(D):
    return sorted({1, math.ceil(0.8 * D), D - 1, D})


def _rel(got, want):
    return float(np.max(np.abs(got - want) / np.abs(want)))


# ------------------------------------------------------------------ 1. stage parity
@pytest.mark.parametrize('D,T,F,B', SHAPES)
def test_scores_and_band_variances_match_the_reference(gpu_ctx, D, T, F, B):
    from pb_chime5_amd import ops
    _, Obs, W, scores, V = _case(D, T, F, B)
    got, gotV = ops.channel_scores(Obs, bank=W, return_band_variances=True, ctx=gpu_ctx)
    assert got.shape == (D,) and gotV.shape == (B, D)
    es, ev = _rel(got, scores), _rel(gotV, V)
    print(f'{(D, T, F, B)}: scores {es:.1e}, band variances {ev:.1e}')
    assert es <= BAR and ev <= BAR
    assert np.all(got >= 0) and np.all(got <= B)
    assert np.array_equal(ops.channel_scores(Obs, bank=W, ctx=gpu_ctx), got)


@pytest.mark.parametrize('D,T,F,B', SHAPES)
def test_selected_channels_are_the_references_and_gathered_bit_for_bit(gpu_ctx, D, T, F, B):
    from pb_chime5_amd import ops
    _, Obs, W, scores, _ = _case(D, T, F, B)
    for keep in _keeps(D):
        gap = ref.boundary_gap(scores, keep)
        assert gap > MARGIN, (keep, gap)        # (a scene that comes close is to be changed)
        want = ref.pick(scores, keep)
        sel, channels = ops.select_channels(Obs, keep, bank=W, ctx=gpu_ctx)
        assert np.array_equal(channels, want), (keep, channels, want)
        assert np.all(np.diff(channels) > 0)
        assert sel.shape == (keep, T, F) and np.array_equal(sel, Obs[channels]), keep
        assert gpu_ctx.last_selected_channels() == list(want)
    # a share and a count beyond D
    assert np.array_equal(ops.select_channels(Obs, 0.8, bank=W, ctx=gpu_ctx)[1],
                          ref.pick(scores, math.ceil(0.8 * D)))
    assert np.array_equal(ops.select_channels(Obs, D + 5, bank=W, ctx=gpu_ctx)[0], Obs)


def test_default_bank_is_the_mel_bank(gpu_ctx):
    from pb_chime5_amd import ops
    _, Obs, W, scores, _ = _case(24, 130, 513, 40)
    assert _rel(ops.channel_scores(Obs, ctx=gpu_ctx), scores) <= BAR
    W24 = ref.mel_bank(24, 1024)
    assert _rel(ops.channel_scores(Obs, bands=24, ctx=gpu_ctx),
                ref.channel_scores(_case(24, 130, 513, 40)[0], W24)[0]) <= BAR


# ------------------------------------------------------------------ 2. edge scenes
def test_a_dead_channel_scores_zero_and_ranks_last(gpu_ctx):
    from pb_chime5_amd import ops
    D, T, F, B = 7, 200, 17, 5
    Y, _, W, _, _ = _case(D, T, F, B)
    Y = Y.copy()
    Y[:, :, 3] = 0
    Obs = np.ascontiguousarray(Y.transpose(2, 1, 0))
    want, wantV = ref.channel_scores(Y, W)
    got, gotV = ops.channel_scores(Obs, bank=W, return_band_variances=True, ctx=gpu_ctx)
    assert got[3] == 0.0 and np.all(gotV[:, 3] == 0.0)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(gotV))
    live = np.arange(D) != 3
    assert _rel(got[live], want[live]) <= BAR and _rel(gotV[:, live], wantV[:, live]) <= BAR
    assert ref.boundary_gap(want, D - 1) > MARGIN
    _, channels = ops.select_channels(Obs, D - 1, bank=W, ctx=gpu_ctx)
    assert list(channels) == [0, 1, 2, 4, 5, 6]
    # all channels dead: scores 0, ties go to the lowest indices, nothing is NaN
    zero = np.zeros_like(Obs)
    assert np.array_equal(ops.channel_scores(zero, bank=W, ctx=gpu_ctx), np.zeros(D))
    sel, channels = ops.select_channels(zero, 3, bank=W, ctx=gpu_ctx)
    assert list(channels) == [0, 1, 2] and not sel.any()


def test_an_all_zero_bank_row_contributes_nothing(gpu_ctx):
    from pb_chime5_amd import ops
    D, T, F, B = 12, 333, 33, 8
    Y, Obs, W, _, V = _case(D, T, F, B)
    W0 = W.copy()
    W0[2] = 0
    want, wantV = ref.channel_scores(Y, W0)
    got, gotV = ops.channel_scores(Obs, bank=W0, return_band_variances=True, ctx=gpu_ctx)
    assert np.all(gotV[2] == 0.0) and np.all(np.isfinite(got))
    assert _rel(got, want) <= BAR
    assert _rel(np.delete(gotV, 2, axis=0), np.delete(V, 2, axis=0)) <= BAR


@pytest.mark.parametrize('D,T,F,B', [(7, 200, 17, 5), (24, 941, 65, 12), (24, 130, 513, 40)])
def test_scores_do_not_depend_on_the_gain_of_a_channel(gpu_ctx, D, T, F, B):
    from pb_chime5_amd import ops
    _, Obs, W, scores, _ = _case(D, T, F, B)
    gain = 10.0 ** np.random.default_rng(D).choice([-3.0, 3.0], size=D)
    base = ops.channel_scores(Obs, bank=W, ctx=gpu_ctx)
    got = ops.channel_scores(Obs * gain[:, None, None], bank=W, ctx=gpu_ctx)
    print(f'{(D, T, F, B)}: gain deviation {_rel(got, base):.1e}')
    assert _rel(got, base) <= BAR and _rel(got, scores) <= BAR
    keep = math.ceil(0.8 * D)
    assert np.array_equal(
        ops.select_channels(Obs * gain[:, None, None], keep, bank=W, ctx=gpu_ctx)[1],
        ref.pick(scores, keep))


@pytest.mark.parametrize('D,T,F,B', [(24, 941, 65, 12), (24, 130, 513, 40), (5, 37, 4, 2)])
def test_the_same_call_gives_the_same_bits(gpu_ctx, D, T, F, B):
    from pb_chime5_amd import ops
    _, Obs, W, _, _ = _case(D, T, F, B)
    a = ops.channel_scores(Obs, bank=W, return_band_variances=True, ctx=gpu_ctx)
    b = ops.channel_scores(Obs, bank=W, return_band_variances=True, ctx=gpu_ctx)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ------------------------------------------------------------------ 4. fused identities
def _tiny_scene(D):
    from test_gpu_guided import _context_samples, _tiny
    u, kw = _tiny(D)
    return u, kw, _context_samples(u)


@pytest.mark.parametrize('D', [4, 24])
def test_keeping_every_channel_is_the_plain_call_bit_for_bit(gpu_ctx, D):
    from pb_chime5_amd import ops
    u, kw, (cs, ce) = _tiny_scene(D)
    x, det = ops.enhance_observation(u.obs, u.activity_array, u.target_index, cs, ce, debug=True,
                                     ctx=gpu_ctx, **kw)
    for keep in (D, 1.0, D + 3):
        sx, sdet = ops.enhance_observation_select(u.obs, u.activity_array, u.target_index, cs, ce,
                                                  keep=keep, debug=True, ctx=gpu_ctx, **kw)
        assert np.array_equal(sx, x)
        for key in ('Obs', 'acitivity_freq', 'posterior', 'target_mask', 'distortion_mask',
                    'X_hat'):
            assert np.array_equal(sdet[key], det[key]), key
        assert sdet['ref_channel'] == det['ref_channel']
        assert list(sdet['selected_channels']) == list(range(D))
    assert gpu_ctx.last_ref_channel() == det['ref_channel']


@pytest.mark.parametrize('D,keep', [(4, 3), (24, 20), (24, 0.5)])
def test_fused_selection_equals_the_blocks_on_the_selected_channels(gpu_ctx, D, keep):
    """fused=True (gss_enhance_observation_select) against fused=False: stage STFT ->
    ops.select_channels -> the blocks on the selected channels; the bar of
    test_block_by_block_path_equals_fused."""
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import get_enhancer
    u, kw, (cs, ce) = _tiny_scene(D)
    n = ops.check_channel_keep(keep, D)
    enh = get_enhancer(wpe_tabs=kw['wpe_taps'], wpe_iterations=kw['wpe_iterations'],
                       bss_iterations=kw['bss_iterations'], channel_keep=keep)
    assert enh._fusable()
    fused = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, debug=True)
    loc = enh.enhance_observation_locals
    fused_channels, fused_Obs, ref_channel = (loc['selected_channels'], loc['Obs'],
                                              loc['details']['ref_channel'])
    assert fused_Obs.shape[0] == n and len(fused_channels) == n      # the Obs_ftd tap
    assert np.all(np.diff(fused_channels) > 0)
    assert gpu_ctx.last_selected_channels() == list(fused_channels)
    assert 0 <= ref_channel < n and gpu_ctx.last_ref_channel() == ref_channel
    assert 0 <= fused_channels[ref_channel] < D                      # mapped back: a kept channel

    # the stage's selection on the stage STFT
    stage_channels = ops.select_channels(enh.stft(u.obs), keep, ctx=gpu_ctx)[1]
    assert np.array_equal(stage_channels, fused_channels)
    blocks = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, fused=False,
                                     debug=True)
    bloc = enh.enhance_observation_locals
    assert np.array_equal(bloc['selected_channels'], fused_channels)
    err = rel_err(fused, blocks)
    print(f'D={D} keep={keep}: kept {list(fused_channels)}, fused vs blocks {err:.1e}')
    assert err < 1e-10
    assert rel_err(fused_Obs, bloc['Obs']) < 1e-10
    # (not compared bit for bit with the plain call on u.obs[channels]: the STFT kernel
    # transforms two real channels in one complex FFT, so the last bits of a channel's STFT
    # depend on its partner -- the selection gathers from the STFT of all D channels, as the
    # blocks above do)


@pytest.mark.parametrize('D,keep', [(4, 3), (24, 20)])
def test_pcm16_twin_equals_the_float_call_bit_for_bit(gpu_ctx, D, keep):
    from pb_chime5_amd import ops
    u, kw, (cs, ce) = _tiny_scene(D)
    pcm = np.clip(np.round(u.obs / np.max(np.abs(u.obs)) * 20000), -32768, 32767).astype(np.int16)
    args = (u.activity_array, u.target_index, cs, ce)
    a, adet = ops.enhance_observation_select(pcm, *args, keep=keep, debug=True, ctx=gpu_ctx, **kw)
    b, bdet = ops.enhance_observation_select(pcm / 2.0 ** 15, *args, keep=keep, debug=True,
                                             ctx=gpu_ctx, **kw)
    assert np.array_equal(a, b) and np.all(np.isfinite(a))
    for key in ('Obs', 'posterior', 'X_hat', 'selected_channels'):
        assert np.array_equal(adet[key], bdet[key]), key
    assert adet['Obs'].shape[0] == keep


# ------------------------------------------------------------------ 5. beyond the old limit
def test_32_channels_reach_the_beamformer(gpu_ctx):
    from pb_chime5_amd import ops, synthetic
    u = synthetic.tiny(seed=7, num_channels=32, num_samples=64000, num_speakers=3, context=4096,
                       noise=3e-2)
    kw = dict(wpe_taps=2, wpe_iterations=2, bss_iterations=6, bf='mvdrSouden_ban')
    from test_gpu_guided import _context_samples
    cs, ce = _context_samples(u)
    args = (u.obs, u.activity_array, u.target_index, cs, ce)
    x, det = ops.enhance_observation_select(*args, keep=29, debug=True, ctx=gpu_ctx, **kw)
    assert np.all(np.isfinite(x)) and np.any(x != 0)
    assert det['Obs'].shape[0] == 29 and len(det['selected_channels']) == 29
    assert 0 <= det['ref_channel'] < 29 and det['selected_channels'].max() <= 31
    with pytest.raises(AssertionError, match='D < 30'):
        ops.enhance_observation_select(*args, keep=30, ctx=gpu_ctx, **kw)
    with pytest.raises(AssertionError, match='D < 30'):
        ops.enhance_observation(*args, ctx=gpu_ctx, **kw)


# ------------------------------------------------------------------ 6. errors through the ABI
def _struct(bank_d, **fields):
    from pb_chime5_amd import _capi
    base = dict(bank_dev=bank_d.ptr, bands=3, keep=2, floor=1e-10)
    base.update(fields)
    return _capi.GssChannelSelect(**base)


def test_abi_errors_name_the_field(gpu_ctx):
    from pb_chime5_amd import ops
    from pb_chime5_amd._capi import c_void_p
    ctx, lib = gpu_ctx, gpu_ctx.lib
    D, T, F = 4, 100, 6
    _, Obs, W, _, _ = _case(D, T, F, 3)
    Y_d, _ = ops._obs_to_device_ftd(ctx, Obs)
    bank_d = ctx.to_device(W)
    out_d, s_d, c_d = ctx.empty(16 * F * T * D), ctx.empty(8 * D), ctx.empty(4 * D)

    def scores(st):
        ctx._check(lib.gss_channel_scores(ctx.handle, c_void_p(Y_d.ptr), F, T, D, st,
                                          c_void_p(s_d.ptr), None), 'gss_channel_scores')

    def select(st):
        ctx._check(lib.gss_select_channels(ctx.handle, c_void_p(Y_d.ptr), F, T, D, st,
                                           c_void_p(out_d.ptr), c_void_p(c_d.ptr)),
                   'gss_select_channels')

    u, kw, (cs, ce) = _tiny_scene(4)

    def fused(st, **params):
        p = ops.make_params(**{**kw, **params})
        ops._prepare_windows(ctx, p.stft_size, p.stft_shift)
        utt = ops.ResidentUtterance(ctx, u.obs, u.activity_array, p)
        ctx._check(lib.gss_enhance_observation_select(
            ctx.handle, ctypes.byref(p), c_void_p(utt.obs_d.ptr), utt.D, utt.N,
            c_void_p(utt.act_d.ptr), utt.K, utt.N_act, u.target_index, cs, ce, st,
            c_void_p(utt.out_d.ptr), None), 'gss_enhance_observation_select')
        ctx.synchronize()

    bank513 = ctx.to_device(ref.mel_bank(40, 1024))
    for call, good in ((scores, _struct(bank_d)), (select, _struct(bank_d)),
                       (fused, _struct(bank513, bands=40, keep=3))):
        call(ctypes.byref(good))                        # the good descriptor passes
        with pytest.raises(ValueError, match='sel is NULL'):
            call(None)
        for field, values in (('bank_dev', [None]), ('bands', [0, -1, 65]),
                              ('floor', [-1e-3, 1.0, 2.0, float('nan'), float('inf')])):
            for v in values:
                bad = type(good).from_buffer_copy(good)
                setattr(bad, field, v)
                with pytest.raises(ValueError, match=field):
                    call(ctypes.byref(bad))
        for v in (0, -1, D + 1):
            bad = type(good).from_buffer_copy(good)
            bad.keep = v
            if call is scores:
                call(ctypes.byref(bad))                 # sel->keep is unread
            else:
                with pytest.raises(ValueError, match='keep'):
                    call(ctypes.byref(bad))

    good = _struct(bank513, bands=40, keep=3)
    with pytest.raises(NotImplementedError, match='wpe_arrays'):
        fused(ctypes.byref(good), wpe_arrays=2)
    with pytest.raises(NotImplementedError, match='ch2'):
        fused(ctypes.byref(good), bf='ch2')
    fused(ctypes.byref(good), bf='sum')
    fused(ctypes.byref(good), wpe=False, wpe_arrays=2)  # (no WPE: the field is not read)

    # gss_last_selected_channels: at most the last call's count
    select(ctypes.byref(_struct(bank_d, keep=2)))
    assert len(ctx.last_selected_channels(2)) == 2 and len(ctx.last_selected_channels(1)) == 1
    for n in (0, 3, -1):
        with pytest.raises(ValueError, match='n='):
            ctx.last_selected_channels(n)


def test_no_selection_yet_on_a_fresh_context():
    from pb_chime5_amd import _capi
    ctx = _capi.Context(0)
    try:
        with pytest.raises(ValueError, match='kept 0'):
            ctx.last_selected_channels(1)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 7. workspace
def _samples_for_frames(T):
    from pb_chime5_amd import ops
    n = max((T - 1) * 256 - 512, 1)
    while ops.stft_frames(n, 1024, 256, True) < T:
        n += 1
    assert ops.stft_frames(n, 1024, 256, True) == T
    return n


@pytest.mark.parametrize('D', [4, 24])
@pytest.mark.parametrize('T', [63, 64, 65, 130, 941])
def test_workspace_of_the_select_call_on_a_fresh_context(D, T):
    """The arena of a fresh context is reserved from pipeline_workspace alone: a selection
    buffer it forgets is GSS_ERR_NOMEM (MemoryError) here, whatever slack an earlier, larger
    call would have left."""
    from pb_chime5_amd import _capi, ops
    N = _samples_for_frames(T)
    rng = np.random.default_rng(T + D)
    obs = rng.standard_normal((D, N))
    act = np.ones((2, N), bool)
    act[0, N // 2:] = False
    keep = math.ceil(0.8 * D)
    ctx = _capi.Context(0)
    try:
        for kw in (dict(wpe_taps=2, wpe_iterations=1, bss_iterations=2),
                   dict(wpe=False, bss_iterations=1)):
            x, det = ops.enhance_observation_select(obs, act, 0, 0, 0, keep=keep, debug=True,
                                                    ctx=ctx, **kw)
            assert det['Obs'].shape == (keep, T, 513) and len(det['selected_channels']) == keep
            assert ctx.workspace_bytes() > 16 * 513 * T * (D + keep)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 8. session
def test_pipelined_session_with_selection_equals_sequential(tmp_path_factory, tmp_path):
    """enhance_session with channel_keep stays pipelined (two utterances in flight, the pcm16
    select call, no wait for the selection) and writes the bytes of the one-at-a-time loop."""
    from test_chime5_frontdoor import _enhancer, _load_fixture, _write_corpus
    fixture = _load_fixture('chime5_session')
    corpus = _write_corpus(fixture, tmp_path_factory.mktemp('chime5_corpus_select'))
    a, b, c = tmp_path / 'seq', tmp_path / 'pipe', tmp_path / 'all'
    seq = _enhancer(corpus, fixture, channel_keep=0.75)
    seq.inflight = 1
    seq.enhance_session('S02', a)
    pipe = _enhancer(corpus, fixture, channel_keep=0.75)
    assert pipe.inflight == 2
    pipe.enhance_session('S02', b)
    files = sorted(p.relative_to(a) for p in a.rglob('*.wav'))
    assert len(files) == len(fixture['examples'])
    assert files == sorted(p.relative_to(b) for p in b.rglob('*.wav'))
    for rel in files:
        assert (a / rel).read_bytes() == (b / rel).read_bytes(), rel
    assert pipe.session_clock['examples'] == len(files)
    # the selection did something: the files differ from those of all channels
    every = _enhancer(corpus, fixture)
    every.enhance_session('S02', c, dataset_slice=slice(0, 2))
    assert any((c / rel).read_bytes() != (a / rel).read_bytes()
               for rel in sorted(p.relative_to(c) for p in c.rglob('*.wav')))
