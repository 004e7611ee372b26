"""Segment-wise MVDR-Souden (gss_mvdr_souden_segments, gss_enhance_observation_segments) on the
GPU against the NumPy composition of the oracle's functions (tests/segments_reference.py,
DESIGN.md section 12): stage parity, identities with the whole-window beamformer, the fused
pipeline, the front doors, and the structure of a call (launch counts, workspace)."""
import ctypes

import numpy as np
import pytest

import gss_oracle as oracle
import segments_reference as sr
from conftest import rel_err
from test_chime5_frontdoor import _enhancer, corpus, fixture  # noqa: F401 (fixtures)
from test_gpu_guided import _context_samples, _tiny
from test_gpu_pipeline import TOL_STFT_MAG
from test_gpu_stages import _scene

pytestmark = pytest.mark.gpu

MIN_MASS = 8        # of the stage scenes: the closest window mass is 37 % away from it
# (D, T, F, L, c): share of (b, f) that fall back 0.20 0.00 0.20 0.33 0.25 0.25 0.20 0.50
STAGE_SCENES = [(4, 300, 6, 64, 0), (4, 300, 6, 64, 1), (7, 515, 5, 128, 1), (12, 700, 4, 128, 1),
                (24, 1000, 3, 256, 0), (24, 1000, 3, 128, 1), (24, 941, 3, 64, 2),
                (29, 640, 2, 192, 0)]


def _stage_scene(D, T, F):
    """The scene and masks of test_mvdr_matches_oracle."""
    rng = np.random.default_rng(D * 7 + T)
    Y, act = _scene(rng, D, T, F, 3)
    xm = rng.uniform(size=(T, F)) * act[0][:, None]
    return Y, xm, 1 - xm


# ------------------------------------------------------------------ 1. stage parity
@pytest.mark.parametrize('ban', [False, True])
@pytest.mark.parametrize('D,T,F,L,c', STAGE_SCENES)
def test_segments_match_the_reference(gpu_ctx, D, T, F, L, c, ban):
    """X_hat at the bar of test_mvdr_matches_oracle (the reference moves by at most 6.3e-14
    under a last-bit change of Y on these scenes); reference channel and fallback count exact.
    The discrete decision cannot hide behind rounding: no window mass of the scene lies within
    1e-6 relative of min_mass (change min_mass with a scene, never the margin)."""
    from pb_chime5_amd import ops
    Y, xm, nm = _stage_scene(D, T, F)
    margin = sr.mass_margin(xm, nm, L, c, MIN_MASS)
    assert margin > 1e-6, margin
    want, det = sr.mvdr_souden_segments(Y, xm, nm, ban, L, c, MIN_MASS)
    assert np.all(np.isfinite(want))
    whole = ops.mvdr_souden_from_masks(Y, xm, nm, ban=ban, ctx=gpu_ctx)
    got, ref, fallbacks = ops.mvdr_souden_segments_from_masks(
        Y, xm, nm, ban=ban, segment_frames=L, segment_context=c, min_mass=MIN_MASS,
        return_ref_channel=True, return_fallbacks=True, ctx=gpu_ctx)
    print(f'{(D, T, F, L, c)} ban={ban}: rel err {rel_err(got, want):.1e}, ref {ref} / '
          f'{det["ref_channel"]}, fallbacks {fallbacks} / {int(det["fallbacks"].sum())} of '
          f'{det["fallbacks"].size}, margin {margin:.2f}, whole-window vs reference '
          f'{rel_err(whole, want):.2f}')
    assert ref == det['ref_channel'] == gpu_ctx.last_ref_channel()
    assert fallbacks == int(det['fallbacks'].sum()) == gpu_ctx.last_segment_fallbacks()
    assert rel_err(got, want) < 1e-9
    # what the tree could do before: one filter per window is another signal on these scenes
    assert rel_err(whole, want) > 0.05


def test_stage_scenes_exercise_both_branches():
    shares = []
    for D, T, F, L, c in STAGE_SCENES:
        Y, xm, nm = _stage_scene(D, T, F)
        shares.append(float((sr.window_masses(xm, nm, L, c).min(-1) < MIN_MASS).mean()))
    assert min(shares) == 0.0 and max(shares) == 0.5 and sum(s > 0 for s in shares) == 7, shares


def test_default_min_mass_is_twice_the_channels(gpu_ctx):
    from pb_chime5_amd import ops
    D, T, F, L, c = 7, 515, 5, 128, 1
    Y, xm, nm = _stage_scene(D, T, F)
    assert sr.mass_margin(xm, nm, L, c, 2 * D) > 1e-6
    want, det = sr.mvdr_souden_segments(Y, xm, nm, True, L, c, None)
    got, fallbacks = ops.mvdr_souden_segments_from_masks(
        Y, xm, nm, ban=True, segment_frames=L, segment_context=c, return_fallbacks=True,
        ctx=gpu_ctx)
    assert fallbacks == int(det['fallbacks'].sum())
    assert rel_err(got, want) < 1e-9


# ------------------------------------------------------------------ 2. identities
@pytest.mark.parametrize('ban', [False, True])
@pytest.mark.parametrize('D,T,F,L,c', [
    (4, 300, 6, 320, 0), (4, 300, 6, 64000, 0), (24, 941, 3, 960, 0), (12, 700, 4, 1024, 3),
    (4, 300, 6, 64, 5), (4, 300, 6, 64, 2 ** 31 - 1), (24, 941, 3, 64, 15), (12, 700, 4, 128, 6),
    (29, 640, 2, 192, 4)])
def test_one_segment_or_full_context_is_the_whole_window_beamformer(gpu_ctx, D, T, F, L, c, ban):
    """L >= T (one segment) and c >= B (every window is the whole utterance): the same sums in
    another order.  Within 1e-12 of the whole-window call, same reference channel."""
    from pb_chime5_amd import ops
    assert L >= T or c >= -(-T // L)
    Y, xm, nm = _stage_scene(D, T, F)
    want, wref = ops.mvdr_souden_from_masks(Y, xm, nm, ban=ban, return_ref_channel=True,
                                            ctx=gpu_ctx)
    for min_mass in (MIN_MASS, 0):
        got, ref, fallbacks = ops.mvdr_souden_segments_from_masks(
            Y, xm, nm, ban=ban, segment_frames=L, segment_context=c, min_mass=min_mass,
            return_ref_channel=True, return_fallbacks=True, ctx=gpu_ctx)
        print(f'{(D, T, F, L, c)} ban={ban} min_mass={min_mass}: vs whole window '
              f'{rel_err(got, want):.1e}')
        assert ref == wref and fallbacks == 0
        assert rel_err(got, want) < 1e-12


def test_forced_reference_channel_is_honoured(gpu_ctx):
    from pb_chime5_amd import ops
    D, T, F, L, c = 7, 515, 5, 128, 1
    Y, xm, nm = _stage_scene(D, T, F)
    outs = []
    for r in range(D):
        want, det = sr.mvdr_souden_segments(Y, xm, nm, True, L, c, MIN_MASS, ref_channel=r)
        got, ref = ops.mvdr_souden_segments_from_masks(
            Y, xm, nm, ban=True, segment_frames=L, segment_context=c, min_mass=MIN_MASS,
            ref_channel=r, return_ref_channel=True, ctx=gpu_ctx)
        assert ref == r == det['ref_channel'] == gpu_ctx.last_ref_channel()
        assert rel_err(got, want) < 1e-9
        outs.append(got)
    assert all(rel_err(outs[0], o) > 1e-3 for o in outs[1:])        # the channel matters


def test_an_empty_segment_without_fallback_is_nan_under_ban(gpu_ctx):
    """min_mass = 0 never falls back: a segment whose target mask is all zero gives Phi_X = 0,
    w = 0 and 0 / 0 = NaN in the blind analytic normalisation, as the reference gives for an
    empty utterance -- in exactly that segment's frames."""
    from pb_chime5_amd import ops
    D, T, F, L = 5, 300, 4, 64
    rng = np.random.default_rng(21)
    Y, _ = _scene(rng, D, T, F, 3)
    xm = rng.uniform(0.1, 0.9, size=(T, F))
    xm[2 * L:3 * L] = 0.0
    nm = 1 - xm
    want, det = sr.mvdr_souden_segments(Y, xm, nm, True, L, 0, 0)
    got, fallbacks = ops.mvdr_souden_segments_from_masks(
        Y, xm, nm, ban=True, segment_frames=L, min_mass=0, return_fallbacks=True, ctx=gpu_ctx)
    nan = np.zeros((T, F), bool)
    nan[2 * L:3 * L] = True
    assert fallbacks == 0 and not det['fallbacks'].any()
    assert np.array_equal(np.isnan(want), nan)
    assert np.array_equal(np.isnan(got.real), nan) and np.array_equal(np.isnan(got.imag), nan)
    assert np.all(np.isfinite(got[~nan]))
    assert rel_err(got[~nan], want[~nan]) < 1e-9
    # without the normalisation the empty segment's filter is zero, not NaN
    plain = ops.mvdr_souden_segments_from_masks(Y, xm, nm, ban=False, segment_frames=L,
                                                min_mass=0, ctx=gpu_ctx)
    assert np.all(plain[nan] == 0) and np.all(np.isfinite(plain))
    # and with a threshold the segment takes the whole-window statistics: finite everywhere
    safe, fallbacks = ops.mvdr_souden_segments_from_masks(
        Y, xm, nm, ban=True, segment_frames=L, min_mass=MIN_MASS, return_fallbacks=True,
        ctx=gpu_ctx)
    assert fallbacks == F and np.all(np.isfinite(safe))


def test_nonfinite_snr_raises_like_the_whole_window_call(gpu_ctx):
    from pb_chime5_amd import ops
    D, T, F, L, c = 4, 300, 6, 64, 1
    Y, xm, nm = _stage_scene(D, T, F)
    kw = dict(ban=True, segment_frames=L, segment_context=c, min_mass=MIN_MASS, ctx=gpu_ctx)
    X = ops.mvdr_souden_segments_from_masks(Y, xm, nm, **kw)
    Ybad = Y.copy()
    Ybad[2, 70, 3] = np.nan
    with pytest.raises(AssertionError):
        sr.mvdr_souden_segments(Ybad, xm, nm, True, L, c, MIN_MASS)
    with pytest.raises(AssertionError):
        ops.mvdr_souden_segments_from_masks(Ybad, xm, nm, **kw)
    assert gpu_ctx.last_ref_channel() == -1
    # the next utterance on the same context is not affected
    assert np.array_equal(ops.mvdr_souden_segments_from_masks(Y, xm, nm, **kw), X)


def test_wrapper_and_block_reach_the_segment_kernels(gpu_ctx):
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import Beamformer
    from pb_chime5_amd.speech_enhancement.beamforming_wrapper import (
        beamform_mvdr_souden_from_masks)
    D, T, F, L, c = 4, 300, 6, 64, 1
    Y, xm, nm = _stage_scene(D, T, F)
    direct = ops.mvdr_souden_segments_from_masks(Y, xm, nm, ban=True, segment_frames=L,
                                                 segment_context=c, ctx=gpu_ctx)
    assert np.array_equal(beamform_mvdr_souden_from_masks(
        Y, xm, nm, ban=True, segment_frames=L, segment_context=c), direct)
    block = Beamformer('mvdrSouden_ban', 'mask_mul', segment_frames=L, segment_context=c)
    assert np.array_equal(block(Y, xm, nm), direct * xm)
    # None is the whole-window call, untouched
    assert np.array_equal(beamform_mvdr_souden_from_masks(Y, xm, nm, ban=True),
                          ops.mvdr_souden_from_masks(Y, xm, nm, ban=True, ctx=gpu_ctx))


def test_c_abi_argument_errors_name_the_field(gpu_ctx):
    from pb_chime5_amd import _capi
    ctx = gpu_ctx
    F, T, D = 3, 130, 4
    buf = ctx.empty(16 * F * T * D)
    p = _capi.c_void_p(buf.ptr)

    def call(seg, ref=-1):
        return ctx.lib.gss_mvdr_souden_segments(ctx.handle, p, F, T, D, p, p, 1, ref,
                                                ctypes.byref(seg) if seg is not None else None,
                                                p, None)
    good = dict(segment_frames=64, context_segments=0, min_mass=1.0)
    for bad, word in ((dict(segment_frames=0), 'segment_frames'),
                      (dict(segment_frames=96), 'segment_frames'),
                      (dict(segment_frames=-64), 'segment_frames'),
                      (dict(context_segments=-1), 'context_segments'),
                      (dict(min_mass=-0.5), 'min_mass'), (dict(min_mass=float('nan')), 'min_mass'),
                      (dict(min_mass=float('inf')), 'min_mass')):
        assert call(_capi.GssBfSegments(**{**good, **bad})) == _capi.GSS_ERR_INVALID, bad
        assert word in ctx.lib.gss_last_error(ctx.handle).decode(), bad
    assert call(None) == _capi.GSS_ERR_INVALID
    assert 'seg' in ctx.lib.gss_last_error(ctx.handle).decode()
    assert call(_capi.GssBfSegments(**good), ref=D) == _capi.GSS_ERR_INVALID
    assert 'ref_channel' in ctx.lib.gss_last_error(ctx.handle).decode()
    out = ctypes.c_int64(-1)
    assert ctx.lib.gss_last_segment_fallbacks(ctx.handle, None) == _capi.GSS_ERR_INVALID
    assert ctx.lib.gss_last_segment_fallbacks(ctx.handle, ctypes.byref(out)) == 0 <= out.value


# ------------------------------------------------------------------ 3. fused
# (D = 4: T = 97 frames, two segments, the default min_mass = 2 D.  D = 24: T = 253; the 16
# context frames are zeroed, so the first segment holds 48 = 2 D frames of distortion mask of
# nearly 1 -- a mass 3e-7 relative from the default threshold, and saturated posteriors put
# masses next to other whole numbers too.  The threshold there is moved to 30.5, not the margin:
# with the oracle's masks on the CPU the closest mass is 3 % away and 25 % / 50 % of the (b, f)
# fall back.  The reference's own X_hat moves by 3e-15 (D = 4) and 1e-11 (D = 24) when Obs
# changes in its last bit.  (24, 64, 0) is left out on purpose: with a threshold low enough not
# to fall back everywhere, 45 to 64 frames estimate a 24 x 24 Phi_N, cond(Phi_N) reaches 1e18,
# and the reference's own reference channel moves from 19 to 2 under that last-bit change.)
@pytest.mark.parametrize('D,L,c,min_mass', [(4, 64, 0, None), (24, 64, 1, 30.5),
                                            (24, 128, 0, 30.5)])
def test_fused_segments_against_the_reference_on_its_own_taps(gpu_ctx, D, L, c, min_mass):
    """Enhancer.enhance_observation(debug=True) with segments: X_hat against the segmented
    reference computed from the call's OWN tapped Obs and masks (isolates the new stage from
    WPE / EM round-off) at 1e-9, x_hat against the oracle's istft of it at the iSTFT bar of
    test_gpu_stages (1e-12); the block path equals the fused call at 1e-10."""
    from pb_chime5_amd.core import get_enhancer
    u, kw = _tiny(D)
    enh = get_enhancer(wpe_tabs=kw['wpe_taps'], wpe_iterations=kw['wpe_iterations'],
                       bss_iterations=kw['bss_iterations'], bf_segment_frames=L,
                       bf_segment_context=c, bf_segment_min_mass=min_mass)
    assert enh._fusable()
    got = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, debug=True)
    loc = enh.enhance_observation_locals
    det = loc['details']
    margin = sr.mass_margin(det['target_mask'], det['distortion_mask'], L, c,
                            2 * D if min_mass is None else min_mass)
    assert margin > 1e-6, margin
    want, wdet = sr.mvdr_souden_segments(det['Obs'], det['target_mask'], det['distortion_mask'],
                                         True, L, c, min_mass)
    share = wdet['fallbacks'].mean()
    print(f'D={D} L={L} c={c}: X_hat vs reference on own taps {rel_err(det["X_hat"], want):.1e}, '
          f'fallback share {share:.2f}, margin {margin:.1e}')
    assert det['ref_channel'] == wdet['ref_channel'] == enh._ctx().last_ref_channel()
    assert det['segment_fallbacks'] == int(wdet['fallbacks'].sum())
    assert rel_err(det['X_hat'], want) < 1e-9
    assert rel_err(got, oracle.istft(det['X_hat'])) < 1e-12
    # the taps keep their shapes
    T, F = det['X_hat'].shape
    assert det['Obs'].shape == (D, T, F) and det['target_mask'].shape == (T, F)
    assert det['posterior'].shape[1:] == (T, F) and det['acitivity_freq'].shape[1] == T
    # segments change the signal; without them the call is the parent's
    plain = get_enhancer(wpe_tabs=kw['wpe_taps'], wpe_iterations=kw['wpe_iterations'],
                         bss_iterations=kw['bss_iterations'])
    whole = plain.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex)
    assert rel_err(got, whole) > 1e-3
    blocks = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, fused=False)
    print(f'D={D} L={L} c={c}: block path vs fused {rel_err(blocks, got):.1e}')
    assert rel_err(blocks, got) < 1e-10


# End to end: the recipe of test_other_channel_and_class_counts at (D, K) = (6, 4).  Measured on
# the CPU: the oracle pipeline with the segmented reference as its beamformer moves |X_hat| by
# 2.6e-13 when every sample changes in its last bit (below 1e-6: the README's 1e-4 bar
# applies); 23 % of the (b, f) fall back; the window masses next to min_mass = 13.2 are 12.81
# and 13.62 (3 % away: the device's masks agree with the oracle's to 1e-4 per element, which
# moves a mass of up to 192 frames by less than 0.02).
E2E = dict(D=6, K=4, L=64, c=1, min_mass=13.2)


def test_end_to_end_against_the_oracle_pipeline(gpu_ctx):
    from pb_chime5_amd import ops, synthetic
    D, K, L, c, min_mass = (E2E[k] for k in ('D', 'K', 'L', 'c', 'min_mass'))
    u = synthetic.tiny(seed=D + K, num_channels=D, num_samples=64000, num_speakers=K - 1,
                       context=4096, noise=3e-2)
    kw = dict(wpe=True, wpe_taps=2, wpe_delay=2, wpe_iterations=2, bss_iterations=6)
    _, wdet = oracle.enhance_observation(u.obs, u.activity_array, u.target_index, u.ex,
                                         return_details=True, gss_fn=oracle.gss_block_batched,
                                         **kw)
    X_want, sdet = sr.mvdr_souden_segments(wdet['Obs'], wdet['target_mask'],
                                           wdet['distortion_mask'], True, L, c, min_mass)
    want = oracle.istft(X_want)
    cs, ce = _context_samples(u)
    got, det = ops.enhance_observation_segments(
        u.obs, u.activity_array, u.target_index, cs, ce, segment_frames=L, segment_context=c,
        min_mass=min_mass, debug=True, ctx=gpu_ctx, **kw)
    for masks in (wdet, det):
        margin = sr.mass_margin(masks['target_mask'], masks['distortion_mask'], L, c, min_mass)
        assert margin > 1e-2, margin
    share = sdet['fallbacks'].mean()
    err = rel_err(np.abs(det['X_hat']), np.abs(X_want))
    print(f'end to end: |X_hat| rel err {err:.1e}, x_hat {rel_err(got, want):.1e}, fallback '
          f'share {share:.2f}, whole-window oracle vs segmented '
          f'{rel_err(np.abs(wdet["X_hat"]), np.abs(X_want)):.2f}')
    assert 0.1 < share < 0.9                      # both branches
    assert np.linalg.cond(sdet['cov_n']).max() < 1e8
    assert det['ref_channel'] == sdet['ref_channel']
    assert det['segment_fallbacks'] == int(sdet['fallbacks'].sum())
    assert err < TOL_STFT_MAG
    assert rel_err(got, want) < TOL_STFT_MAG
    assert rel_err(np.abs(wdet['X_hat']), np.abs(X_want)) > 0.05


def test_session_with_segments_writes_what_enhance_example_gives(corpus, fixture, tmp_path):  # noqa: F811
    a, b, c = tmp_path / 'session', tmp_path / 'examples', tmp_path / 'whole'
    kw = dict(wpe_tabs=2, bss_iterations=3, bf_segment_frames=64, bf_segment_context=1)
    enh = _enhancer(corpus, fixture, **kw)
    assert enh.inflight == 2        # the default: the session itself leaves the pipelined path
    enh.enhance_session('S02', a, dataset_slice=slice(0, 4))
    per = _enhancer(corpus, fixture, **kw)
    (b / 'dev').mkdir(parents=True)
    for ex in per.get_iterator('S02')[:4]:
        per._write(ex, per.enhance_example(ex), b)
    _enhancer(corpus, fixture, wpe_tabs=2, bss_iterations=3).enhance_session(
        'S02', c, dataset_slice=slice(0, 4))
    files = sorted(p.relative_to(a) for p in a.rglob('*.wav'))
    assert len(files) == 4 and files == sorted(p.relative_to(b) for p in b.rglob('*.wav'))
    for rel in files:
        assert (a / rel).read_bytes() == (b / rel).read_bytes(), rel
    assert any((a / rel).read_bytes() != (c / rel).read_bytes() for rel in files)


# ------------------------------------------------------------------ 4. structure
def _profile_calls(ctx, run):
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        run()
        return {k: v['calls'] for k, v in ctx.profile_report().items()}
    finally:
        ctx.profile_enable(False)


def test_launch_count_does_not_depend_on_the_number_of_segments(gpu_ctx):
    """The same (F, T, D) as B = 4 and as B = 30 segments, with and without context: the same
    kernels the same number of times, the PSD accumulation once."""
    from pb_chime5_amd import ops
    D, T, F = 6, 1900, 5
    Y, xm, nm = _stage_scene(D, T, F)
    seen = []
    for L, c in ((512, 0), (64, 0), (64, 3)):
        assert -(-T // L) == (4 if L == 512 else 30)
        seen.append(_profile_calls(gpu_ctx, lambda: ops.mvdr_souden_segments_from_masks(
            Y, xm, nm, ban=True, segment_frames=L, segment_context=c, min_mass=MIN_MASS,
            ctx=gpu_ctx)))
    print(seen[0])
    assert seen[0] == seen[1] == seen[2]
    for name in ('psd_segments', 'mvdr_window_segments', 'mvdr_solve_segments',
                 'mvdr_ref_segments', 'mvdr_apply_segments'):
        assert seen[0][name] == 1, name
    assert not {'psd', 'mvdr_solve', 'mvdr_ref', 'mvdr_apply'} & set(seen[0])


def _sweep_frames():
    frames = [int(t) + (int(t) % 64 == 0) for t in np.linspace(100, 8000, 41)]
    assert len(frames) >= 40 and all(t % 64 for t in frames)
    return frames


@pytest.mark.parametrize('D', [4, 24])
def test_fresh_context_over_a_sweep_of_frames_stage_call(gpu_ctx, D):
    """A context that has never grown its arena, for every T: mvdr_segments_workspace_bytes
    covers what the segment path allocates (the 1 MiB rounding of a warm arena would hide an
    allocation missing from the formula)."""
    from pb_chime5_amd import _capi
    F, frames = 513, _sweep_frames()
    rng = np.random.default_rng(D)
    Tmax = max(frames)
    flat = rng.standard_normal(2 * 513 * 64 * D)
    Y_d = gpu_ctx.to_device(np.resize(flat, 2 * F * Tmax * D).view(np.complex128))
    m = rng.uniform(0.05, 0.95, size=F * Tmax)
    mx_d, mn_d = gpu_ctx.to_device(m), gpu_ctx.to_device(1 - m)
    X_d = gpu_ctx.empty(16 * F * Tmax)
    for i, T in enumerate(frames):
        seg = _capi.GssBfSegments(*[(64, 1, 8.0), (256, 0, 8.0), (128, 2, 0.0)][i % 3])
        ctx = _capi.Context(0)
        try:
            status = ctx.lib.gss_mvdr_souden_segments(
                ctx.handle, _capi.c_void_p(Y_d.ptr), F, T, D, _capi.c_void_p(mx_d.ptr),
                _capi.c_void_p(mn_d.ptr), 1, -1, ctypes.byref(seg), _capi.c_void_p(X_d.ptr), None)
            assert status != _capi.GSS_ERR_NOMEM, (T, ctx.lib.gss_last_error(ctx.handle))
            ctx._check(status, f'gss_mvdr_souden_segments T={T}')
            ctx.synchronize()
        finally:
            ctx.close()


@pytest.mark.parametrize('D', [4, 24])
def test_fresh_context_over_a_sweep_of_frames_fused_call(gpu_ctx, D):
    from pb_chime5_amd import _capi, ops
    K = 3
    # (no WPE and one EM iteration: the beamformer's workspace is the largest stage)
    params = ops.make_params(wpe=False, bss_iterations=1)
    analysis = ops.analysis_window(1024)
    synthesis = ops.synthesis_window(analysis, 256)
    samples = []
    for t in _sweep_frames():
        n = t * 256 - 700
        while ops.stft_frames(n, 1024, 256, True) % 64 == 0:
            n += 256
        samples.append(n)
    Nmax = max(samples)
    rng = np.random.default_rng(D)
    obs_d = gpu_ctx.to_device(rng.standard_normal((D, Nmax)))           # (D,N): its head
    act = rng.random((K, Nmax)) < 0.7
    act[-1] = True
    act_d = gpu_ctx.to_device(act.astype(np.uint8))
    Tmax = ops.stft_frames(Nmax, 1024, 256, True)
    out_d = gpu_ctx.empty(8 * int(gpu_ctx.lib.gss_istft_num_samples(Tmax, 1024, 256, 1)))
    for i, N in enumerate(samples):
        seg = _capi.GssBfSegments(*[(64, 1, 8.0), (256, 0, 8.0), (128, 2, 0.0)][i % 3])
        ctx = _capi.Context(0)
        try:
            ctx.set_windows(1024, 256, analysis, synthesis)
            # (rows of the (K, Nmax) activity: N_act = Nmax >= N)
            status = ctx.lib.gss_enhance_observation_segments(
                ctx.handle, ctypes.byref(params), _capi.c_void_p(obs_d.ptr), D, N,
                _capi.c_void_p(act_d.ptr), K, Nmax, 0, 0, 0, ctypes.byref(seg),
                _capi.c_void_p(out_d.ptr), None)
            assert status != _capi.GSS_ERR_NOMEM, (N, ctx.lib.gss_last_error(ctx.handle))
            ctx._check(status, f'gss_enhance_observation_segments N={N}')
            ctx.synchronize()
        finally:
            ctx.close()


def test_fused_call_refuses_other_beamformers(gpu_ctx):
    from pb_chime5_amd import _capi, ops
    ctx = gpu_ctx
    ops._prepare_windows(ctx, 1024, 256)
    seg = _capi.GssBfSegments(64, 0, 1.0)
    buf = ctx.empty(8 * 4 * 4096)
    p = _capi.c_void_p(buf.ptr)
    for bf in ('gev_ban', 'ch2', 'sum'):
        params = ops.make_params(bf=bf)
        status = ctx.lib.gss_enhance_observation_segments(
            ctx.handle, ctypes.byref(params), p, 4, 4096, p, 2, 4096, 0, 0, 0,
            ctypes.byref(seg), p, None)
        assert status == _capi.GSS_ERR_UNSUPPORTED, bf
    params = ops.make_params()
    assert ctx.lib.gss_enhance_observation_segments(
        ctx.handle, ctypes.byref(params), p, 4, 4096, p, 2, 4096, 0, 0, 0, None, p,
        None) == _capi.GSS_ERR_INVALID
