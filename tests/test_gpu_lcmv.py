"""Interferer-nulling LCMV (gss_lcmv_souden, gss_lcmv_masks_from_posteriors,
gss_enhance_observation_lcmv) on the GPU against the plain-NumPy reference
(tests/lcmv_reference.py): stage parity, the fallback to the MVDR, the
null itself, a singular noise matrix, the choice of the interferer, the fused pipeline and its
block path, the workspace of a fresh context and the error codes of the C entry points."""
import ctypes
import functools

import numpy as np
import pytest

import lcmv_reference as lr
from conftest import rel_err

pytestmark = pytest.mark.gpu

STAGE_BAR = 1e-9        # the project's stage bar
# (D, T, F): the smallest D, an odd D (padding of the Jacobi block), T off the 64-frame tile,
# LDS above 64 KB (D = 29)
STAGE_SHAPES = [(2, 70, 3), (5, 130, 4), (12, 333, 3), (24, 200, 2), (29, 96, 2)]


@functools.lru_cache(maxsize=None)
def _stage_scene(D, T, F):
    rng = np.random.default_rng(1000 * D + T)
    Y, xm, im, nm, info = lr.scene(rng, D, T, F)
    for a in (Y, xm, im, nm):
        a.setflags(write=False)
    return Y, xm, im, nm, info


@functools.lru_cache(maxsize=None)
def _stage_reference(D, T, F, ban, ref_channel):
    Y, xm, im, nm, _ = _stage_scene(D, T, F)
    want, det = lr.lcmv_souden_from_masks(Y, xm, im, nm, ban, 0.0, ref_channel)
    # a badly drawn scene fails loudly
    assert np.linalg.cond(det['phi_n']).max() <= 1e4, np.linalg.cond(det['phi_n'])
    assert np.all(np.isfinite(want))
    return want, det


def _last_bit(Y, seed=1):
    """Y with every sample moved by one unit in the last place, up or down."""
    rng = np.random.default_rng(seed)
    return Y * (1 + (rng.integers(0, 2, Y.shape) * 2 - 1) * 2.0 ** -52)


# ------------------------------------------------------------------ 1. stage parity
@pytest.mark.parametrize('named', [False, True], ids=['chosen', 'named'])
@pytest.mark.parametrize('ban', [False, True])
@pytest.mark.parametrize('D,T,F', STAGE_SHAPES)
def test_stage_matches_the_reference(gpu_ctx, D, T, F, ban, named):
    """max|X_hat - ref| <= 1e-9 max|ref|, the reference channel equal as an integer; with the
    channel chosen and with another one named."""
    from pb_chime5_amd import ops
    Y, xm, im, nm, _ = _stage_scene(D, T, F)
    _, chosen = _stage_reference(D, T, F, ban, None)
    name = (chosen['ref_channel'] + 1) % D if named else None
    want, det = _stage_reference(D, T, F, ban, name)
    got, ref, fallbacks = ops.lcmv_souden_from_masks(
        Y, xm, im, nm, ban=ban, ref_channel=name, return_ref_channel=True, return_fallbacks=True,
        ctx=gpu_ctx)
    print(f'{(D, T, F)} ban={ban} named={named}: rel err {rel_err(got, want):.1e}, ref {ref} / '
          f'{det["ref_channel"]}, cond(Phi_N) {np.linalg.cond(det["phi_n"]).max():.0f}, gamma >= '
          f'{det["gamma"].min():.1f}')
    assert ref == det['ref_channel'] == gpu_ctx.last_ref_channel()
    assert fallbacks == 0 == gpu_ctx.last_lcmv_fallbacks()
    assert rel_err(got, want) <= STAGE_BAR
    if named:       # the channel matters
        assert rel_err(got, _stage_reference(D, T, F, ban, None)[0]) > 1e-3


def test_wrapper_and_block_reach_the_lcmv_kernels(gpu_ctx):
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import Beamformer
    from pb_chime5_amd.speech_enhancement.beamforming_wrapper import (
        beamform_lcmv_souden_from_masks)
    D, T, F = 5, 130, 4
    Y, xm, im, nm, _ = _stage_scene(D, T, F)
    for ban in (False, True):
        direct = ops.lcmv_souden_from_masks(Y, xm, im, nm, ban=ban, ctx=gpu_ctx)
        assert np.array_equal(beamform_lcmv_souden_from_masks(Y, xm, im, nm, ban), direct)
        assert np.array_equal(beamform_lcmv_souden_from_masks(
            Y[None], *(np.broadcast_to(m, (1, D, T, F)) for m in (xm, im, nm)), ban=ban), direct)
    block = Beamformer('mvdrSouden_ban', 'mask_mul', null_interferer=True, null_min_mass=1.0)
    assert np.array_equal(block(Y, xm, im + nm, interferer_mask=im, noise_mask=nm), direct * xm)
    # it is another signal than the MVDR of the merged mask
    assert rel_err(direct, ops.mvdr_souden_from_masks(Y, xm, im + nm, ban=True, ctx=gpu_ctx)) > 1e-2


# ------------------------------------------------------------------ 2. fallback
def test_a_frequency_without_interferer_takes_the_mvdr_of_the_merged_mask(gpu_ctx):
    from pb_chime5_amd import ops
    D, T, F, f0 = 5, 130, 4, 2
    Y, xm, im, nm, _ = _stage_scene(D, T, F)
    im = im.copy()
    im[:, f0] = 0.0                 # the interferer is silent in one frequency
    assert np.delete(im.sum(0), f0).min() > 1.5 * 2 * D      # the others are far from the bar
    for ban in (False, True):
        want, det = lr.lcmv_souden_from_masks(Y, xm, im, nm, ban, 2 * D)
        assert det['fallbacks'].tolist() == [f == f0 for f in range(F)]
        got, ref, fallbacks = ops.lcmv_souden_from_masks(
            Y, xm, im, nm, ban=ban, min_mass=2 * D, return_ref_channel=True,
            return_fallbacks=True, ctx=gpu_ctx)
        assert fallbacks == 1 == gpu_ctx.last_lcmv_fallbacks()
        assert ref == det['ref_channel']
        assert rel_err(got, want) <= STAGE_BAR
        mvdr = ops.mvdr_souden_from_masks(Y, xm, im + nm, ban=ban, ref_channel=ref, ctx=gpu_ctx)
        print(f'ban={ban}: fallback frequency vs gss_mvdr_souden {rel_err(got[:, f0], mvdr[:, f0]):.1e}')
        assert rel_err(got[:, f0], mvdr[:, f0]) <= STAGE_BAR
        assert rel_err(got[:, 0], mvdr[:, 0]) > 1e-3        # the others are no MVDR
    # min_mass = 0 never falls back: W = 0 in that frequency
    plain, fallbacks = ops.lcmv_souden_from_masks(Y, xm, im, nm, ban=False, min_mass=0,
                                                  return_fallbacks=True, ctx=gpu_ctx)
    assert fallbacks == 0 and np.all(plain[:, f0] == 0) and np.all(np.isfinite(plain))
    # ... which is 0 / 0 under the normalisation, as in the reference function
    nan = ops.lcmv_souden_from_masks(Y, xm, im, nm, ban=True, min_mass=0, ctx=gpu_ctx)
    assert np.all(np.isnan(nan[:, f0])) and np.all(np.isfinite(np.delete(nan, f0, axis=1)))


# ------------------------------------------------------------------ 3. it nulls
def test_the_interferer_is_nulled_and_the_target_passes(gpu_ctx):
    """Frames split into target-only, interferer-only and noise-only thirds with binary masks:
    Phi_X and Phi_I are rank one up to rounding.  The LCMV output on the interferer's frames is
    1e-9 of what the MVDR of the merged mask leaves there, and on the target's frames it is the
    reference channel's observation.  Cannot pass without the feature."""
    from pb_chime5_amd import ops
    D, T, F = 6, 192, 3
    rng = np.random.default_rng(63)
    d, a = lr.crandn(rng, F, D), lr.crandn(rng, F, D)
    third = T // 3
    tx, ti, tn = slice(0, third), slice(third, 2 * third), slice(2 * third, T)
    Yf = np.zeros((F, T, D), np.complex128)
    Yf[:, tx] = lr.crandn(rng, F, third)[..., None] * d[:, None]
    Yf[:, ti] = lr.crandn(rng, F, third)[..., None] * a[:, None]
    Yf[:, tn] = 0.3 * np.einsum('fde,fte->ftd', lr.crandn(rng, F, D, D),
                                lr.crandn(rng, F, T - 2 * third, D))
    Y = Yf.transpose(2, 1, 0)
    xm, im, nm = (np.zeros((T, F)) for _ in range(3))
    xm[tx], im[ti], nm[tn] = 1.0, 1.0, 1.0
    want, det = lr.lcmv_souden_from_masks(Y, xm, im, nm, False)
    assert np.linalg.cond(det['phi_n']).max() <= 1e4
    got, ref = ops.lcmv_souden_from_masks(Y, xm, im, nm, ban=False, return_ref_channel=True,
                                          ctx=gpu_ctx)
    mvdr = ops.mvdr_souden_from_masks(Y, xm, im + nm, ban=False, ref_channel=ref, ctx=gpu_ctx)
    left = np.abs(mvdr[ti]).max()
    print(f'interferer frames: LCMV {np.abs(got[ti]).max():.1e}, reference '
          f'{np.abs(want[ti]).max():.1e}, MVDR of N + I {left:.1e}; target frames vs channel {ref}: '
          f'{rel_err(got[tx], Y[ref, tx]):.1e}')
    assert ref == det['ref_channel']
    assert np.abs(want[ti]).max() <= 1e-9 * left        # the reference meets the bar too
    assert np.abs(got[ti]).max() <= 1e-9 * left
    assert rel_err(got[tx], Y[ref, tx]) <= 1e-9
    assert rel_err(got, want) <= STAGE_BAR


# ------------------------------------------------------------------ 4. singular Phi_N
def test_a_dead_channel_takes_the_minimum_norm_solution(gpu_ctx):
    """One dead channel at (5, 130, 2): Phi_N is exactly singular, both sides take lstsq.  Bar:
    max(1e-9, 10 x the reference's own movement under a last-bit change of Y on this scene).
    Measured on the reference: the movement is 6e-16, so the bar is 1e-9."""
    from pb_chime5_amd import ops
    D, T, F, dead = 5, 130, 2, 3
    Y, xm, im, nm, _ = lr.scene(np.random.default_rng(5130), D, T, F)
    Y[dead] = 0.0
    for ban in (False, True):
        want, det = lr.lcmv_souden_from_masks(Y, xm, im, nm, ban)
        assert np.all(det['phi_n'][:, dead] == 0) and np.all(det['phi_n'][:, :, dead] == 0)
        moved, mdet = lr.lcmv_souden_from_masks(_last_bit(Y), xm, im, nm, ban)
        assert mdet['ref_channel'] == det['ref_channel'] != dead
        movement = rel_err(moved, want)
        bar = max(1e-9, 10 * movement)
        got, ref = ops.lcmv_souden_from_masks(Y, xm, im, nm, ban=ban, return_ref_channel=True,
                                              ctx=gpu_ctx)
        print(f'dead channel, ban={ban}: rel err {rel_err(got, want):.1e}, reference moves '
              f'{movement:.1e}, bar {bar:.1e}')
        assert ref == det['ref_channel'] and np.all(np.isfinite(got))
        assert rel_err(got, want) <= bar


@pytest.mark.parametrize('ban', [False, True])
def test_the_fallback_on_a_dead_channel_gives_the_bits_of_the_mvdr(gpu_ctx, ban):
    """An empty interferer mask (every frequency falls back) and a dead channel (the merged matrix
    is exactly singular): the block is filled a second time with the merged sums and takes the
    minimum-norm branch.  The merged sums are S_N + 0 and s_N + 0, so the MVDR of (X, N) is the
    same arithmetic: equal bits, the same chosen channel.  On the CPU the reference
    (lcmv_reference.py) is finite on this scene and chooses channel 5."""
    from pb_chime5_amd import ops
    D, T, F, dead = 6, 130, 3, 2
    Y, xm, im, nm, _ = lr.scene(np.random.default_rng(6130), D, T, F)
    Y[dead] = 0.0
    im = np.zeros_like(im)
    got, ref, fallbacks = ops.lcmv_souden_from_masks(
        Y, xm, im, nm, ban=ban, min_mass=1.0, return_ref_channel=True, return_fallbacks=True,
        ctx=gpu_ctx)
    want, wref = ops.mvdr_souden_from_masks(Y, xm, nm, ban=ban, return_ref_channel=True,
                                            ctx=gpu_ctx)
    assert fallbacks == F == gpu_ctx.last_lcmv_fallbacks()
    assert np.all(np.isfinite(got))
    assert ref == wref
    assert np.array_equal(got, want)


# ------------------------------------------------------------------ 5. pick and masks
def _posteriors():
    """K = 5 posteriors (K,T,F), target 1, the noise class last; masses 2 > 3 > 0 > 4."""
    rng = np.random.default_rng(55)
    K, T, F = 5, 150, 3
    g = rng.uniform(0.05, 1.0, size=(K, T, F)) * np.array([0.8, 1.0, 3.0, 2.0, 0.5])[:, None, None]
    return g / g.sum(0)


PICK_CASES = [
    # candidates, interferer, drop_context, start, end -> expected class
    ([0, 2, 3], None, True, 7, 9, 2), ([0, 3], None, True, 7, 9, 3), ([0, 3, 4], None, True, 5, 0, 3),
    ([0, 1, 2, 3, 4], None, False, 7, 9, 2), ([], None, True, 7, 9, -1), ([1], None, True, 7, 9, -1),
    ([2, 3], 0, True, 7, 9, 0), ([], 4, True, 0, 0, 4), (None, None, True, 200, 0, -1),
]


@pytest.mark.parametrize('candidates,interferer,drop,start,end,expected', PICK_CASES)
def test_interferer_choice_and_masks_are_the_reference_bits(gpu_ctx, candidates, interferer, drop,
                                                           start, end, expected):
    from pb_chime5_amd import ops
    g = _posteriors()
    K, target = g.shape[0], 1
    cand = [k for k in range(K) if k != target] if candidates is None else candidates
    mass = lr.class_masses(g, start, end, drop)
    top = np.sort(mass[[k for k in set(cand) if k != target]])[::-1]
    if len(top) >= 2 and top[0] > 0:       # no near tie hides behind the summation order
        assert (top[0] - top[1]) / top[0] > 1e-6, top
    want = interferer if interferer is not None else lr.pick_interferer(g, target, cand, start,
                                                                         end, drop)
    assert want == expected
    wx, wi, wn = lr.masks_from_posteriors(g, target, want, start, end, drop)
    x, i, n, found = ops.lcmv_masks_from_posteriors(
        g, target, interferer=interferer, candidates=candidates, drop_context=drop,
        start_context_frames=start, end_context_frames=end, ctx=gpu_ctx)
    assert found == want == gpu_ctx.last_lcmv_interferer()
    assert np.array_equal(x, wx) and np.array_equal(i, wi) and np.array_equal(n, wn)
    if want < 0:
        assert np.all(i == 0)
    # X and I + N are the two masks of the MVDR's mask call where nothing is zeroed twice
    if drop and 0 < start < g.shape[1]:
        assert np.all(x[:start] == 0) and np.all(n[:start] == 0) and np.all(i[:start] == 0)


def test_the_context_decides_the_interferer(gpu_ctx):
    """Class 0 talks in the context frames only: with the context dropped, class 2 is chosen."""
    from pb_chime5_amd import ops
    g = _posteriors().copy()
    g[0, :10] = 50.0
    assert lr.pick_interferer(g, 1, [0, 2], 0, 0, False) == 0
    assert lr.pick_interferer(g, 1, [0, 2], 10, 0, True) == 2
    assert ops.lcmv_masks_from_posteriors(g, 1, candidates=[0, 2], drop_context=False,
                                          ctx=gpu_ctx)[3] == 0
    assert ops.lcmv_masks_from_posteriors(g, 1, candidates=[0, 2], start_context_frames=10,
                                          ctx=gpu_ctx)[3] == 2


# ------------------------------------------------------------------ 6. fused
FUSED = dict(stft_size=256, stft_shift=64, wpe_tabs=2, wpe_iterations=2, bss_iterations=5)


def _fused_scene(D, speakers):
    from pb_chime5_amd import synthetic
    # (a few hundred frames of 64 samples; sensor noise 30 dB below the speech keeps the WPE and
    # Phi_N well conditioned, as in the small pipeline tests)
    return synthetic.tiny(seed=40 + D, num_channels=D, num_samples=19200, num_speakers=speakers,
                          context=2048, noise=3e-2)


@pytest.mark.parametrize('D,speakers', [(6, 3), (4, 3)])
def test_fused_call_against_the_composition_of_stages_and_reference(gpu_ctx, D, speakers):
    """Enhancer.enhance_observation(bf_null_interferer=True) against STFT -> WPE -> posteriors
    (the existing stage operators) -> reference masks -> reference LCMV -> iSTFT: |X_hat| and
    x_hat at 1e-6 relative (the bar the issue of this feature sets; the small pipeline tests'
    TOL_STFT_MAG = 1e-4 against the oracle is wider), the same interferer; the block path
    equals the fused call at 1e-9; debug carries the interferer mask."""
    from pb_chime5_amd import ops
    from pb_chime5_amd.core import get_enhancer, start_end_context_frames
    from pb_chime5_amd.database.chime5 import activity_time_to_frequency
    u = _fused_scene(D, speakers)
    keys = list(u.activity)
    K, target = len(keys), keys.index(u.speaker_id)
    assert K == speakers + 1 and keys[-1] == 'Noise'
    enh = get_enhancer(**FUSED, bf_null_interferer=True)
    assert enh._fusable()
    got = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, debug=True)
    loc = enh.enhance_observation_locals
    det = loc['details']

    size, shift = FUSED['stft_size'], FUSED['stft_shift']
    Obs = ops.wpe_dtf(ops.stft(u.obs, size, shift, ctx=gpu_ctx), taps=2, delay=2, iterations=2,
                      ctx=gpu_ctx)
    actf = activity_time_to_frequency(np.array(list(u.activity.values())),
                                      stft_window_length=size, stft_shift=shift,
                                      stft_fading=True, stft_pad=True)
    posterior = ops.cacgmm_posteriors(Obs, actf, iterations=5, ctx=gpu_ctx)
    sf, ef = start_end_context_frames(u.ex, size, shift, True)
    assert sf > 0 and ef > 0
    cand = [k for k in range(K) if k != target and keys[k] != 'Noise']
    mass = np.sort(lr.class_masses(posterior, sf, ef)[cand])[::-1]
    assert (mass[0] - mass[1]) / mass[0] > 1e-3, mass
    interferer = lr.pick_interferer(posterior, target, cand, sf, ef)
    xm, im, nm = lr.masks_from_posteriors(posterior, target, interferer, sf, ef)
    margin = np.min(np.abs(im.sum(0) - 2 * D)) / (2 * D)
    assert margin > 1e-3, margin            # no frequency sits on the fallback threshold
    X_want, wdet = lr.lcmv_souden_from_masks(Obs, xm, im, nm, True, 2 * D)
    assert np.linalg.cond(wdet['phi_n']).max() <= 1e8
    want = ops.istft(X_want, size, shift, ctx=gpu_ctx)
    err = rel_err(np.abs(det['X_hat']), np.abs(X_want))
    print(f'D={D}: interferer {det["interferer"]} / {interferer}, fallbacks '
          f'{det["lcmv_fallbacks"]} / {int(wdet["fallbacks"].sum())} of {im.shape[1]}, |X_hat| '
          f'rel err {err:.1e}, x_hat {rel_err(got, want):.1e}, cond(Phi_N) '
          f'{np.linalg.cond(wdet["phi_n"]).max():.1e}')
    assert det['interferer'] == interferer == loc['interferer_index'] >= 0
    assert det['lcmv_fallbacks'] == int(wdet['fallbacks'].sum())
    assert det['ref_channel'] == wdet['ref_channel'] == enh._ctx().last_ref_channel()
    assert err <= 1e-6
    assert rel_err(got, want) <= 1e-6
    # the taps: the interferer's mask, and the distortion mask I + N
    assert np.array_equal(loc['interferer_mask'], lr.zero_context(det['posterior'], sf, ef)[interferer])
    assert rel_err(det['distortion_mask'], im + nm) <= 1e-9
    assert np.array_equal(det['target_mask'], lr.zero_context(det['posterior'], sf, ef)[target])
    # the block path
    blocks = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, fused=False,
                                     debug=True)
    bloc = enh.enhance_observation_locals
    print(f'D={D}: block path vs fused {rel_err(blocks, got):.1e}')
    assert bloc['interferer_index'] == interferer
    assert rel_err(blocks, got) <= 1e-9
    assert rel_err(bloc['distortion_mask'], im + nm) <= 1e-9
    # the option changes the signal
    plain = get_enhancer(**FUSED).enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex)
    assert rel_err(got, plain) > 1e-3


def test_fused_call_with_wpe_per_array(gpu_ctx):
    from pb_chime5_amd.core import get_enhancer
    u = _fused_scene(6, 3)
    enh = get_enhancer(**FUSED, bf_null_interferer=True, wpe_per_array=True,
                       multiarray='outer_array_mics')
    got = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, wpe_arrays=3)
    blocks = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, wpe_arrays=3,
                                     fused=False)
    joint = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, wpe_arrays=1)
    assert np.all(np.isfinite(got)) and rel_err(blocks, got) <= 1e-9
    assert rel_err(got, joint) > 1e-6


@pytest.mark.parametrize('D', [6, 4])
def test_target_and_noise_alone_give_the_bits_of_the_mvdr(gpu_ctx, D):
    """No competing talker: no candidate, every frequency falls back, and the fallback is the
    MVDR's arithmetic -- the output equals the enhancer without the option bit for bit."""
    from pb_chime5_amd.core import get_enhancer
    u = _fused_scene(D, 1)
    assert list(u.activity) == [u.speaker_id, 'Noise']
    enh = get_enhancer(**FUSED, bf_null_interferer=True)
    got = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, debug=True)
    det = enh.enhance_observation_locals['details']
    F = FUSED['stft_size'] // 2 + 1
    assert det['interferer'] == -1 and det['lcmv_fallbacks'] == F
    assert np.all(enh.enhance_observation_locals['interferer_mask'] == 0)
    plain = get_enhancer(**FUSED)
    want = plain.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, debug=True)
    wdet = plain.enhance_observation_locals['details']
    assert np.all(np.isfinite(want))
    assert det['ref_channel'] == wdet['ref_channel']
    assert np.array_equal(det['X_hat'], wdet['X_hat'])
    assert np.array_equal(got, want)
    assert np.array_equal(det['distortion_mask'], wdet['distortion_mask'])


# ------------------------------------------------------------------ 7. workspace
WORKSPACE_FRAMES = (64, 70, 1000, 2172)


@pytest.mark.parametrize('D', [4, 24])
def test_fresh_context_per_shape_stage_call(gpu_ctx, D):
    """A context that has never grown its arena, for every T: lcmv_workspace_bytes covers what
    the run allocates (a warmed arena would hide a missing term)."""
    from pb_chime5_amd import _capi
    F, Tmax = 513, max(WORKSPACE_FRAMES)
    rng = np.random.default_rng(D)
    flat = rng.standard_normal(2 * F * 64 * D)
    Y_d = gpu_ctx.to_device(np.resize(flat, 2 * F * Tmax * D).view(np.complex128))
    m = rng.uniform(0.05, 0.95, size=(3, F * Tmax))
    masks = [gpu_ctx.to_device(row / 3) for row in m]
    X_d = gpu_ctx.empty(16 * F * Tmax)
    p = _capi.c_void_p
    for i, T in enumerate(WORKSPACE_FRAMES):
        ctx = _capi.Context(0)
        try:
            status = ctx.lib.gss_lcmv_souden(
                ctx.handle, p(Y_d.ptr), F, T, D, p(masks[0].ptr), p(masks[1].ptr),
                p(masks[2].ptr), 1, -1, [0.0, 1e9][i % 2], p(X_d.ptr), None)
            assert status != _capi.GSS_ERR_NOMEM, (T, ctx.lib.gss_last_error(ctx.handle))
            ctx._check(status, f'gss_lcmv_souden T={T}')
            assert ctx.last_lcmv_fallbacks() == [0, F][i % 2]
        finally:
            ctx.close()


@pytest.mark.parametrize('D', [4, 24])
def test_fresh_context_per_shape_fused_call(gpu_ctx, D):
    from pb_chime5_amd import _capi, ops
    K = 3
    # (no WPE and one EM iteration: the beamformer's workspace is the largest stage)
    params = ops.make_params(wpe=False, bss_iterations=1)
    analysis = ops.analysis_window(1024)
    synthesis = ops.synthesis_window(analysis, 256)
    samples = []
    for t in WORKSPACE_FRAMES:
        n = max(t * 256 - 1024 - 700, 256)
        while ops.stft_frames(n, 1024, 256, True) < t:
            n += 256
        assert ops.stft_frames(n, 1024, 256, True) == t
        samples.append(n)
    Nmax = max(samples)
    rng = np.random.default_rng(D)
    obs_d = gpu_ctx.to_device(rng.standard_normal((D, Nmax)))           # (D,N): its head
    act = rng.random((K, Nmax)) < 0.7
    act[-1] = True
    act_d = gpu_ctx.to_device(act.astype(np.uint8))
    Tmax = ops.stft_frames(Nmax, 1024, 256, True)
    out_d = gpu_ctx.empty(8 * int(gpu_ctx.lib.gss_istft_num_samples(Tmax, 1024, 256, 1)))
    p = _capi.c_void_p
    for i, N in enumerate(samples):
        bf = ops.check_bf_lcmv(K, 0, None, None, [0.0, 2.0 * D][i % 2])
        ctx = _capi.Context(0)
        try:
            ctx.set_windows(1024, 256, analysis, synthesis)
            status = ctx.lib.gss_enhance_observation_lcmv(
                ctx.handle, ctypes.byref(params), p(obs_d.ptr), D, N, p(act_d.ptr), K, Nmax, 0,
                0, 0, ctypes.byref(bf), p(out_d.ptr), None)
            assert status != _capi.GSS_ERR_NOMEM, (N, ctx.lib.gss_last_error(ctx.handle))
            ctx._check(status, f'gss_enhance_observation_lcmv N={N}')
            assert ctx.last_lcmv_interferer() in (1, 2)
        finally:
            ctx.close()


# ------------------------------------------------------------------ 8. error codes
def test_c_abi_argument_errors_name_the_field(gpu_ctx):
    from pb_chime5_amd import _capi, ops
    ctx = gpu_ctx
    F, T, D, K = 3, 130, 4, 3
    buf = ctx.empty(16 * F * T * max(D, K))
    p = _capi.c_void_p(buf.ptr)
    INVALID = _capi.GSS_ERR_INVALID

    def error():
        return ctx.lib.gss_last_error(ctx.handle).decode()

    def stage(D=D, ref=-1, min_mass=0.0, mask=p):
        return ctx.lib.gss_lcmv_souden(ctx.handle, p, F, T, D, p, mask, p, 1, ref, min_mass, p, None)
    for kw, word in ((dict(D=1), 'D = 1'), (dict(D=30), 'D < 30'), (dict(D=0), 'D = 0'),
                     (dict(ref=D), 'ref_channel'), (dict(ref=-2), 'ref_channel'),
                     (dict(min_mass=-0.5), 'min_mass'), (dict(min_mass=float('nan')), 'min_mass'),
                     (dict(min_mass=float('inf')), 'min_mass'), (dict(mask=None), 'bad arguments')):
        assert stage(**kw) == INVALID, kw
        assert word in error(), (kw, error())

    def masks(bf, target=0, K=K):
        return ctx.lib.gss_lcmv_masks_from_posteriors(
            ctx.handle, p, F, K, T, target, ctypes.byref(bf) if bf is not None else None, 1, 0, 0,
            p, p, p, None)
    good = dict(interferer=-1, candidates=0b110, min_mass=1.0)
    for bad, word in ((dict(interferer=K), 'interferer'), (dict(interferer=-2), 'interferer'),
                      (dict(interferer=0), 'interferer'), (dict(min_mass=-1.0), 'min_mass'),
                      (dict(min_mass=float('nan')), 'min_mass')):
        assert masks(_capi.GssBfLcmv(**{**good, **bad})) == INVALID, bad
        assert word in error(), (bad, error())
    assert masks(None) == INVALID and 'lcmv' in error()
    assert masks(_capi.GssBfLcmv(**good), target=K) == INVALID and 'target_index' in error()
    assert masks(_capi.GssBfLcmv(**good), K=20) == INVALID and 'K' in error()

    ops._prepare_windows(ctx, 1024, 256)
    big = ctx.empty(8 * 4 * 4096)
    q = _capi.c_void_p(big.ptr)

    def fused(bf, params=None, D=4, target=0):
        params = params or ops.make_params()
        return ctx.lib.gss_enhance_observation_lcmv(
            ctx.handle, ctypes.byref(params), q, D, 4096, q, 2, 4096, target, 0, 0,
            ctypes.byref(bf) if bf is not None else None, q, None)
    ok = _capi.GssBfLcmv(-1, 0b10, 1.0)
    for name in ('gev_ban', 'ch2', 'sum'):
        assert fused(ok, ops.make_params(bf=name)) == _capi.GSS_ERR_UNSUPPORTED, name
    assert fused(None) == INVALID and 'lcmv' in error()
    assert fused(ok, D=1) == INVALID and 'D = 1' in error()
    assert fused(ok, D=30) == INVALID and 'D < 30' in error()
    assert fused(ok, target=2) == INVALID and 'target_index' in error()
    assert fused(_capi.GssBfLcmv(0, 0, 1.0)) == INVALID and 'interferer' in error()
    assert fused(_capi.GssBfLcmv(2, 0, 1.0)) == INVALID and 'interferer' in error()
    assert fused(_capi.GssBfLcmv(-1, 0, -1.0)) == INVALID and 'min_mass' in error()

    out32, out64 = ctypes.c_int32(7), ctypes.c_int64(-1)
    assert ctx.lib.gss_last_lcmv_interferer(ctx.handle, None) == INVALID
    assert ctx.lib.gss_last_lcmv_fallbacks(ctx.handle, None) == INVALID
    assert ctx.lib.gss_last_lcmv_interferer(ctx.handle, ctypes.byref(out32)) == 0
    assert ctx.lib.gss_last_lcmv_fallbacks(ctx.handle, ctypes.byref(out64)) == 0 <= out64.value
    assert -1 <= out32.value < 19


def test_nonfinite_snr_raises_like_the_mvdr(gpu_ctx):
    from pb_chime5_amd import ops
    D, T, F = 5, 130, 4
    Y, xm, im, nm, _ = _stage_scene(D, T, F)
    X = ops.lcmv_souden_from_masks(Y, xm, im, nm, ban=True, ctx=gpu_ctx)
    Ybad = Y.copy()
    Ybad[2, 70, 3] = np.nan
    with pytest.raises(AssertionError):
        lr.lcmv_souden_from_masks(Ybad, xm, im, nm, True)
    with pytest.raises(AssertionError):
        ops.lcmv_souden_from_masks(Ybad, xm, im, nm, ban=True, ctx=gpu_ctx)
    assert gpu_ctx.last_ref_channel() == -1
    # the next utterance on the same context is not affected
    assert np.array_equal(ops.lcmv_souden_from_masks(Y, xm, im, nm, ban=True, ctx=gpu_ctx), X)
