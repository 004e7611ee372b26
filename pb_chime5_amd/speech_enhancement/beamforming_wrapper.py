"""Mask-based beamforming front door with the reference's call surface
(/root/reference/pb_chime5/speech_enhancement/beamforming_wrapper.py:11-171).

``beamform_mvdr_souden_from_masks(Y, X_mask, N_mask, ban=False)`` accepts the same
layouts as the reference -- Y (D,T,F) or (1,D,T,F); masks (T,F), (D,T,F) or
(1,D,T,F), median-reduced over the channel axis -- and returns X_hat (T,F)
complex128.  PSD accumulation, the Souden MVDR solve, the cross-frequency
reference-channel choice, BAN and the filter application run in the HIP library.
"""
import numpy as np

from pb_chime5_amd import ops
from pb_chime5_amd.utils.numpy_utils import morph


class _Beamformer:
    """Layout normalisation + lazily evaluated results, like the reference's
    helper class; the arithmetic is one ``gss_mvdr_souden`` call per variant."""

    def __init__(self, Y, X_mask, N_mask, debug=False, ctx=None, segments=None):
        self.debug = debug
        self._ctx = ctx
        # segments: keyword arguments of ops.mvdr_souden_segments_from_masks (the statistics
        # per segment of frames) or None: one window, the reference's beamformer
        self._segments = segments
        if np.ndim(Y) == 4:
            self.Y = morph('1DTF->FDT', Y)
        else:
            self.Y = morph('DTF->FDT', Y)

        if np.ndim(X_mask) == 4:
            self.X_mask = morph('1DTF->FT', X_mask, reduce=np.median)
            self.N_mask = morph('1DTF->FT', N_mask, reduce=np.median)
        elif np.ndim(X_mask) == 3:
            self.X_mask = morph('DTF->FT', X_mask, reduce=np.median)
            self.N_mask = morph('DTF->FT', N_mask, reduce=np.median)
        elif np.ndim(X_mask) == 2:
            self.X_mask = morph('TF->FT', X_mask)
            self.N_mask = morph('TF->FT', N_mask)
        else:
            raise NotImplementedError(np.shape(X_mask))

        assert self.Y.ndim == 3, self.Y.shape
        F, D, T = self.Y.shape
        assert D < 30, (D, self.Y.shape)
        assert self.X_mask.shape == (F, T), (self.X_mask.shape, F, T)
        assert self.N_mask.shape == (F, T), (self.N_mask.shape, F, T)
        self._cache = {}

    def _run(self, ban):
        if ban not in self._cache and self._segments is not None:
            self._cache[ban] = ops.mvdr_souden_segments_from_masks(
                self.Y.transpose(1, 2, 0), self.X_mask.T, self.N_mask.T, ban=ban,
                return_ref_channel=True, ctx=self._ctx, **self._segments)
        elif ban not in self._cache:
            self._cache[ban] = ops.mvdr_souden_from_masks(
                self.Y.transpose(1, 2, 0), self.X_mask.T, self.N_mask.T, ban=ban,
                return_ref_channel=True, ctx=self._ctx)
        return self._cache[ban]

    @property
    def X_hat_mvdr_souden(self):
        return self._run(False)[0]

    @property
    def X_hat_mvdr_souden_ban(self):
        return self._run(True)[0]

    @property
    def ref_channel(self):
        return self._run(True)[1]

    def _gev(self, ban):
        key = ('gev', ban)
        if key not in self._cache:
            self._cache[key] = ops.gev_from_masks(
                self.Y.transpose(1, 2, 0), self.X_mask.T, self.N_mask.T, ban=ban, ctx=self._ctx)
        return self._cache[key]

    @property
    def X_hat_gev(self):
        return self._gev(False)

    @property
    def X_hat_gev_ban(self):
        return self._gev(True)


def beamform_gev_from_masks(Y, X_mask, N_mask, ban=True, debug=False, ctx=None):
    """beamforming_wrapper.py:192-208."""
    bf = _Beamformer(Y=Y, X_mask=X_mask, N_mask=N_mask, debug=debug, ctx=ctx)
    if ban:
        return bf.X_hat_gev_ban
    return bf.X_hat_gev


def beamform_mvdr_souden_from_masks(Y, X_mask, N_mask, ban=False, debug=False, ctx=None, *,
                                    segment_frames=None, segment_context=0,
                                    segment_min_mass=None):
    """``segment_frames`` (an addition; None: the reference's one window per call): a
    time-varying filter with statistics per segment of that many frames, see
    ``ops.mvdr_souden_segments_from_masks``."""
    segments = None
    if segment_frames is not None:
        ops.check_bf_segments(segment_frames, segment_context, segment_min_mass)
        segments = dict(segment_frames=segment_frames, segment_context=segment_context,
                        min_mass=segment_min_mass)
    bf = _Beamformer(Y=Y, X_mask=X_mask, N_mask=N_mask, debug=debug, ctx=ctx,
                     segments=segments)
    if ban:
        return bf.X_hat_mvdr_souden_ban
    return bf.X_hat_mvdr_souden


def beamform_lcmv_souden_from_masks(Y, X_mask, I_mask, N_mask, ban=False, debug=False, *,
                                    ref_channel=None, ctx=None):
    """beamforming_wrapper.py:127-171: Souden's LCMV from target, interferer and noise masks,
    with the reference's layouts -- Y (D,T,F) or (1,D,T,F); masks (T,F), (D,T,F) or (1,D,T,F),
    median-reduced over the channel axis.  Nothing falls back to the MVDR (``min_mass=0`` of
    ``ops.lcmv_souden_from_masks``): an empty interferer mask gives NaN under ``ban``, as
    upstream.  ``ref_channel`` (an addition): the reference channel; None = the SNR argmax."""
    if np.ndim(Y) == 4:
        Y = morph('1DTF->FDT', Y)
    else:
        Y = morph('DTF->FDT', Y)
    if np.ndim(X_mask) == 4:
        pattern = '1DTF->FT'
    elif np.ndim(X_mask) == 3:
        pattern = 'DTF->FT'
    elif np.ndim(X_mask) == 2:
        pattern = 'TF->FT'
    else:
        raise NotImplementedError(np.shape(X_mask))
    if pattern == 'TF->FT':
        X_mask, I_mask, N_mask = (morph(pattern, m) for m in (X_mask, I_mask, N_mask))
    else:
        X_mask, I_mask, N_mask = (morph(pattern, m, reduce=np.median)
                                  for m in (X_mask, I_mask, N_mask))
    assert Y.ndim == 3, Y.shape
    F, D, T = Y.shape
    assert D < 30, (D, Y.shape)
    for m in (X_mask, I_mask, N_mask):
        assert m.shape == (F, T), (m.shape, F, T)
    return ops.lcmv_souden_from_masks(Y.transpose(1, 2, 0), X_mask.T, I_mask.T, N_mask.T,
                                      ban=ban, min_mass=0.0, ref_channel=ref_channel, ctx=ctx)


def beamform_wpd_souden_from_masks(Y, X_mask, ban=False, *, taps=10, delay=2, iterations=1,
                                   power_floor=ops.WPD_POWER_FLOOR, frame_gate=None,
                                   ref_channel=None, ctx=None):
    """The WPD convolutional beamformer (an addition; ``ops.wpd_souden_from_masks``) with the
    layouts of its siblings -- Y (D,T,F) or (1,D,T,F), the observation BEFORE dereverberation;
    X_mask (T,F), (D,T,F) or (1,D,T,F), median-reduced over the channel axis -- and X_hat (T,F)
    out.  ``frame_gate`` (T,) of 0 / 1: frames that enter no statistic (None: none).
    ``power_floor`` = 1e-3 is a choice, not a measurement."""
    if np.ndim(Y) == 4:
        Y = morph('1DTF->FDT', Y)
    else:
        Y = morph('DTF->FDT', Y)
    if np.ndim(X_mask) == 4:
        X_mask = morph('1DTF->FT', X_mask, reduce=np.median)
    elif np.ndim(X_mask) == 3:
        X_mask = morph('DTF->FT', X_mask, reduce=np.median)
    elif np.ndim(X_mask) == 2:
        X_mask = morph('TF->FT', X_mask)
    else:
        raise NotImplementedError(np.shape(X_mask))
    assert Y.ndim == 3, Y.shape
    F, D, T = Y.shape
    assert D < 30, (D, Y.shape)
    assert X_mask.shape == (F, T), (X_mask.shape, F, T)
    return ops.wpd_souden_from_masks(Y.transpose(1, 2, 0), X_mask.T, ban=ban, taps=taps,
                                     delay=delay, iterations=iterations, power_floor=power_floor,
                                     frame_gate=frame_gate, ref_channel=ref_channel, ctx=ctx)
