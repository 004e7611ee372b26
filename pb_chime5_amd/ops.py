"""NumPy-in / NumPy-out operators of the hot path, executed on the GPU through the
C ABI (include/gss_hip.h).  Shapes, dtypes and argument meaning follow the
third-party functions the reference calls, so the blocks in ``core.py`` read like
the reference's:

=========================  ====================================================
here                        reference call (file:line)
=========================  ====================================================
``stft`` / ``istft``        nara_wpe.utils.stft / istft   (core.py:305-321)
``wpe_v8``                  nara_wpe.wpe.wpe_v8           (core.py:52-58)
``wpe_online_dtf`` / ``OnlineWPEState`` / ``enhance_observation_wpe_online``
                            nara_wpe's online (frame-recursive) WPE with a carried state, which
                            the reference never calls
``cacgmm_posteriors``       CACGMMTrainer.fit + predict   (core.py:165-208)
``cacgmm_posteriors_guided``  the same from any initialisation / source_activity_mask
``cacgmm_posteriors_shared_prior`` / ``cacgmm_posteriors_blind`` / ``blind_initialization``
                            the same with one prior per class and frame for all frequencies
                            (pb_bss ``weight_constant_axis=-3``, which the reference never
                            calls): separation without an annotation
``align_posteriors`` / ``alignment_plan`` / ``cacgmm_model_permute`` / ``cacgmm_fit_blind``
                            the classes of a per-frequency model aligned across frequencies
                            (what pb_bss users run after a blind fit; the reference never does):
                            an annotation-free model object
``link_posteriors`` / ``separate_observation``
                            the classes of two overlapping windows linked on the frames they
                            share, and the annotation-free window as one fused call (what
                            `Enhancer.enhance_recording_blind` is built of; not in the reference)
``mvdr_souden_from_masks``  pb_bss beamformer chain       (beamforming_wrapper.py:51-97)
``mvdr_souden_segments_from_masks``  the same with statistics per segment of frames
``mvdr_souden_online_from_masks`` / ``OnlineMVDRState`` / ``enhance_observation_bf_online``
                            the same with exponentially forgetting running sums, a filter per
                            frame and a carried state (not in the reference)
``cacgmm_posteriors_online`` / ``OnlineCACGMMState`` / ``enhance_observation_gss_online``
                            the recursive (online) EM of the mixture model: running sums that
                            forget, causal posteriors and a carried state (not in the reference)
``StreamState`` / ``stft_stream`` / ``istft_stream`` / ``stream_block`` / ``masks_from_posteriors``
                            the two ends of a sample-block stream with a carried state and one
                            block through the three online stages (not in the reference; the
                            front door is ``streaming.StreamingEnhancer``)
``StreamTails`` / ``mvdr_souden_online_targets`` / ``istft_stream_targets`` / ``stream_block_targets``
                            the same for several targets of one stream from one pass (not in
                            the reference; ``StreamingEnhancer(targets=...)``)
``lcmv_souden_from_masks``  beamform_lcmv_souden_from_masks (beamforming_wrapper.py:127-171)
``lcmv_masks_from_posteriors`` / ``enhance_observation_lcmv``
                            the interferer-nulling LCMV fed from the posteriors
``enhance_observation``     Enhancer.enhance_observation  (core.py:514-571)
``channel_scores`` / ``select_channels`` / ``enhance_observation_select``
                            envelope-variance channel selection ahead of WPE (not in the
                            reference, which picks microphones by position)
``posterior_activity`` / ``enhance_observation_activity``
                            the power-weighted share of every frame that the posteriors give
                            each class (not in the reference)
=========================  ====================================================

All of them raise if libgss_hip.so or a GPU is missing.
"""
import ctypes
from types import SimpleNamespace

import numpy as np

from . import _capi
from ._capi import (Context, GssBfLcmv, GssBfSegments, GssBfWpd, GssCacgmmModel,
                    GssCacgmmOnlineState, GssChannelSelect, GssEmOnline,
                    GssBfOnline, GssDebugTaps, GssGuidance, GssMvdrOnlineHold, GssMvdrOnlineState,
                    GssParams,
                    GssStreamCfg, GssStreamState, GssWpeOnlineCfg, GssWpeOnlineState, c_void_p,
                    default_context)
from .cacgmm import CACGMM

_BF_CODES = {'mvdrSouden_ban': 0, 'ch2': 1, 'sum': 2, 'gev_ban': 3}
_POSTFILTER_CODES = {None: 0, 'mask_mul': 1}
_MAX_CHANNELS, _MAX_CLASSES = 32, 19      # include/gss_hip.h: GSS_MAX_CHANNELS, GSS_MAX_CLASSES


# --------------------------------------------------------------------------
# windows (host logic, float64; nara_wpe.utils.stft / istft)
# --------------------------------------------------------------------------
def analysis_window(size, window=None):
    """Periodic window ``window(size + 1)[:-1]`` (nara_wpe ``symmetric_window=False``);
    default scipy.signal blackman."""
    if window is None:
        from scipy.signal.windows import blackman as window
    if callable(window):
        return np.asarray(window(size + 1)[:-1], dtype=np.float64)
    w = np.asarray(window, dtype=np.float64)
    assert w.shape == (size,), (w.shape, size)
    return w


def synthesis_window(analysis, shift):
    """Biorthogonal synthesis window as nara_wpe's istft builds it: analysis /
    (sum over the size/shift shifted copies of analysis**2), where the upstream
    loop leaves the very last sample out of that sum."""
    w = np.asarray(analysis, dtype=np.float64)
    size = len(w)
    assert size % shift == 0, (size, shift)
    number_of_shifts = size // shift
    sq = w ** 2
    sq[-1] = 0.0
    # upstream accumulates shift by shift in increasing order
    sum_of_squares = np.zeros(shift)
    for j in range(number_of_shifts):
        sum_of_squares += sq[j * shift:(j + 1) * shift]
    return w / np.tile(sum_of_squares, number_of_shifts)


def _prepare_windows(ctx, size, shift, window=None):
    # (the shift has to divide the window: nara_wpe's istft asserts it for its synthesis window,
    # and the library keeps one (size, shift) pair of windows per context for both directions)
    a = analysis_window(size, window)
    s = synthesis_window(a, shift)
    ctx.set_windows(size, shift, a, s)


def stft_frames(num_samples, size, shift, fading=True):
    return int(_capi.load_library().gss_stft_num_frames(
        int(num_samples), size, shift, int(bool(fading))))


def samples_to_stft_frames(samples, size, shift, *, fading=False):
    """nara_wpe.utils._samples_to_stft_frames(pad=True) (core.py:224-237)."""
    return int(_capi.load_library().gss_samples_to_stft_frames(
        int(samples), size, shift, int(bool(fading))))


# --------------------------------------------------------------------------
# stage operators
# --------------------------------------------------------------------------
def stft(time_signal, size=1024, shift=256, *, window=None, fading=True, ctx=None):
    """(..., N) real -> (..., T, size//2+1) complex128."""
    ctx = ctx or default_context()
    x = np.asarray(time_signal, dtype=np.float64)
    lead = x.shape[:-1]
    N = x.shape[-1]
    D = int(np.prod(lead, dtype=np.int64)) if lead else 1
    x2 = np.ascontiguousarray(x.reshape(D, N))
    _prepare_windows(ctx, size, shift, window)
    F = size // 2 + 1
    T = stft_frames(N, size, shift, fading)
    if D == 0 or T == 0:
        return np.zeros(lead + (T, F), np.complex128)
    if N == 0:          # nothing but the fading pad: frames of zeros
        return np.zeros(lead + (T, F), np.complex128)
    x_d = ctx.to_device(x2)
    Y_d = ctx.empty(16 * F * T * D)
    O_d = ctx.empty(16 * F * T * D)
    lib = ctx.lib
    ctx._check(lib.gss_stft(ctx.handle, c_void_p(x_d.ptr), D, N, int(bool(fading)),
                            c_void_p(Y_d.ptr)), 'gss_stft')
    ctx._check(lib.gss_layout_ftd_to_dtf(ctx.handle, c_void_p(Y_d.ptr), F, T, D,
                                         c_void_p(O_d.ptr)), 'gss_layout_ftd_to_dtf')
    out = ctx.to_host(O_d, (D, T, F), np.complex128)
    return out.reshape(lead + (T, F))


def istft(stft_signal, size=1024, shift=256, *, window=None, fading=True, ctx=None):
    """(..., T, size//2+1) complex -> (..., N') float64."""
    ctx = ctx or default_context()
    X = np.asarray(stft_signal, dtype=np.complex128)
    F = size // 2 + 1
    assert X.shape[-1] == F, X.shape
    lead = X.shape[:-2]
    T = X.shape[-2]
    X2 = np.ascontiguousarray(X.reshape((-1, T, F)))
    _prepare_windows(ctx, size, shift, window)
    n_out = int(ctx.lib.gss_istft_num_samples(T, size, shift, int(bool(fading))))
    out = np.empty((X2.shape[0], n_out))
    x_d = ctx.empty(8 * max(n_out, 1))
    for i in range(X2.shape[0]):
        X_d = ctx.to_device(X2[i])
        ctx._check(ctx.lib.gss_istft(ctx.handle, c_void_p(X_d.ptr), T, int(bool(fading)),
                                     c_void_p(x_d.ptr)), 'gss_istft')
        out[i] = ctx.to_host(x_d, (n_out,), np.float64)
    return out.reshape(lead + (n_out,))


def _obs_to_device_ftd(ctx, Obs):
    """(D,T,F) complex host array -> device (F,T,D)."""
    Obs = np.asarray(Obs, dtype=np.complex128)
    assert Obs.ndim == 3, Obs.shape
    D, T, F = Obs.shape
    src = ctx.to_device(Obs)
    dst = ctx.empty(16 * F * T * D)
    ctx._check(ctx.lib.gss_layout_dtf_to_ftd(ctx.handle, c_void_p(src.ptr), D, T, F,
                                             c_void_p(dst.ptr)), 'gss_layout_dtf_to_ftd')
    return dst, (D, T, F)


def _ftd_to_host_dtf(ctx, buf, D, T, F):
    tmp = ctx.empty(16 * F * T * D)
    ctx._check(ctx.lib.gss_layout_ftd_to_dtf(ctx.handle, c_void_p(buf.ptr), F, T, D,
                                             c_void_p(tmp.ptr)), 'gss_layout_ftd_to_dtf')
    return ctx.to_host(tmp, (D, T, F), np.complex128)


PSD_CONTEXT_ALL = 2 ** 31 - 1      # "every frame": what np.inf means upstream


def check_psd_context(psd_context):
    """nara_wpe.wpe.get_power takes a non-negative integer (frames either side of t, default 0:
    core.py:56,583) or np.inf (the mean over all frames); both are implemented -- np.inf as a
    window that always covers the whole utterance.  Everything else ((left, right) tuples --
    an argument of upstream's window_mean, not of get_power --, fractions, negative values)
    is refused in ONE place with NotImplementedError: never truncated, never a TypeError /
    OverflowError out of int()."""
    if isinstance(psd_context, (float, np.floating)) and np.isposinf(psd_context):
        return PSD_CONTEXT_ALL
    ok = isinstance(psd_context, (int, np.integer)) and not isinstance(psd_context, bool)
    if not ok and isinstance(psd_context, (float, np.floating)):
        ok = np.isfinite(psd_context) and float(psd_context).is_integer()
    if not ok or psd_context < 0 or psd_context > PSD_CONTEXT_ALL:
        raise NotImplementedError(
            f'psd_context={psd_context!r}: a non-negative integer number of frames or np.inf')
    return int(psd_context)


def wpe_dtf(Obs, taps=10, delay=2, iterations=3, psd_context=0, *, ctx=None):
    """WPE on the reference's (D,T,F) layout (what ``WPE.__call__`` hands over
    transposed to wpe_v8 and transposes back, core.py:52-58)."""
    psd_context = check_psd_context(psd_context)
    ctx = ctx or default_context()
    Y_d, (D, T, F) = _obs_to_device_ftd(ctx, Obs)
    X_d = ctx.empty(16 * F * T * D)
    ctx._check(ctx.lib.gss_wpe(ctx.handle, c_void_p(Y_d.ptr), F, T, D, int(taps), int(delay),
                               int(iterations), int(psd_context), c_void_p(X_d.ptr)), 'gss_wpe')
    return _ftd_to_host_dtf(ctx, X_d, D, T, F)


def wpe_arrays_dtf(Obs, arrays, taps=10, delay=2, iterations=3, psd_context=0, *, ctx=None):
    """WPE per microphone array on the reference's (A*C, T, F) layout: the ``arrays`` groups
    of C = D / arrays consecutive channels (array-major, the morph('ACN->A*CN') order of
    enhance_example) are dereverberated independently, in ONE device call (gss_wpe_arrays) --
    ``WPE.__call__(Obs.reshape(A, C, T, F), stack=False).reshape(A * C, T, F)``."""
    psd_context = check_psd_context(psd_context)
    ctx = ctx or default_context()
    D = np.shape(Obs)[0]
    A = check_wpe_arrays(arrays, D)
    Y_d, (D, T, F) = _obs_to_device_ftd(ctx, Obs)
    X_d = ctx.empty(16 * F * T * D)
    ctx._check(ctx.lib.gss_wpe_arrays(ctx.handle, c_void_p(Y_d.ptr), F, T, A, D // A, int(taps),
                                      int(delay), int(iterations), int(psd_context),
                                      c_void_p(X_d.ptr)), 'gss_wpe_arrays')
    return _ftd_to_host_dtf(ctx, X_d, D, T, F)


def check_wpe_arrays(arrays, num_channels=None):
    """The number of microphone arrays of a per-array WPE (0, 1 or None: one joint WPE -> 1).
    It must split ``num_channels`` into arrays of equal size: ValueError otherwise."""
    if arrays is None:
        arrays = 0
    if isinstance(arrays, bool) or not isinstance(arrays, (int, np.integer)) or arrays < 0:
        raise ValueError(f'wpe_arrays={arrays!r}: a non-negative integer')
    A = max(int(arrays), 1)
    if num_channels is not None and num_channels % A:
        raise ValueError(f'wpe_arrays={A} does not divide the {num_channels} channels into '
                         'arrays of equal size')
    return A


def get_power_inverse(signal, psd_context=0, *, ctx=None):
    """nara_wpe.wpe.get_power_inverse: signal (F, D, T) -> (F, T), the weights of one WPE
    iteration (mean channel power, smoothed over [t - psd_context, t + psd_context], floored
    at 1e-10 of its maximum over time, inverted)."""
    psd_context = check_psd_context(psd_context)
    ctx = ctx or default_context()
    signal = np.asarray(signal, dtype=np.complex128)
    Y_d, (D, T, F) = _obs_to_device_ftd(ctx, signal.transpose(1, 2, 0))
    w_d = ctx.empty(8 * F * T)
    ctx._check(ctx.lib.gss_wpe_inverse_power(ctx.handle, c_void_p(Y_d.ptr), F, T, D,
                                             int(psd_context), c_void_p(w_d.ptr)),
               'gss_wpe_inverse_power')
    return ctx.to_host(w_d, (F, T), np.float64)


def wpe_v8(Y, taps=10, delay=3, iterations=3, psd_context=0, *, ctx=None):
    """nara_wpe.wpe.wpe_v8 signature: Y (..., D, T) with the frequency (independent)
    axes leading; returns the same shape."""
    Y = np.asarray(Y, dtype=np.complex128)
    if Y.ndim == 2:
        return wpe_v8(Y[None], taps, delay, iterations, psd_context, ctx=ctx)[0]
    lead = Y.shape[:-2]
    D, T = Y.shape[-2:]
    Yf = Y.reshape((-1, D, T))
    out = wpe_dtf(Yf.transpose(1, 2, 0), taps, delay, iterations, psd_context, ctx=ctx)
    return out.transpose(2, 0, 1).reshape(lead + (D, T))


# --------------------------------------------------------------------------
# online WPE (gss_wpe_online): frame-recursive, exponentially forgetting, with a carried state
# --------------------------------------------------------------------------
WPE_ONLINE_ALPHA = 0.9999   # the forgetting factor: a choice, not a measurement
WPE_ONLINE_MAX_N = 512      # include/gss_hip.h: taps * channels per array


def check_wpe_online(taps=10, delay=2, alpha=WPE_ONLINE_ALPHA, num_channels=None, arrays=1):
    """The settings of the online WPE -- the one place that validates them, before any device
    work.  ValueError naming the argument: ``taps`` an integer >= 1, ``delay`` an integer >= 0,
    ``alpha`` a finite number in (0, 1], ``arrays`` as `check_wpe_arrays` (it must divide
    ``num_channels``), ``num_channels`` a positive integer.  NotImplementedError for what the
    kernels are not built for: more than 32 channels, taps * channels per array > 512.
    Returns (A, C) -- C None without ``num_channels``."""
    for name, value, low in (('taps', taps, 1), ('delay', delay, 0)):
        if not _is_integer(value) or value < low or value >= 2 ** 20:
            raise ValueError(f'{name}={value!r}: an integer >= {low} (and below 2^20)')
    if not _is_real(alpha) or not np.isfinite(alpha) or not 0 < alpha <= 1:
        raise ValueError(f'alpha={alpha!r}: a finite number in (0, 1]')
    if num_channels is not None and (not _is_integer(num_channels) or num_channels < 1):
        raise ValueError(f'num_channels={num_channels!r}: a positive integer')
    A = check_wpe_arrays(arrays, num_channels)
    if num_channels is None:
        return A, None
    C = int(num_channels) // A
    if num_channels > _MAX_CHANNELS:
        raise NotImplementedError(f'num_channels={num_channels}: at most {_MAX_CHANNELS}')
    if taps * C > WPE_ONLINE_MAX_N:
        raise NotImplementedError(f'taps={taps} on {C} channels per array: taps * channels = '
                                  f'{taps * C} is larger than {WPE_ONLINE_MAX_N}')
    return A, C


class _OnlineState:
    """What the states of the online stages share: named buffers in HBM whose shapes follow from
    the sizes the state is built for (``key``), and their way to the host and back.  A subclass
    says how the shapes follow from the sizes (`_shapes`), names the sizes (``_sizes``, for the
    messages) and the buffers that are not complex128 (``dtypes``), and has its own ``struct``,
    ``fresh`` and the shape inference at the head of ``from_host``."""
    dtypes = {}

    def __init__(self, ctx, *sizes):
        self.ctx = ctx
        self.key = tuple(int(v) for v in sizes)
        self.shapes = self._shapes(*self.key)
        self.bufs = {k: ctx.empty(np.dtype(self.dtypes.get(k, np.complex128)).itemsize
                                  * int(np.prod(shape, dtype=np.int64)))
                     for k, shape in self.shapes.items()}

    def to_host(self):
        """The buffers as NumPy arrays by name: everything `from_host` needs (synchronises)."""
        return {k: self.ctx.to_host(self.bufs[k], shape, self.dtypes.get(k, np.complex128))
                for k, shape in self.shapes.items()}

    @classmethod
    def _from_host(cls, host, sizes, ctx, expected=str):
        """The tail of ``from_host``: every array of ``host`` against the shapes of ``sizes``
        (ValueError; ``expected(shape)`` words the shape it should have had), then the upload."""
        arrays = {}
        for k, shape in cls._shapes(*sizes).items():
            arrays[k] = a = np.ascontiguousarray(host[k], dtype=cls.dtypes.get(k, np.complex128))
            if a.shape != shape:
                raise ValueError(f'{k}: shape {a.shape} is not {expected(shape)}')
        ctx = ctx or default_context()
        state = cls(ctx, *sizes)
        for k, a in arrays.items():
            ctx.upload(state.bufs[k], a)
        return state

    def copy(self):
        """An independent state with the same bits, in the same context."""
        return type(self).from_host(self.to_host(), ctx=self.ctx)


def _state_context(state, cls, key, ctx):
    """A caller's ``state=`` against this call: of the class ``cls``, built for the call's sizes
    ``key``, living in ``ctx`` where one is given.  Returns the context to use (``ctx`` without
    a state)."""
    if state is None:
        return ctx
    if not isinstance(state, cls):
        raise ValueError(f'state: {type(state).__name__} is not an {cls.__name__}')
    if state.key != key:
        raise ValueError(f'state: built for ({cls._sizes}) = {state.key}, the call has {key}')
    if ctx is not None and ctx is not state.ctx:
        raise ValueError('state: it lives in another context than ctx')
    return state.ctx


class OnlineWPEState(_OnlineState):
    """The state of the online WPE in HBM (gss_wpe_online_state), caller-owned like a
    `DeviceModel`: inv_cov P (F,A,n,n), filter G (F,A,n,C) and history (F,A,taps + delay,C) -- the
    last frames, oldest first --, complex128, n = taps * C."""
    _sizes = 'F, A, C, taps, delay'

    def __init__(self, ctx, F, A, C, taps, delay):
        super().__init__(ctx, F, A, C, taps, delay)
        self.F, self.A, self.C, self.taps, self.delay = self.key
        self.n, self.L = self.taps * self.C, self.taps + self.delay

    @staticmethod
    def _shapes(F, A, C, taps, delay):
        n = taps * C
        return {'inv_cov': (F, A, n, n), 'filter': (F, A, n, C), 'history': (F, A, taps + delay, C)}

    def struct(self):
        return GssWpeOnlineState(inv_cov_dev=self.bufs['inv_cov'].ptr,
                                 filter_dev=self.bufs['filter'].ptr,
                                 history_dev=self.bufs['history'].ptr)

    @classmethod
    def fresh(cls, F, A, C, taps, delay, *, ctx=None):
        """P = I, G = 0, history = 0 (gss_wpe_online_init)."""
        if not _is_integer(F) or F < 1:
            raise ValueError(f'F={F!r}: a positive integer')
        if not _is_integer(C) or C < 1:
            raise ValueError(f'C={C!r}: a positive integer')
        A = check_wpe_arrays(A)
        check_wpe_online(taps, delay, num_channels=A * C, arrays=A)
        ctx = ctx or default_context()
        state = cls(ctx, F, A, C, taps, delay)
        ctx._check(ctx.lib.gss_wpe_online_init(ctx.handle, state.F, state.A, state.C, state.taps,
                                               state.delay, ctypes.byref(state.struct())),
                   'gss_wpe_online_init')
        return state

    def to_host(self):
        """{'inv_cov', 'filter', 'history'} as NumPy arrays plus 'taps' and 'delay': everything
        `from_host` needs (synchronises)."""
        return dict(super().to_host(), taps=self.taps, delay=self.delay)

    @classmethod
    def from_host(cls, host, *, ctx=None):
        """A device state from the dict of `to_host` (in any context: a state saved in one
        process continues in another).  ValueError for shapes that do not fit each other."""
        G = np.asarray(host['filter'])
        if G.ndim != 4:
            raise ValueError(f'filter: shape {G.shape} is not (F,A,n,C)')
        F, A, n, C = G.shape
        taps, delay = int(host['taps']), int(host['delay'])
        check_wpe_online(taps, delay, num_channels=A * C, arrays=A)
        return cls._from_host(host, (F, A, C, taps, delay), ctx,
                              lambda shape: f'{shape} (taps={taps}, delay={delay})')


def wpe_online_dtf(Obs, taps=10, delay=2, alpha=WPE_ONLINE_ALPHA, *, arrays=1, state=None,
                   ctx=None):
    """The online WPE on the reference's (D,T,F) layout (gss_wpe_online): every frame is filtered
    with the filter as it stands BEFORE that frame updates it, and the filter forgets at the rate
    ``alpha``.  ``arrays`` = A > 1: per array, A groups of D / A consecutive channels.  ``state``:
    an `OnlineWPEState` to continue from, advanced IN PLACE by the T frames (feeding a recording in
    blocks through one state gives the bits of one call); None: a fresh state, thrown away.
    Returns (D,T,F)."""
    Obs = np.asarray(Obs)
    if Obs.ndim != 3:
        raise ValueError(f'Obs: shape {Obs.shape} is not (D,T,F)')
    D, T, F = Obs.shape
    A, C = check_wpe_online(taps, delay, alpha, D, arrays)
    ctx = _state_context(state, OnlineWPEState, (F, A, C, int(taps), int(delay)), ctx)
    ctx = ctx or default_context()
    if T == 0 or F == 0:
        return np.zeros((D, T, F), np.complex128)
    Y_d, _ = _obs_to_device_ftd(ctx, Obs)
    X_d = ctx.empty(16 * F * T * D)
    ctx._check(ctx.lib.gss_wpe_online(
        ctx.handle, c_void_p(Y_d.ptr), F, T, A, C, int(taps), int(delay), float(alpha),
        ctypes.byref(state.struct()) if state is not None else None, c_void_p(X_d.ptr)),
        'gss_wpe_online')
    return _ftd_to_host_dtf(ctx, X_d, D, T, F)


def cacgmm_posteriors(Obs, activity_freq, iterations=20, iterations_post=1, *, ctx=None):
    """``GSS.__call__`` (core.py:154-214): Obs (D,T,F) complex, activity (K,T) bool
    -> posterior (K,T,F) float64."""
    ctx = ctx or default_context()
    Y_d, (D, T, F) = _obs_to_device_ftd(ctx, Obs)
    act = np.ascontiguousarray(np.asarray(activity_freq).astype(bool).astype(np.uint8))
    K = act.shape[0]
    # "T: Consider end of signal" (core.py:177-184): activity may be longer than Obs
    assert act.shape[1] >= T, (act.shape, T)
    act = np.ascontiguousarray(act[:, :T])
    act_d = ctx.to_device(act)
    g_d = ctx.empty(8 * F * K * T)
    o_d = ctx.empty(8 * F * K * T)
    ctx._check(ctx.lib.gss_cacgmm(ctx.handle, c_void_p(Y_d.ptr), F, T, D, c_void_p(act_d.ptr),
                                  K, int(iterations), int(iterations_post),
                                  c_void_p(g_d.ptr)), 'gss_cacgmm')
    # (F, K*T) -> (K*T, F)
    ctx._check(ctx.lib.gss_layout_permute_f64(ctx.handle, c_void_p(g_d.ptr), F, K * T, 1, 2,
                                              c_void_p(o_d.ptr)), 'gss_layout_permute_f64')
    return ctx.to_host(o_d, (K, T, F), np.float64)


def guidance_from_activity(activity_freq):
    """core.py:156-163 on the host: activity (K,T) or (K,T,F), any dtype -> (initialization
    float64, source_activity_mask bool) of the same shape.  The initialisation is computed
    from the activity AS FLOAT64, so a value of 0.3 is a weight of 0.3:
    ``where(a == 0, 1e-10, a) / sum_k``; the mask is ``a != 0``."""
    initialization = np.asarray(activity_freq, dtype=np.float64)
    initialization = np.where(initialization == 0, 1e-10, initialization)
    initialization = initialization / np.sum(initialization, keepdims=True, axis=0)
    return initialization, np.asarray(activity_freq, dtype=bool)


def activity_is_binary(activity_freq, initialization=None):
    """Whether ``GSS.__call__`` may take the unweighted call (`cacgmm_posteriors`): a (K,T)
    activity whose non-zero values are all 1 (bool, uint8, 0/1 floats) and no explicit
    initialisation.  Weights, NaN, a per-frequency (K,T,F) activity or an initialisation need
    the guided call -- the unweighted one would binarise them."""
    if initialization is not None:
        return False
    a = np.asarray(activity_freq)
    if a.ndim != 2:
        return False
    if a.dtype == bool:
        return True
    return bool(np.all((a == 0) | (a == 1)))


def guidance_tables(initialization, source_activity_mask, T, F):
    """Shape rules of the guided calls.  Each table is (K,T') for all frequencies or
    (K,T',F) -- the layout posteriors come out in --, T' >= T (cut to T like the activity:
    core.py:177-184); at least one is given.  Returns (init, mask, K): float64 / uint8 arrays,
    C-contiguous, (K,T) or (F,K,T), or None.  ValueError for anything else."""
    if initialization is None and source_activity_mask is None:
        raise ValueError('guidance: initialization and source_activity_mask are both None')
    out, K = [], None
    for name, table, dtype in (('initialization', initialization, np.float64),
                               ('source_activity_mask', source_activity_mask, np.uint8)):
        if table is None:
            out.append(None)
            continue
        a = np.asarray(table)
        if dtype is np.uint8:
            a = a != 0
        if a.ndim not in (2, 3):
            raise ValueError(f'{name}: shape {a.shape} is neither (K,T) nor (K,T,F)')
        if a.shape[1] < T:
            raise ValueError(f'{name}: {a.shape[1]} frames but the observation has {T}')
        if a.ndim == 3 and a.shape[2] != F:
            raise ValueError(f'{name}: {a.shape[2]} frequencies but the observation has {F}')
        if K is not None and a.shape[0] != K:
            raise ValueError(f'{name}: {a.shape[0]} classes but initialization has {K}')
        K = a.shape[0]
        a = a[:, :T]
        if a.ndim == 3:
            a = a.transpose(2, 0, 1)     # (F,K,T)
        out.append(np.ascontiguousarray(a, dtype=dtype))
    return out[0], out[1], K


class DeviceGuidance:
    """Guidance tables (as `guidance_tables` returns them) in HBM and their gss_guidance."""

    def __init__(self, ctx, init, mask, T):
        self.init_d = ctx.to_device(init) if init is not None else None
        self.mask_d = ctx.to_device(mask) if mask is not None else None
        K = (init if init is not None else mask).shape[-2]

        def f_stride(a):
            return K * T if a is not None and a.ndim == 3 else 0
        self.struct = GssGuidance(
            init_dev=self.init_d.ptr if self.init_d else None,
            mask_dev=self.mask_d.ptr if self.mask_d else None,
            init_f_stride=f_stride(init), init_k_stride=T,
            mask_f_stride=f_stride(mask), mask_k_stride=T)


def cacgmm_posteriors_guided(Obs, initialization=None, source_activity_mask=None,
                             iterations=20, iterations_post=1, *, ctx=None):
    """``CACGMMTrainer.fit(y, initialization, iterations, source_activity_mask=...)`` and the
    post step of ``GSS.__call__`` for every frequency: Obs (D,T,F) complex; initialization
    (K,T) or (K,T,F) float, used as given (None: derived from the mask as core.py:156-159);
    source_activity_mask (K,T) or (K,T,F), non-zero = active (None: every step unmasked)
    -> posterior (K,T,F) float64.  Tables longer than T are cut."""
    Obs = np.asarray(Obs)
    if Obs.ndim != 3:
        raise ValueError(f'Obs: shape {Obs.shape} is not (D,T,F)')
    init, mask, K = guidance_tables(initialization, source_activity_mask, *Obs.shape[1:])
    ctx = ctx or default_context()
    Y_d, (D, T, F) = _obs_to_device_ftd(ctx, Obs)
    guide = DeviceGuidance(ctx, init, mask, T)
    g_d = ctx.empty(8 * F * K * T)
    o_d = ctx.empty(8 * F * K * T)
    ctx._check(ctx.lib.gss_cacgmm_guided(
        ctx.handle, c_void_p(Y_d.ptr), F, T, D, ctypes.byref(guide.struct), K, int(iterations),
        int(iterations_post), c_void_p(g_d.ptr)), 'gss_cacgmm_guided')
    # (F, K*T) -> (K*T, F)
    ctx._check(ctx.lib.gss_layout_permute_f64(ctx.handle, c_void_p(g_d.ptr), F, K * T, 1, 2,
                                              c_void_p(o_d.ptr)), 'gss_layout_permute_f64')
    return ctx.to_host(o_d, (K, T, F), np.float64)


def _check_em_iterations(iterations, iterations_post):
    for name, value, least in (('iterations', iterations, 1),
                               ('iterations_post', iterations_post, 0)):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < least:
            raise ValueError(f'{name}: {value!r} is not an integer >= {least}')


def _check_em_obs(Obs):
    Obs = np.asarray(Obs)
    if Obs.ndim != 3:
        raise ValueError(f'Obs: shape {Obs.shape} is not (D,T,F)')
    if not np.iscomplexobj(Obs):
        raise ValueError(f'Obs: dtype {Obs.dtype} is not complex')
    D, T, F = Obs.shape
    if not 2 <= D <= _MAX_CHANNELS:
        raise ValueError(f'Obs: {D} channels outside [2, {_MAX_CHANNELS}]')
    if T < 1 or F < 1:
        raise ValueError(f'Obs: shape {Obs.shape} has no frames or no frequencies')
    return Obs


def cacgmm_posteriors_shared_prior(Obs, initialization=None, source_activity_mask=None,
                                   iterations=20, iterations_post=1, *, return_prior=False,
                                   ctx=None):
    """`cacgmm_posteriors_guided` with one prior ``prior[k, t]`` per class and frame, shared by
    all frequencies, in place of the mixture weight ``pi[f, k]``: pb_bss's
    ``CACGMMTrainer(...).fit(..., weight_constant_axis=-3)``.  The M-step forms the prior as the
    mean over f of the (clipped) affiliations; the first one takes it from the initialisation.
    Obs (D,T,F) complex; tables as in `cacgmm_posteriors_guided` -> posterior (K,T,F) float64,
    with ``return_prior`` also the prior (K,T) of the last M-step, the one the final predict
    used.  Every argument error is a ValueError before any device work."""
    Obs = _check_em_obs(Obs)
    _check_em_iterations(iterations, iterations_post)
    init, mask, K = guidance_tables(initialization, source_activity_mask, *Obs.shape[1:])
    if not 1 <= K <= _MAX_CLASSES:
        raise ValueError(f'{K} classes outside [1, {_MAX_CLASSES}]')
    ctx = ctx or default_context()
    Y_d, (D, T, F) = _obs_to_device_ftd(ctx, Obs)
    guide = DeviceGuidance(ctx, init, mask, T)
    g_d = ctx.empty(8 * F * K * T)
    o_d = ctx.empty(8 * F * K * T)
    p_d = ctx.empty(8 * K * T) if return_prior else None
    ctx._check(ctx.lib.gss_cacgmm_shared_prior(
        ctx.handle, c_void_p(Y_d.ptr), F, T, D, ctypes.byref(guide.struct), K, int(iterations),
        int(iterations_post), c_void_p(g_d.ptr), c_void_p(p_d.ptr if p_d else None)),
        'gss_cacgmm_shared_prior')
    # (F, K*T) -> (K*T, F)
    ctx._check(ctx.lib.gss_layout_permute_f64(ctx.handle, c_void_p(g_d.ptr), F, K * T, 1, 2,
                                              c_void_p(o_d.ptr)), 'gss_layout_permute_f64')
    posterior = ctx.to_host(o_d, (K, T, F), np.float64)
    if return_prior:
        return posterior, ctx.to_host(p_d, (K, T), np.float64)
    return posterior


def blind_initialization(num_classes, num_frames, seed=0):
    """The start of the annotation-free EM: ``np.random.default_rng(seed).uniform(size=(K, T))``
    divided by its sum over k -- one (K,T) table for every frequency, which is what lets the
    shared prior keep class k the same source in every bin.  The definition is exact (the same
    seed gives the same bits)."""
    for name, value in (('num_classes', num_classes), ('num_frames', num_frames), ('seed', seed)):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
            raise ValueError(f'{name}: {value!r} is not an integer')
    if not 1 <= num_classes <= _MAX_CLASSES:
        raise ValueError(f'num_classes: {num_classes} outside [1, {_MAX_CLASSES}]')
    if num_frames < 1:
        raise ValueError(f'num_frames: {num_frames} < 1')
    if seed < 0:
        raise ValueError(f'seed: {seed} is negative')
    table = np.random.default_rng(int(seed)).uniform(size=(int(num_classes), int(num_frames)))
    return table / np.sum(table, axis=0, keepdims=True)


BLIND_METHODS = ('shared_prior', 'aligned')


def check_blind_method(method):
    if method not in BLIND_METHODS:
        raise ValueError(f'method: {method!r} is not one of {BLIND_METHODS}')
    return method


def cacgmm_posteriors_blind(Obs, num_classes, iterations=20, *, seed=0, return_prior=False,
                            method='shared_prior', plan=None, ctx=None):
    """Separation without an annotation.  Obs (D,T,F) -> posterior (K,T,F) (and a (K,T) per-frame
    activity of every class).  Classes carry indices, not names.
    ``method='shared_prior'``: `cacgmm_posteriors_shared_prior` from `blind_initialization`, no
    mask, ``iterations_post=1``; ``return_prior`` gives the prior.
    ``method='aligned'``: the per-frequency model (`cacgmm_posteriors_guided`) from the same
    start, then `align_posteriors` with ``plan`` (None: `alignment_plan`); ``return_prior`` gives
    the aligned posteriors' mean over f.  At most 8 classes."""
    Obs = _check_em_obs(Obs)
    check_blind_method(method)
    init = blind_initialization(num_classes, Obs.shape[1], seed)
    if method == 'shared_prior':
        if plan is not None:
            raise ValueError("plan: only method='aligned' takes an alignment plan")
        return cacgmm_posteriors_shared_prior(Obs, init, None, iterations, 1,
                                              return_prior=return_prior, ctx=ctx)
    _check_em_iterations(iterations, 1)
    _check_align_classes(num_classes)
    plan = check_alignment_plan(alignment_plan(Obs.shape[2]) if plan is None else plan,
                                Obs.shape[2])
    ctx = ctx or default_context()
    posterior = cacgmm_posteriors_guided(Obs, init, None, iterations, 1, ctx=ctx)
    return align_posteriors(posterior, plan, return_activity=return_prior, ctx=ctx)


# --------------------------------------------------------------------------
# permutation alignment (include/gss_hip.h: gss_cacgmm_align; not in the reference)
# --------------------------------------------------------------------------
_ALIGN_MAX_CLASSES = 8                      # include/gss_hip.h: GSS_ALIGN_MAX_CLASSES


def _check_align_classes(K):
    if not 1 <= K <= _ALIGN_MAX_CLASSES:
        raise ValueError(f'{K} classes outside [1, {_ALIGN_MAX_CLASSES}]: the alignment searches '
                         'all K! permutations')


def alignment_plan(num_frequencies, *, segment_start=None, segment_width=None, segment_shift=None,
                   main_iterations=20, sub_iterations=2):
    """The customary plan of `align_posteriors`: ``main_iterations`` passes over a band of
    ``segment_width`` frequencies from ``segment_start``, then ``sub_iterations`` passes over the
    band widened by ``segment_shift`` on either side, again and again until it is [0, F).  The
    defaults scale the usual setting of a 512-point STFT (70, 100, 20 of 257 bins) to F; they
    are choices, not measurements.  Returns [(iterations, start, end), ...]."""
    values = dict(num_frequencies=num_frequencies, main_iterations=main_iterations,
                  sub_iterations=sub_iterations)
    for name, value in (('segment_start', segment_start), ('segment_width', segment_width),
                        ('segment_shift', segment_shift)):
        if value is not None:
            values[name] = value
    for name, value in values.items():
        if not _is_integer(value):
            raise ValueError(f'{name}: {value!r} is not an integer')
    F = int(num_frequencies)
    if F < 1:
        raise ValueError(f'num_frequencies: {F} < 1')
    for name in ('main_iterations', 'sub_iterations'):
        if values[name] < 1:
            raise ValueError(f'{name}: {values[name]} < 1')
    segment_start = F * 70 // 257 if segment_start is None else int(segment_start)
    segment_width = F * 100 // 257 if segment_width is None else int(segment_width)
    segment_shift = max(F * 20 // 257, 1) if segment_shift is None else int(segment_shift)
    if segment_start < 0:
        raise ValueError(f'segment_start: {segment_start} is negative')
    if segment_width < 0:
        raise ValueError(f'segment_width: {segment_width} is negative')
    if segment_shift < 1:
        raise ValueError(f'segment_shift: {segment_shift} < 1')
    start = max(min(segment_start, F - 1), 0)
    end = min(start + max(segment_width, 1), F)
    plan = [(int(main_iterations), start, end)]
    while (start, end) != (0, F):
        start = max(start - segment_shift, 0)
        end = min(end + segment_shift, F)
        plan.append((int(sub_iterations), start, end))
    return plan


def check_alignment_plan(plan, num_frequencies):
    """The one place a plan is validated: a non-empty sequence of (iterations, start, end)
    integers with iterations >= 1 and 0 <= start < end <= F.  Returns it as a list of int
    tuples; ValueError otherwise."""
    if isinstance(plan, (str, bytes)) or not hasattr(plan, '__iter__'):
        raise ValueError(f'plan: {plan!r} is not a sequence of (iterations, start, end)')
    plan = list(plan)
    if not plan:
        raise ValueError('plan: no entries')
    out = []
    for index, entry in enumerate(plan):
        try:
            entry = tuple(entry)
        except TypeError:
            entry = None
        if entry is None or len(entry) != 3 or not all(_is_integer(v) for v in entry):
            raise ValueError(f'plan entry {index}: {plan[index]!r} is not (iterations, start, end) '
                             'of three integers')
        iterations, start, end = (int(v) for v in entry)
        if not 1 <= iterations <= 2 ** 31 - 1:
            raise ValueError(f'plan entry {index}: iterations = {iterations} < 1 (or not an int32)')
        if not 0 <= start < end <= num_frequencies:
            raise ValueError(f'plan entry {index}: not 0 <= start = {start} < end = {end} <= '
                             f'F = {num_frequencies}')
        out.append((iterations, start, end))
    return out


def check_mapping(mapping, num_frequencies, num_classes):
    """mapping (F,K) integers, every row a permutation of 0..K-1 -> int32 array; ValueError."""
    m = np.asarray(mapping)
    if m.shape != (num_frequencies, num_classes):
        raise ValueError(f'mapping: shape {m.shape} is not (F,K) = '
                         f'{(num_frequencies, num_classes)}')
    if m.dtype.kind not in 'iu':
        raise ValueError(f'mapping: dtype {m.dtype} is not an integer type')
    if not np.array_equal(np.sort(m, axis=1),
                          np.broadcast_to(np.arange(num_classes), m.shape)):
        bad = int(np.argmax(np.any(np.sort(m, axis=1) != np.arange(num_classes), axis=1)))
        raise ValueError(f'mapping: row {bad} = {m[bad].tolist()} is not a permutation of '
                         f'0..{num_classes - 1}')
    return np.ascontiguousarray(m, dtype=np.int32)


class DeviceAlignPlan:
    """A validated plan as the host arrays of a gss_align_plan (read during the call)."""

    def __init__(self, plan):
        self.arrays = [np.ascontiguousarray([entry[i] for entry in plan], dtype=np.int32)
                       for i in range(3)]
        self.struct = _capi.GssAlignPlan(*(a.ctypes.data for a in self.arrays), len(plan))


def _check_posterior_ktf(posterior):
    posterior = np.asarray(posterior)
    if posterior.ndim != 3:
        raise ValueError(f'posterior: shape {posterior.shape} is not (K,T,F)')
    if posterior.dtype.kind not in 'fiu':
        raise ValueError(f'posterior: dtype {posterior.dtype} is not real')
    K, T, F = posterior.shape
    if T < 1 or F < 1:
        raise ValueError(f'posterior: shape {posterior.shape} has no frames or no frequencies')
    _check_align_classes(K)
    return posterior


def align_posteriors(posterior, plan=None, *, return_mapping=False, return_activity=False,
                     ctx=None):
    """Align the classes of per-frequency posteriors across frequencies (`gss_cacgmm_align`):
    posterior (K,T,F), plan as `alignment_plan` returns it (None: its defaults for F) -> the
    aligned posterior (K,T,F), ``aligned[k, :, f] = posterior[mapping[f, k], :, f]``; with
    ``return_mapping`` also the mapping (F,K) int32, every row a permutation; with
    ``return_activity`` also the aligned posteriors' mean over f, (K,T) -- what the shared
    prior calls its prior.  Every argument error is a ValueError before any device work."""
    posterior = _check_posterior_ktf(posterior)
    K, T, F = posterior.shape
    plan = check_alignment_plan(alignment_plan(F) if plan is None else plan, F)
    ctx = ctx or default_context()
    dplan = DeviceAlignPlan(plan)
    g_d = ctx.to_device(np.ascontiguousarray(posterior.transpose(2, 0, 1), dtype=np.float64))
    m_d = ctx.empty(4 * F * K)
    a_d = ctx.empty(8 * F * K * T)
    o_d = ctx.empty(8 * F * K * T)
    act_d = ctx.empty(8 * K * T) if return_activity else None
    ctx._check(ctx.lib.gss_cacgmm_align(
        ctx.handle, c_void_p(g_d.ptr), F, K, T, ctypes.byref(dplan.struct), c_void_p(m_d.ptr),
        c_void_p(a_d.ptr), c_void_p(act_d.ptr if act_d else None)), 'gss_cacgmm_align')
    # (F, K*T) -> (K*T, F)
    ctx._check(ctx.lib.gss_layout_permute_f64(ctx.handle, c_void_p(a_d.ptr), F, K * T, 1, 2,
                                              c_void_p(o_d.ptr)), 'gss_layout_permute_f64')
    out = [ctx.to_host(o_d, (K, T, F), np.float64)]
    if return_mapping:
        out.append(ctx.to_host(m_d, (F, K), np.int32))
    if return_activity:
        out.append(ctx.to_host(act_d, (K, T), np.float64))
    return out[0] if len(out) == 1 else tuple(out)


def cacgmm_model_permute(model, mapping, *, ctx=None):
    """`cacgmm.CACGMM.permuted` on the device (`gss_cacgmm_model_permute`): class k of frequency
    f of the result is class ``mapping[f, k]`` of ``model``."""
    if not isinstance(model, CACGMM):
        raise ValueError(f'model: a CACGMM, not {type(model).__name__}')
    F, K, D = model.shape
    mapping = check_mapping(mapping, F, K)
    ctx = ctx or default_context()
    src = DeviceModel(ctx, F, K, D, model)
    dst = DeviceModel(ctx, F, K, D)
    m_d = ctx.to_device(mapping)
    ctx._check(ctx.lib.gss_cacgmm_model_permute(
        ctx.handle, ctypes.byref(src.struct), F, K, D, c_void_p(m_d.ptr),
        ctypes.byref(dst.struct)), 'gss_cacgmm_model_permute')
    return dst.to_host(ctx)


# --------------------------------------------------------------------------
# cross-window class linking (include/gss_hip.h: gss_cacgmm_link; not in the reference)
# --------------------------------------------------------------------------
def check_link_frames(frames, num_frames, name):
    """A ``(begin, end)`` pair of integers with 0 <= begin < end <= num_frames (None: all
    frames) -> (begin, end) as ints; ValueError."""
    if frames is None:
        return 0, int(num_frames)
    try:
        frames = tuple(frames)
    except TypeError:
        frames = None
    if frames is None or len(frames) != 2 or not all(_is_integer(v) for v in frames):
        raise ValueError(f'{name}: {frames!r} is not a (begin, end) pair of integers')
    begin, end = (int(v) for v in frames)
    if not 0 <= begin < end <= num_frames:
        raise ValueError(f'{name}: not 0 <= begin = {begin} < end = {end} <= T = {num_frames}')
    return begin, end


def link_posteriors_device(ctx, prev_d, T_prev, prev_begin, cur_d, T_cur, cur_begin, L, F, K,
                           mapping_d, scores_d):
    """`gss_cacgmm_link` on tables that sit in HBM in the device layout (F,K,T): enqueues, copies
    nothing.  ``mapping_d`` (K,) int32 and ``scores_d`` (K,K) float64 are device buffers."""
    ctx._check(ctx.lib.gss_cacgmm_link(
        ctx.handle, c_void_p(prev_d.ptr), int(T_prev), int(prev_begin), c_void_p(cur_d.ptr),
        int(T_cur), int(cur_begin), int(L), int(F), int(K), c_void_p(mapping_d.ptr),
        c_void_p(scores_d.ptr)), 'gss_cacgmm_link')


def link_gather_device(ctx, gamma_d, F, K, T, mapping_d, out_d):
    """`gss_cacgmm_link_gather`: ``out[f, a, :] = gamma[f, mapping[a], :]`` in HBM, the mapping
    read on the device (no host round trip after the link).  Not in place."""
    ctx._check(ctx.lib.gss_cacgmm_link_gather(
        ctx.handle, c_void_p(gamma_d.ptr), int(F), int(K), int(T), c_void_p(mapping_d.ptr),
        c_void_p(out_d.ptr)), 'gss_cacgmm_link_gather')


def link_posteriors(prev, cur, *, prev_frames=None, cur_frames=None, ctx=None):
    """Link the classes of two windows' posteriors on the frames they share
    (`gss_cacgmm_link`): prev (K,T_prev,F), cur (K,T_cur,F); ``prev_frames`` / ``cur_frames``
    ``(begin, end)`` pairs of equally many frames (None: the whole table) -> mapping (K,) int32
    and scores (K,K): ``scores[a, b]`` is the cosine similarity, over the frames and all
    frequencies, of class a of ``prev`` and class b of ``cur``; the mapping is the permutation
    that maximises ``sum_a scores[a, mapping[a]]`` (the lexicographically smallest among exact
    maxima), so that ``cur[mapping]`` continues ``prev``.  At most 8 classes.  Every argument
    error is a ValueError before any device work."""
    prev = _check_posterior_ktf(prev)
    cur = _check_posterior_ktf(cur)
    K, T_prev, F = prev.shape
    if cur.shape[0] != K or cur.shape[2] != F:
        raise ValueError(f'cur: shape {cur.shape} does not have the {K} classes and {F} '
                         f'frequencies of prev {prev.shape}')
    T_cur = cur.shape[1]
    pb, pe = check_link_frames(prev_frames, T_prev, 'prev_frames')
    cb, ce = check_link_frames(cur_frames, T_cur, 'cur_frames')
    if pe - pb != ce - cb:
        raise ValueError(f'prev_frames covers {pe - pb} frames, cur_frames {ce - cb}')
    ctx = ctx or default_context()
    p_d = ctx.to_device(np.ascontiguousarray(prev.transpose(2, 0, 1), dtype=np.float64))
    c_d = ctx.to_device(np.ascontiguousarray(cur.transpose(2, 0, 1), dtype=np.float64))
    m_d = ctx.empty(max(4 * K, 16))
    s_d = ctx.empty(max(8 * K * K, 16))
    link_posteriors_device(ctx, p_d, T_prev, pb, c_d, T_cur, cb, pe - pb, F, K, m_d, s_d)
    return ctx.to_host(m_d, (K,), np.int32), ctx.to_host(s_d, (K, K), np.float64)


def cacgmm_fit_blind(Obs, num_classes, iterations=20, *, seed=0, plan=None,
                     return_posterior=False, ctx=None):
    """The annotation-free model object: `cacgmm_fit` from `blind_initialization` with no mask,
    `cacgmm_predict` on the fitted frames, `align_posteriors` and `cacgmm_model_permute` -> a
    `cacgmm.CACGMM` whose class k is the same source in every frequency; its ``predict`` on the
    fitted frames gives the aligned posteriors (``return_posterior``: returned as well, (K,T,F)).
    At most 8 classes."""
    Obs = _check_em_obs(Obs)
    _check_em_iterations(iterations, 1)
    init = blind_initialization(num_classes, Obs.shape[1], seed)
    _check_align_classes(num_classes)
    F = Obs.shape[2]
    plan = check_alignment_plan(alignment_plan(F) if plan is None else plan, F)
    ctx = ctx or default_context()
    model = cacgmm_fit(Obs, init, None, int(iterations), ctx=ctx)
    posterior = cacgmm_predict(model, Obs, ctx=ctx)
    aligned, mapping = align_posteriors(posterior, plan, return_mapping=True, ctx=ctx)
    model = cacgmm_model_permute(model, mapping, ctx=ctx)
    return (model, aligned) if return_posterior else model


class DeviceModel:
    """The three arrays of a `cacgmm.CACGMM` in HBM and their gss_cacgmm_model."""

    def __init__(self, ctx, F, K, D, model=None):
        self.shape = (F, K, D)
        if model is not None:
            self.precision_d = ctx.to_device(model.precision)
            self.log_det_d = ctx.to_device(model.log_determinant)
            self.weight_d = ctx.to_device(model.weight)
        else:
            self.precision_d = ctx.empty(16 * F * K * D * D)
            self.log_det_d = ctx.empty(8 * F * K)
            self.weight_d = ctx.empty(8 * F * K)
        self.struct = GssCacgmmModel(precision_dev=self.precision_d.ptr,
                                     log_det_dev=self.log_det_d.ptr,
                                     weight_dev=self.weight_d.ptr)

    def to_host(self, ctx):
        F, K, D = self.shape
        return CACGMM(ctx.to_host(self.precision_d, (F, K, D, D), np.complex128),
                      ctx.to_host(self.log_det_d, (F, K), np.float64),
                      ctx.to_host(self.weight_d, (F, K), np.float64))


def _model_call_tables(model, Obs, source_activity_mask):
    """Shape rules of a call that takes a model: ValueError before any device work.
    Returns (mask (K,T) / (F,K,T) uint8 or None, K)."""
    if not isinstance(model, CACGMM):
        raise ValueError(f'model: a CACGMM, not {type(model).__name__}')
    model.check_observation(Obs)
    K = model.shape[1]
    mask = None
    if source_activity_mask is not None:
        _, mask, mask_K = guidance_tables(None, source_activity_mask, *np.shape(Obs)[1:])
        if mask_K != K:
            raise ValueError(f'source_activity_mask: {mask_K} classes but the model has {K}')
    return mask, K


def _check_iterations(iterations):
    if not _is_integer(iterations):
        raise ValueError(f'iterations: {iterations!r} is not an integer')
    return int(iterations)


def cacgmm_fit(Obs, initialization=None, source_activity_mask=None, iterations=100, *,
               model=None, ctx=None):
    """``CACGMMTrainer.fit`` for every frequency -> `cacgmm.CACGMM`.  Obs (D,T,F) complex.
    Without ``model``: ``iterations`` M-steps from the initialisation (K,T) / (K,T,F) (None:
    derived from the mask as core.py:156-159), masked with ``source_activity_mask`` if given --
    the fit of `cacgmm_posteriors_guided`.  With ``model`` (``fit(initialization=model)``):
    ``iterations`` E-step + M-step pairs from it, masked if a mask is given; ``iterations=0``
    returns the model's bits."""
    Obs = np.asarray(Obs)
    if Obs.ndim != 3:
        raise ValueError(f'Obs: shape {Obs.shape} is not (D,T,F)')
    iterations = _check_iterations(iterations)
    if model is not None:
        if initialization is not None:
            raise ValueError('initialization: both an array and a model were given')
        init, (mask, K) = None, _model_call_tables(model, Obs, source_activity_mask)
    else:
        init, mask, K = guidance_tables(initialization, source_activity_mask, *Obs.shape[1:])
    ctx = ctx or default_context()
    Y_d, (D, T, F) = _obs_to_device_ftd(ctx, Obs)
    guide = DeviceGuidance(ctx, init, mask, T) if (init is not None or mask is not None) else None
    start = DeviceModel(ctx, F, K, D, model) if model is not None else None
    out = DeviceModel(ctx, F, K, D)
    ctx._check(ctx.lib.gss_cacgmm_fit(
        ctx.handle, c_void_p(Y_d.ptr), F, T, D, ctypes.byref(guide.struct) if guide else None, K,
        iterations, ctypes.byref(start.struct) if start else None, ctypes.byref(out.struct)),
        'gss_cacgmm_fit')
    return out.to_host(ctx)


def _cacgmm_predict(model, Obs, source_activity_mask, want_gamma, want_loglik, ctx):
    Obs = np.asarray(Obs)
    mask, K = _model_call_tables(model, Obs, source_activity_mask)
    ctx = ctx or default_context()
    Y_d, (D, T, F) = _obs_to_device_ftd(ctx, Obs)
    guide = DeviceGuidance(ctx, None, mask, T) if mask is not None else None
    dev = DeviceModel(ctx, F, K, D, model)
    g_d = ctx.empty(8 * F * K * T) if want_gamma else None
    ll_d = ctx.empty(8 * F * T) if want_loglik else None
    ctx._check(ctx.lib.gss_cacgmm_predict(
        ctx.handle, c_void_p(Y_d.ptr), F, T, D, ctypes.byref(dev.struct), K,
        ctypes.byref(guide.struct) if guide else None, c_void_p(g_d.ptr if g_d else None),
        c_void_p(ll_d.ptr if ll_d else None)), 'gss_cacgmm_predict')
    posterior = loglik = None
    if want_gamma:
        o_d = ctx.empty(8 * F * K * T)
        # (F, K*T) -> (K*T, F)
        ctx._check(ctx.lib.gss_layout_permute_f64(ctx.handle, c_void_p(g_d.ptr), F, K * T, 1, 2,
                                                  c_void_p(o_d.ptr)), 'gss_layout_permute_f64')
        posterior = ctx.to_host(o_d, (K, T, F), np.float64)
    if want_loglik:
        loglik = np.ascontiguousarray(ctx.to_host(ll_d, (F, T), np.float64).T)
    return posterior, loglik


def cacgmm_predict(model, Obs, source_activity_mask=None, *, log_likelihood=False, ctx=None):
    """``CACGMM.predict`` (affiliation_eps = 0) under a `cacgmm.CACGMM`: Obs (D,T,F) of any
    frame count -> posterior (K,T,F); ``log_likelihood=True``: (posterior, log-likelihood
    (T,F)) from the same call."""
    posterior, loglik = _cacgmm_predict(model, Obs, source_activity_mask, True,
                                        bool(log_likelihood), ctx)
    return (posterior, loglik) if log_likelihood else posterior


def cacgmm_log_likelihood(model, Obs, source_activity_mask=None, *, ctx=None):
    """ln sum_k pi_k m_kt exp(-D ln q_kt - ln det B_k) per frame, (T,F): the log-likelihood of
    the unit-normalised frames under the model up to the constant ln((D-1)! / (2 pi^D)); -inf
    where the mask turns every class off.  No posteriors are computed."""
    return _cacgmm_predict(model, Obs, source_activity_mask, False, True, ctx)[1]


def _mask_to_device_ft(ctx, mask, T, F):
    m = np.ascontiguousarray(np.asarray(mask, dtype=np.float64).T)   # (F,T)
    assert m.shape == (F, T), (m.shape, F, T)
    return ctx.to_device(m)


def _raise_for_ref_channel(ref, name=None):
    """The beamformer's status word (gss_last_ref_channel) as the exception the reference
    raises.  -1: pb_bss get_optimal_reference_channel ``assert np.all(np.isfinite(SNR)), SNR``;
    <= -2: pb_bss get_gev_vector re-raises scipy.linalg.eigh's LinAlgError ("Error for
    frequency f ...") when the noise PSD matrix of a frequency is not positive definite."""
    prefix = f'{name}: ' if name is not None else ''
    if ref == -1:       # (not an `assert` statement: those vanish under python -O)
        raise AssertionError(f'{prefix}get_optimal_reference_channel: the SNR is not finite')
    if -2 - (1 << 24) < ref <= -2:
        raise np.linalg.LinAlgError(f'{prefix}Error for frequency {-2 - ref}: the noise PSD '
                                    'matrix is not positive definite (get_gev_vector)')


def _check_ref_channel(ctx):
    """Raises what the reference raises for the last beamformer run on ``ctx``; returns the
    reference channel otherwise."""
    ref = ctx.last_ref_channel()
    _raise_for_ref_channel(ref)
    return ref


def mvdr_souden_from_masks(Y, X_mask, N_mask, ban=False, *, ref_channel=None,
                           return_ref_channel=False, ctx=None):
    """Y (D,T,F), 2-D masks (T,F) -> X_hat (T,F) complex128.  ``ref_channel`` names the
    reference channel (pb_bss get_mvdr_vector_souden(ref_channel=...)); None = the SNR
    argmax.  Raises AssertionError when an SNR is not finite, like the reference."""
    ctx = ctx or default_context()
    Y_d, (D, T, F) = _obs_to_device_ftd(ctx, Y)
    mx = _mask_to_device_ft(ctx, X_mask, T, F)
    mn = _mask_to_device_ft(ctx, N_mask, T, F)
    X_d = ctx.empty(16 * F * T)
    if ref_channel is None:
        ctx._check(ctx.lib.gss_mvdr_souden(ctx.handle, c_void_p(Y_d.ptr), F, T, D,
                                           c_void_p(mx.ptr), c_void_p(mn.ptr), int(bool(ban)),
                                           c_void_p(X_d.ptr), None), 'gss_mvdr_souden')
    else:
        ctx._check(ctx.lib.gss_mvdr_souden_ref(ctx.handle, c_void_p(Y_d.ptr), F, T, D,
                                               c_void_p(mx.ptr), c_void_p(mn.ptr),
                                               int(bool(ban)), int(ref_channel),
                                               c_void_p(X_d.ptr)), 'gss_mvdr_souden_ref')
    ref = _check_ref_channel(ctx)
    X_hat = ctx.to_host(X_d, (T, F), np.complex128)
    if return_ref_channel:
        return X_hat, ref
    return X_hat


SEGMENT_TILE = 64       # frames: segment_frames is a multiple of the PSD kernel's frame tile


def check_bf_segments(segment_frames, segment_context=0, min_mass=None, num_channels=None):
    """The settings of the segment-wise beamformer as a gss_bf_segments, or ValueError naming
    the argument: ``segment_frames`` a positive multiple of 64, ``segment_context`` an integer
    >= 0, ``min_mass`` finite and >= 0.  ``min_mass=None`` is ``2 * num_channels`` (it stays
    0 in the returned struct while ``num_channels`` is not known: checks without an
    observation)."""
    def integer(value):
        return isinstance(value, (int, np.integer)) and not isinstance(value, bool)
    if not integer(segment_frames) or segment_frames < SEGMENT_TILE \
            or segment_frames % SEGMENT_TILE:
        raise ValueError(f'segment_frames={segment_frames!r}: a positive multiple of '
                         f'{SEGMENT_TILE} frames')
    if not integer(segment_context) or segment_context < 0 or segment_context >= 2 ** 31:
        raise ValueError(f'segment_context={segment_context!r}: a non-negative integer number '
                         'of segments')
    if min_mass is None:
        min_mass = 2 * num_channels if num_channels is not None else 0
    if isinstance(min_mass, bool) or not isinstance(min_mass, (int, float, np.integer,
                                                               np.floating)) \
            or not np.isfinite(min_mass) or min_mass < 0:
        raise ValueError(f'min_mass={min_mass!r}: a finite number >= 0')
    return GssBfSegments(segment_frames=int(segment_frames),
                         context_segments=int(segment_context), min_mass=float(min_mass))


def mvdr_souden_segments_from_masks(Y, X_mask, N_mask, ban=False, *, segment_frames,
                                    segment_context=0, min_mass=None, ref_channel=None,
                                    return_ref_channel=False, return_fallbacks=False, ctx=None):
    """`mvdr_souden_from_masks` with a time-varying filter (gss_mvdr_souden_segments): the T
    frames are cut into segments of ``segment_frames`` frames (a positive multiple of 64, the
    last one may be short); segment b's PSD matrices are taken over segments
    b - segment_context .. b + segment_context, its filter is applied to its own frames.  One
    reference channel for the whole call (the SNR summed over all segments and frequencies, or
    ``ref_channel``).  A window whose target or distortion mask sums to less than ``min_mass``
    at a frequency takes the whole-window matrices there; ``min_mass=None`` is ``2 * D``: a
    Phi_N from fewer than D frames' worth of mask is singular, and the factor 2 on top of that
    is a choice, not a measurement.  ``min_mass=0`` never falls back.

    Y (D,T,F), masks (T,F) -> X_hat (T,F); with ``return_ref_channel`` / ``return_fallbacks``
    a tuple (X_hat[, ref_channel][, number of (segment, frequency) pairs that fell back]).
    Argument errors are ValueError before any device work; a non-finite SNR raises
    AssertionError like the whole-window call."""
    Y = np.asarray(Y)
    if Y.ndim != 3:
        raise ValueError(f'Y: shape {Y.shape} is not (D,T,F)')
    D, T, F = Y.shape
    seg = check_bf_segments(segment_frames, segment_context, min_mass, D)
    for name, m in (('X_mask', X_mask), ('N_mask', N_mask)):
        if np.shape(m) != (T, F):
            raise ValueError(f'{name}: shape {np.shape(m)} is not (T,F) = {(T, F)}')
    if ref_channel is not None and not 0 <= int(ref_channel) < D:
        raise ValueError(f'ref_channel={ref_channel!r} outside [0, {D})')
    ctx = ctx or default_context()
    Y_d, _ = _obs_to_device_ftd(ctx, Y)
    mx = _mask_to_device_ft(ctx, X_mask, T, F)
    mn = _mask_to_device_ft(ctx, N_mask, T, F)
    X_d = ctx.empty(16 * F * T)
    ctx._check(ctx.lib.gss_mvdr_souden_segments(
        ctx.handle, c_void_p(Y_d.ptr), F, T, D, c_void_p(mx.ptr), c_void_p(mn.ptr),
        int(bool(ban)), -1 if ref_channel is None else int(ref_channel), ctypes.byref(seg),
        c_void_p(X_d.ptr), None), 'gss_mvdr_souden_segments')
    ref = _check_ref_channel(ctx)
    out = (ctx.to_host(X_d, (T, F), np.complex128),)
    if return_ref_channel:
        out += (ref,)
    if return_fallbacks:
        out += (ctx.last_segment_fallbacks(),)
    return out if len(out) > 1 else out[0]


# --------------------------------------------------------------------------
# online MVDR (gss_mvdr_online): frame-recursive Souden MVDR with a carried state
# --------------------------------------------------------------------------
# Both defaults are choices, not measurements: 0.99 is a memory of
# 1 / (1 - 0.99) = 100 frames, 1.6 s at the 16 ms frame shift; the loading is relative to the mean
# power of the frames the state is initialised from.
BF_ONLINE_FORGET = 0.99
BF_ONLINE_LOADING = 1e-2


def check_bf_online(forget=BF_ONLINE_FORGET, loading=BF_ONLINE_LOADING, ref_channel=0,
                    num_channels=None):
    """The settings of the online MVDR -- the one place that validates them, before any device
    work.  ValueError naming the argument: ``forget`` a finite number in (0, 1], ``loading`` a
    finite number > 0, ``num_channels`` an integer in [1, 32], ``ref_channel`` an integer in
    [-1, num_channels) (-1: the whole-window beamformer's choice over the call's frames, which
    needs fewer than 30 channels like that beamformer).  Returns (forget, loading, ref_channel)."""
    if not _is_real(forget) or not np.isfinite(forget) or not 0 < forget <= 1:
        raise ValueError(f'forget={forget!r}: a finite number in (0, 1]')
    if not _is_real(loading) or not np.isfinite(loading) or not loading > 0:
        raise ValueError(f'loading={loading!r}: a finite number > 0')
    if num_channels is not None and (not _is_integer(num_channels)
                                     or not 1 <= num_channels <= _MAX_CHANNELS):
        raise ValueError(f'num_channels={num_channels!r}: an integer in [1, {_MAX_CHANNELS}]')
    if not _is_integer(ref_channel) or ref_channel < -1 or (
            num_channels is not None and ref_channel >= num_channels):
        raise ValueError(f'ref_channel={ref_channel!r}: an integer in [-1, '
                         f'{"num_channels" if num_channels is None else num_channels})')
    if ref_channel == -1 and num_channels is not None and num_channels >= 30:
        raise ValueError(f'ref_channel=-1 on num_channels={num_channels}: the whole-window '
                         'beamformer that picks the channel asserts D < 30')
    return float(forget), float(loading), int(ref_channel)


def _bf_online_cfg(forget, loading, ref_channel, wpe_online=False, wpe_alpha=WPE_ONLINE_ALPHA):
    return GssBfOnline(forget=forget, loading=loading, ref_channel=ref_channel,
                       wpe_online=int(bool(wpe_online)), wpe_alpha=float(wpe_alpha))


class OnlineMVDRState(_OnlineState):
    """The state of the online MVDR in HBM (gss_mvdr_online_state), caller-owned like an
    `OnlineWPEState`: the running sums phi_x and phi_n (F,D,D), complex128, Hermitian."""
    _sizes = 'F, D'

    def __init__(self, ctx, F, D):
        super().__init__(ctx, F, D)
        self.F, self.D = self.key

    @staticmethod
    def _shapes(F, D):
        return {'phi_x': (F, D, D), 'phi_n': (F, D, D)}

    def struct(self):
        return GssMvdrOnlineState(phi_x=self.bufs['phi_x'].ptr, phi_n=self.bufs['phi_n'].ptr,
                                  F=self.F, D=self.D)

    @classmethod
    def fresh(cls, F, D, loading=BF_ONLINE_LOADING, Y=None, *, ctx=None):
        """phi_x = 0, phi_n = loading * p_f * I (gss_mvdr_online_init); p_f is the mean power of
        frequency f of ``Y`` (D,T,F), 1 without ``Y`` or where that mean is exactly 0."""
        if not _is_integer(F) or F < 1:
            raise ValueError(f'F={F!r}: a positive integer')
        check_bf_online(loading=loading, num_channels=D)
        T = 0
        if Y is not None:
            Y = np.asarray(Y)
            if Y.ndim != 3 or Y.shape[0] != D or Y.shape[2] != F:
                raise ValueError(f'Y: shape {Y.shape} is not (D,T,F) = ({D},T,{F})')
            T = Y.shape[1]
        ctx = ctx or default_context()
        state = cls(ctx, F, D)
        Y_d = _obs_to_device_ftd(ctx, Y)[0] if T > 0 else None
        ctx._check(ctx.lib.gss_mvdr_online_init(
            ctx.handle, state.F, state.D, c_void_p(Y_d.ptr) if Y_d is not None else None, T,
            float(loading), ctypes.byref(state.struct())), 'gss_mvdr_online_init')
        return state

    @classmethod
    def from_host(cls, host, *, ctx=None):
        """A device state from the dict of `to_host` ({'phi_x', 'phi_n'}; in any context: a state
        saved in one process continues in another).  ValueError for shapes that do not fit each
        other."""
        px = np.asarray(host['phi_x'])
        if px.ndim != 3 or px.shape[1] != px.shape[2]:
            raise ValueError(f'phi_x: shape {px.shape} is not (F,D,D)')
        F, D, _ = px.shape
        if F < 1:
            raise ValueError(f'phi_x: shape {px.shape} has no frequency')
        check_bf_online(num_channels=D)
        return cls._from_host(host, (F, D), ctx)


BF_ONLINE_MAX_LOOKAHEAD = 64   # include/gss_hip.h: GSS_MVDR_ONLINE_MAX_LOOKAHEAD, a choice


def check_bf_lookahead(lookahead=0, ref_channel=0):
    """The look-ahead of the online MVDR -- the one place that validates it, before any device
    work.  ValueError naming the argument: ``lookahead`` an integer in [0, 64]; with a look-ahead
    ``ref_channel`` = -1 is refused (the whole-window choice is per call, a delay line outlives a
    call).  Returns the look-ahead as an int."""
    if not _is_integer(lookahead) or not 0 <= lookahead <= BF_ONLINE_MAX_LOOKAHEAD:
        raise ValueError(f'lookahead={lookahead!r}: an integer in [0, {BF_ONLINE_MAX_LOOKAHEAD}]')
    if lookahead > 0 and ref_channel == -1:
        raise ValueError('ref_channel=-1 with lookahead > 0: the whole-window choice is per call, '
                         'a delay line outlives a call')
    return int(lookahead)


class OnlineMVDRHold(_OnlineState):
    """The delay line of the online MVDR's look-ahead in HBM (gss_mvdr_online_hold), caller-owned
    and separate from the `OnlineMVDRState`: the held frames (F,L,D) oldest first, their
    target-mask values (F,L), the filter of the last frame that entered (F,D), and the host counter
    ``held`` in [0, L], which the calls advance."""
    _sizes = 'F, D, L'
    dtypes = {'mask': np.float64}

    def __init__(self, ctx, F, D, L):
        super().__init__(ctx, F, D, L)
        self.F, self.D, self.L = self.key
        self.held = 0

    @staticmethod
    def _shapes(F, D, L):
        return {'frames': (F, L, D), 'mask': (F, L), 'filter': (F, D)}

    def struct(self):
        return GssMvdrOnlineHold(frames=self.bufs['frames'].ptr, mask=self.bufs['mask'].ptr,
                                 filter=self.bufs['filter'].ptr, F=self.F, D=self.D, L=self.L,
                                 held=self.held)

    @classmethod
    def fresh(cls, F, D, L, *, ctx=None):
        """An empty line of zeros (gss_mvdr_online_hold_init)."""
        if not _is_integer(F) or F < 1:
            raise ValueError(f'F={F!r}: a positive integer')
        check_bf_online(num_channels=D)
        if check_bf_lookahead(L) < 1:
            raise ValueError(f'lookahead={L!r}: a delay line holds at least one frame')
        ctx = ctx or default_context()
        hold = cls(ctx, F, D, L)
        ctx._check(ctx.lib.gss_mvdr_online_hold_init(ctx.handle, ctypes.byref(hold.struct())),
                   'gss_mvdr_online_hold_init')
        return hold

    def to_host(self):
        """{'frames', 'mask', 'filter'} as NumPy arrays plus 'held': everything `from_host` needs
        (synchronises)."""
        return dict(super().to_host(), held=self.held)

    @classmethod
    def from_host(cls, host, *, ctx=None):
        """A device line from the dict of `to_host` (in any context).  ValueError for shapes or a
        counter that do not fit each other."""
        frames = np.asarray(host['frames'])
        if frames.ndim != 3:
            raise ValueError(f'frames: shape {frames.shape} is not (F,L,D)')
        F, L, D = frames.shape
        if F < 1:
            raise ValueError(f'frames: shape {frames.shape} has no frequency')
        check_bf_online(num_channels=D)
        if check_bf_lookahead(L) < 1:
            raise ValueError(f'frames: shape {frames.shape} holds no frame')
        held = host['held']
        if not _is_integer(held) or not 0 <= held <= L:
            raise ValueError(f'held={held!r}: an integer in [0, {L}]')
        hold = cls._from_host(host, (F, D, L), ctx)
        hold.held = int(held)
        return hold


def _check_holds(holds, S, key, ctx, name='hold'):
    """S different `OnlineMVDRHold`s built for ``key`` = (F, D, L) that hold equally many frames,
    all in ``ctx`` (None: the first one's).  Returns the context and the list."""
    holds = [holds] if isinstance(holds, OnlineMVDRHold) else (
        list(holds) if hasattr(holds, '__iter__') else None)
    if holds is None or len(holds) != S:
        raise ValueError(f'{name}: {S} OnlineMVDRHold, one per target')
    for hold in holds:
        if not isinstance(hold, OnlineMVDRHold):
            raise ValueError(f'{name}: {type(hold).__name__} is not an OnlineMVDRHold')
        if hold.key != key:
            raise ValueError(f'{name}: built for ({hold._sizes}) = {hold.key}, the call has {key}')
        if ctx is not None and ctx is not hold.ctx:
            raise ValueError(f'{name}: it lives in another context than the call')
        ctx = hold.ctx
    if len({id(hold) for hold in holds}) != S:
        raise ValueError(f'{name}: the same line for two targets')
    if len({hold.held for hold in holds}) != 1:
        raise ValueError(f'{name}: the lines hold {[hold.held for hold in holds]} frames')
    return ctx, holds


def _hold_structs(holds):
    return (GssMvdrOnlineHold * len(holds))(*(hold.struct() for hold in holds))


def _holds_advance(holds, structs):
    """The host counters the library advanced -> the Python objects."""
    for hold, struct in zip(holds, structs):
        hold.held = int(struct.held)


def mvdr_online_release(hold, *, postfilter=None, return_filters=False):
    """The end of a delay line (gss_mvdr_online_release): the h held frames, filtered with the
    filter of the last frame that entered -> (h,F) complex128 for one `OnlineMVDRHold`, (S,h,F)
    for a sequence of S (times their own target-mask values with ``postfilter='mask_mul'``), then
    with ``return_filters`` the filters (h,F,D) / (S,h,F,D).  The line is empty afterwards, the
    running sums are not touched; with nothing held nothing is launched."""
    single = isinstance(hold, OnlineMVDRHold)
    if not single and (not hasattr(hold, '__len__') or len(hold) < 1
                       or not isinstance(hold[0], OnlineMVDRHold)):
        raise ValueError('hold: an OnlineMVDRHold or a sequence of them')
    if postfilter not in (None, 'mask_mul'):
        raise ValueError(f"postfilter={postfilter!r}: None or 'mask_mul'")
    first = hold if single else hold[0]
    S = 1 if single else len(hold)
    ctx, holds = _check_holds(hold, S, first.key, None)
    F, D, h = first.F, first.D, first.held
    if h == 0:
        X, W = np.zeros((S, 0, F), np.complex128), np.zeros((S, 0, F, D), np.complex128)
    else:
        structs = _hold_structs(holds)
        X_d = ctx.empty(16 * S * h * F)
        W_d = ctx.empty(16 * S * F * h * D) if return_filters else None
        ctx._check(ctx.lib.gss_mvdr_online_release(
            ctx.handle, structs, S, int(postfilter == 'mask_mul'), c_void_p(X_d.ptr),
            c_void_p(W_d.ptr) if W_d is not None else None, None), 'gss_mvdr_online_release')
        _holds_advance(holds, structs)
        X = ctx.to_host(X_d, (S, h, F), np.complex128)
        W = (np.ascontiguousarray(ctx.to_host(W_d, (S, F, h, D), np.complex128)
                                  .transpose(0, 2, 1, 3)) if return_filters else None)
    if single:
        X, W = X[0], (W[0] if W is not None else None)
    return (X, W) if return_filters else X


def _mvdr_online_lookahead(Y, X_mask, N_mask, ban, forget, loading, ref_channel, L, state, hold,
                           return_filters, return_fallbacks, ctx):
    """`mvdr_souden_online_from_masks` with a look-ahead L >= 1 (gss_mvdr_online_lookahead)."""
    D, T, F = Y.shape
    one_shot = hold is None
    if not one_shot:
        if state is None:
            raise ValueError('state: a delay line needs the state it belongs to (hold= without '
                             'state=)')
        ctx = _check_holds(hold, 1, (F, D, L), ctx)[0]
    ctx = _state_context(state, OnlineMVDRState, (F, D), ctx) or default_context()
    fallbacks = 0
    if T == 0 or F == 0:
        X_hat, W = np.zeros((0, F), np.complex128), np.zeros((0, F, D), np.complex128)
    else:
        if state is None:
            state = OnlineMVDRState.fresh(F, D, loading, Y, ctx=ctx)
        if one_shot:
            hold = OnlineMVDRHold.fresh(F, D, L, ctx=ctx)
        R = max(0, hold.held + T - L)
        Y_d, _ = _obs_to_device_ftd(ctx, Y)
        mx = _mask_to_device_ft(ctx, X_mask, T, F)
        mn = _mask_to_device_ft(ctx, N_mask, T, F)
        X_d = ctx.empty(max(16 * F * R, 16))
        W_d = ctx.empty(max(16 * F * R * D, 16)) if return_filters else None
        cfg = _bf_online_cfg(forget, loading, ref_channel)
        struct = hold.struct()
        ctx._check(ctx.lib.gss_mvdr_online_lookahead(
            ctx.handle, c_void_p(Y_d.ptr), F, T, D, c_void_p(mx.ptr), c_void_p(mn.ptr),
            int(bool(ban)), ctypes.byref(cfg), ctypes.byref(state.struct()), ctypes.byref(struct),
            c_void_p(X_d.ptr), c_void_p(W_d.ptr) if W_d is not None else None, None),
            'gss_mvdr_online_lookahead')
        _holds_advance([hold], [struct])
        if R:
            X_hat = np.ascontiguousarray(ctx.to_host(X_d, (F, R), np.complex128).T)
        else:
            X_hat = np.zeros((0, F), np.complex128)
        W = None
        if return_filters:
            W = (np.ascontiguousarray(ctx.to_host(W_d, (F, R, D), np.complex128).transpose(1, 0, 2))
                 if R else np.zeros((0, F, D), np.complex128))
        if return_fallbacks:
            fallbacks = ctx.last_mvdr_online_fallbacks()
        if one_shot:
            tail = mvdr_online_release(hold, return_filters=return_filters)
            if return_filters:
                X_hat, W = np.concatenate([X_hat, tail[0]]), np.concatenate([W, tail[1]])
            else:
                X_hat = np.concatenate([X_hat, tail])
    out = (X_hat,) + ((W,) if return_filters else ()) + ((fallbacks,) if return_fallbacks else ())
    return out if len(out) > 1 else X_hat


def _check_online_mask(mask, name, T, F):
    mask = np.asarray(mask, dtype=np.float64)
    if mask.shape != (T, F):
        raise ValueError(f'{name}: shape {mask.shape} is not (T,F) = ({T},{F})')
    if not np.all(np.isfinite(mask)) or np.any(mask < 0):
        raise ValueError(f'{name}: a mask value is negative or not finite')
    return mask


def mvdr_souden_online_from_masks(Y, X_mask, N_mask, ban=False, *, forget=BF_ONLINE_FORGET,
                                  loading=BF_ONLINE_LOADING, ref_channel=0, state=None,
                                  return_filters=False, return_fallbacks=False, ctx=None,
                                  lookahead=0, hold=None):
    """The online MVDR (gss_mvdr_online): Y (D,T,F), 2-D masks (T,F) -> X_hat (T,F) complex128.
    Both PSD matrices are running sums that forget at the rate ``forget``; the filter of frame t
    is solved from the sums INCLUDING frame t (look-ahead ``lookahead``, default 0).  ``state``: an
    `OnlineMVDRState` to continue from, advanced IN PLACE by the T frames (feeding a recording in
    blocks through one state gives the bits of one call); None: a fresh state initialised from
    ``Y`` with ``loading``, thrown away.  ``ref_channel`` = -1: the whole-window beamformer's
    choice over the call's frames (not causal; AssertionError when an SNR is not finite, like
    there).  Returns X_hat, then with ``return_filters`` the filters (T,F,D), then with
    ``return_fallbacks`` the number of (frequency, frame) pairs whose noise matrix had no Cholesky
    factor (their X_hat and filter are 0).

    ``lookahead`` = L >= 1 (gss_mvdr_online_lookahead): frame g is filtered with the filter of
    frame g + L -- L frames of latency for a filter that has already seen what follows, a
    speaker's onset above all; the sums, the filters and the fallback counts are those of L = 0.
    ``hold`` None: the one-shot form, the call plus the release of its line -> (T,F), the last L
    frames with the filter of frame T - 1.  ``hold``: an `OnlineMVDRHold` built for (F,D,L),
    advanced IN PLACE with ``state`` (required): the call returns the max(0, held + T - L) frames
    it releases, `mvdr_online_release` ends the line.  ``ref_channel`` = -1 is refused."""
    Y = np.asarray(Y)
    if Y.ndim != 3:
        raise ValueError(f'Y: shape {Y.shape} is not (D,T,F)')
    D, T, F = Y.shape
    forget, loading, ref_channel = check_bf_online(forget, loading, ref_channel, D)
    lookahead = check_bf_lookahead(lookahead, ref_channel)
    if hold is not None and lookahead == 0:
        raise ValueError('hold: a delay line with lookahead=0')
    X_mask = _check_online_mask(X_mask, 'X_mask', T, F)
    N_mask = _check_online_mask(N_mask, 'N_mask', T, F)
    if lookahead:
        return _mvdr_online_lookahead(Y, X_mask, N_mask, ban, forget, loading, ref_channel,
                                      lookahead, state, hold, return_filters, return_fallbacks, ctx)
    ctx = _state_context(state, OnlineMVDRState, (F, D), ctx) or default_context()
    fallbacks = 0
    if T == 0 or F == 0:
        X_hat, W = np.zeros((T, F), np.complex128), np.zeros((T, F, D), np.complex128)
    else:
        Y_d, _ = _obs_to_device_ftd(ctx, Y)
        mx = _mask_to_device_ft(ctx, X_mask, T, F)
        mn = _mask_to_device_ft(ctx, N_mask, T, F)
        X_d = ctx.empty(16 * F * T)
        W_d = ctx.empty(16 * F * T * D) if return_filters else None
        cfg = _bf_online_cfg(forget, loading, ref_channel)
        ctx._check(ctx.lib.gss_mvdr_online(
            ctx.handle, c_void_p(Y_d.ptr), F, T, D, c_void_p(mx.ptr), c_void_p(mn.ptr),
            int(bool(ban)), ctypes.byref(cfg),
            ctypes.byref(state.struct()) if state is not None else None, c_void_p(X_d.ptr),
            c_void_p(W_d.ptr) if W_d is not None else None), 'gss_mvdr_online')
        _check_ref_channel(ctx)
        X_hat = np.ascontiguousarray(ctx.to_host(X_d, (F, T), np.complex128).T)
        W = (np.ascontiguousarray(ctx.to_host(W_d, (F, T, D), np.complex128).transpose(1, 0, 2))
             if return_filters else None)
        if return_fallbacks:
            fallbacks = ctx.last_mvdr_online_fallbacks()
    out = (X_hat,) + ((W,) if return_filters else ()) + ((fallbacks,) if return_fallbacks else ())
    return out if len(out) > 1 else X_hat


GSS_ONLINE_FORGET = 0.99       # choices, not measurements
GSS_ONLINE_PRIOR_MASS = 1.0
_ONLINE_MAX_CLASSES = 8        # include/gss_hip.h: GSS_CACGMM_ONLINE_MAX_CLASSES


def check_gss_online(forget=GSS_ONLINE_FORGET, prior_mass=GSS_ONLINE_PRIOR_MASS, num_classes=None,
                     num_channels=None):
    """The settings of the online CACGMM -- the one place that validates them, before any device
    work.  ValueError naming the argument: ``forget`` a finite number in (0, 1], ``prior_mass``
    (the mass of a fresh state, or the mass a model is given) a finite number > 0,
    ``num_classes`` an integer in [1, 8], ``num_channels`` an integer in [1, 32].  Returns
    (forget, prior_mass)."""
    if not _is_real(forget) or not np.isfinite(forget) or not 0 < forget <= 1:
        raise ValueError(f'forget={forget!r}: a finite number in (0, 1]')
    if not _is_real(prior_mass) or not np.isfinite(prior_mass) or not prior_mass > 0:
        raise ValueError(f'prior_mass={prior_mass!r}: a finite number > 0')
    if num_classes is not None and (not _is_integer(num_classes)
                                    or not 1 <= num_classes <= _ONLINE_MAX_CLASSES):
        raise ValueError(f'num_classes={num_classes!r}: an integer in [1, {_ONLINE_MAX_CLASSES}]')
    if num_channels is not None and (not _is_integer(num_channels)
                                     or not 1 <= num_channels <= _MAX_CHANNELS):
        raise ValueError(f'num_channels={num_channels!r}: an integer in [1, {_MAX_CHANNELS}]')
    return float(forget), float(prior_mass)


class OnlineCACGMMState(_OnlineState):
    """The state of the online CACGMM in HBM (gss_cacgmm_online_state), caller-owned like an
    `OnlineMVDRState`: the running sums ``s`` (F,K,D,D), complex128, Hermitian, and the masses
    ``n`` (F,K).  The model they stand for is B_k = s_k / n_k, pi_k = n_k / sum_j n_j."""
    _sizes = 'F, K, D'
    dtypes = {'s': np.complex128, 'n': np.float64}

    def __init__(self, ctx, F, K, D):
        super().__init__(ctx, F, K, D)
        self.F, self.K, self.D = self.key

    @staticmethod
    def _shapes(F, K, D):
        return {'s': (F, K, D, D), 'n': (F, K)}

    def struct(self):
        return GssCacgmmOnlineState(s=self.bufs['s'].ptr, n=self.bufs['n'].ptr, F=self.F, K=self.K,
                                    D=self.D)

    @classmethod
    def fresh(cls, F, K, D, prior_mass=GSS_ONLINE_PRIOR_MASS, *, ctx=None):
        """s_k = prior_mass * I, n_k = prior_mass (gss_cacgmm_online_init): all classes are the
        same, so only a mask tells them apart."""
        if not _is_integer(F) or F < 1:
            raise ValueError(f'F={F!r}: a positive integer')
        check_gss_online(prior_mass=prior_mass, num_classes=K, num_channels=D)
        ctx = ctx or default_context()
        state = cls(ctx, F, K, D)
        ctx._check(ctx.lib.gss_cacgmm_online_init(
            ctx.handle, state.F, state.K, state.D, float(prior_mass), None, 0.0,
            ctypes.byref(state.struct())), 'gss_cacgmm_online_init')
        return state

    @classmethod
    def from_model(cls, model, mass=GSS_ONLINE_PRIOR_MASS, *, ctx=None):
        """Continue a fitted `cacgmm.CACGMM`: n_k = mass * weight_k, s_k = n_k * precision_k^-1,
        inverted on the device.  ``mass`` is how many frames the model counts for against the
        new ones.  ValueError when a precision has no Cholesky factor."""
        if not isinstance(model, CACGMM):
            raise ValueError(f'model: a CACGMM, not {type(model).__name__}')
        F, K, D = model.shape
        check_gss_online(prior_mass=mass, num_classes=K, num_channels=D)
        ctx = ctx or default_context()
        state = cls(ctx, F, K, D)
        dev = DeviceModel(ctx, F, K, D, model)
        ctx._check(ctx.lib.gss_cacgmm_online_init(
            ctx.handle, F, K, D, 0.0, ctypes.byref(dev.struct), float(mass),
            ctypes.byref(state.struct())), 'gss_cacgmm_online_init')
        return state

    def to_model(self):
        """The `cacgmm.CACGMM` the state stands for (gss_cacgmm_online_model): precision B_k^-1,
        ln det B_k and pi_k; `cacgmm_predict`, `cacgmm_fit`, ``save`` and `cacgmm_model_permute`
        work on it."""
        dev = DeviceModel(self.ctx, self.F, self.K, self.D)
        self.ctx._check(self.ctx.lib.gss_cacgmm_online_model(
            self.ctx.handle, ctypes.byref(self.struct()), ctypes.byref(dev.struct)),
            'gss_cacgmm_online_model')
        return dev.to_host(self.ctx)

    @classmethod
    def from_host(cls, host, *, ctx=None):
        """A device state from the dict of `to_host` ({'s', 'n'}; in any context: a state saved
        in one process continues in another).  ValueError for shapes that do not fit each other."""
        s = np.asarray(host['s'])
        if s.ndim != 4 or s.shape[2] != s.shape[3]:
            raise ValueError(f's: shape {s.shape} is not (F,K,D,D)')
        F, K, D, _ = s.shape
        if F < 1:
            raise ValueError(f's: shape {s.shape} has no frequency')
        check_gss_online(num_classes=K, num_channels=D)
        return cls._from_host(host, (F, K, D), ctx, lambda shape: f'(F,K) = {shape}')


def cacgmm_posteriors_online(Obs, source_activity_mask=None, *, num_classes=None,
                             forget=GSS_ONLINE_FORGET, prior_mass=GSS_ONLINE_PRIOR_MASS,
                             state=None, return_fallbacks=False, ctx=None):
    """The online CACGMM (gss_cacgmm_online): Obs (D,T,F) complex -> posterior (K,T,F) float64.
    Frame t is classified by the model of the frames before it (causal, no look-ahead) and then
    enters the running sums, which forget at the rate ``forget``.  ``source_activity_mask``
    (K,T) or (K,T,F), non-zero = active, or None.  ``state``: an `OnlineCACGMMState` to continue
    from, advanced IN PLACE by the T frames (feeding a recording in blocks through one state
    gives the bits of one call); None: a fresh state of ``prior_mass``, thrown away.  A fresh
    state has identical classes, so without a mask every posterior would stay 1 / K: no mask
    together with no state is a ValueError -- start from a model
    (`OnlineCACGMMState.from_model`).  ``num_classes``: K, needed only when neither a mask nor a
    state gives it.  With ``return_fallbacks`` also the number of (frequency, frame, class)
    triples whose s_k had no Cholesky factor (the class was taken as B_k = I for that frame)."""
    Obs = np.asarray(Obs)
    if Obs.ndim != 3:
        raise ValueError(f'Obs: shape {Obs.shape} is not (D,T,F)')
    D, T, F = Obs.shape
    if source_activity_mask is None and state is None:
        raise ValueError('source_activity_mask and state are both None: a fresh state has '
                         'identical classes and every posterior would be 1 / K; start from a '
                         'model (OnlineCACGMMState.from_model)')
    mask, K = None, None
    if source_activity_mask is not None:
        _, mask, K = guidance_tables(None, source_activity_mask, T, F)
    if K is None:       # (no mask: the state's, once `_state_context` has seen what it is)
        K = getattr(state, 'K', None)
    ctx = _state_context(state, OnlineCACGMMState, (F, K, D), ctx)
    if num_classes is not None and num_classes != K:
        raise ValueError(f'num_classes={num_classes!r} but the mask / state has {K} classes')
    forget, prior_mass = check_gss_online(forget, prior_mass, K, D)
    ctx = ctx or default_context()
    fallbacks = 0
    if T == 0 or F == 0:
        posterior = np.zeros((K, T, F), np.float64)
    else:
        Y_d, _ = _obs_to_device_ftd(ctx, Obs)
        guide = DeviceGuidance(ctx, None, mask, T) if mask is not None else None
        g_d = ctx.empty(8 * F * K * T)
        o_d = ctx.empty(8 * F * K * T)
        cfg = GssEmOnline(forget=forget, prior_mass=prior_mass)
        ctx._check(ctx.lib.gss_cacgmm_online(
            ctx.handle, c_void_p(Y_d.ptr), F, T, D, ctypes.byref(guide.struct) if guide else None,
            K, ctypes.byref(cfg), ctypes.byref(state.struct()) if state is not None else None,
            c_void_p(g_d.ptr)), 'gss_cacgmm_online')
        # (F, K*T) -> (K*T, F)
        ctx._check(ctx.lib.gss_layout_permute_f64(ctx.handle, c_void_p(g_d.ptr), F, K * T, 1, 2,
                                                  c_void_p(o_d.ptr)), 'gss_layout_permute_f64')
        posterior = ctx.to_host(o_d, (K, T, F), np.float64)
        if return_fallbacks:
            fallbacks = ctx.last_cacgmm_online_fallbacks()
    return (posterior, fallbacks) if return_fallbacks else posterior


def check_bf_lcmv(num_classes, target_index, interferer=None, candidates=None, min_mass=None,
                  num_channels=None):
    """The settings of the interferer-nulling LCMV as a gss_bf_lcmv, or ValueError naming the
    argument: ``interferer`` a class index other than the target (None: chosen among
    ``candidates``, an iterable of class indices -- None: every class but the target -- by its
    mass), ``min_mass`` finite and >= 0.  ``min_mass=None`` is ``2 * num_channels`` (0 while
    ``num_channels`` is not known, as in `check_bf_segments`)."""
    K = num_classes
    if not _is_integer(K) or not 1 <= K <= 19:
        raise ValueError(f'num_classes={K!r}: an integer in [1, 19]')
    if not _is_integer(target_index) or not 0 <= target_index < K:
        raise ValueError(f'target_index={target_index!r} outside [0, {K})')
    if interferer is not None:
        if not _is_integer(interferer) or not 0 <= interferer < K:
            raise ValueError(f'interferer={interferer!r} outside [0, {K})')
        if interferer == target_index:
            raise ValueError(f'interferer={interferer!r} is the target')
    bits = 0
    if candidates is None:
        candidates = [k for k in range(K) if k != target_index]
    elif isinstance(candidates, (str, bytes)) or not hasattr(candidates, '__iter__'):
        raise ValueError(f'candidates={candidates!r}: an iterable of class indices')
    for k in candidates:
        if not _is_integer(k) or not 0 <= k < K:
            raise ValueError(f'candidates: {k!r} outside [0, {K})')
        if k != target_index:
            bits |= 1 << int(k)
    if min_mass is None:
        min_mass = 2 * num_channels if num_channels is not None else 0
    if not _is_real(min_mass) or not np.isfinite(min_mass) or min_mass < 0:
        raise ValueError(f'min_mass={min_mass!r}: a finite number >= 0')
    return GssBfLcmv(interferer=-1 if interferer is None else int(interferer), candidates=bits,
                     min_mass=float(min_mass))


def _check_lcmv_channels(D):
    if D < 2:
        raise ValueError(f'D={D}: the LCMV needs at least 2 channels')
    if D >= 30:     # (not an `assert` statement: those vanish under python -O)
        raise AssertionError(f'assert D < 30 failed: D={D}')


def lcmv_souden_from_masks(Y, X_mask, I_mask, N_mask, ban=False, *, min_mass=0.0,
                           ref_channel=None, return_ref_channel=False, return_fallbacks=False,
                           ctx=None):
    """beamform_lcmv_souden_from_masks (gss_lcmv_souden): Souden's LCMV, distortionless for the
    target and with a null on the interferer, from three masks.  A frequency whose interferer
    mask sums to less than ``min_mass`` takes the MVDR of ``N_mask + I_mask`` instead;
    ``min_mass=0`` (the reference's behaviour) never falls back.  ``ref_channel`` names the
    reference channel; None = the SNR argmax against Phi_I + Phi_N.

    Y (D,T,F), masks (T,F) -> X_hat (T,F); with ``return_ref_channel`` / ``return_fallbacks`` a
    tuple (X_hat[, ref_channel][, number of frequencies that fell back]).  Argument errors are
    ValueError before any device work; a non-finite SNR raises AssertionError like the MVDR."""
    Y = np.asarray(Y)
    if Y.ndim != 3:
        raise ValueError(f'Y: shape {Y.shape} is not (D,T,F)')
    D, T, F = Y.shape
    _check_lcmv_channels(D)
    for name, m in (('X_mask', X_mask), ('I_mask', I_mask), ('N_mask', N_mask)):
        if np.shape(m) != (T, F):
            raise ValueError(f'{name}: shape {np.shape(m)} is not (T,F) = {(T, F)}')
    if not _is_real(min_mass) or not np.isfinite(min_mass) or min_mass < 0:
        raise ValueError(f'min_mass={min_mass!r}: a finite number >= 0')
    if ref_channel is not None and (not _is_integer(ref_channel) or not 0 <= ref_channel < D):
        raise ValueError(f'ref_channel={ref_channel!r} outside [0, {D})')
    ctx = ctx or default_context()
    Y_d, _ = _obs_to_device_ftd(ctx, Y)
    mx = _mask_to_device_ft(ctx, X_mask, T, F)
    mi = _mask_to_device_ft(ctx, I_mask, T, F)
    mn = _mask_to_device_ft(ctx, N_mask, T, F)
    X_d = ctx.empty(16 * F * T)
    ctx._check(ctx.lib.gss_lcmv_souden(
        ctx.handle, c_void_p(Y_d.ptr), F, T, D, c_void_p(mx.ptr), c_void_p(mi.ptr),
        c_void_p(mn.ptr), int(bool(ban)), -1 if ref_channel is None else int(ref_channel),
        float(min_mass), c_void_p(X_d.ptr), None), 'gss_lcmv_souden')
    ref = _check_ref_channel(ctx)
    out = (ctx.to_host(X_d, (T, F), np.complex128),)
    if return_ref_channel:
        out += (ref,)
    if return_fallbacks:
        out += (ctx.last_lcmv_fallbacks(),)
    return out if len(out) > 1 else out[0]


def lcmv_masks_from_posteriors(posterior, target_index, *, interferer=None, candidates=None,
                               drop_context=True, start_context_frames=0, end_context_frames=0,
                               ctx=None):
    """The three masks of the LCMV from the posteriors (gss_lcmv_masks_from_posteriors):
    posterior (K,T,F) -> (X_mask, I_mask, N_mask, interferer), masks (T,F).  The interferer is
    ``interferer``, or the class among ``candidates`` (None: every class but the target) of
    largest mass over the frames the context zeroing keeps; -1 (an all-zero I_mask) when there
    is no candidate or no mass.  N_mask is the sum of the remaining classes; the context frames
    are zeroed by the rule of ``masks[:, :start] = 0; if end > 0: masks[:, -end:] = 0``."""
    g = np.asarray(posterior, dtype=np.float64)
    if g.ndim != 3:
        raise ValueError(f'posterior: shape {g.shape} is not (K,T,F)')
    K, T, F = g.shape
    bf = check_bf_lcmv(K, target_index, interferer, candidates, 0)
    for name, v in (('start_context_frames', start_context_frames),
                    ('end_context_frames', end_context_frames)):
        if not _is_integer(v):
            raise ValueError(f'{name}={v!r} is not an integer')
    ctx = ctx or default_context()
    g_d = ctx.to_device(g.transpose(2, 0, 1))                       # (F,K,T)
    bufs = [ctx.empty(8 * F * T) for _ in range(3)]
    which = ctx.empty(16)
    ctx._check(ctx.lib.gss_lcmv_masks_from_posteriors(
        ctx.handle, c_void_p(g_d.ptr), F, K, T, int(target_index), ctypes.byref(bf),
        int(bool(drop_context)), int(start_context_frames), int(end_context_frames),
        *(c_void_p(b.ptr) for b in bufs), c_void_p(which.ptr)),
        'gss_lcmv_masks_from_posteriors')
    masks = [np.ascontiguousarray(ctx.to_host(b, (F, T), np.float64).T) for b in bufs]
    found = int(ctx.to_host(which, (1,), np.int32)[0])
    assert found == ctx.last_lcmv_interferer(), (found, ctx.last_lcmv_interferer())
    return (*masks, found)


WPD_POWER_FLOOR = 1e-3      # a choice, not a measurement


def check_bf_wpd(taps=10, delay=2, iterations=1, power_floor=WPD_POWER_FLOOR, ban=False,
                 num_channels=None, *, bf=None, segment_frames=None, null_interferer=False,
                 channel_keep=None, multi_target=False, activity=False):
    """The settings of the WPD beamformer as a gss_bf_wpd -- the one place that validates them.
    ValueError naming the argument: ``taps`` an integer >= 1, ``delay`` an integer >= 0,
    ``iterations`` an integer >= 1, ``power_floor`` finite in (0, 1]; AssertionError for
    ``num_channels`` >= 30 like the MVDR.  NotImplementedError for what the WPD does not combine
    with: a ``bf`` other than 'wpdSouden' / 'wpdSouden_ban' (None: not checked), the segment-wise
    and the interferer-nulling beamformer, the channel selection, the multi-target and the
    activity calls.  All before any device work."""
    for name, value, low in (('taps', taps, 1), ('delay', delay, 0), ('iterations', iterations, 1)):
        if not _is_integer(value) or value < low or value >= 2 ** 31:
            raise ValueError(f'{name}={value!r}: an integer >= {low}')
    if not _is_real(power_floor) or not np.isfinite(power_floor) \
            or not 0 < power_floor <= 1:
        raise ValueError(f'power_floor={power_floor!r}: a finite number in (0, 1]')
    if num_channels is not None:
        if not _is_integer(num_channels) or num_channels < 1:
            raise ValueError(f'num_channels={num_channels!r}: a positive integer')
        if num_channels >= 30:     # (not an `assert` statement: those vanish under python -O)
            raise AssertionError(f'assert D < 30 failed: D={num_channels}')
    if bf is not None and bf not in WPD_BF_TYPES:
        raise NotImplementedError(f'bf={bf!r} with WPD settings: only {sorted(WPD_BF_TYPES)}')
    for name, on in (('bf_segment_frames', segment_frames is not None),
                     ('bf_null_interferer', bool(null_interferer)),
                     ('channel_keep', channel_keep is not None),
                     ('several targets from one separation', bool(multi_target)),
                     ('the posterior activity', bool(activity))):
        if on:
            raise NotImplementedError(f'the WPD beamformer does not combine with {name}')
    return GssBfWpd(taps=int(taps), delay=int(delay), iterations=int(iterations),
                    ban=int(bool(ban)), power_floor=float(power_floor))


WPD_BF_TYPES = {'wpdSouden': False, 'wpdSouden_ban': True}      # type -> ban


def _gate_to_device(ctx, frame_gate, T):
    """frame_gate (T,) of 0 / 1 (bool or numbers; None: every frame counts) -> device uint8."""
    if frame_gate is None:
        return None
    g = np.asarray(frame_gate)
    if g.shape != (T,):
        raise ValueError(f'frame_gate: shape {g.shape} is not (T,) = {(T,)}')
    return ctx.to_device((g != 0).astype(np.uint8))


def wpe_weighted(Obs, weights, taps=10, delay=2, *, ctx=None):
    """One WPE step with the caller's weights (gss_wpe_weighted): Obs (D,T,F), weights (F,T) ->
    (D,T,F).  With ``get_power_inverse`` of the observation it is ``wpe_dtf(iterations=1)`` bit
    for bit."""
    Obs = np.asarray(Obs)
    if Obs.ndim != 3:
        raise ValueError(f'Obs: shape {Obs.shape} is not (D,T,F)')
    D, T, F = Obs.shape
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (F, T):
        raise ValueError(f'weights: shape {w.shape} is not (F,T) = {(F, T)}')
    check_bf_wpd(taps, delay)
    ctx = ctx or default_context()
    Y_d, _ = _obs_to_device_ftd(ctx, Obs)
    w_d = ctx.to_device(w)
    X_d = ctx.empty(16 * F * T * D)
    ctx._check(ctx.lib.gss_wpe_weighted(ctx.handle, c_void_p(Y_d.ptr), F, T, D, int(taps),
                                        int(delay), c_void_p(w_d.ptr), c_void_p(X_d.ptr)),
               'gss_wpe_weighted')
    return _ftd_to_host_dtf(ctx, X_d, D, T, F)


def wpd_weights(Y=None, X_mask=None, *, X_hat=None, frame_gate=None,
                power_floor=WPD_POWER_FLOOR, ctx=None):
    """The weights of one WPD iteration (gss_wpd_weights), (F,T): from Y (D,T,F) and the target
    mask X_mask (T,F) -- ``a = gate / max(mask * mean_d |Y|^2, power_floor * its gated maximum)``
    -- or from a beamformed signal ``X_hat`` (T,F) -- its power in the place of the masked
    one.  All zero at a frequency whose gated maximum is 0."""
    check_bf_wpd(power_floor=power_floor)
    if X_hat is not None:
        if Y is not None or X_mask is not None:
            raise ValueError('wpd_weights: either Y with X_mask, or X_hat')
        xh = np.ascontiguousarray(X_hat, dtype=np.complex128)
        if xh.ndim != 2:
            raise ValueError(f'X_hat: shape {xh.shape} is not (T,F)')
        T, F = xh.shape
        ctx = ctx or default_context()
        g_d = _gate_to_device(ctx, frame_gate, T)
        x_d = ctx.to_device(xh)
        a_d = ctx.empty(8 * F * T)
        ctx._check(ctx.lib.gss_wpd_weights(
            ctx.handle, None, F, T, 1, None, c_void_p(x_d.ptr),
            c_void_p(g_d.ptr) if g_d is not None else None, float(power_floor),
            c_void_p(a_d.ptr)), 'gss_wpd_weights')
        return ctx.to_host(a_d, (F, T), np.float64)
    if Y is None or X_mask is None:
        raise ValueError('wpd_weights: either Y with X_mask, or X_hat')
    Y = np.asarray(Y)
    if Y.ndim != 3:
        raise ValueError(f'Y: shape {Y.shape} is not (D,T,F)')
    D, T, F = Y.shape
    check_bf_wpd(power_floor=power_floor, num_channels=D)
    if np.shape(X_mask) != (T, F):
        raise ValueError(f'X_mask: shape {np.shape(X_mask)} is not (T,F) = {(T, F)}')
    ctx = ctx or default_context()
    g_d = _gate_to_device(ctx, frame_gate, T)
    Y_d, _ = _obs_to_device_ftd(ctx, Y)
    m_d = _mask_to_device_ft(ctx, X_mask, T, F)
    a_d = ctx.empty(8 * F * T)
    ctx._check(ctx.lib.gss_wpd_weights(
        ctx.handle, c_void_p(Y_d.ptr), F, T, D, c_void_p(m_d.ptr), None,
        c_void_p(g_d.ptr) if g_d is not None else None, float(power_floor),
        c_void_p(a_d.ptr)), 'gss_wpd_weights')
    return ctx.to_host(a_d, (F, T), np.float64)


def wpd_souden_from_masks(Y, X_mask, ban=False, *, taps=10, delay=2, iterations=1,
                          power_floor=WPD_POWER_FLOOR, frame_gate=None, ref_channel=None,
                          return_ref_channel=False, return_zero_pivots=False, ctx=None):
    """The WPD convolutional beamformer from a target mask (gss_wpd_souden): per iteration one
    WPE step on Y whose weights are 1 / target power (the masked observation power first, the
    power of the previous iteration's output afterwards; floored at ``power_floor`` times its
    maximum over the frames ``frame_gate`` keeps), then the Souden MVDR of the result with the
    target mask and those weights as the distortion mask.  ``frame_gate`` (T,) of 0 / 1 takes
    frames out of every statistic (None: none); ``ref_channel`` names the reference channel
    (None: the SNR argmax, chosen anew in every iteration).

    Y (D,T,F) -- the observation BEFORE any dereverberation --, X_mask (T,F) -> X_hat (T,F); with
    ``return_ref_channel`` / ``return_zero_pivots`` a tuple (X_hat[, ref_channel][, pivots the
    WPE solves zeroed]).  Argument errors are ValueError before any device work; a non-finite
    SNR raises AssertionError like the MVDR."""
    Y = np.asarray(Y)
    if Y.ndim != 3:
        raise ValueError(f'Y: shape {Y.shape} is not (D,T,F)')
    D, T, F = Y.shape
    bf = check_bf_wpd(taps, delay, iterations, power_floor, ban, D)
    if np.shape(X_mask) != (T, F):
        raise ValueError(f'X_mask: shape {np.shape(X_mask)} is not (T,F) = {(T, F)}')
    if ref_channel is not None and (not _is_integer(ref_channel) or not 0 <= ref_channel < D):
        raise ValueError(f'ref_channel={ref_channel!r} outside [0, {D})')
    if frame_gate is not None and np.shape(frame_gate) != (T,):
        raise ValueError(f'frame_gate: shape {np.shape(frame_gate)} is not (T,) = {(T,)}')
    ctx = ctx or default_context()
    g_d = _gate_to_device(ctx, frame_gate, T)
    Y_d, _ = _obs_to_device_ftd(ctx, Y)
    mx = _mask_to_device_ft(ctx, X_mask, T, F)
    X_d = ctx.empty(16 * F * T)
    ctx._check(ctx.lib.gss_wpd_souden(
        ctx.handle, c_void_p(Y_d.ptr), F, T, D, c_void_p(mx.ptr),
        c_void_p(g_d.ptr) if g_d is not None else None, ctypes.byref(bf),
        -1 if ref_channel is None else int(ref_channel), c_void_p(X_d.ptr), None),
        'gss_wpd_souden')
    ref = _check_ref_channel(ctx)
    out = (ctx.to_host(X_d, (T, F), np.complex128),)
    if return_ref_channel:
        out += (ref,)
    if return_zero_pivots:
        out += (ctx.last_wpd_zero_pivots(),)
    return out if len(out) > 1 else out[0]


def gev_from_masks(Y, X_mask, N_mask, ban=True, *, ctx=None):
    """beamform_gev_from_masks: Y (D,T,F), 2-D masks (T,F) -> X_hat (T,F).  The phase
    of a generalised eigenvector is arbitrary (upstream too); magnitudes are defined.
    Raises numpy.linalg.LinAlgError when the noise PSD matrix of a frequency is not positive
    definite, like scipy.linalg.eigh inside pb_bss get_gev_vector."""
    ctx = ctx or default_context()
    Y_d, (D, T, F) = _obs_to_device_ftd(ctx, Y)
    mx = _mask_to_device_ft(ctx, X_mask, T, F)
    mn = _mask_to_device_ft(ctx, N_mask, T, F)
    X_d = ctx.empty(16 * F * T)
    ctx._check(ctx.lib.gss_gev(ctx.handle, c_void_p(Y_d.ptr), F, T, D, c_void_p(mx.ptr),
                               c_void_p(mn.ptr), int(bool(ban)), c_void_p(X_d.ptr)), 'gss_gev')
    _check_ref_channel(ctx)
    return ctx.to_host(X_d, (T, F), np.complex128)


def activity_time_to_frequency_device(time_activity, size, shift, fading, *, ctx=None):
    """Device twin of database.chime5.activity_time_to_frequency (stft_pad=True)."""
    ctx = ctx or default_context()
    act = np.asarray(time_activity)
    lead = act.shape[:-1]
    N = act.shape[-1]
    a2 = np.ascontiguousarray((act.reshape(-1, N) != 0).astype(np.uint8))
    K = a2.shape[0]
    _prepare_windows(ctx, size, shift)
    T = stft_frames(N, size, shift, fading)
    a_d = ctx.to_device(a2)
    o_d = ctx.empty(max(K * T, 16))
    ctx._check(ctx.lib.gss_activity_time_to_frequency(
        ctx.handle, c_void_p(a_d.ptr), K, N, int(bool(fading)), c_void_p(o_d.ptr)),
        'gss_activity_time_to_frequency')
    return ctx.to_host(o_d, (K, T), np.uint8).astype(bool).reshape(lead + (T,))


# --------------------------------------------------------------------------
# envelope-variance channel selection (gss_channel_select; Wolf & Nadeu 2014)
# --------------------------------------------------------------------------
MAX_BANDS = 64          # bands of a band table (the accumulators of chsel_bands)


def _is_integer(value):
    return isinstance(value, (int, np.integer)) and not isinstance(value, bool)


def _is_real(value):
    return isinstance(value, (int, float, np.integer, np.floating)) \
        and not isinstance(value, bool)


def check_channel_bands(bands):
    if not _is_integer(bands) or not 1 <= bands <= MAX_BANDS:
        raise ValueError(f'bands={bands!r}: an integer in [1, {MAX_BANDS}]')
    return int(bands)


def check_channel_floor(floor):
    if not _is_real(floor) or not np.isfinite(floor) or not 0 <= floor < 1:
        raise ValueError(f'floor={floor!r}: a finite number in [0, 1)')
    return float(floor)


def check_channel_keep(keep, num_channels=None):
    """How many of ``num_channels`` channels a selection keeps.  An ``int`` >= 1 is a count (a
    count >= D keeps all channels); a ``float`` in (0, 1] is a share, n = max(1, ceil(share *
    D)), where a product within 1e-9 of an integer counts as that integer (0.8 of 20 channels
    is 16, not the 17 that 16.000000000000004 rounds up to).  bool, strings, NaN, 0, negative
    values and floats above 1 are ValueError.  Without ``num_channels`` the value is only
    checked and returned as it is."""
    if _is_integer(keep):
        if keep < 1:
            raise ValueError(f'keep={keep!r}: a count >= 1 or a share in (0, 1]')
        return int(keep) if num_channels is None else min(int(keep), int(num_channels))
    if isinstance(keep, (float, np.floating)) and 0 < keep <= 1:     # (NaN compares false)
        if num_channels is None:
            return float(keep)
        return max(1, int(np.ceil(np.round(float(keep) * int(num_channels), 9))))
    raise ValueError(f'keep={keep!r}: a count >= 1 or a share in (0, 1]')


def mel_bank(bands, stft_size, sample_rate=16000):
    """The default band table (B, F) of the channel selection, F = stft_size // 2 + 1: ``bands``
    triangular filters equally spaced on the HTK mel scale, mel = 2595 log10(1 + f / 700),
    between 0 and sample_rate / 2.  Filter b rises linearly (in Hz) from edge b to edge b + 1
    and falls to edge b + 2; it is evaluated at the centre frequencies k * sample_rate /
    stft_size of the F bins.  Built on the host, like the windows: the library holds no band
    policy."""
    bands = check_channel_bands(bands)
    if not _is_integer(stft_size) or stft_size < 2 or stft_size % 2:
        raise ValueError(f'stft_size={stft_size!r}: an even integer >= 2')
    if not _is_real(sample_rate) or not np.isfinite(sample_rate) or sample_rate <= 0:
        raise ValueError(f'sample_rate={sample_rate!r}: a positive number')
    F = int(stft_size) // 2 + 1
    top = 2595.0 * np.log10(1.0 + (float(sample_rate) / 2.0) / 700.0)
    edges = 700.0 * (10.0 ** (np.linspace(0.0, top, bands + 2) / 2595.0) - 1.0)
    freqs = np.arange(F) * (float(sample_rate) / int(stft_size))
    lo, mid, hi = edges[:-2, None], edges[1:-1, None], edges[2:, None]
    rise = (freqs[None, :] - lo) / (mid - lo)
    fall = (hi - freqs[None, :]) / (hi - mid)
    return np.maximum(0.0, np.minimum(rise, fall))


def check_channel_bank(bank, bands, num_frequencies, sample_rate=16000):
    """The band table of a selection on ``num_frequencies`` bins as a (B, F) float64 array:
    ``bank`` checked (2-D, 1 .. 64 rows, F columns, finite, non-negative), or None: the
    `mel_bank` of ``bands`` filters.  ValueError otherwise."""
    F = int(num_frequencies)
    if bank is None:
        bands = check_channel_bands(bands)
        if F < 2:
            raise ValueError(f'bank: the default mel bank needs at least 2 frequencies, not {F}')
        return mel_bank(bands, 2 * (F - 1), sample_rate)
    try:
        W = np.ascontiguousarray(bank, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('bank: not a real array') from None
    if W.ndim != 2 or not 1 <= W.shape[0] <= MAX_BANDS or W.shape[1] != F:
        raise ValueError(f'bank: shape {W.shape} is not (B, F) with 1 <= B <= {MAX_BANDS} '
                         f'and F = {F}')
    if not np.all(np.isfinite(W)) or np.any(W < 0):
        raise ValueError('bank: weights must be finite and >= 0')
    return W


class ChannelSelect:
    """The checked settings of a channel selection -- ``keep`` (count or share, see
    `check_channel_keep`; None: scores only), the band table (B, F) and the relative floor --
    and the table's copy in HBM per context.  `struct(ctx, D)` is the gss_channel_select of a
    call on D channels."""

    def __init__(self, keep, num_frequencies, bank=None, bands=40, floor=1e-10,
                 sample_rate=16000):
        self.keep = None if keep is None else check_channel_keep(keep)
        self.floor = check_channel_floor(floor)
        self.bank = check_channel_bank(bank, bands, num_frequencies, sample_rate)
        self._device = {}

    @property
    def bands(self):
        return self.bank.shape[0]

    def count(self, num_channels):
        return check_channel_keep(self.keep, num_channels)

    def struct(self, ctx, num_channels):
        buf = self._device.get(id(ctx))
        if buf is None or buf[0] is not ctx or buf[1].ptr is None:
            buf = self._device[id(ctx)] = (ctx, ctx.to_device(self.bank))
        return GssChannelSelect(bank_dev=buf[1].ptr, bands=self.bands,
                                keep=0 if self.keep is None else self.count(num_channels),
                                floor=self.floor)


def _check_obs_dtf(Obs):
    Obs = np.asarray(Obs)
    if Obs.ndim != 3:
        raise ValueError(f'Obs: shape {Obs.shape} is not (D,T,F)')
    if 0 in Obs.shape:
        raise ValueError(f'Obs: shape {Obs.shape} has an empty axis')
    return Obs


def channel_scores(Obs, bank=None, bands=40, floor=1e-10, return_band_variances=False, *,
                   sample_rate=16000, ctx=None):
    """The envelope-variance score of every channel of an STFT (gss_channel_scores): Obs
    (D,T,F) complex -> scores (D,) float64 in [0, B], high for channels that are close to the
    speaker and dry, 0 for a channel that is zero in every frame.  ``bank`` (B,F) >= 0 is the
    band table (None: `mel_bank` of ``bands`` filters for a ``sample_rate`` Hz signal),
    ``floor`` the floor of a band energy relative to its maximum over time.  With
    ``return_band_variances`` also V (B,D), the variance of the compressed envelope per band.
    The measure is written down in tests/channel_select_reference.py.  Argument errors are
    ValueError before any device work."""
    Obs = _check_obs_dtf(Obs)
    sel = ChannelSelect(None, Obs.shape[2], bank, bands, floor, sample_rate)
    ctx = ctx or default_context()
    Y_d, (D, T, F) = _obs_to_device_ftd(ctx, Obs)
    st = sel.struct(ctx, D)
    s_d = ctx.empty(8 * D)
    v_d = ctx.empty(8 * sel.bands * D) if return_band_variances else None
    ctx._check(ctx.lib.gss_channel_scores(
        ctx.handle, c_void_p(Y_d.ptr), F, T, D, ctypes.byref(st), c_void_p(s_d.ptr),
        c_void_p(v_d.ptr) if v_d is not None else None), 'gss_channel_scores')
    scores = ctx.to_host(s_d, (D,), np.float64)
    if return_band_variances:
        return scores, ctx.to_host(v_d, (sel.bands, D), np.float64)
    return scores


def select_channels(Obs, keep, bank=None, bands=40, floor=1e-10, *, sample_rate=16000,
                    ctx=None):
    """Keep the ``keep`` channels of highest `channel_scores` (gss_select_channels): Obs
    (D,T,F) -> (Obs[channels] (n,T,F), channels (n,) int in ascending order -- the array-major
    order of the observation survives).  ``keep``: a count or a share of D, see
    `check_channel_keep`; equal scores go to the lower channel index.  Argument errors are
    ValueError before any device work."""
    Obs = _check_obs_dtf(Obs)
    sel = ChannelSelect(keep, Obs.shape[2], bank, bands, floor, sample_rate)
    n = sel.count(Obs.shape[0])
    ctx = ctx or default_context()
    Y_d, (D, T, F) = _obs_to_device_ftd(ctx, Obs)
    st = sel.struct(ctx, D)
    o_d = ctx.empty(16 * F * T * n)
    c_d = ctx.empty(max(4 * n, 16))
    ctx._check(ctx.lib.gss_select_channels(
        ctx.handle, c_void_p(Y_d.ptr), F, T, D, ctypes.byref(st), c_void_p(o_d.ptr),
        c_void_p(c_d.ptr)), 'gss_select_channels')
    ctx.selected_count = n
    channels = ctx.to_host(c_d, (n,), np.int32).astype(int)
    return _ftd_to_host_dtf(ctx, o_d, n, T, F), channels


def _check_select_params(params, what):
    """What a selection cannot be combined with, before any device work."""
    if params.bf == _BF_CODES['ch2']:
        raise NotImplementedError(f"{what} with bf='ch2': 'ch2' names a physical channel")
    if params.wpe and params.wpe_arrays > 1:
        raise NotImplementedError(f'{what} with wpe_arrays={params.wpe_arrays}: a selection '
                                  'breaks the equal arrays of the per-array WPE')


def enhance_observation_select(obs, activity, target_index, start_context_samples,
                               end_context_samples, *, keep, bank=None, bands=40, floor=1e-10,
                               sample_rate=16000, params=None, window=None, debug=False,
                               ctx=None, **param_kwargs):
    """`enhance_observation` on the ``keep`` channels the envelope-variance measure ranks best
    (gss_enhance_observation_select): the STFT runs on all D channels, `select_channels` on the
    device, then the unchanged pipeline on the kept n.  obs (D,N) float64 or int16 PCM.  With
    n = D the result equals `enhance_observation` bit for bit.  ``debug=True`` details as
    there -- ``Obs`` is (n,T,F) and ``ref_channel`` an index into the kept channels -- plus
    ``selected_channels`` (n,), which maps it back.  The limits of the beamformers (fewer than
    30 channels) apply to n, not D.  bf='ch2' and a per-array WPE are NotImplementedError, bad
    settings ValueError, both before any device work."""
    params = _fused_params(params, param_kwargs)
    _check_select_params(params, 'channel selection')
    obs = _obs_dn(obs)
    sel = ChannelSelect(keep, params.stft_size // 2 + 1, bank, bands, floor, sample_rate)
    n = sel.count(obs.shape[0])
    ctx = ctx or default_context()
    _prepare_windows(ctx, params.stft_size, params.stft_shift, window)
    utt = ResidentUtterance(ctx, obs, activity, params, pcm=obs.dtype == np.int16)
    bufs, taps = _debug_taps(utt, D=n) if debug else ({}, None)
    utt.enqueue(target_index, start_context_samples, end_context_samples, taps,
                channel_select=sel)
    x_hat, details = _one_target_result(utt, bufs, debug, D=n)
    if not debug:
        return x_hat
    details['selected_channels'] = np.array(ctx.last_selected_channels(n), dtype=int)
    return x_hat, details


# --------------------------------------------------------------------------
# posterior activity
# --------------------------------------------------------------------------
def check_freq_weights(freq_weights, num_frequencies):
    """The frequency weights of the posterior activity as a float64 (F,) array, or None for all
    ones.  ValueError for another shape and for negative or non-finite values (the library does
    not inspect the table)."""
    if freq_weights is None:
        return None
    try:
        if np.iscomplexobj(freq_weights):
            raise TypeError
        w = np.asarray(freq_weights, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('freq_weights: not an array of real numbers') from None
    if w.shape != (int(num_frequencies),):
        raise ValueError(f'freq_weights: shape {w.shape} is not ({int(num_frequencies)},)')
    if not np.all(np.isfinite(w)):
        raise ValueError('freq_weights: not finite')
    if np.any(w < 0):
        raise ValueError('freq_weights: negative')
    return np.ascontiguousarray(w)


def check_posterior_activity_args(Obs, posterior, freq_weights=None):
    """Obs (D,T,F) complex, posterior (K,T,F) and the weights of `posterior_activity` as arrays;
    ValueError for anything else, before any device work."""
    Obs, posterior = np.asarray(Obs), np.asarray(posterior)
    if Obs.ndim != 3:
        raise ValueError(f'Obs: shape {Obs.shape} is not (D,T,F)')
    if posterior.ndim != 3:
        raise ValueError(f'posterior: shape {posterior.shape} is not (K,T,F)')
    if 0 in Obs.shape or 0 in posterior.shape:
        raise ValueError(f'Obs {Obs.shape}, posterior {posterior.shape}: an empty axis')
    if Obs.shape[1:] != posterior.shape[1:]:
        raise ValueError(f'Obs (D,T,F) = {Obs.shape} and posterior (K,T,F) = {posterior.shape} '
                         'differ in T or F')
    return Obs, posterior, check_freq_weights(freq_weights, Obs.shape[2])


def posterior_activity(Obs, posterior, freq_weights=None, return_power=False, *, ctx=None):
    """The power-weighted share of every frame that the posteriors give each class
    (gss_posterior_activity): Obs (D,T,F) complex -- the signal the EM saw, i.e. after WPE --,
    posterior (K,T,F) -> scores (K,T) float64,

        score[k,t] = sum_f w[f] posterior[k,t,f] p[t,f] / power[t],   p = sum_d |Obs|^2,
        power[t] = sum_f w[f] p[t,f]          (score 0 where power[t] is 0),

    in [0, 1] up to rounding, not clamped.  ``freq_weights`` (F,) >= 0, None: all ones.  With
    ``return_power`` also power (T,).  The measure is written down in
    tests/posterior_activity_reference.py; `pb_chime5_amd.posterior_activity.decide` turns the
    scores into a decision.  Argument errors are ValueError before any device work."""
    Obs, posterior, w = check_posterior_activity_args(Obs, posterior, freq_weights)
    ctx = ctx or default_context()
    Y_d, (D, T, F) = _obs_to_device_ftd(ctx, Obs)
    K = posterior.shape[0]
    g_d = ctx.to_device(np.ascontiguousarray(
        np.asarray(posterior, dtype=np.float64).transpose(2, 0, 1)))
    w_d = ctx.to_device(w) if w is not None else None
    s_d = ctx.empty(8 * K * T)
    p_d = ctx.empty(8 * T) if return_power else None
    ctx._check(ctx.lib.gss_posterior_activity(
        ctx.handle, c_void_p(Y_d.ptr), c_void_p(g_d.ptr), F, K, T, D,
        c_void_p(w_d.ptr) if w_d is not None else None, c_void_p(s_d.ptr),
        c_void_p(p_d.ptr) if p_d is not None else None), 'gss_posterior_activity')
    scores = ctx.to_host(s_d, (K, T), np.float64)
    if return_power:
        return scores, ctx.to_host(p_d, (T,), np.float64)
    return scores


def enhance_observation_activity(obs, activity, target_index, start_context_samples,
                                 end_context_samples, *, freq_weights=None, params=None,
                                 window=None, debug=False, ctx=None, wpe_arrays=None,
                                 **param_kwargs):
    """`enhance_observation` plus `posterior_activity` of the pipeline's own post-WPE observation
    and its posteriors before context zeroing, in one call and without copying either
    (gss_enhance_observation_activity).  Returns (x_hat, scores (K,T), power (T,)), or
    (x_hat, scores, power, details) with ``debug=True``; x_hat and the details have the bits of
    `enhance_observation`.  ``freq_weights`` (stft_size // 2 + 1,) >= 0, None: all ones; a bad
    table is ValueError before any device work."""
    params = _fused_params(params, param_kwargs)
    w = check_freq_weights(freq_weights, params.stft_size // 2 + 1)
    obs = _obs_dn(obs)
    ctx, utt, bufs, taps = _resident_call(obs, activity, params, wpe_arrays, window, debug, ctx)
    w_d = ctx.to_device(w) if w is not None else None
    s_d = ctx.empty(8 * utt.K * max(utt.T, 1))
    p_d = ctx.empty(8 * max(utt.T, 1))
    utt.enqueue(target_index, start_context_samples, end_context_samples, taps,
                activity=(w_d, s_d, p_d))
    x_hat, details = _one_target_result(utt, bufs, debug)
    scores = ctx.to_host(s_d, (utt.K, utt.T), np.float64)
    power = ctx.to_host(p_d, (utt.T,), np.float64)
    return (x_hat, scores, power, details) if debug else (x_hat, scores, power)


# --------------------------------------------------------------------------
# fused pipeline
# --------------------------------------------------------------------------
def make_params(*, stft_size=1024, stft_shift=256, stft_fading=True, wpe=True, wpe_taps=10,
                wpe_delay=2, wpe_iterations=3, wpe_psd_context=0, bss_iterations=20,
                bss_iterations_post=1, bf_drop_context=True, bf='mvdrSouden_ban',
                postfilter=None, wpe_arrays=0):
    """gss_params.  ``wpe_arrays``: 0 or 1 = one joint WPE over all channels (the reference's
    multiarray pipeline); A > 1 = WPE per microphone array, A arrays of D / A channels in
    array-major order (checked against D when an utterance is enhanced)."""
    if bf not in _BF_CODES:
        raise NotImplementedError(bf)
    if postfilter not in _POSTFILTER_CODES:
        raise NotImplementedError(postfilter)
    return GssParams(
        stft_size=stft_size, stft_shift=stft_shift, stft_fading=int(bool(stft_fading)),
        wpe=int(bool(wpe)), wpe_taps=wpe_taps, wpe_delay=wpe_delay,
        wpe_iterations=wpe_iterations, bss_iterations=bss_iterations,
        bss_iterations_post=bss_iterations_post, bf_drop_context=int(bool(bf_drop_context)),
        bf=_BF_CODES[bf], postfilter=_POSTFILTER_CODES[postfilter],
        wpe_psd_context=check_psd_context(wpe_psd_context),
        wpe_arrays=check_wpe_arrays(wpe_arrays) and int(wpe_arrays or 0))


def params_for(params, num_channels, wpe_arrays=None):
    """``params`` for one utterance of ``num_channels`` channels with ``wpe_arrays`` microphone
    arrays (None: as ``params`` says).  Raises ValueError when the arrays do not divide the
    channels and WPE runs (without WPE the field is not read)."""
    if wpe_arrays is None:
        wpe_arrays = params.wpe_arrays
    check_wpe_arrays(wpe_arrays, num_channels if params.wpe else None)
    if int(wpe_arrays) == params.wpe_arrays:
        return params
    p = GssParams.from_buffer_copy(params)
    p.wpe_arrays = int(wpe_arrays)
    return p


# The fused one-target entries by the option a call adds to the plain one (None): option ->
# (entry, its _pcm16 twin or None, what the assertions call it).  Every entry but 'activity'
# inserts one descriptor before out_dev.
_FUSED_ENTRIES = {
    None: ('gss_enhance_observation', 'gss_enhance_observation_pcm16', 'plain'),
    'wpd': ('gss_enhance_observation_wpd', None, 'WPD'),
    'wpe_online': ('gss_enhance_observation_wpe_online', None, 'online WPE'),
    'bf_online': ('gss_enhance_observation_bf_online', None, 'online MVDR'),
    'gss_online': ('gss_enhance_observation_gss_online', None, 'online CACGMM'),
    'activity': ('gss_enhance_observation_activity', None, 'activity'),
    'lcmv': ('gss_enhance_observation_lcmv', None, 'LCMV'),
    'channel_select': ('gss_enhance_observation_select', 'gss_enhance_observation_select_pcm16',
                       'selection'),
    'segments': ('gss_enhance_observation_segments', None, 'segment-wise'),
}


def _enqueue_fused(ctx, params, obs_d, D, N, act_d, K, N_act, target_index, start_context,
                   end_context, out_d, taps=None, pcm=False, option=None, value=None):
    """The one place that issues a fused one-target call on inputs in HBM.  ``option``: a key of
    `_FUSED_ENTRIES`; ``value``: the struct that entry takes (gss_bf_wpd, gss_wpe_online_cfg,
    gss_bf_online, gss_bf_lcmv, gss_bf_segments, gss_channel_select), for 'activity' the device
    buffers (weights or None, scores, power or None), for 'gss_online' the pair (gss_em_online,
    gss_bf_online or None).  ``pcm``: int16 samples, the entry's _pcm16 twin."""
    name, twin, label = _FUSED_ENTRIES[option]
    assert twin is not None or not pcm, f'the {label} call has no pcm16 twin'

    def ptr(buf):
        return c_void_p(buf.ptr) if buf is not None else None
    before, after = (), ()
    if option == 'activity':    # the weights before out_dev, the scores and the power after it
        before, after = (ptr(value[0]),), (ptr(value[1]), ptr(value[2]))
    elif option == 'gss_online':
        before = (ctypes.byref(value[0]), ctypes.byref(value[1]) if value[1] is not None else None)
    elif option is not None:
        before = (ctypes.byref(value),)
    ctx._check(getattr(ctx.lib, twin if pcm else name)(
        ctx.handle, ctypes.byref(params), ptr(obs_d), D, N, ptr(act_d), K, N_act,
        int(target_index), int(start_context), int(end_context), *before, ptr(out_d), *after,
        ctypes.byref(taps) if taps is not None else None), name)
    if option == 'channel_select':
        ctx.selected_count = value.keep


class ResidentUtterance:
    """An utterance whose inputs already sit in HBM (what bench.py times).  ``pcm=True``: the
    samples are int16 PCM, scaled by 2^-15 on the device (the _pcm16 entries); otherwise they
    are taken as float64."""

    def __init__(self, ctx, obs, activity, params, wpe_arrays=None, pcm=False):
        self.pcm = bool(pcm)
        obs = np.ascontiguousarray(obs, dtype=np.int16 if self.pcm else np.float64)
        act = np.ascontiguousarray((np.asarray(activity) != 0).astype(np.uint8))
        self.ctx = ctx
        self.D, self.N = obs.shape
        self.K = act.shape[0]
        self.N_act = act.shape[1]
        self.params = params = params_for(params, self.D, wpe_arrays)
        self.T = stft_frames(self.N, params.stft_size, params.stft_shift,
                             params.stft_fading)
        self.n_out = int(ctx.lib.gss_istft_num_samples(
            self.T, params.stft_size, params.stft_shift, params.stft_fading))
        self.obs_d = ctx.to_device(obs)
        self.act_d = ctx.to_device(act)
        self.out_d = ctx.empty(8 * max(self.n_out, 1))

    def enqueue(self, target_index, start_context, end_context, taps=None, segments=None,
                channel_select=None, lcmv=None, activity=None, wpd=None, wpe_online=None,
                bf_online=None, gss_online=None):
        """``gss_online``: a pair (gss_em_online, gss_bf_online or None) for the online CACGMM in
        the place of the guided EM, with the second member the online MVDR (and through its
        ``wpe_online`` field the online WPE) as well (gss_enhance_observation_gss_online; float64
        samples only, on its own).
        ``bf_online``: a gss_bf_online for the online MVDR in the place of the whole-window one,
        with its ``wpe_online`` field the online WPE as well (gss_enhance_observation_bf_online;
        float64 samples only, on its own).
        ``wpe_online``: a gss_wpe_online_cfg for the online WPE in the place of the offline one
        (gss_enhance_observation_wpe_online; float64 samples only, on its own).
        ``wpd``: a gss_bf_wpd (`check_bf_wpd`) for the WPD beamformer on the STFT before WPE
        (gss_enhance_observation_wpd; float64 samples only, on its own).
        ``segments``: a gss_bf_segments (`check_bf_segments`) for the segment-wise
        beamformer (gss_enhance_observation_segments; float64 samples only).
        ``channel_select``: a `ChannelSelect` for the envelope-variance selection ahead of WPE
        (gss_enhance_observation_select / its pcm16 twin; not together with segments).
        ``lcmv``: a gss_bf_lcmv (`check_bf_lcmv`) for the interferer-nulling beamformer
        (gss_enhance_observation_lcmv; float64 samples only, on its own).
        ``activity``: device buffers (weights (F,) or None, scores (K,T), power (T,) or None) for
        the posterior activity of the call's own observation and posteriors
        (gss_enhance_observation_activity; float64 samples only, on its own)."""
        given = [(name, v) for name, v in (('gss_online', gss_online),
                                           ('bf_online', bf_online), ('wpe_online', wpe_online),
                                           ('wpd', wpd),
                                           ('activity', activity), ('lcmv', lcmv),
                                           ('channel_select', channel_select),
                                           ('segments', segments)) if v is not None]
        option, value = given[0] if given else (None, None)
        assert len(given) <= 1, ('no selection inside the segment-wise call'
                                 if option == 'channel_select'
                                 else f'the {_FUSED_ENTRIES[option][2]} call stands alone')
        if option == 'channel_select':
            value = value.struct(self.ctx, self.D)
        _enqueue_fused(self.ctx, self.params, self.obs_d, self.D, self.N, self.act_d, self.K,
                       self.N_act, target_index, start_context, end_context, self.out_d, taps,
                       self.pcm, option, value)

    def enqueue_targets(self, target_indices, start_contexts, end_contexts, out_d, taps=None):
        """gss_enhance_observation_targets: len(target_indices) rows of n_out samples into
        ``out_d``; the contexts are one per target."""
        ctx = self.ctx
        targets = np.ascontiguousarray(target_indices, dtype=np.int32)
        starts = np.ascontiguousarray(start_contexts, dtype=np.int64)
        ends = np.ascontiguousarray(end_contexts, dtype=np.int64)
        assert starts.shape == ends.shape == targets.shape
        assert out_d.nbytes >= 8 * len(targets) * self.n_out
        entry = (ctx.lib.gss_enhance_observation_targets_pcm16 if self.pcm
                 else ctx.lib.gss_enhance_observation_targets)
        ctx._check(entry(
            ctx.handle, ctypes.byref(self.params), c_void_p(self.obs_d.ptr), self.D, self.N,
            c_void_p(self.act_d.ptr), self.K, self.N_act, len(targets),
            targets.ctypes.data_as(c_void_p), starts.ctypes.data_as(c_void_p),
            ends.ctypes.data_as(c_void_p), c_void_p(out_d.ptr),
            ctypes.byref(taps) if taps is not None else None), 'gss_enhance_observation_targets')

    def result(self):
        x_hat = self.ctx.to_host(self.out_d, (self.n_out,), np.float64)
        if self.params.bf in (_BF_CODES['mvdrSouden_ban'], _BF_CODES['gev_ban']):
            _check_ref_channel(self.ctx)
        return x_hat


class HostStaging:
    """One utterance's inputs in page-locked host memory: ``obs`` (D, N) int16 PCM followed by
    ``act`` (K, N_act) uint8, in one block (grow-only).  Loader threads fill the rows (WAV
    slices by preadv, activity tracks by slice_into), the feeder hands the set to
    `UtterancePipeline.enqueue_staged`, which starts two DMAs from it."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.block = None
        self.obs = self.act = None
        self._retired = []

    def shape(self, D, N, K, N_act):
        off = (2 * D * N + 255) // 256 * 256
        need = off + K * N_act
        if self.block is None or self.block.nbytes < need:
            # hipHostFree waits for the whole device (every stream of every utterance in
            # flight): an outgrown block is parked until free(), and blocks at least double, so
            # a session parks a handful of them
            have = 0
            if self.block is not None:
                self._retired.append(self.block)
                have = self.block.nbytes
            self.block = self.ctx.pinned(max(int(need * 1.25) + 4096, 2 * have))
        self.obs = self.block.view((D, N), np.int16, 0)
        self.act = self.block.view((K, N_act), np.uint8, off)
        return self.obs, self.act

    def free(self):
        self.obs = self.act = None
        for block in self._retired + ([self.block] if self.block is not None else []):
            block.free()
        self.block, self._retired = None, []


class UtterancePipeline:
    """Keeps up to ``depth`` utterances in flight on one GPU, each on its own context
    (HIP stream + workspace), so that one utterance's latency-bound kernels overlap the
    other's MFMA / VALU-bound ones and host work (audio I/O, H2D, D2H, writing) overlaps
    device work -- SURVEY.md section 8e "keep >= 2 utterances in flight per GPU".

        pipe = UtterancePipeline(params, depth=2)
        for ex in examples:
            prepared = load(ex)                       # host work first ...
            if pipe.full():
                tag, x_hat = pipe.pop()               # ... then wait for the oldest
            pipe.enqueue(ex, *prepared)
        while len(pipe): tag, x_hat = pipe.pop()

    Device buffers are per slot and grow-only (no hipMalloc / hipFree between
    utterances: hipFree synchronises the whole device)."""

    def __init__(self, params, depth=2, device_id=None, window=None, first_ctx=None,
                 staging_sets=0):
        from collections import deque
        import queue
        assert depth >= 1
        first = first_ctx or default_context(device_id)
        self.params = params
        self.slots = [first] + [Context(first.device_id) for _ in range(depth - 1)]
        for c in self.slots:
            _prepare_windows(c, params.stft_size, params.stft_shift, window)
            # (with utterances in flight beside each other a call stays on its own stream)
            c.set_utterances_in_flight(depth)
        self._bufs = [dict() for _ in self.slots]
        self._pending = deque()
        self._next = 0
        self.dropped = []       # tags close() drained without handing out their result
        # page-locked input sets for enqueue_staged (acquire_staging blocks until one is free;
        # a set is free again once its utterance was popped)
        self._staging = queue.Queue()
        self._all_staging = [HostStaging(first) for _ in range(staging_sets)]
        for st in self._all_staging:
            self._staging.put(st)
        self._out_host = [None for _ in self.slots]
        self._out_retired = []

    def __len__(self):
        return len(self._pending)

    def full(self):
        return len(self._pending) == len(self.slots)

    def _buffer(self, slot, name, nbytes):
        buf = self._bufs[slot].get(name)
        if buf is None or buf.nbytes < nbytes:
            buf = self._bufs[slot][name] = self.slots[slot].empty(max(int(nbytes * 1.25), 16))
        return buf

    def _next_slot(self, obs, act, wpe_arrays, select=False):
        """The set-up both enqueue calls share, for inputs ``obs`` (D,N) and ``act`` (K,N_act):
        the utterance's params (checked against a selection with ``select``), the next slot and
        its context, the length of the result and the slot's grow-only device buffers."""
        p = params_for(self.params, obs.shape[0], wpe_arrays)
        if select:
            _check_select_params(p, 'channel selection')
        slot = self._next
        self._next = (self._next + 1) % len(self.slots)
        ctx = self.slots[slot]
        T = stft_frames(obs.shape[1], p.stft_size, p.stft_shift, p.stft_fading)
        n_out = int(ctx.lib.gss_istft_num_samples(T, p.stft_size, p.stft_shift, p.stft_fading))
        return SimpleNamespace(
            slot=slot, ctx=ctx, params=p, n_out=n_out,
            obs_d=self._buffer(slot, 'obs', obs.nbytes),
            act_d=self._buffer(slot, 'act', act.nbytes),
            out_d=self._buffer(slot, 'out', 8 * max(n_out, 1)))

    def enqueue(self, tag, obs, activity, target_index, start_context, end_context,
                wpe_arrays=None):
        """``wpe_arrays``: microphone arrays of this utterance for a per-array WPE (None: as
        the pipeline's params say)."""
        assert not self.full(), 'pop() the oldest utterance first'
        # int16 = PCM straight from the WAV files: converted on the device
        pcm = np.asarray(obs).dtype == np.int16
        obs = np.ascontiguousarray(obs, dtype=np.int16 if pcm else np.float64)
        act = np.ascontiguousarray((np.asarray(activity) != 0).astype(np.uint8))
        s = self._next_slot(obs, act, wpe_arrays)
        s.ctx.upload(s.obs_d, obs)
        s.ctx.upload(s.act_d, act)
        _enqueue_fused(s.ctx, s.params, s.obs_d, *obs.shape, s.act_d, *act.shape, target_index,
                       start_context, end_context, s.out_d, pcm=pcm)
        self._pending.append((tag, s.slot, s.n_out))

    # ---- page-locked staging (the session driver's path) ----------------------------
    def acquire_staging(self, timeout=None):
        """A free HostStaging set; blocks while all are in use (loader threads call this)."""
        return self._staging.get(timeout=timeout)

    def release_staging(self, staging):
        self._staging.put(staging)

    def enqueue_staged(self, tag, staging, target_index, start_context, end_context, keep=None,
                       wpe_arrays=None, channel_select=None):
        """Like enqueue() for inputs sitting in a HostStaging set: two asynchronous DMAs, the
        kernels behind them, and an asynchronous D2H of the samples ``keep = (a, b)`` of the
        result (default: all) into page-locked memory -- the host thread does not wait for any
        of it.  The set goes back to the free list when the utterance is popped.
        ``channel_select``: a `ChannelSelect`; the utterance takes
        gss_enhance_observation_select_pcm16, still without any wait."""
        assert not self.full(), 'pop() the oldest utterance first'
        obs, act = staging.obs, staging.act
        s = self._next_slot(obs, act, wpe_arrays, select=channel_select is not None)
        slot, ctx, n_out = s.slot, s.ctx, s.n_out
        a, b = (0, n_out) if keep is None else (min(max(int(keep[0]), 0), n_out),
                                                 min(max(int(keep[1]), 0), n_out))
        b = max(a, b)
        out_h = self._out_host[slot]
        if out_h is None or out_h.nbytes < 8 * (b - a):
            have = 0
            if out_h is not None:            # parked until close(), see HostStaging.shape
                self._out_retired.append(out_h)
                have = out_h.nbytes
            out_h = self._out_host[slot] = ctx.pinned(
                max(int(8 * (b - a) * 1.25) + 4096, 2 * have))
        out_view = out_h.view((b - a,), np.float64)
        # (the band table of a selection is copied to the slot's GPU once, on its first use)
        st = channel_select.struct(ctx, obs.shape[0]) if channel_select is not None else None
        ctx.upload_async(s.obs_d, obs)
        ctx.upload_async(s.act_d, act)
        _enqueue_fused(ctx, s.params, s.obs_d, *obs.shape, s.act_d, *act.shape, target_index,
                       start_context, end_context, s.out_d, pcm=True,
                       option='channel_select' if st is not None else None, value=st)
        if b > a:
            ctx.download_async(out_view, s.out_d, offset=8 * a)
        self._pending.append((tag, slot, n_out, staging, out_view))

    def pop(self):
        entry = self._pending.popleft()
        tag, slot, n_out = entry[:3]
        if len(entry) == 5:
            staging, out_view = entry[3:]
            try:
                self.slots[slot].synchronize()
                x_hat = out_view.copy()      # the slot's pinned block is reused by the next one
            finally:
                self.release_staging(staging)
        else:
            x_hat = self.slots[slot].to_host(self._bufs[slot]['out'], (n_out,), np.float64)
        if self.params.bf in (_BF_CODES['mvdrSouden_ban'], _BF_CODES['gev_ban']):
            # what the reference raises for this utterance (raised explicitly: an `assert`
            # statement disappears under python -O and NaN audio would be written silently);
            # `tag` may be a whole example dict: name it by its id.
            name = tag.get('example_id', '?') if isinstance(tag, dict) else tag
            _raise_for_ref_channel(self.slots[slot].last_ref_channel(), name)
        return tag, x_hat

    def close(self):
        """Drain what is still in flight WITHOUT the status check (close() runs in `finally`
        blocks: a second exception here would mask the first one and leak the extra
        contexts), then release buffers and contexts.  Consequence for a caller that enqueues
        and closes without pop(): the AssertionError / LinAlgError the reference would raise
        for those utterances (non-finite SNR, indefinite noise PSD) is NOT raised -- their
        results are discarded unseen.  pop() every utterance whose outcome matters
        (`Enhancer._enhance_and_write` does); `self.dropped` lists the tags close() drained."""
        try:
            while self._pending:
                tag, slot = self._pending.popleft()[:2]
                self.dropped.append(tag)
                try:
                    self.slots[slot].synchronize()
                except Exception:
                    pass
        finally:
            self._bufs = [dict() for _ in self.slots]
            for block in (self._all_staging + self._out_retired
                          + [h for h in self._out_host if h is not None]):
                try:
                    block.free()
                except Exception:
                    pass
            self._all_staging, self._out_host = [], [None for _ in self.slots]
            self._out_retired = []
            for c in self.slots[1:]:
                try:
                    c.close()
                except Exception:
                    pass
            self.slots = self.slots[:1]
            try:        # the first slot is the caller's context: nothing said again
                self.slots[0].set_utterances_in_flight(0)
            except Exception:
                pass


def _resident_call(obs, activity, params, wpe_arrays, window, debug, ctx):
    """The head that the one-target wrappers on a time-domain activity share once their own
    arguments are checked: (context, the utterance in HBM, tap buffers, taps); the last two
    empty without ``debug``."""
    params = params_for(params, np.shape(obs)[0], wpe_arrays)
    ctx = ctx or default_context()
    _prepare_windows(ctx, params.stft_size, params.stft_shift, window)
    utt = ResidentUtterance(ctx, obs, activity, params)
    bufs, taps = _debug_taps(utt) if debug else ({}, None)
    return ctx, utt, bufs, taps


def _fused_params(params, param_kwargs):
    """``params`` of a fused wrapper: as given, or (None) made from its loose keywords."""
    return make_params(**param_kwargs) if params is None else params


def _obs_dn(obs):
    obs = np.asarray(obs)
    if obs.ndim != 2:
        raise ValueError(f'obs: shape {obs.shape} is not (D,N)')
    return obs


def _check_fused_wpe_online(params, alpha, num_channels, wpe_arrays):
    """An online WPE inside a fused call, before any device work: it replaces a WPE stage that
    runs, has no PSD context, and its settings are `check_wpe_online`'s."""
    if not params.wpe:
        raise ValueError('wpe_online with wpe=False: there is no WPE stage to replace')
    if params.wpe_psd_context != 0:
        raise ValueError(f'wpe_online with wpe_psd_context={params.wpe_psd_context}: the online '
                         'WPE has no PSD context')
    check_wpe_online(params.wpe_taps, params.wpe_delay, alpha, num_channels,
                     params.wpe_arrays if wpe_arrays is None else wpe_arrays)


def _fused_one_target(call, params, wpe_arrays, window, debug, ctx, option=None, extras=None):
    """The tail that the one-target wrappers on a time-domain activity share once their own
    arguments are checked.  ``call``: (obs, activity, target_index, start_context_samples,
    end_context_samples); ``option``: the one keyword of `ResidentUtterance.enqueue` the wrapper
    adds (None: the plain call); ``extras(ctx, details)``: what it adds to the ``debug`` details."""
    obs, activity, *target_and_contexts = call
    ctx, utt, bufs, taps = _resident_call(obs, activity, params, wpe_arrays, window, debug, ctx)
    utt.enqueue(*target_and_contexts, taps, **(option or {}))
    x_hat, details = _one_target_result(utt, bufs, debug)
    if not debug:
        return x_hat
    if extras is not None:
        extras(ctx, details)
    return x_hat, details


def _require_souden(params, setting, form):
    """What only bf='mvdrSouden_ban' combines with, before any device work."""
    if params.bf != _BF_CODES['mvdrSouden_ban']:
        names = {v: k for k, v in _BF_CODES.items()}
        raise NotImplementedError(f"bf={names[params.bf]!r} with {setting}: only "
                                  f"'mvdrSouden_ban' has {form}")


def enhance_observation(obs, activity, target_index, start_context_samples,
                        end_context_samples, *, params=None, window=None, debug=False,
                        ctx=None, wpe_arrays=None, **param_kwargs):
    """Fused per-utterance pipeline (core.py:514-571), intermediates resident in HBM.

    obs (D,N) float64, activity (K,N) bool in dict order.  Returns x_hat, or
    (x_hat, details) with ``debug=True`` where details holds the reference's
    debug locals in the reference's layouts.  ``wpe_arrays`` = A > 1: WPE per microphone
    array (A arrays of D / A channels, array-major) instead of one joint WPE."""
    params = _fused_params(params, param_kwargs)
    return _fused_one_target(
        (obs, activity, target_index, start_context_samples, end_context_samples), params,
        wpe_arrays, window, debug, ctx)


def enhance_observation_segments(obs, activity, target_index, start_context_samples,
                                 end_context_samples, *, segment_frames, segment_context=0,
                                 min_mass=None, params=None, window=None, debug=False, ctx=None,
                                 wpe_arrays=None, **param_kwargs):
    """`enhance_observation` with the segment-wise beamformer of
    `mvdr_souden_segments_from_masks` (gss_enhance_observation_segments) in the place of the
    whole-window one; everything else, the ``debug`` details included, as there, plus
    ``details['segment_fallbacks']``.  Only ``bf='mvdrSouden_ban'`` has segments
    (NotImplementedError otherwise); bad segment settings are ValueError, both before any
    device work."""
    params = _fused_params(params, param_kwargs)
    _require_souden(params, 'segment_frames', 'a segment-wise form')
    obs = _obs_dn(obs)
    seg = check_bf_segments(segment_frames, segment_context, min_mass, obs.shape[0])
    return _fused_one_target(
        (obs, activity, target_index, start_context_samples, end_context_samples), params,
        wpe_arrays, window, debug, ctx, dict(segments=seg),
        lambda ctx, details: details.update(segment_fallbacks=ctx.last_segment_fallbacks()))


def enhance_observation_lcmv(obs, activity, target_index, start_context_samples,
                             end_context_samples, *, interferer=None, candidates=None,
                             min_mass=None, params=None, window=None, debug=False, ctx=None,
                             wpe_arrays=None, **param_kwargs):
    """`enhance_observation` with the interferer-nulling LCMV of `lcmv_souden_from_masks`
    (gss_enhance_observation_lcmv) in the place of the MVDR: the interferer is ``interferer`` or
    the class among ``candidates`` (None: every class but the target) with the most posterior
    mass; frequencies where its mask sums to less than ``min_mass`` (None: 2 * channels) take
    the MVDR.  ``debug`` details as there -- ``distortion_mask`` is I + N -- plus
    ``interferer`` (-1: none), ``interferer_mask`` (T,F) and ``lcmv_fallbacks``.  Only
    ``bf='mvdrSouden_ban'`` has it (NotImplementedError otherwise); bad settings are
    ValueError, both before any device work."""
    params = _fused_params(params, param_kwargs)
    _require_souden(params, 'null_interferer', 'an interferer-nulling form')
    obs = _obs_dn(obs)
    _check_lcmv_channels(obs.shape[0])
    K = np.shape(activity)[0]
    bf = check_bf_lcmv(K, target_index, interferer, candidates, min_mass, obs.shape[0])

    def extras(ctx, details):
        found = details['interferer'] = ctx.last_lcmv_interferer()
        details['lcmv_fallbacks'] = ctx.last_lcmv_fallbacks()
        # the interferer's posterior with the context frames zeroed: the bits the call used
        mask = np.zeros_like(details['target_mask'])
        if found >= 0:
            mask[...] = details['posterior'][found]
            if params.bf_drop_context:
                sf, ef = (samples_to_stft_frames(c, params.stft_size, params.stft_shift,
                                                 fading=params.stft_fading)
                          for c in (start_context_samples, end_context_samples))
                mask[:sf] = 0
                if ef > 0:
                    mask[-ef:] = 0
        details['interferer_mask'] = mask
    return _fused_one_target(
        (obs, activity, target_index, start_context_samples, end_context_samples), params,
        wpe_arrays, window, debug, ctx, dict(lcmv=bf), extras)


def enhance_observation_wpd(obs, activity, target_index, start_context_samples,
                            end_context_samples, *, taps=None, delay=None, iterations=1,
                            power_floor=WPD_POWER_FLOOR, ban=True, params=None, window=None,
                            debug=False, ctx=None, wpe_arrays=None, **param_kwargs):
    """`enhance_observation` with the WPD beamformer of `wpd_souden_from_masks`
    (gss_enhance_observation_wpd) in the place of the MVDR: the beamformer works on the STFT
    BEFORE WPE with the target mask of the mixture model, which still sees the WPE output; the
    context frames that ``bf_drop_context`` zeroes are gated out of its statistics.  ``taps`` /
    ``delay`` None: those of the WPE block.  ``debug`` details as there (``Obs`` is the input of
    the mixture model) plus ``wpd_zero_pivots``.  ``params.bf`` must be 'mvdrSouden_ban' (its
    code selects the Souden solve; ``ban`` decides the normalisation): NotImplementedError
    otherwise; bad settings are ValueError, both before any device work."""
    params = _fused_params(params, param_kwargs)
    _require_souden(params, 'the WPD beamformer', 'a WPD form')
    obs = _obs_dn(obs)
    bf = check_bf_wpd(params.wpe_taps if taps is None else taps,
                      params.wpe_delay if delay is None else delay, iterations, power_floor, ban,
                      obs.shape[0])
    return _fused_one_target(
        (obs, activity, target_index, start_context_samples, end_context_samples), params,
        wpe_arrays, window, debug, ctx, dict(wpd=bf),
        lambda ctx, details: details.update(wpd_zero_pivots=ctx.last_wpd_zero_pivots()))


def enhance_observation_wpe_online(obs, activity, target_index, start_context_samples,
                                   end_context_samples, *, alpha=WPE_ONLINE_ALPHA, params=None,
                                   window=None, debug=False, ctx=None, wpe_arrays=None,
                                   **param_kwargs):
    """`enhance_observation` with the online WPE of `wpe_online_dtf` from a fresh state
    (gss_enhance_observation_wpe_online) in the place of the offline one: taps, delay and the
    arrays are those of ``params``, its ``wpe_iterations`` is not read.  ``debug`` details as
    there (``Obs`` is the output of the online WPE).  ValueError for bad settings, ``wpe=False``
    or a PSD context, before any device work."""
    params = _fused_params(params, param_kwargs)
    obs = _obs_dn(obs)
    _check_fused_wpe_online(params, alpha, obs.shape[0], wpe_arrays)
    return _fused_one_target(
        (obs, activity, target_index, start_context_samples, end_context_samples), params,
        wpe_arrays, window, debug, ctx, dict(wpe_online=GssWpeOnlineCfg(alpha=float(alpha))))


def enhance_observation_bf_online(obs, activity, target_index, start_context_samples,
                                  end_context_samples, *, forget=BF_ONLINE_FORGET,
                                  loading=BF_ONLINE_LOADING, ref_channel=-1, wpe_online=False,
                                  wpe_alpha=WPE_ONLINE_ALPHA, params=None, window=None,
                                  debug=False, ctx=None, wpe_arrays=None, **param_kwargs):
    """`enhance_observation` with the online MVDR of `mvdr_souden_online_from_masks` (BAN on, a
    fresh state initialised from the window; gss_enhance_observation_bf_online) in the place of
    the whole-window one.  ``ref_channel`` = -1: the window's.  ``wpe_online``: the online WPE
    with ``wpe_alpha`` in the place of the offline one as well, as
    `enhance_observation_wpe_online`.  ``debug`` details as there plus ``bf_online_fallbacks``.
    Only ``bf='mvdrSouden_ban'`` has it (NotImplementedError otherwise); bad settings are
    ValueError, both before any device work."""
    params = _fused_params(params, param_kwargs)
    _require_souden(params, 'bf_online', 'an online form')
    obs = _obs_dn(obs)
    forget, loading, ref_channel = check_bf_online(forget, loading, ref_channel, obs.shape[0])
    if wpe_online:
        _check_fused_wpe_online(params, wpe_alpha, obs.shape[0], wpe_arrays)
    elif wpe_alpha != WPE_ONLINE_ALPHA:
        raise ValueError(f'wpe_alpha={wpe_alpha!r} without wpe_online: nobody reads it')
    bf = _bf_online_cfg(forget, loading, ref_channel, wpe_online, wpe_alpha)
    return _fused_one_target(
        (obs, activity, target_index, start_context_samples, end_context_samples), params,
        wpe_arrays, window, debug, ctx, dict(bf_online=bf),
        lambda ctx, details: details.update(bf_online_fallbacks=ctx.last_mvdr_online_fallbacks()))


def enhance_observation_gss_online(obs, activity, target_index, start_context_samples,
                                   end_context_samples, *, forget=GSS_ONLINE_FORGET,
                                   prior_mass=GSS_ONLINE_PRIOR_MASS, bf_online=False,
                                   bf_forget=BF_ONLINE_FORGET, bf_loading=BF_ONLINE_LOADING,
                                   ref_channel=-1, wpe_online=False, wpe_alpha=WPE_ONLINE_ALPHA,
                                   params=None, window=None, debug=False, ctx=None,
                                   wpe_arrays=None, **param_kwargs):
    """`enhance_observation` with the online CACGMM of `cacgmm_posteriors_online` (a fresh state
    of ``prior_mass`` per call, masked by the call's frame activity;
    gss_enhance_observation_gss_online) in the place of the guided EM; ``bss_iterations`` and
    ``bss_iterations_post`` are not read.  ``bf_online``: the online MVDR follows as in
    `enhance_observation_bf_online` (``bf_forget``, ``bf_loading``, ``ref_channel``), and with
    ``wpe_online`` the online WPE precedes: the whole zero-look-ahead chain in one call.
    ``debug`` details as there plus ``gss_online_fallbacks`` (and ``bf_online_fallbacks``).
    Bad settings are ValueError before any device work."""
    params = _fused_params(params, param_kwargs)
    obs = _obs_dn(obs)
    forget, prior_mass = check_gss_online(forget, prior_mass, np.shape(activity)[0], obs.shape[0])
    em = GssEmOnline(forget=forget, prior_mass=prior_mass)
    bf = None
    if bf_online:
        _require_souden(params, 'bf_online', 'an online form')
        bf_forget, bf_loading, ref_channel = check_bf_online(bf_forget, bf_loading, ref_channel,
                                                             obs.shape[0])
        if wpe_online:
            _check_fused_wpe_online(params, wpe_alpha, obs.shape[0], wpe_arrays)
        bf = _bf_online_cfg(bf_forget, bf_loading, ref_channel, wpe_online, wpe_alpha)
    elif wpe_online:
        raise ValueError('wpe_online without bf_online inside the gss_online call: the online WPE '
                         'rides on the online MVDR\'s descriptor')

    def extras(ctx, details):
        if bf is not None:
            details['bf_online_fallbacks'] = ctx.last_mvdr_online_fallbacks()
        details['gss_online_fallbacks'] = ctx.last_cacgmm_online_fallbacks()
    return _fused_one_target(
        (obs, activity, target_index, start_context_samples, end_context_samples), params,
        wpe_arrays, window, debug, ctx, dict(gss_online=(em, bf)), extras)


class GuidedUtterance:
    """`ResidentUtterance` of a guided call: observation and per-frame guidance in HBM."""

    def __init__(self, ctx, obs, initialization, source_activity_mask, params, wpe_arrays=None):
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        if obs.ndim != 2:
            raise ValueError(f'obs: shape {obs.shape} is not (D,N)')
        self.ctx = ctx
        self.D, self.N = obs.shape
        self.params = params = params_for(params, self.D, wpe_arrays)
        self.T = stft_frames(self.N, params.stft_size, params.stft_shift, params.stft_fading)
        init, mask, self.K = guidance_tables(initialization, source_activity_mask, self.T,
                                             params.stft_size // 2 + 1)
        self.n_out = int(ctx.lib.gss_istft_num_samples(
            self.T, params.stft_size, params.stft_shift, params.stft_fading))
        self.obs_d = ctx.to_device(obs)
        self.guide = DeviceGuidance(ctx, init, mask, self.T)
        self.out_d = ctx.empty(8 * max(self.n_out, 1))

    def enqueue(self, target_index, start_context, end_context, taps=None):
        ctx = self.ctx
        ctx._check(ctx.lib.gss_enhance_observation_guided(
            ctx.handle, ctypes.byref(self.params), c_void_p(self.obs_d.ptr), self.D, self.N,
            ctypes.byref(self.guide.struct), self.K, int(target_index), int(start_context),
            int(end_context), c_void_p(self.out_d.ptr),
            ctypes.byref(taps) if taps is not None else None),
            'gss_enhance_observation_guided')

    result = ResidentUtterance.result


def enhance_observation_guided(obs, initialization, source_activity_mask, target_index,
                               start_context_samples, end_context_samples, *, params=None,
                               window=None, debug=False, ctx=None, wpe_arrays=None,
                               **param_kwargs):
    """`enhance_observation` guided per STFT frame (gss_enhance_observation_guided): the tables
    of `cacgmm_posteriors_guided`, (K,T) or (K,T,F) over the T frames of the observation's
    STFT, take the place of the time-domain activity.  Everything else -- STFT, WPE,
    beamformer, postfilter, iSTFT, ``debug`` details (without ``acitivity_freq``) -- as
    there."""
    params = _fused_params(params, param_kwargs)
    params = params_for(params, np.shape(obs)[0], wpe_arrays)
    ctx = ctx or default_context()
    _prepare_windows(ctx, params.stft_size, params.stft_shift, window)
    utt = GuidedUtterance(ctx, obs, initialization, source_activity_mask, params)
    bufs, taps = _debug_taps(utt) if debug else ({}, None)
    if debug:
        del bufs['act_frames']
        taps.act_frames = None
    utt.enqueue(target_index, start_context_samples, end_context_samples, taps)
    x_hat, details = _one_target_result(utt, bufs, debug)
    if not debug:
        return x_hat
    return x_hat, details


_PER_TARGET = ('target_mask', 'distortion_mask', 'X_hat', 'ref_channel')


def _one_target_result(utt, bufs, debug, D=None):
    """The tail the one-target wrappers share: (x_hat, None), or with ``debug`` (x_hat, details)
    with the per-target entries of `_debug_details` squeezed and ``ref_channel`` an int."""
    x_hat = utt.result()
    if not debug:
        return x_hat, None
    details = _debug_details(utt, bufs, D=D)
    details.update({k: v[0] for k, v in details.items() if k in _PER_TARGET})
    details['ref_channel'] = int(details['ref_channel'])
    return x_hat, details


def _debug_taps(utt, S=1, D=None):
    """Device buffers for the debug taps of a call on ``utt`` with S targets (per-target taps
    S blocks), the reference channels preset to -1.  ``D``: the channels of the ``Obs_ftd`` tap
    when a selection kept fewer than the utterance has."""
    ctx, D, K, T = utt.ctx, utt.D if D is None else D, utt.K, utt.T
    F = utt.params.stft_size // 2 + 1
    bufs = {
        'Obs_ftd': ctx.empty(16 * F * T * D), 'act_frames': ctx.empty(max(K * T, 16)),
        'gamma': ctx.empty(8 * F * K * T), 'target_mask': ctx.empty(8 * S * F * T),
        'distortion_mask': ctx.empty(8 * S * F * T), 'Xhat': ctx.empty(16 * S * F * T),
        'ref_channel': ctx.empty(max(4 * S, 16)),
    }
    ctx._check(ctx.lib.gss_memset(ctx.handle, c_void_p(bufs['ref_channel'].ptr), 0xFF,
                                  bufs['ref_channel'].nbytes), 'gss_memset')
    return bufs, GssDebugTaps(**{k: v.ptr for k, v in bufs.items()})


def _debug_details(utt, bufs, S=1, D=None):
    """The taps in the reference's layouts; the per-target ones stacked over S."""
    ctx, D, K, T = utt.ctx, utt.D if D is None else D, utt.K, utt.T
    F = utt.params.stft_size // 2 + 1
    details = {}
    if 'act_frames' in bufs:     # (a guided call has no frame activity)
        details['acitivity_freq'] = ctx.to_host(bufs['act_frames'], (K, T), np.uint8).astype(bool)
    return {
        'Obs': _ftd_to_host_dtf(ctx, bufs['Obs_ftd'], D, T, F),
        **details,
        'posterior': ctx.to_host(bufs['gamma'], (F, K, T), np.float64).transpose(1, 2, 0),
        'target_mask': ctx.to_host(bufs['target_mask'], (S, F, T), np.float64).transpose(0, 2, 1),
        'distortion_mask': ctx.to_host(bufs['distortion_mask'], (S, F, T),
                                       np.float64).transpose(0, 2, 1),
        'X_hat': ctx.to_host(bufs['Xhat'], (S, T, F), np.complex128),
        'ref_channel': ctx.to_host(bufs['ref_channel'], (S,), np.int32).astype(int),
    }


def target_contexts(contexts, S, what='context samples'):
    """A context (samples) for each of S targets: an int for all of them, or a length-S
    sequence."""
    if isinstance(contexts, (int, np.integer)) and not isinstance(contexts, bool):
        return [int(contexts)] * S
    values = [int(c) for c in contexts]
    if len(values) != S:
        raise ValueError(f'{what}: {len(values)} values for {S} targets')
    return values


def enhance_observation_targets(obs, activity, target_indices, start_context_samples,
                                end_context_samples, *, params=None, window=None, debug=False,
                                ctx=None, wpe_arrays=None, target_names=None, **param_kwargs):
    """S targets of one window from ONE separation (gss_enhance_observation_targets): STFT, WPE
    and the guided CACGMM run once, the target-dependent tail once for all S targets.

    obs (D,N) float64 (or int16 PCM, scaled by 2^-15 on the device), activity (K,N) bool in
    dict order, target_indices S distinct class indices; the contexts are ints (the same for
    every target) or length-S sequences.  Returns x_hat (S, N'), row s bit for bit what
    `enhance_observation` returns for target_indices[s] and its contexts; with ``debug=True``
    (x_hat, details) where the per-target entries are stacked: ``target_mask`` /
    ``distortion_mask`` / ``X_hat`` (S,T,F), ``ref_channel`` (S,).  A failing target raises
    what the one-target call raises, for the first such target in target order
    (``target_names[s]`` names it in the message)."""
    params = _fused_params(params, param_kwargs)
    params = params_for(params, np.shape(obs)[0], wpe_arrays)
    targets = [int(t) for t in target_indices]
    S = len(targets)
    starts = target_contexts(start_context_samples, S)
    ends = target_contexts(end_context_samples, S)
    if target_names is None:
        target_names = [f'target {t}' for t in targets]
    ctx = ctx or default_context()
    _prepare_windows(ctx, params.stft_size, params.stft_shift, window)
    utt = ResidentUtterance(ctx, obs, activity, params, pcm=np.asarray(obs).dtype == np.int16)
    out_d = ctx.empty(8 * max(S * utt.n_out, 1))
    bufs, taps = _debug_taps(utt, S) if debug else ({}, None)
    utt.enqueue_targets(targets, starts, ends, out_d, taps)
    x_hat = ctx.to_host(out_d, (S, utt.n_out), np.float64)
    if params.bf in (_BF_CODES['mvdrSouden_ban'], _BF_CODES['gev_ban']):
        for ref, name in zip(ctx.last_ref_channels(S), target_names):
            _raise_for_ref_channel(ref, name)
    if not debug:
        return x_hat
    return x_hat, _debug_details(utt, bufs, S)


# --------------------------------------------------------------------------
# annotation-free separation of one window in one call (gss_separate_observation)
# --------------------------------------------------------------------------
def check_separate_args(obs, initialization, params):
    """obs (D,N) real, initialization (K,T) with T the STFT frames of N samples -> (obs float64,
    initialization float64, D, N, K, T); ValueError before any device work."""
    obs = np.asarray(obs)
    if obs.ndim != 2 or obs.dtype.kind not in 'fiu':
        raise ValueError(f'obs: shape {obs.shape}, dtype {obs.dtype} is not a real (D,N) array')
    D, N = obs.shape
    if not 2 <= D <= _MAX_CHANNELS:
        raise ValueError(f'obs: {D} channels outside [2, {_MAX_CHANNELS}]')
    if N < 1:
        raise ValueError('obs: no samples')
    init = np.asarray(initialization)
    if init.ndim != 2 or init.dtype.kind not in 'fiu':
        raise ValueError(f'initialization: shape {init.shape}, dtype {init.dtype} is not a real '
                         '(K,T) table')
    K = init.shape[0]
    if not 1 <= K <= _MAX_CLASSES:
        raise ValueError(f'{K} classes outside [1, {_MAX_CLASSES}]')
    T = stft_frames(N, params.stft_size, params.stft_shift, params.stft_fading)
    if init.shape[1] != T:
        raise ValueError(f'initialization: {init.shape[1]} frames, the observation has {T}')
    return (np.ascontiguousarray(obs, dtype=np.float64),
            np.ascontiguousarray(init, dtype=np.float64), D, N, K, T)


class ResidentSeparation:
    """One window of `gss_separate_observation` whose inputs sit in HBM: obs (D,N),
    initialization (K,T).  ``gamma_d``: a device buffer of at least 8 F K T bytes that receives
    the posteriors in the device layout (F,K,T) (None: one of the call's own)."""

    def __init__(self, ctx, obs, initialization, params, gamma_d=None):
        obs, init, self.D, self.N, self.K, self.T = check_separate_args(obs, initialization,
                                                                        params)
        self.ctx, self.params = ctx, params
        self.F = params.stft_size // 2 + 1
        self.n_out = int(ctx.lib.gss_istft_num_samples(
            self.T, params.stft_size, params.stft_shift, params.stft_fading))
        self.obs_d = ctx.to_device(obs)
        self.init_d = ctx.to_device(init)
        self.out_d = ctx.empty(8 * max(self.K * self.n_out, 1))
        self.prior_d = ctx.empty(8 * self.K * self.T)
        self.power_d = ctx.empty(max(8 * self.T, 16))
        self.gamma_d = gamma_d if gamma_d is not None else ctx.empty(8 * self.F * self.K * self.T)
        assert self.gamma_d.nbytes >= 8 * self.F * self.K * self.T

    def enqueue(self, taps=None):
        ctx = self.ctx
        ctx._check(ctx.lib.gss_separate_observation(
            ctx.handle, ctypes.byref(self.params), c_void_p(self.obs_d.ptr), self.D, self.N,
            c_void_p(self.init_d.ptr), self.K, c_void_p(self.out_d.ptr),
            c_void_p(self.prior_d.ptr), c_void_p(self.power_d.ptr), c_void_p(self.gamma_d.ptr),
            ctypes.byref(taps) if taps is not None else None), 'gss_separate_observation')

    def result(self):
        """(x_hat (K,N'), prior (K,T), power (T,)) on the host; a class whose beamformer failed
        raises what `enhance_observation` raises, naming the class."""
        ctx = self.ctx
        x_hat = ctx.to_host(self.out_d, (self.K, self.n_out), np.float64)
        prior = ctx.to_host(self.prior_d, (self.K, self.T), np.float64)
        power = ctx.to_host(self.power_d, (self.T,), np.float64)
        if self.params.bf in (_BF_CODES['mvdrSouden_ban'], _BF_CODES['gev_ban']):
            for k, ref in enumerate(ctx.last_ref_channels(self.K)):
                _raise_for_ref_channel(ref, f'class {k}')
        return x_hat, prior, power

    def posterior(self):
        """The posteriors as the host has them elsewhere: (K,T,F)."""
        g = self.ctx.to_host(self.gamma_d, (self.F, self.K, self.T), np.float64)
        return np.ascontiguousarray(g.transpose(1, 2, 0))


def separate_observation(obs, initialization, *, params=None, window=None, debug=False,
                         return_posterior=False, ctx=None, **param_kwargs):
    """Annotation-free separation of one window in ONE call (`gss_separate_observation`): STFT,
    the joint WPE, the CACGMM with a frequency-shared prior from ``initialization`` (K,T) -- no
    mask, ``bss_iterations`` iterations, one post iteration: `cacgmm_posteriors_blind` with
    ``method='shared_prior'`` from that table --, the frame power of `posterior_activity`, the
    beamformer for every class (target k = class k, no context frames) and K iSTFTs.

    obs (D,N) float64.  Returns (x_hat (K,N'), prior (K,T), power (T,)); with
    ``return_posterior`` also the posteriors (K,T,F); with ``debug=True`` also the details of
    `enhance_observation_targets` (no ``acitivity_freq``: there is no activity).  The per-array
    WPE is NotImplementedError; every argument error is a ValueError before any device work."""
    params = _fused_params(params, param_kwargs)
    check_separate_args(obs, initialization, params)
    ctx = ctx or default_context()
    _prepare_windows(ctx, params.stft_size, params.stft_shift, window)
    win = ResidentSeparation(ctx, obs, initialization, params)
    bufs, taps = ({}, None)
    if debug:
        bufs, taps = _debug_taps(win, win.K)
        del bufs['act_frames']
        taps.act_frames = None
    win.enqueue(taps)
    out = list(win.result())
    if return_posterior:
        out.append(win.posterior())
    if debug:
        out.append(_debug_details(win, bufs, win.K))
    return tuple(out)


# --------------------------------------------------------------------------
# sample-block stream (gss_stream_state; include/gss_hip.h)
# --------------------------------------------------------------------------
def _check_stream_geometry(size, shift):
    for name, value in (('size', size), ('shift', shift)):
        if not _is_integer(value) or value < 1:
            raise ValueError(f'{name}={value!r}: a positive integer')
    if size % shift != 0:
        raise ValueError(f'shift={shift} does not divide size={size}')


def _check_stream_count(value, name):
    if not _is_integer(value) or value < 0:
        raise ValueError(f'{name}={value!r}: a non-negative integer')
    return int(value)


def stream_num_frames(received, n, size, shift):
    """Frames that ``n`` more samples complete after ``received`` samples of a stream:
    floor((received + n) / shift) - floor(received / shift) (gss_stream_num_frames)."""
    _check_stream_geometry(size, shift)
    return int(_capi.load_library().gss_stream_num_frames(
        _check_stream_count(received, 'received'), _check_stream_count(n, 'n'), size, shift))


def stream_num_samples_out(received, n, size, shift):
    """Output samples that ``n`` more samples finish after ``received``: the growth of
    max(0, floor(M / shift) * shift - (size - shift)) (gss_stream_num_samples_out)."""
    _check_stream_geometry(size, shift)
    return int(_capi.load_library().gss_stream_num_samples_out(
        _check_stream_count(received, 'received'), _check_stream_count(n, 'n'), size, shift))


def stream_flush_samples(received, size, shift):
    """Zeros that end a stream of ``received`` samples: afterwards its frames are those of
    `stft` (fading=True) on the whole signal (gss_stream_flush_samples)."""
    _check_stream_geometry(size, shift)
    return int(_capi.load_library().gss_stream_flush_samples(
        _check_stream_count(received, 'received'), size, shift))


def check_stream(num_channels, num_classes, size, shift):
    """The sizes of a stream -- the one place that validates them.  ValueError naming the
    argument: ``num_channels`` an integer in [1, 32], ``num_classes`` an integer in [0, 8] (0: an
    unguided stream, no activity), ``shift`` dividing ``size``.  NotImplementedError:
    ``shift`` == ``size`` (a stream needs overlapping frames), a ``size`` the STFT is not built
    for."""
    if not _is_integer(num_channels) or not 1 <= num_channels <= _MAX_CHANNELS:
        raise ValueError(f'num_channels={num_channels!r}: an integer in [1, {_MAX_CHANNELS}]')
    if not _is_integer(num_classes) or not 0 <= num_classes <= _ONLINE_MAX_CLASSES:
        raise ValueError(f'num_classes={num_classes!r}: an integer in [0, {_ONLINE_MAX_CLASSES}]')
    _check_stream_geometry(size, shift)
    if size % 2 or not 4 <= size <= 4096:
        raise NotImplementedError(f'size={size}: an even length in [4, 4096]')
    if shift == size:
        raise NotImplementedError(f'shift == size == {size}: a stream needs overlapping frames')
    return int(num_channels), int(num_classes), int(size), int(shift)


class StreamState(_OnlineState):
    """The state of the two ends of a sample-block stream in HBM (gss_stream_state), caller-owned
    like an `OnlineWPEState`: ``x_hist`` (D,size) float64, the last samples; ``act_hist`` (K,size)
    uint8, their activity (absent for K = 0, an unguided stream); ``ola_tail`` (size - shift), the
    partial overlap-add sums; and the host counters ``received`` and ``frames_out``."""
    _sizes = 'D, K, size, shift'
    dtypes = {'x_hist': np.float64, 'act_hist': np.uint8, 'ola_tail': np.float64}

    def __init__(self, ctx, D, K, size, shift):
        super().__init__(ctx, D, K, size, shift)
        self.D, self.K, self.size, self.shift = self.key
        self._struct = GssStreamState(
            x_hist=self.bufs['x_hist'].ptr,
            act_hist=self.bufs['act_hist'].ptr if self.K else None,
            ola_tail=self.bufs['ola_tail'].ptr, received=0, frames_out=0, D=self.D, K=self.K,
            size=self.size, shift=self.shift)

    @staticmethod
    def _shapes(D, K, size, shift):
        shapes = {'x_hist': (D, size), 'ola_tail': (size - shift,)}
        if K:
            shapes['act_hist'] = (K, size)
        return shapes

    def struct(self):
        """The ONE struct of this state: the library advances its counters."""
        return self._struct

    received = property(lambda self: int(self._struct.received))
    frames_out = property(lambda self: int(self._struct.frames_out))

    @classmethod
    def fresh(cls, D, K, size=1024, shift=256, *, window=None, ctx=None):
        """Zeros: the leading fading pad, no sample yet (gss_stream_init)."""
        check_stream(D, K, size, shift)
        ctx = ctx or default_context()
        _prepare_windows(ctx, size, shift, window)
        state = cls(ctx, D, K, size, shift)
        ctx._check(ctx.lib.gss_stream_init(ctx.handle, ctypes.byref(state._struct)),
                   'gss_stream_init')
        return state

    def to_host(self):
        """The buffers by name plus 'size', 'shift', 'received' and 'frames_out': everything
        `from_host` needs (synchronises)."""
        return dict(super().to_host(), size=self.size, shift=self.shift, received=self.received,
                    frames_out=self.frames_out)

    @classmethod
    def from_host(cls, host, *, ctx=None):
        """A device state from the dict of `to_host` (in any context).  ValueError for shapes or
        counters that do not fit each other."""
        x = np.asarray(host['x_hist'])
        if x.ndim != 2:
            raise ValueError(f'x_hist: shape {x.shape} is not (D,size)')
        size, shift = int(host['size']), int(host['shift'])
        K = np.asarray(host['act_hist']).shape[0] if 'act_hist' in host else 0
        check_stream(x.shape[0], K, size, shift)
        received = _check_stream_count(host['received'], 'received')
        frames_out = _check_stream_count(host['frames_out'], 'frames_out')
        if frames_out > received // shift:
            raise ValueError(f'frames_out={frames_out} after received={received} samples: at most '
                             f'{received // shift} frames exist')
        state = cls._from_host(host, (x.shape[0], K, size, shift), ctx,
                               lambda shape: f'{shape} (size={size}, shift={shift})')
        state._struct.received, state._struct.frames_out = received, frames_out
        return state


def _stream_block_to_device(ctx, block, activity, state):
    """A block (D,n) float64 / int16 and its activity (K,n) or None against ``state``:
    (x_d, in_type, act_d, n)."""
    block = np.asarray(block)
    if block.ndim != 2 or block.shape[0] != state.D:
        raise ValueError(f'block: shape {block.shape} is not (D,n) = ({state.D},n)')
    pcm = block.dtype == np.int16
    if not pcm:
        block = np.asarray(block, dtype=np.float64)
    n = block.shape[1]
    if (activity is None) != (state.K == 0):
        raise ValueError('activity: missing for a stream that carries one' if activity is None
                         else 'activity: given to an unguided stream (num_classes = 0)')
    act_d = None
    if activity is not None:
        activity = np.asarray(activity)
        if activity.shape != (state.K, n):
            raise ValueError(f'activity: shape {activity.shape} is not (K,n) = ({state.K},{n})')
        act_d = ctx.to_device((activity != 0).astype(np.uint8)) if n else None
    return (ctx.to_device(block) if n else None), int(pcm), act_d, n


def stft_stream(block, activity=None, *, state, window=None):
    """The analysis side of a stream (gss_stft_stream): the next ``block`` (D,n) of samples,
    float64 or int16 PCM, and its ``activity`` (K,n) (None for an unguided stream) -> the frames
    the block completes, (D,Tn,F) complex128, and their frame activity (K,Tn) bool or None.
    ``state``: a `StreamState`, advanced IN PLACE.  Over all blocks the frames have the bits of
    `stft` (fading=True) on the whole signal."""
    if not isinstance(state, StreamState):
        raise ValueError(f'state: {type(state).__name__} is not a StreamState')
    ctx = state.ctx
    x_d, in_type, act_d, n = _stream_block_to_device(ctx, block, activity, state)
    D, K, F = state.D, state.K, state.size // 2 + 1
    Tn = stream_num_frames(state.received, n, state.size, state.shift)
    if n == 0:
        return np.zeros((D, 0, F), np.complex128), (np.zeros((K, 0), bool) if K else None)
    _prepare_windows(ctx, state.size, state.shift, window)
    Y_d = ctx.empty(max(16 * F * Tn * D, 16))
    a_d = ctx.empty(max(K * Tn, 16))
    ctx._check(ctx.lib.gss_stft_stream(
        ctx.handle, c_void_p(x_d.ptr), in_type, c_void_p(act_d.ptr) if act_d else None, n,
        ctypes.byref(state.struct()), c_void_p(Y_d.ptr), c_void_p(a_d.ptr)), 'gss_stft_stream')
    if Tn == 0:
        ctx.synchronize()      # (the block's device copy is read until then)
        return np.zeros((D, 0, F), np.complex128), (np.zeros((K, 0), bool) if K else None)
    Y = _ftd_to_host_dtf(ctx, Y_d, D, Tn, F)
    return Y, (ctx.to_host(a_d, (K, Tn), np.uint8).astype(bool) if K else None)


def _istft_stream_call(stft_signal, state, window, targets=False, tails=None):
    """What `istft_stream` (frames (Tn,F)) and `istft_stream_targets` (``targets``: frames
    (S,Tn,F) and their `StreamTails`) share: the checks, the sample count and the call of the
    entry of either -> (S,m)."""
    if not isinstance(state, StreamState):
        raise ValueError(f'state: {type(state).__name__} is not a StreamState')
    if targets and not isinstance(tails, StreamTails):
        raise ValueError(f'tails: {type(tails).__name__} is not a StreamTails')
    X = np.asarray(stft_signal, dtype=np.complex128)
    F, lead = state.size // 2 + 1, '(S,Tn,' if targets else '(Tn,'
    if X.ndim != (3 if targets else 2) or X.shape[-1] != F:
        raise ValueError(f'stft_signal: shape {X.shape} is not {lead}F) = {lead}{F})')
    S, Tn = X.shape[:2] if targets else (1, X.shape[0])
    ctx, pad = state.ctx, state.size - state.shift
    if targets:
        if tails.key != (S, pad):
            raise ValueError(f'tails: built for ({tails._sizes}) = {tails.key}, the call has '
                             f'{(S, pad)}')
        if tails.ctx is not ctx:
            raise ValueError('tails: they live in another context than the stream')
    if Tn == 0:
        return np.zeros((S, 0))
    m = (max(0, (state.frames_out + Tn) * state.shift - pad)
         - max(0, state.frames_out * state.shift - pad))
    _prepare_windows(ctx, state.size, state.shift, window)
    X_d = ctx.to_device(X)
    o_d = ctx.empty(max(8 * S * m, 16))
    if targets:
        ctx._check(ctx.lib.gss_istft_stream_targets(
            ctx.handle, c_void_p(X_d.ptr), Tn, S, ctypes.byref(state.struct()),
            c_void_p(tails.ptr), c_void_p(o_d.ptr)), 'gss_istft_stream_targets')
    else:
        ctx._check(ctx.lib.gss_istft_stream(ctx.handle, c_void_p(X_d.ptr), Tn,
                                            ctypes.byref(state.struct()), c_void_p(o_d.ptr)),
                   'gss_istft_stream')
    return ctx.to_host(o_d, (S, m), np.float64)


def istft_stream(stft_signal, *, state, window=None):
    """The synthesis side of a stream (gss_istft_stream): the next frames (Tn,F) -> the samples
    they finish, `stream_num_samples_out` of them.  ``state``: the `StreamState` whose analysis
    side produced the frames, advanced IN PLACE.  Every frame is transformed on its own: the
    samples do not depend on where the blocks were cut."""
    return _istft_stream_call(stft_signal, state, window)[0]


def _stream_block_call(entry, block, activity, params, stream, em_state, wpe_state, states,
                       bf_args, cfg, window, debug):
    """What `stream_block` and `stream_block_targets` share around the library call ``entry``:
    the checks of ``stream`` and of ``states`` ((name, state, class), in this order), then
    ``bf_args()``, the caller's own checks of its targets and beamformer states -> (S, the
    entry's arguments after the CACGMM state, those after n); the block on the device, the
    counts, the windows, the taps, ``cfg`` = (wpe_alpha, em_forget, bf_forget, ref_channel), the
    call and the download.  Returns (samples (S,m), details of `_debug_details` or None)."""
    if not isinstance(stream, StreamState):
        raise ValueError(f'stream: {type(stream).__name__} is not a StreamState')
    ctx = stream.ctx
    for name, state, cls in states:
        if state is None and name == 'wpe_state':
            continue
        if not isinstance(state, cls):
            raise ValueError(f'{name}: {type(state).__name__} is not an {cls.__name__}')
        if state.ctx is not ctx:
            raise ValueError(f'{name}: it lives in another context than the stream')
    S, bf_head, bf_tail = bf_args()
    x_d, in_type, act_d, n = _stream_block_to_device(ctx, block, activity, stream)
    if n == 0:
        return np.zeros((S, 0)), None
    Tn = stream_num_frames(stream.received, n, stream.size, stream.shift)
    m = stream_num_samples_out(stream.received, n, stream.size, stream.shift)
    _prepare_windows(ctx, stream.size, stream.shift, window)
    o_d = ctx.empty(max(8 * S * m, 16))
    utt = SimpleNamespace(ctx=ctx, D=stream.D, K=em_state.K, T=Tn, params=params)
    bufs, taps = _debug_taps(utt, S) if debug and Tn > 0 else (None, None)
    wpe_alpha, em_forget, bf_forget, ref_channel = cfg
    cfg = GssStreamCfg(wpe_alpha=float(wpe_alpha), em_forget=float(em_forget),
                       bf_forget=float(bf_forget), ref_channel=int(ref_channel))
    ctx._check(getattr(ctx.lib, entry)(
        ctx.handle, ctypes.byref(params), ctypes.byref(cfg), ctypes.byref(stream.struct()),
        ctypes.byref(wpe_state.struct()) if wpe_state is not None else None,
        ctypes.byref(em_state.struct()), *bf_head, c_void_p(x_d.ptr), in_type,
        c_void_p(act_d.ptr) if act_d else None, n, *bf_tail, c_void_p(o_d.ptr),
        ctypes.byref(taps) if taps is not None else None), entry)
    samples = ctx.to_host(o_d, (S, m), np.float64)
    if m == 0:
        ctx.synchronize()      # (the block's device copies are read until then)
    if bufs is None:
        return samples, None
    if act_d is None:
        del bufs['act_frames']
    return samples, _debug_details(utt, bufs, S)


def stream_block(block, activity=None, *, params, stream, em_state, bf_state, wpe_state=None,
                 target_index=0, ref_channel=0, wpe_alpha=WPE_ONLINE_ALPHA,
                 em_forget=GSS_ONLINE_FORGET, bf_forget=BF_ONLINE_FORGET, window=None,
                 debug=False):
    """One block of a stream through the whole front-end as ONE library call (gss_stream_block):
    `stft_stream` -> `wpe_online_dtf` -> `cacgmm_posteriors_online` masked by the block's frame
    activity -> masks with no frames zeroed -> `mvdr_souden_online_from_masks` with BAN ->
    postfilter -> `istft_stream`, every stage with the caller's state, all four advanced IN
    PLACE.  ``wpe_state`` is None exactly when ``params.wpe`` is 0.  Returns (samples, details):
    the samples the block finishes, and with ``debug`` the taps over the block's frames (else
    None), with 'fallbacks' = (online MVDR, online CACGMM) counts of the block."""
    samples, details = _stream_block_call(
        'gss_stream_block', block, activity, params, stream, em_state, wpe_state,
        (('em_state', em_state, OnlineCACGMMState), ('bf_state', bf_state, OnlineMVDRState),
         ('wpe_state', wpe_state, OnlineWPEState)),
        lambda: (1, [ctypes.byref(bf_state.struct())], [int(target_index)]),
        (wpe_alpha, em_forget, bf_forget, ref_channel), window, debug)
    if details is not None:
        ctx = stream.ctx
        details.update({k: v[0] for k, v in details.items() if k in _PER_TARGET})
        details['ref_channel'] = int(details['ref_channel'])
        details['fallbacks'] = (ctx.last_mvdr_online_fallbacks(),
                                ctx.last_cacgmm_online_fallbacks())
    return samples[0], details


# --------------------------------------------------------------------------
# several targets of one stream (gss_stream_block_targets)
# --------------------------------------------------------------------------
def check_online_targets(targets, num_classes=None):
    """The targets of a multi-target stream -- the one place that validates them.  ValueError:
    not a sequence, empty, more than 8, not integers, one given twice, one outside
    [0, num_classes).  Returns them as a tuple of ints."""
    if isinstance(targets, (str, bytes)) or not hasattr(targets, '__len__'):
        raise ValueError(f'targets={targets!r}: a sequence of class indices')
    values = list(targets)
    if not 1 <= len(values) <= _ONLINE_MAX_CLASSES:
        raise ValueError(f'targets={targets!r}: 1 to {_ONLINE_MAX_CLASSES} class indices')
    for t in values:
        if not _is_integer(t) or t < 0 or (num_classes is not None and t >= num_classes):
            raise ValueError(f'targets={targets!r}: {t!r} is not an integer in [0, '
                             f'{"num_classes" if num_classes is None else num_classes})')
    if len(set(int(t) for t in values)) != len(values):
        raise ValueError(f'targets={targets!r}: a class is given twice')
    return tuple(int(t) for t in values)


class StreamTails(_OnlineState):
    """The overlap-add tails of the S signals of a multi-target stream in HBM, caller-owned:
    ``tails`` (S, size - shift) float64, zero at the start of a stream."""
    _sizes = 'S, size - shift'
    dtypes = {'tails': np.float64}

    def __init__(self, ctx, S, pad):
        super().__init__(ctx, S, pad)
        self.S, self.pad = self.key

    @staticmethod
    def _shapes(S, pad):
        return {'tails': (S, pad)}

    @property
    def ptr(self):
        return self.bufs['tails'].ptr

    @classmethod
    def fresh(cls, S, size=1024, shift=256, *, ctx=None):
        check_stream(1, 0, size, shift)
        if not _is_integer(S) or not 1 <= S <= _ONLINE_MAX_CLASSES:
            raise ValueError(f'S={S!r}: an integer in [1, {_ONLINE_MAX_CLASSES}]')
        return cls.from_host({'tails': np.zeros((S, size - shift))}, ctx=ctx)

    @classmethod
    def from_host(cls, host, *, ctx=None):
        tails = np.asarray(host['tails'])
        if tails.ndim != 2 or not 1 <= tails.shape[0] <= _ONLINE_MAX_CLASSES or tails.shape[1] < 1:
            raise ValueError(f'tails: shape {tails.shape} is not (S, size - shift)')
        return cls._from_host(host, tails.shape, ctx)


def _check_target_states(states, S, key, ctx, name='states'):
    """S different `OnlineMVDRState`s built for ``key`` = (F, D), all in ``ctx`` (None: the
    first one's).  Returns the context and the ctypes array of their structs."""
    states = list(states) if hasattr(states, '__iter__') else None
    if states is None or len(states) != S:
        raise ValueError(f'{name}: a sequence of {S} OnlineMVDRState, one per target')
    for state in states:
        ctx = _state_context(state, OnlineMVDRState, key, ctx)
    if len({id(state) for state in states}) != S:
        raise ValueError(f'{name}: the same state for two targets')
    return ctx, (GssMvdrOnlineState * S)(*(state.struct() for state in states))


def mvdr_souden_online_targets(Y, posterior, targets, *, states, forget=BF_ONLINE_FORGET,
                               ref_channel=0, ban=False, postfilter=None, return_fallbacks=False,
                               return_filters=False, lookahead=0, hold=None):
    """The online MVDR for S targets in one launch (gss_mvdr_online_targets): Y (D,T,F), the
    posteriors (K,T,F), ``targets`` S distinct class indices, ``states`` S `OnlineMVDRState`s,
    each advanced IN PLACE -> X_hat (S,T,F) complex128.  The masks are formed on the device as
    `masks_from_posteriors` forms them; row s has the bits of `mvdr_souden_online_from_masks` on
    the masks of class targets[s] with states[s] (times the target mask with
    ``postfilter='mask_mul'``).  Then with ``return_filters`` the filters (S,T,F,D), then with
    ``return_fallbacks`` the list of S fallback counts.

    ``lookahead`` = L >= 1 (gss_mvdr_online_lookahead_targets): as in
    `mvdr_souden_online_from_masks`; the postfilter multiplies by the target mask of the OUTPUT
    frame.  ``hold`` None: the one-shot form -> (S,T,F); ``hold``: S `OnlineMVDRHold`s built for
    (F,D,L), advanced IN PLACE -> the (S, max(0, held + T - L), F) frames released."""
    Y = np.asarray(Y)
    if Y.ndim != 3:
        raise ValueError(f'Y: shape {Y.shape} is not (D,T,F)')
    D, T, F = Y.shape
    g = np.asarray(posterior, dtype=np.float64)
    if g.ndim != 3 or g.shape[1:] != (T, F):
        raise ValueError(f'posterior: shape {g.shape} is not (K,T,F) = (K,{T},{F})')
    K = g.shape[0]
    if not 1 <= K <= _ONLINE_MAX_CLASSES:
        raise ValueError(f'posterior: {K} classes, 1 to {_ONLINE_MAX_CLASSES} are supported')
    if not np.all(np.isfinite(g)) or np.any(g < 0):
        raise ValueError('posterior: a value is negative or not finite')
    targets = check_online_targets(targets, K)
    S = len(targets)
    forget, _, ref_channel = check_bf_online(forget, BF_ONLINE_LOADING, ref_channel, D)
    if ref_channel < 0:
        raise ValueError(f'ref_channel={ref_channel!r}: an integer in [0, {D})')
    if postfilter not in (None, 'mask_mul'):
        raise ValueError(f"postfilter={postfilter!r}: None or 'mask_mul'")
    ctx, structs = _check_target_states(states, S, (F, D), None)
    lookahead = check_bf_lookahead(lookahead, ref_channel)
    if hold is not None and lookahead == 0:
        raise ValueError('hold: delay lines with lookahead=0')
    fallbacks = [0] * S
    if lookahead:
        holds = None if hold is None else _check_holds(hold, S, (F, D, lookahead), ctx)[1]
        X_hat, W = np.zeros((S, 0, F), np.complex128), np.zeros((S, 0, F, D), np.complex128)
        if T > 0 and F > 0:
            one_shot = holds is None
            if one_shot:
                holds = [OnlineMVDRHold.fresh(F, D, lookahead, ctx=ctx) for _ in range(S)]
            R = max(0, holds[0].held + T - lookahead)
            Y_d, _ = _obs_to_device_ftd(ctx, Y)
            g_d = ctx.to_device(g.transpose(2, 0, 1))                       # (F,K,T)
            X_d = ctx.empty(max(16 * S * F * R, 16))
            W_d = ctx.empty(max(16 * S * F * R * D, 16)) if return_filters else None
            cfg = _bf_online_cfg(forget, BF_ONLINE_LOADING, ref_channel)
            lines = _hold_structs(holds)
            ctx._check(ctx.lib.gss_mvdr_online_lookahead_targets(
                ctx.handle, c_void_p(Y_d.ptr), F, T, D, c_void_p(g_d.ptr), K,
                (ctypes.c_int32 * S)(*targets), S, int(bool(ban)), ctypes.byref(cfg), structs, lines,
                int(postfilter == 'mask_mul'), None, None, c_void_p(X_d.ptr),
                c_void_p(W_d.ptr) if W_d is not None else None, None),
                'gss_mvdr_online_lookahead_targets')
            _holds_advance(holds, lines)
            if R:
                X_hat = ctx.to_host(X_d, (S, R, F), np.complex128)
                if return_filters:
                    W = np.ascontiguousarray(ctx.to_host(W_d, (S, F, R, D), np.complex128)
                                             .transpose(0, 2, 1, 3))
            if return_fallbacks:
                fallbacks = ctx.last_mvdr_online_fallbacks_targets(S)
            if one_shot:
                tail = mvdr_online_release(holds, postfilter=postfilter,
                                           return_filters=return_filters)
                if return_filters:
                    tail, W = tail[0], np.concatenate([W, tail[1]], axis=1)
                X_hat = np.concatenate([X_hat, tail], axis=1)
    elif T == 0 or F == 0:
        X_hat, W = np.zeros((S, T, F), np.complex128), np.zeros((S, T, F, D), np.complex128)
    else:
        Y_d, _ = _obs_to_device_ftd(ctx, Y)
        g_d = ctx.to_device(g.transpose(2, 0, 1))                       # (F,K,T)
        X_d = ctx.empty(16 * S * F * T)
        W_d = ctx.empty(16 * S * F * T * D) if return_filters else None
        cfg = _bf_online_cfg(forget, BF_ONLINE_LOADING, ref_channel)
        ctx._check(ctx.lib.gss_mvdr_online_targets(
            ctx.handle, c_void_p(Y_d.ptr), F, T, D, c_void_p(g_d.ptr), K,
            (ctypes.c_int32 * S)(*targets), S, int(bool(ban)), ctypes.byref(cfg), structs,
            int(postfilter == 'mask_mul'), None, None, c_void_p(X_d.ptr),
            c_void_p(W_d.ptr) if W_d is not None else None), 'gss_mvdr_online_targets')
        X_hat = ctx.to_host(X_d, (S, T, F), np.complex128)
        W = (np.ascontiguousarray(ctx.to_host(W_d, (S, F, T, D), np.complex128)
                                  .transpose(0, 2, 1, 3)) if return_filters else None)
        if return_fallbacks:
            fallbacks = ctx.last_mvdr_online_fallbacks_targets(S)
    out = (X_hat,) + ((W,) if return_filters else ()) + ((fallbacks,) if return_fallbacks else ())
    return out if len(out) > 1 else X_hat


def istft_stream_targets(stft_signal, *, state, tails, window=None):
    """`istft_stream` for S signals in one set of launches (gss_istft_stream_targets): the next
    frames (S,Tn,F) -> (S,m), row s with the bits of `istft_stream` on stft_signal[s].  ``state``:
    the `StreamState` of the analysis side, its frame counter advanced once, its own tail left
    alone; ``tails``: the `StreamTails` of the S signals, advanced IN PLACE."""
    return _istft_stream_call(stft_signal, state, window, True, tails)


def stream_block_targets(block, activity=None, *, params, stream, em_state, bf_states, tails,
                         target_indices, wpe_state=None, ref_channel=0,
                         wpe_alpha=WPE_ONLINE_ALPHA, em_forget=GSS_ONLINE_FORGET,
                         bf_forget=BF_ONLINE_FORGET, window=None, debug=False):
    """`stream_block` for S targets as ONE library call (gss_stream_block_targets): the analysis,
    the online WPE and the online CACGMM once, then `mvdr_souden_online_targets` with BAN and the
    postfilter and `istft_stream_targets`.  ``bf_states``: S `OnlineMVDRState`s, ``tails``: the
    `StreamTails`, all advanced IN PLACE.  Returns (samples (S,m), details): row s has the bits of
    `stream_block` with target_indices[s]; with ``debug`` the per-target taps are stacked over S as
    in `enhance_observation_targets`, 'fallbacks' = (online MVDR summed over the targets, online
    CACGMM) and 'fallbacks_targets' the online MVDR's per target."""
    def bf_args():
        targets = check_online_targets(target_indices, em_state.K)
        S = len(targets)
        _, structs = _check_target_states(bf_states, S, (stream.size // 2 + 1, stream.D),
                                          stream.ctx, 'bf_states')
        if tails.key != (S, stream.size - stream.shift):
            raise ValueError(f'tails: built for ({tails._sizes}) = {tails.key}, the call has '
                             f'{(S, stream.size - stream.shift)}')
        return S, [structs, c_void_p(tails.ptr)], [(ctypes.c_int32 * S)(*targets), S]

    samples, details = _stream_block_call(
        'gss_stream_block_targets', block, activity, params, stream, em_state, wpe_state,
        (('em_state', em_state, OnlineCACGMMState), ('wpe_state', wpe_state, OnlineWPEState),
         ('tails', tails, StreamTails)),
        bf_args, (wpe_alpha, em_forget, bf_forget, ref_channel), window, debug)
    if details is not None:
        ctx = stream.ctx
        details['fallbacks'] = (ctx.last_mvdr_online_fallbacks(),
                                ctx.last_cacgmm_online_fallbacks())
        details['fallbacks_targets'] = ctx.last_mvdr_online_fallbacks_targets(samples.shape[0])
    return samples, details


def stream_block_lookahead(block, activity=None, *, params, stream, em_state, bf_states, holds,
                           tails, target_indices, release=False, wpe_state=None, ref_channel=0,
                           wpe_alpha=WPE_ONLINE_ALPHA, em_forget=GSS_ONLINE_FORGET,
                           bf_forget=BF_ONLINE_FORGET, window=None, debug=False):
    """`stream_block_targets` (S >= 1) with a filter look-ahead as ONE library call
    (gss_stream_block_lookahead): its front up to the posteriors, then
    `mvdr_souden_online_targets` with ``hold=holds`` (BAN, the postfilter on the mask of the
    output frame) and `istft_stream_targets` on the frames RELEASED; with ``release`` (the last
    block of a stream) `mvdr_online_release` follows and its frames are synthesised too -- a block
    of no samples with ``release`` only ends the lines.  ``holds``: S `OnlineMVDRHold`s, advanced
    IN PLACE like every other state.  Returns (samples (S,m), details): the samples the released
    frames finish; with ``debug`` the taps, 'X_hat' over the frames released, the others over the
    block's frames."""
    if not isinstance(stream, StreamState):
        raise ValueError(f'stream: {type(stream).__name__} is not a StreamState')
    ctx = stream.ctx
    for name, state, cls in (('em_state', em_state, OnlineCACGMMState),
                             ('wpe_state', wpe_state, OnlineWPEState), ('tails', tails, StreamTails)):
        if state is None and name == 'wpe_state':
            continue
        if not isinstance(state, cls):
            raise ValueError(f'{name}: {type(state).__name__} is not an {cls.__name__}')
        if state.ctx is not ctx:
            raise ValueError(f'{name}: it lives in another context than the stream')
    targets = check_online_targets(target_indices, em_state.K)
    S, F, D, K = len(targets), stream.size // 2 + 1, stream.D, em_state.K
    _, structs = _check_target_states(bf_states, S, (F, D), ctx, 'bf_states')
    first = holds if isinstance(holds, OnlineMVDRHold) else (
        holds[0] if hasattr(holds, '__len__') and len(holds) else None)
    if not isinstance(first, OnlineMVDRHold):
        raise ValueError('holds: a sequence of OnlineMVDRHold, one per target')
    _, holds = _check_holds(holds, S, (F, D, first.L), ctx, 'holds')
    if tails.key != (S, stream.size - stream.shift):
        raise ValueError(f'tails: built for ({tails._sizes}) = {tails.key}, the call has '
                         f'{(S, stream.size - stream.shift)}')
    x_d, in_type, act_d, n = _stream_block_to_device(ctx, block, activity, stream)
    L, held = first.L, first.held
    Tn = stream_num_frames(stream.received, n, stream.size, stream.shift)
    rows = max(0, held + Tn - L) + (min(L, held + Tn) if release else 0)
    if n == 0 and rows == 0:
        return np.zeros((S, 0)), None
    m = stream_num_samples_out(stream.frames_out * stream.shift, rows * stream.shift, stream.size,
                               stream.shift)
    _prepare_windows(ctx, stream.size, stream.shift, window)
    if n == 0:      # (the entry wants the pointers of a block even where it reads no sample)
        x_d = ctx.empty(16)
        act_d = ctx.empty(16) if activity is not None else None
    o_d = ctx.empty(max(8 * S * m, 16))
    utt = SimpleNamespace(ctx=ctx, D=D, K=K, T=Tn, params=params)
    bufs = taps = None
    if debug and (Tn > 0 or rows > 0):
        bufs, taps = _debug_taps(utt, S) if Tn > 0 else ({}, GssDebugTaps())
        bufs['Xhat'] = ctx.empty(max(16 * S * F * rows, 16))
        taps.Xhat = bufs['Xhat'].ptr
    cfg = GssStreamCfg(wpe_alpha=float(wpe_alpha), em_forget=float(em_forget),
                       bf_forget=float(bf_forget), ref_channel=int(ref_channel))
    lines = _hold_structs(holds)
    ctx._check(ctx.lib.gss_stream_block_lookahead(
        ctx.handle, ctypes.byref(params), ctypes.byref(cfg), ctypes.byref(stream.struct()),
        ctypes.byref(wpe_state.struct()) if wpe_state is not None else None,
        ctypes.byref(em_state.struct()), structs, lines, c_void_p(tails.ptr), c_void_p(x_d.ptr),
        in_type, c_void_p(act_d.ptr) if act_d else None, n, (ctypes.c_int32 * S)(*targets), S,
        int(bool(release)), c_void_p(o_d.ptr), None,
        ctypes.byref(taps) if taps is not None else None), 'gss_stream_block_lookahead')
    _holds_advance(holds, lines)
    samples = ctx.to_host(o_d, (S, m), np.float64)
    if m == 0:
        ctx.synchronize()      # (the block's device copies are read until then)
    if bufs is None:
        return samples, None
    X_hat = ctx.to_host(bufs.pop('Xhat'), (S, rows, F), np.complex128)
    if Tn == 0:
        return samples, {'X_hat': X_hat}
    if act_d is None:
        del bufs['act_frames']
    details = _debug_details_without_xhat(utt, bufs, S)
    details['X_hat'] = X_hat
    details['fallbacks'] = (ctx.last_mvdr_online_fallbacks(), ctx.last_cacgmm_online_fallbacks())
    details['fallbacks_targets'] = ctx.last_mvdr_online_fallbacks_targets(S)
    return samples, details


def _debug_details_without_xhat(utt, bufs, S):
    """`_debug_details` of a call whose 'X_hat' tap covers other frames than the rest."""
    ctx, D, K, T = utt.ctx, utt.D, utt.K, utt.T
    F = utt.params.stft_size // 2 + 1
    details = {}
    if 'act_frames' in bufs:
        details['acitivity_freq'] = ctx.to_host(bufs['act_frames'], (K, T), np.uint8).astype(bool)
    return {
        'Obs': _ftd_to_host_dtf(ctx, bufs['Obs_ftd'], D, T, F),
        **details,
        'posterior': ctx.to_host(bufs['gamma'], (F, K, T), np.float64).transpose(1, 2, 0),
        'target_mask': ctx.to_host(bufs['target_mask'], (S, F, T), np.float64).transpose(0, 2, 1),
        'distortion_mask': ctx.to_host(bufs['distortion_mask'], (S, F, T),
                                       np.float64).transpose(0, 2, 1),
        'ref_channel': ctx.to_host(bufs['ref_channel'], (S,), np.int32).astype(int),
    }


def masks_from_posteriors(posterior, target_index, *, ctx=None):
    """Target and distortion mask from the posteriors with no frames zeroed
    (gss_masks_from_posteriors, drop_context = 0): posterior (K,T,F) -> (X_mask, N_mask) (T,F),
    the target's row and the sum of the others -- the masks of a stream, which has no context."""
    g = np.asarray(posterior, dtype=np.float64)
    if g.ndim != 3:
        raise ValueError(f'posterior: shape {g.shape} is not (K,T,F)')
    K, T, F = g.shape
    if not _is_integer(target_index) or not 0 <= target_index < K:
        raise ValueError(f'target_index={target_index!r}: an integer in [0, {K})')
    if T == 0 or F == 0:
        return np.zeros((T, F)), np.zeros((T, F))
    ctx = ctx or default_context()
    g_d = ctx.to_device(g.transpose(2, 0, 1))                       # (F,K,T)
    bufs = [ctx.empty(8 * F * T) for _ in range(2)]
    ctx._check(ctx.lib.gss_masks_from_posteriors(
        ctx.handle, c_void_p(g_d.ptr), F, K, T, int(target_index), 0, 0, 0,
        *(c_void_p(b.ptr) for b in bufs)), 'gss_masks_from_posteriors')
    return tuple(np.ascontiguousarray(ctx.to_host(b, (F, T), np.float64).T) for b in bufs)
