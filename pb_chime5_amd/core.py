"""Per-utterance guided source separation with the reference's Python surface
(/root/reference/pb_chime5/core.py), running on MI355X.

Legend (as in the reference):  n, N time | t, T frame | f, F frequency |
d, D channel | a, A array | k, K class (speakers + ``Noise``).

Kept from the reference: ``get_enhancer(**same kwargs)``, the ``WPE`` / ``GSS`` /
``Beamformer`` / ``Enhancer`` blocks with their call signatures, shapes, dtypes
(complex128 / float64 at the Python edge) and exception types,
``start_end_context_frames`` and the ``debug=True`` contract (intermediates kept
on the block).  Different by design: the numeric work is done by hand-written HIP
kernels behind ``include/gss_hip.h``; ``Enhancer.enhance_observation`` uses the
fused device pipeline (one H2D of the time signal, one D2H of the result) unless
a block was replaced or ``fused=False`` is passed; work is distributed over GPUs
by ``pb_chime5_amd.parallel`` instead of ``dlp_mpi``.
"""
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

from pb_chime5_amd import mapping, ops
from pb_chime5_amd import posterior_activity as pact
from pb_chime5_amd.database.chime5 import activity_time_to_frequency
from pb_chime5_amd.io import dump_audio, load_audio
from pb_chime5_amd.utils.numpy_utils import morph


@dataclass
class WPE:
    """core.py:41-88 -> nara_wpe.wpe.wpe_v8.
    ``online=True`` (an addition): nara_wpe's online form instead -- a frame-recursive filter that
    forgets at the rate ``alpha``, from a fresh state (`ops.wpe_online_dtf`); ``iterations`` is
    not read, ``stack=False`` means one filter per array, a ``psd_context`` other than 0 is
    NotImplementedError.  alpha = 0.9999 is a choice, not a measurement."""
    taps: int
    delay: int
    iterations: int
    psd_context: int
    online: bool = False
    alpha: float = ops.WPE_ONLINE_ALPHA

    def __post_init__(self):
        if self.online:
            ops.check_wpe_online(self.taps, self.delay, self.alpha)

    def _call_online(self, Obs, stack, debug):
        if self.psd_context != 0:
            raise NotImplementedError(
                f'online=True with psd_context={self.psd_context!r}: the online WPE has no PSD '
                'context')
        kw = dict(taps=self.taps, delay=self.delay, alpha=self.alpha)
        if Obs.ndim == 3:
            assert stack is None, stack
            Obs = ops.wpe_online_dtf(Obs, **kw)
        elif Obs.ndim == 4:
            if stack is not True and stack is not False:
                raise NotImplementedError(stack)
            _A = Obs.shape[0]
            Obs = morph('ACTF->A*CTF', Obs)
            Obs = ops.wpe_online_dtf(Obs, arrays=1 if stack else _A, **kw)
            Obs = morph('A*CTF->ACTF', Obs, A=_A)
        else:
            raise NotImplementedError(Obs.shape)
        if debug:
            self.locals = locals()
        return Obs

    def __call__(self, Obs, stack=None, debug=False):
        if self.online:
            return self._call_online(Obs, stack, debug)
        kw = dict(taps=self.taps, delay=self.delay, iterations=self.iterations,
                  psd_context=self.psd_context)
        if Obs.ndim == 3:
            assert stack is None, stack
            Obs = ops.wpe_dtf(Obs, **kw)
        elif Obs.ndim == 4:
            if stack is True:
                _A = Obs.shape[0]
                Obs = morph('ACTF->A*CTF', Obs)
                Obs = ops.wpe_dtf(Obs, **kw)
                Obs = morph('A*CTF->ACTF', Obs, A=_A)
            elif stack is False:
                # one wpe_v8 per array (core.py:71-79), all arrays in one device call
                _A = Obs.shape[0]
                Obs = morph('ACTF->A*CTF', Obs)
                Obs = ops.wpe_arrays_dtf(Obs, _A, **kw)
                Obs = morph('A*CTF->ACTF', Obs, A=_A)
            else:
                raise NotImplementedError(stack)
        else:
            raise NotImplementedError(Obs.shape)
        if debug:
            self.locals = locals()
        return Obs


def default_database_path():
    """The reference looks for ``<git root>/cache/chime5.json`` (core.py:20,98); here
    ``$PB_CHIME5_JSON`` if set, else ``cache/chime5.json`` under the working directory."""
    import os
    return os.environ.get('PB_CHIME5_JSON', str(Path('cache') / 'chime5.json'))


@dataclass
class Activity:
    """core.py:91-141.  ``activity[session_id][array][speaker][start:stop] -> bool``.
    ``type='annotation'`` derives the tracks from the utterance boundaries in the CHiME-5
    JSON (one session cached, like the reference's ``lru_cache(1)``); ``type='path'``
    reads the reference's per-session pickles; ``store`` plugs in a ready dict."""
    type: str = 'annotation'
    garbage_class: bool = False
    database_path: str = None
    path: str = None
    store: dict = None

    # sessions kept at a time: the reference keeps one (lru_cache(1), core.py:104); a rank of a
    # multi-session run ('dev' = S02 + S09, longest first) alternates between a few
    _CACHE_SESSIONS = 4

    def __post_init__(self):
        import threading
        self._db = None
        self._cache = {}                 # session_id -> tracks, insertion-ordered (LRU)
        self._cache_lock = threading.Lock()

    @property
    def db(self):
        if self._db is None:
            from pb_chime5_amd.database.chime5.database import Chime5
            self._db = Chime5(self.database_path or default_database_path())
        return self._db

    def _annotation_activity(self, session_id):
        from pb_chime5_amd.activity import get_activity
        return get_activity(
            iterator=self.db.get_datasets(session_id), perspective='array',
            garbage_class=self.garbage_class, dtype=bool,
            use_ArrayIntervall=True)[session_id]

    def _cached_annotation(self, session_id):
        """Called from every loader thread of a session (`Enhancer._prepare_into`): the look-up,
        the computation and the hand-out of ONE session's tracks happen under a lock, and the
        caller gets the object it asked for, never "whatever the cache holds now"."""
        with self._cache_lock:
            tracks = self._cache.pop(session_id, None)
            if tracks is None:
                tracks = self._annotation_activity(session_id)
                while len(self._cache) >= self._CACHE_SESSIONS:
                    self._cache.pop(next(iter(self._cache)))
            self._cache[session_id] = tracks      # most recently used last
            return tracks

    def __getitem__(self, session_id):
        if self.store is not None:
            return self.store[session_id]
        if self.type == 'annotation':
            return self._cached_annotation(session_id)
        if self.type == 'path':
            with open(Path(self.path) / f'{session_id}.pkl', 'rb') as fd:
                return _ReferenceUnpickler(fd).load()
        raise ValueError(self.type)


class _ReferenceUnpickler(__import__('pickle').Unpickler):
    """Activity pickles written with the reference (core.py:135-139, e.g. the alignment-based
    activity of its sacred runs) name classes of the `pb_chime5` package, above all
    pb_chime5.utils.intervall_array.ArrayIntervall; they resolve to their counterparts here
    (same attributes), so such a file loads without the reference installed."""

    def find_class(self, module, name):
        if module == 'pb_chime5' or module.startswith('pb_chime5.'):
            module = 'pb_chime5_amd' + module[len('pb_chime5'):]
        return super().find_class(module, name)


class _DebugLocals(dict):
    """``GSS.locals``: the locals of the call, and under 'learned' the fitted
    `pb_chime5_amd.cacgmm.CACGMM`.  The model costs a fit, so it is fitted when the key is first
    read with ``[]`` or ``get``; ``in`` knows the key without fitting.  Iteration, ``keys()``,
    ``items()`` and ``dict(...)`` show 'learned' only once it has been read.  The mapping holds
    the call's ``Obs`` -- as the reference's ``locals()`` does -- until ``GSS.locals`` is replaced."""

    def __init__(self, values, learned):
        super().__init__((k, v) for k, v in values.items() if k != 'learned')
        self._learned = learned

    def __missing__(self, key):
        if key != 'learned':
            raise KeyError(key)
        self[key] = self._learned()
        return self[key]

    def __contains__(self, key):
        return key == 'learned' or super().__contains__(key)

    def get(self, key, default=None):
        return self[key] if key in self else default


@dataclass
class BlindSeparation:
    """What `Enhancer.enhance_observation_blind` returns.  Classes carry indices, not names."""
    x_hat: np.ndarray          # (K, N) enhanced signal of every class
    prior: np.ndarray          # (K, T) the frequency-shared prior: a per-frame activity estimate
    active: np.ndarray         # (K, T) bool: `posterior_activity.decide(prior, power, rule)`
    intervals: list            # per class [(start, end), ...] in samples


@dataclass
class BlindRecording:
    """What `Enhancer.enhance_recording_blind` returns.  Classes carry indices, not names; one
    index is one source through the whole recording as far as the links hold."""
    x_hat: np.ndarray          # (K, N) the windows' enhanced signals, linked and cross-faded
    prior: np.ndarray          # (K, T) the windows' priors, linked and cross-faded over frames
    active: np.ndarray         # (K, T) bool: `posterior_activity.decide(prior, power, rule)`
    intervals: list            # per class [(start, end), ...] in samples
    windows: list              # [(start, end), ...] in samples
    mappings: np.ndarray       # (n, K) int: class k of the recording is class mappings[w, k] of
    #                            window w's own numbering; row 0 is the identity
    link_scores: np.ndarray    # (n, K): S[k, mappings[w, k]] of window w's link; NaN in row 0


@dataclass
class GSS:
    """core.py:144-214 -> CACGMMTrainer.fit / predict for every frequency."""
    iterations: int
    iterations_post: int
    verbose: bool = True
    # One prior per class and frame for all frequencies in place of a mixture weight per class and
    # frequency (`ops.cacgmm_posteriors_shared_prior`; pb_bss weight_constant_axis=-3, which the
    # reference never calls).  Off: the reference's model, every call as before.
    shared_prior: bool = False
    # Online CACGMM (an addition, see ops.cacgmm_posteriors_online): the recursive EM in the place
    # of the iterated one -- running sums that forget at the rate ``forget``, frame t classified
    # by the model of the frames before it, from a fresh state of ``prior_mass`` per utterance,
    # masked by the activity; ``iterations`` / ``iterations_post`` are not read.  forget = 0.99
    # and prior_mass = 1.0 are choices, not measurements.  Unread without ``online``.
    online: bool = False
    forget: float = ops.GSS_ONLINE_FORGET
    prior_mass: float = ops.GSS_ONLINE_PRIOR_MASS

    def __post_init__(self):
        assert self.online is True or self.online is False, self.online
        if self.online:
            if self.shared_prior:
                raise NotImplementedError(
                    'gss_online with shared_prior: the online mixture model has a weight per '
                    'class and frequency')
            ops.check_gss_online(self.forget, self.prior_mass)
        else:
            for name, value, default in (('gss_forget', self.forget, ops.GSS_ONLINE_FORGET),
                                         ('gss_prior_mass', self.prior_mass,
                                          ops.GSS_ONLINE_PRIOR_MASS)):
                if value != default:
                    raise NotImplementedError(f'{name}={value!r} without gss_online: nobody reads it')

    @property
    def online_settings(self):
        """The keyword arguments of the online calls in ``ops``, or None."""
        if not self.online:
            return None
        return dict(forget=self.forget, prior_mass=self.prior_mass)

    def _call_online(self, Obs, acitivity_freq, debug, initialization):
        """The activity is the mask; its weights have nowhere to go (there is no initialisation:
        the start is the fresh state)."""
        if initialization is not None:
            raise NotImplementedError(
                'gss_online with an initialization: the online mixture model starts from its '
                'fresh state, guided by the mask alone')
        source_active_mask = np.asarray(acitivity_freq) != 0
        posterior, fallbacks = ops.cacgmm_posteriors_online(
            Obs, source_active_mask, forget=self.forget, prior_mass=self.prior_mass,
            return_fallbacks=True)
        if debug:
            def learned():
                raise NotImplementedError(
                    "GSS(online=True) keeps no 'learned' model: run ops.cacgmm_posteriors_online "
                    'with a state and ask it to_model()')
            self.locals = _DebugLocals(locals(), learned)
        return posterior

    def __call__(self, Obs, acitivity_freq, debug=False, *, initialization=None):
        """``acitivity_freq`` (K,T), or (K,T,F) for guidance that differs by frequency: zero =
        the class is off (source activity mask), any other value its weight in the initial
        affiliations, as in the reference (core.py:156-163).  ``initialization`` (K,T) or
        (K,T,F): initial affiliations used as given instead of the ones derived from the
        activity (a neural mask, the posteriors of an earlier pass).  A 0/1 activity without
        ``initialization`` takes the unweighted call; everything else the guided one."""
        if self.online:
            return self._call_online(Obs, acitivity_freq, debug, initialization)
        if self.shared_prior:
            return self._call_shared_prior(Obs, acitivity_freq, debug, initialization)
        binary = ops.activity_is_binary(acitivity_freq, initialization)
        if binary:
            posterior = ops.cacgmm_posteriors(
                Obs, acitivity_freq, iterations=self.iterations,
                iterations_post=self.iterations_post)
            if debug:
                initialization, source_active_mask = ops.guidance_from_activity(acitivity_freq)
        else:
            derived, source_active_mask = ops.guidance_from_activity(acitivity_freq)
            if initialization is None:
                initialization = derived
            posterior = ops.cacgmm_posteriors_guided(
                Obs, initialization, source_active_mask, iterations=self.iterations,
                iterations_post=self.iterations_post)
        if debug:
            # 'learned' (core.py:204-212): the model of the schedule's last fit -- the fits of the
            # schedule once more, as calls that hand the model out, when the key is first read
            # (a 0/1 activity: the initialisation derived on the device, as the call above did)
            def learned():
                model = ops.cacgmm_fit(Obs, None if binary else initialization, source_active_mask,
                                       iterations=self.iterations)
                if self.iterations_post > 1:
                    model = ops.cacgmm_fit(Obs, iterations=self.iterations_post - 1, model=model)
                return model
            self.locals = _DebugLocals(locals(), learned)
        return posterior

    def _call_shared_prior(self, Obs, acitivity_freq, debug, initialization):
        """Every kind of activity through `ops.cacgmm_posteriors_shared_prior`: the activity is
        the mask (weak guidance: who may speak), its weights or ``initialization`` the start."""
        derived, source_active_mask = ops.guidance_from_activity(acitivity_freq)
        if initialization is None:
            initialization = derived
        posterior, prior = ops.cacgmm_posteriors_shared_prior(
            Obs, initialization, source_active_mask, iterations=self.iterations,
            iterations_post=self.iterations_post, return_prior=True)
        if debug:
            def learned():
                raise NotImplementedError(
                    "GSS(shared_prior=True) has no 'learned' model: a model whose weight is "
                    '(K,T) cannot predict other frames')
            self.locals = _DebugLocals(locals(), learned)
        return posterior


def _original(value):
    # CHiME-5 examples carry {'original': ..., 'observation': {...}} (core.py:218-219),
    # CHiME-6 examples plain integers (core_chime6.py:215-216)
    return value['original'] if isinstance(value, dict) else value


def start_end_context_samples(ex):
    """The sample counts core.py:218-222 derives from ``ex`` (asserted >= 0)."""
    start_context_samples = _original(ex['start_orig']) - _original(ex['start'])
    end_context_samples = _original(ex['end']) - _original(ex['end_orig'])
    assert start_context_samples >= 0, (start_context_samples, ex)
    assert end_context_samples >= 0, (end_context_samples, ex)
    return start_context_samples, end_context_samples


def start_end_context_frames(ex, stft_size, stft_shift, stft_fading):
    """core.py:217-238."""
    start, end = start_end_context_samples(ex)
    return (
        ops.samples_to_stft_frames(start, stft_size, stft_shift, fading=stft_fading),
        ops.samples_to_stft_frames(end, stft_size, stft_shift, fading=stft_fading),
    )


@dataclass
class Beamformer:
    """core.py:241-278."""
    type: str
    postfilter: str
    # Time-varying MVDR (an addition): statistics per segment of ``segment_frames`` STFT frames
    # (a positive multiple of 64) over ``segment_context`` segments either side, one reference
    # channel per utterance; windows with less than ``segment_min_mass`` of target or
    # distortion mask (None: 2 * channels) take the whole-utterance statistics.  None: one
    # filter per utterance, the reference's beamformer.  Only 'mvdrSouden_ban' has it.
    segment_frames: int = None
    segment_context: int = 0
    segment_min_mass: float = None
    # Interferer-nulling LCMV (beamform_lcmv_souden_from_masks, beamforming_wrapper.py:127-171;
    # not reachable from the reference's Beamformer): distortionless for the target with a null
    # on the competing talker named by ``interferer_mask``; frequencies where that mask sums to
    # less than ``null_min_mass`` (None: 2 * channels; > 0) take the MVDR.  Only
    # 'mvdrSouden_ban' has it, and not together with segments.
    null_interferer: bool = False
    null_min_mass: float = None
    # WPD convolutional beamformer (types 'wpdSouden' / 'wpdSouden_ban'; an addition, see
    # ops.wpd_souden_from_masks): the tap window, the iterations and the floor of the target
    # power.  Unread by the other types.  wpd_power_floor = 1e-3 is a choice, not a measurement.
    wpd_taps: int = 10
    wpd_delay: int = 2
    wpd_iterations: int = 1
    wpd_power_floor: float = ops.WPD_POWER_FLOOR
    # Online MVDR (an addition, see ops.mvdr_souden_online_from_masks): 'mvdrSouden_ban' on
    # running sums that forget at the rate ``forget``, a filter per frame, from a fresh state per
    # utterance with the relative diagonal ``loading``; the reference channel is the window's.
    # forget = 0.99 and loading = 1e-2 are choices, not measurements.  Unread without ``online``.
    online: bool = False
    forget: float = ops.BF_ONLINE_FORGET
    loading: float = ops.BF_ONLINE_LOADING

    def __post_init__(self):
        assert self.online is True or self.online is False, self.online
        if self.online:
            if self.type != 'mvdrSouden_ban':
                raise NotImplementedError(
                    f"bf={self.type!r} with bf_online: only 'mvdrSouden_ban' has an online form")
            for name, on in (('bf_segment_frames', self.segment_frames is not None),
                             ('bf_null_interferer', self.null_interferer)):
                if on:
                    raise NotImplementedError(
                        f'bf_online with {name}: the online beamformer has a filter per frame '
                        'from two masks')
            ops.check_bf_online(self.forget, self.loading)
        else:
            for name, value, default in (('bf_forget', self.forget, ops.BF_ONLINE_FORGET),
                                         ('bf_loading', self.loading, ops.BF_ONLINE_LOADING)):
                if value != default:
                    raise NotImplementedError(f'{name}={value!r} without bf_online: nobody reads it')
        if self.type in ops.WPD_BF_TYPES:
            ops.check_bf_wpd(self.wpd_taps, self.wpd_delay, self.wpd_iterations,
                             self.wpd_power_floor, segment_frames=self.segment_frames,
                             null_interferer=self.null_interferer)
        if self.null_interferer:
            if self.type != 'mvdrSouden_ban':
                raise NotImplementedError(
                    f"bf={self.type!r} with null_interferer: only 'mvdrSouden_ban' has an "
                    'interferer-nulling form')
            if self.segment_frames is not None:
                raise NotImplementedError(
                    'null_interferer with segment_frames: the interferer-nulling beamformer has '
                    'one filter per utterance')
            m = self.null_min_mass
            if m is not None and (isinstance(m, bool)
                                  or not isinstance(m, (int, float, np.integer, np.floating))
                                  or not np.isfinite(m) or m <= 0):
                raise ValueError(f'null_min_mass={m!r}: a finite number > 0')
        elif self.null_min_mass is not None:
            raise ValueError('null_min_mass without null_interferer')
        if self.segment_frames is None:
            return
        if self.type != 'mvdrSouden_ban':
            raise NotImplementedError(
                f"bf={self.type!r} with segment_frames: only 'mvdrSouden_ban' has a "
                'segment-wise form')
        ops.check_bf_segments(self.segment_frames, self.segment_context, self.segment_min_mass)

    @property
    def segments(self):
        """The keyword arguments of the segment-wise calls in ``ops``, or None."""
        if self.segment_frames is None:
            return None
        return dict(segment_frames=self.segment_frames, segment_context=self.segment_context,
                    min_mass=self.segment_min_mass)

    @property
    def wpd(self):
        """The keyword arguments of the WPD calls in ``ops`` (types 'wpdSouden' /
        'wpdSouden_ban'), or None."""
        if self.type not in ops.WPD_BF_TYPES:
            return None
        return dict(taps=self.wpd_taps, delay=self.wpd_delay, iterations=self.wpd_iterations,
                    power_floor=self.wpd_power_floor, ban=ops.WPD_BF_TYPES[self.type])

    @property
    def online_settings(self):
        """The keyword arguments of the online calls in ``ops``, or None."""
        if not self.online:
            return None
        return dict(forget=self.forget, loading=self.loading)

    def __call__(self, Obs, target_mask, distortion_mask, debug=False, *, interferer_mask=None,
                 noise_mask=None, raw_obs=None, frame_gate=None):
        """``interferer_mask`` (with ``null_interferer``): the competing talker's mask, a part
        of ``distortion_mask``; ``noise_mask``: the rest of it (None: their difference).
        ``raw_obs`` (the WPD types): the STFT before WPE, which the WPD dereverberates itself
        (None: ``Obs``); ``frame_gate`` (T,) of 0 / 1: frames outside its statistics."""
        bf = self.type
        if self.wpd is not None:
            if interferer_mask is not None or noise_mask is not None:
                raise ValueError('interferer_mask / noise_mask without null_interferer')
            from pb_chime5_amd.speech_enhancement.beamforming_wrapper import (
                beamform_wpd_souden_from_masks)
            X_hat = beamform_wpd_souden_from_masks(
                Obs if raw_obs is None else raw_obs, target_mask, frame_gate=frame_gate,
                **self.wpd)
        elif raw_obs is not None or frame_gate is not None:
            raise ValueError(f'raw_obs / frame_gate with bf={bf!r}: only the WPD types read them')
        elif self.null_interferer:
            if interferer_mask is None:
                raise ValueError('null_interferer: the beamformer needs interferer_mask')
            if noise_mask is None:
                noise_mask = distortion_mask - interferer_mask
            min_mass = self.null_min_mass
            if min_mass is None:
                min_mass = 2 * np.shape(Obs)[0]
            X_hat = ops.lcmv_souden_from_masks(
                Obs, target_mask, interferer_mask, noise_mask, ban=True, min_mass=min_mass)
        elif interferer_mask is not None or noise_mask is not None:
            raise ValueError('interferer_mask / noise_mask without null_interferer')
        elif self.online:       # ('mvdrSouden_ban', checked above; the window's reference channel)
            X_hat = ops.mvdr_souden_online_from_masks(
                Obs, target_mask, distortion_mask, ban=True, ref_channel=-1,
                **self.online_settings)
        elif bf == 'mvdrSouden_ban':
            from pb_chime5_amd.speech_enhancement.beamforming_wrapper import (
                beamform_mvdr_souden_from_masks)
            X_hat = beamform_mvdr_souden_from_masks(
                Y=Obs, X_mask=target_mask, N_mask=distortion_mask, ban=True,
                segment_frames=self.segment_frames, segment_context=self.segment_context,
                segment_min_mass=self.segment_min_mass)
        elif bf == 'gev_ban':
            # not selectable in the reference's Beamformer.__call__ (core.py:246-266); the
            # GEV code path exists beside it (beamforming_wrapper.py:192-208)
            from pb_chime5_amd.speech_enhancement.beamforming_wrapper import (
                beamform_gev_from_masks)
            X_hat = beamform_gev_from_masks(Y=Obs, X_mask=target_mask, N_mask=distortion_mask,
                                            ban=True)
        elif bf == 'ch2':
            X_hat = Obs[2]
        elif bf == 'sum':
            X_hat = np.sum(Obs, axis=0)
        else:
            raise NotImplementedError(bf)

        if self.postfilter is None:
            pass
        elif self.postfilter == 'mask_mul':
            X_hat = X_hat * target_mask
        else:
            raise NotImplementedError(self.postfilter)
        if debug:
            self.locals = locals()
        return X_hat


def _garbage_tracks(garbage_class):
    """The activity keys ``Activity.garbage_class`` adds (activity._add_garbage): 'Noise' for
    True / False, 'Noise0' ... for a positive int, none for None."""
    if garbage_class is True or garbage_class is False:
        return {'Noise'}
    if garbage_class is None:
        return set()
    return {f'Noise{i}' for i in range(int(garbage_class))}


@dataclass
class Enhancer:
    """core.py:281-571."""
    wpe_block: WPE
    activity: Activity
    gss_block: GSS
    bf_block: Beamformer

    bf_drop_context: bool

    stft_size: int
    stft_shift: int
    stft_fading: bool

    context_samples: int
    multiarray: bool
    reference_array: [None, str]

    device_id: int = None
    iterator_factory: object = field(default=None, repr=False)
    inflight: int = 2        # utterances kept in flight per GPU by enhance_session
    loaders: int = 3         # host threads that read the next examples' audio ahead of the GPU
    # WPE per microphone array (WPE.__call__(Obs, stack=False), core.py:71-79), then GSS and the
    # beamformer on all channels together; only with a multiarray mode and WPE (otherwise no
    # effect).  Off: the reference's joint WPE over all channels.
    wpe_per_array: bool = False
    # Envelope-variance channel selection ahead of WPE (an addition, see ops.select_channels):
    # keep the ``channel_keep`` channels (an int: a count, a float in (0, 1]: a share of the
    # channels of each utterance) that a mel bank of ``channel_bands`` filters ranks best.
    # None: every channel, the reference's pipeline.
    channel_keep: object = None
    channel_bands: int = 40

    def __post_init__(self):
        if self._bf_wpd() is not None:      # (the one place that validates; raises for combinations)
            ops.check_bf_wpd(**self._bf_wpd(), channel_keep=self.channel_keep)
            if self._wpe_online() is not None:
                raise NotImplementedError(
                    f'wpe_online with bf={self.bf_block.type!r}: the WPD beamformer dereverberates '
                    'with an offline WPE step of its own')
        if self._bf_online() is not None and self.channel_keep is not None:
            raise NotImplementedError(
                'bf_online with channel_keep: the online beamformer has no selection')
        if self._gss_online() is not None:
            for name, on in (('bf_segment_frames', self._bf_segments() is not None),
                             ('bf_null_interferer', self._bf_null()),
                             ('channel_keep', self.channel_keep is not None),
                             (f'bf={getattr(self.bf_block, "type", None)!r}',
                              self._bf_wpd() is not None)):
                if on:
                    raise NotImplementedError(
                        f'gss_online with {name}: the online mixture model feeds the whole-window '
                        'and the online MVDR on all channels only')
        if self.channel_keep is None:
            return
        ops.check_channel_keep(self.channel_keep)
        ops.check_channel_bands(self.channel_bands)
        if self.wpe_per_array:
            raise NotImplementedError(
                'channel_keep with wpe_per_array=True: a selection breaks the equal arrays of '
                'the per-array WPE')
        if getattr(self.bf_block, 'type', None) == 'ch2':
            raise NotImplementedError(
                "channel_keep with bf='ch2': 'ch2' names a physical channel")
        if self._bf_segments() is not None:
            raise NotImplementedError(
                'channel_keep with bf_segment_frames: the segment-wise beamformer has no '
                'selection')
        if self._bf_null():
            raise NotImplementedError(
                'channel_keep with bf_null_interferer: the interferer-nulling beamformer has no '
                'selection')

    def _channel_select(self):
        """The `ops.ChannelSelect` of this enhancer (one object: its band table is copied to a
        GPU once), or None without ``channel_keep``."""
        if self.channel_keep is None:
            return None
        sel = getattr(self, '_channel_select_cache', None)
        key = (self.channel_keep, self.channel_bands, self.stft_size)
        if sel is None or sel[0] != key:
            sel = self._channel_select_cache = (key, ops.ChannelSelect(
                self.channel_keep, self.stft_size // 2 + 1, bands=self.channel_bands))
        return sel[1]

    # channels per array that each multiarray mode loads (core.py:428-441)
    _ARRAY_CHANNELS = {True: 4, 'outer_array_mics': 2, 'first_array_mics': 1}

    def wpe_arrays(self, ex, num_channels):
        """The number of arrays A of the per-array WPE for an observation of ``num_channels``
        channels (1 = one joint WPE): the arrays of ``ex['audio_path']['observation']`` (a
        flat list of channel files, as in the RTTM database, or no example: num_channels / C),
        C channels each as the multiarray mode loads them.  ValueError when A C differs from
        num_channels."""
        if not self.wpe_per_array or self.wpe_block is None or self.multiarray is False:
            return 1
        if self.multiarray not in self._ARRAY_CHANNELS:
            raise ValueError(self.multiarray)
        C = self._ARRAY_CHANNELS[self.multiarray]
        observation = (ex or {}).get('audio_path', {})
        observation = observation.get('observation') if isinstance(observation, dict) else None
        A = len(observation) if isinstance(observation, dict) else num_channels // C
        if A * C != num_channels:
            raise ValueError(f'wpe_per_array: {num_channels} channels are not {A} arrays of {C} '
                             f'(multiarray={self.multiarray!r})')
        return A

    # ------------------------------------------------------------------ STFT
    def stft(self, x):
        return ops.stft(x, size=self.stft_size, shift=self.stft_shift,
                        fading=self.stft_fading, ctx=self._ctx())

    def istft(self, X):
        return ops.istft(X, size=self.stft_size, shift=self.stft_shift,
                         fading=self.stft_fading, ctx=self._ctx())

    def _ctx(self):
        from pb_chime5_amd._capi import default_context
        return default_context(self.device_id)

    # ------------------------------------------------------------------ sessions
    @property
    def db(self):
        return self.activity.db

    def get_iterator(self, session_id):
        """core.py:323-331.  ``iterator_factory(session_ids, context_samples)`` (an
        addition) replaces the JSON database as the example source when given."""
        if self.iterator_factory is not None:
            return self.iterator_factory(session_id, self.context_samples)
        return self.db.get_iterator_for_session(
            session_id, audio_read=False, adjust_times=True,
            drop_unknown_target_speaker=True, context_samples=self.context_samples,
            equal_start_context=True)

    def enhance_session(self, session_ids, audio_dir, dataset_slice=False,
                        audio_dir_exist_ok=False, refined_rttm=False):
        """core.py:333-394; examples are sharded over the visible GPUs by
        pb_chime5_amd.parallel when more than one process is running.
        ``refined_rttm=True`` (an addition): every utterance also writes
        ``<example_id>.rttm`` next to its WAV -- the frames inside the utterance that the
        posteriors give the target speaker (`enhance_example_activity`), file id = the session
        id.  One file per utterance and no merge step (`from_rttm` takes a list of files and
        unites overlapping lines); such a session runs one utterance at a time."""
        from pb_chime5_amd import parallel
        self._refuse('enhance_session', ('bf_null_interferer',))
        if refined_rttm:
            self._refuse('enhance_session(refined_rttm=True)', self._NOT_WITH_ACTIVITY)
        audio_dir = Path(audio_dir)
        it = self.get_iterator(session_ids)

        if parallel.is_master():
            audio_dir.mkdir(exist_ok=audio_dir_exist_ok)
            for dataset in set(mapping.session_to_dataset.values()):
                (audio_dir / dataset).mkdir(exist_ok=audio_dir_exist_ok)
        parallel.barrier()

        if dataset_slice is not False:
            if dataset_slice is True:
                it = it[:2]
            elif isinstance(dataset_slice, int):
                it = it[:dataset_slice]
            elif isinstance(dataset_slice, slice):
                it = it[dataset_slice]
            else:
                raise ValueError(dataset_slice)

        costs = None
        if parallel.world_size() > 1:
            # longest first, so that the last utterances handed out are short ones
            def samples(tree):
                if isinstance(tree, dict):
                    return max((samples(v) for v in tree.values()), default=0)
                return int(tree)
            costs = [samples(ex['num_samples']) for ex in it]
        self._enhance_and_write(parallel.split_managed(it, costs=costs), audio_dir,
                                refined_rttm=refined_rttm)
        # (split_managed ends without a barrier: this rank's pipeline has drained by now)
        parallel.barrier()

    def _write(self, ex, x_hat, audio_dir):
        if not np.all(np.isfinite(x_hat)):
            # Same outcome as the reference: e.g. an utterance so close to the end of the
            # recording that the nominal end context (core.py:217-222 takes it from the
            # example, not from the audio actually read) zeroes every frame of the target
            # mask -> Phi_X = 0 -> 0 / 0 in the blind analytic normalisation.
            import warnings
            warnings.warn(f'{ex.get("example_id")}: the enhanced signal is not finite')
        dataset = mapping.session_to_dataset[ex['session_id']]
        if x_hat.ndim == 1:
            dump_audio(x_hat, Path(audio_dir) / f'{dataset}' / f'{ex["example_id"]}.wav')
        else:
            raise NotImplementedError(x_hat.shape)

    def _write_rttm(self, ex, intervals, audio_dir):
        dataset = mapping.session_to_dataset[ex['session_id']]
        pact.write_rttm(Path(audio_dir) / f'{dataset}' / f'{ex["example_id"]}.rttm',
                        ex['session_id'], {ex['speaker_id']: intervals})

    def _enhance_and_write(self, examples, audio_dir, refined_rttm=False):
        """Enhance the examples and write ``audio_dir/<dataset>/<example_id>.wav``.
        With the fused device pipeline ``self.inflight`` (default 2) utterances are kept
        in flight on separate HIP streams: the host loads the next example's audio
        while the GPU works, and one utterance's latency-bound kernels overlap the
        other's compute-bound ones.  Results are identical to the one-at-a-time loop."""
        # (a segment-wise beamformer has no pipelined pcm16 entry point: one at a time; neither
        # has the posterior activity of a refined RTTM)
        # (nor has the WPD: the pipelined path is out of its scope)
        # (nor has the online WPE, nor the online beamformer, nor the online mixture model)
        if (self.inflight <= 1 or not self._fusable() or self._bf_segments() is not None
                or refined_rttm or self._bf_wpd() is not None
                or self._wpe_online() is not None or self._bf_online() is not None
                or self._gss_online() is not None):
            for ex in examples:
                try:
                    if refined_rttm:
                        x_hat, intervals = self.enhance_example_activity(ex)
                        self._write(ex, x_hat, audio_dir)
                        self._write_rttm(ex, intervals, audio_dir)
                        continue
                    self._write(ex, self.enhance_example(ex), audio_dir)
                except Exception:
                    print('ERROR: Failed example:', ex.get('example_id'))
                    raise
            return
        # Host side of the session (replaces core.py:363-392 + io/audioread.py): `loaders`
        # threads prepare the next examples -- WAV slices by preadv straight into page-locked
        # (D, N) int16 rows, activity tracks sliced into uint8 rows; no float conversion, no
        # stacking copies (the STFT kernel converts the PCM) --, this thread starts the DMAs
        # and the kernels (nothing in it waits for the GPU except pop()), fetches only the
        # samples that survive the context trim, and a writer thread normalises and writes the
        # WAV files.  File reads, memcpy and the ctypes calls release the GIL.
        import threading
        import time
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        from pb_chime5_amd.io.wav_slices import WavSliceReader

        loaders = max(int(self.loaders), 1)
        pipe = ops.UtterancePipeline(self._params(), depth=self.inflight, first_ctx=self._ctx(),
                                     staging_sets=self.inflight + loaders + 1)
        reader = WavSliceReader()
        clock = self.session_clock = dict(
            examples=0, loader_threads=loaders, wall_s=0.0, host_wait_s=0.0, enqueue_s=0.0,
            gpu_wait_s=0.0, write_wait_s=0.0, loader_busy_s=0.0, writer_busy_s=0.0)
        lock = threading.Lock()
        t_begin = time.perf_counter()

        def prepare(ex):
            staging = pipe.acquire_staging()
            if staging is None:
                raise RuntimeError('the session was aborted')
            t0 = time.perf_counter()
            try:
                meta = self._prepare_into(ex, staging, reader)
            except BaseException:
                pipe.release_staging(staging)
                raise
            with lock:
                clock['loader_busy_s'] += time.perf_counter() - t0
            return (staging,) + meta

        def write(ex, x_hat):
            t0 = time.perf_counter()
            self._write(ex, x_hat, audio_dir)
            with lock:
                clock['writer_busy_s'] += time.perf_counter() - t0

        loader = ThreadPoolExecutor(max_workers=loaders, thread_name_prefix='gss-loader')
        writer = ThreadPoolExecutor(max_workers=1, thread_name_prefix='gss-writer')
        ahead = deque()
        writes = deque()
        source = iter(examples)

        def refill():
            while len(ahead) < loaders:
                try:
                    ex = next(source)
                except StopIteration:
                    return
                ahead.append((ex, loader.submit(prepare, ex)))

        def pop_and_write():
            t0 = time.perf_counter()
            done, x_hat = pipe.pop()
            clock['gpu_wait_s'] += time.perf_counter() - t0
            writes.append((done, writer.submit(write, done, x_hat)))
            while len(writes) > 8 or (writes and writes[0][1].done()):
                ex_w, fut = writes.popleft()
                t0 = time.perf_counter()
                try:
                    fut.result()
                except Exception:
                    print('ERROR: Failed example:', ex_w.get('example_id'))
                    raise
                clock['write_wait_s'] += time.perf_counter() - t0

        try:
            refill()
            while ahead:
                ex, future = ahead.popleft()
                t0 = time.perf_counter()
                try:
                    prepared = future.result()
                except Exception:
                    print('ERROR: Failed example:', ex.get('example_id'))
                    raise
                clock['host_wait_s'] += time.perf_counter() - t0
                refill()
                if pipe.full():
                    pop_and_write()
                t0 = time.perf_counter()
                try:
                    pipe.enqueue_staged(ex, *prepared, wpe_arrays=self.wpe_arrays(
                        ex, prepared[0].obs.shape[0]), channel_select=self._channel_select())
                except BaseException:
                    pipe.release_staging(prepared[0])
                    raise
                clock['enqueue_s'] += time.perf_counter() - t0
                clock['examples'] += 1
            while len(pipe):
                pop_and_write()
            t0 = time.perf_counter()
            while writes:
                ex_w, fut = writes.popleft()
                try:
                    fut.result()
                except Exception:
                    print('ERROR: Failed example:', ex_w.get('example_id'))
                    raise
            clock['write_wait_s'] += time.perf_counter() - t0
        finally:
            # wake loader threads that wait for a free staging set (after an error in this
            # thread nobody pops any more); their examples fail with the RuntimeError below
            for _ in range(loaders):
                pipe.release_staging(None)
            loader.shutdown(wait=True, cancel_futures=True)
            writer.shutdown(wait=True, cancel_futures=True)
            pipe.close()
            reader.close()
            clock['wall_s'] = time.perf_counter() - t_begin

    # -- the clock of an example: overridden by the CHiME-6 front doors (one clock for all)
    def _audio_span(self, ex, array):
        return ex['start']['observation'][array], ex['end']['observation'][array]

    def _activity_span(self, ex):
        """(speaker -> track, start, nominal end) of the tracks that guide this example."""
        reference_array = self._reference_array(ex)
        start, end = self._audio_span(ex, reference_array)
        return self.activity[ex['session_id']][reference_array], start, end

    def _keep_range(self, ex):
        """The samples of x_hat that `_trim_context` keeps (None: all)."""
        if self.context_samples <= 0:
            return None
        reference_array = self._reference_array(ex)
        keep_from = (ex['start_orig']['observation'][reference_array]
                     - ex['start']['observation'][reference_array])
        return keep_from, keep_from + ex['num_samples_orig']['observation'][reference_array]

    fast_loader = True      # False: always go through _prepare_example (RTTM front door)

    def _prepare_into(self, ex, staging, reader):
        """Host side of enhance_example (core.py:396-490) for the session driver: fills
        ``staging.obs`` (D, N) int16 with the PCM samples of the selected channels (arrays cut
        to the shortest) and ``staging.act`` (K, N_act) uint8 with the activity tracks; returns
        (target index, start context, end context, kept sample range).  One mono file per
        microphone (CHiME-5 / 6) is read slice by slice straight into the rows; anything else
        goes through `_prepare_example` and one copy."""
        speaker_id = ex['speaker_id']
        plan = None
        if self.fast_loader:
            observation = ex['audio_path']['observation']
            if self.multiarray is False:
                arrays, select = [self._reference_array(ex)], None
            elif self.multiarray is True:
                arrays, select = sorted(observation.keys()), None
            elif self.multiarray == 'outer_array_mics':
                arrays, select = sorted(observation.keys()), (0, -1)
            elif self.multiarray == 'first_array_mics':
                arrays, select = sorted(observation.keys()), (0,)
            else:
                raise ValueError(self.multiarray)
            plan, lengths = [], []
            for array in arrays:
                paths = observation[array]
                start, stop = self._audio_span(ex, array)
                if not isinstance(paths, (list, tuple)) or any(
                        reader.info(p).channels != 1 for p in paths):
                    plan = None
                    break
                n_array = {reader.slice_length(p, start, stop) for p in paths}
                assert len(n_array) == 1, (array, n_array)   # np.array([...]) needs equal lengths
                lengths.append(n_array.pop())
                chosen = paths if select is None else [paths[i] for i in select]
                plan.extend((p, start) for p in chosen)

        if plan is None:
            obs, ex_array_activity, _ = self._prepare_example(ex, dtype=np.int16)
            keys = tuple(ex_array_activity.keys())
            activity = np.array(list(ex_array_activity.values()))
            rows, act = staging.shape(*obs.shape, *activity.shape)
            rows[...] = obs
            act[...] = activity != 0
        else:
            tracks, a, b = self._activity_span(ex)
            keys = tuple(tracks.keys())
            spans = [(a, min(b, len(arr))) for arr in tracks.values()]
            n_act = {hi - lo for lo, hi in spans}
            assert len(n_act) == 1, n_act                    # np.array(list(...)) likewise
            rows, act = staging.shape(len(plan), min(lengths), len(keys), n_act.pop())
            for row, (path, start) in zip(rows, plan):
                reader.read_into(path, start, row)
            for row, arr, (lo, hi) in zip(act, tracks.values(), spans):
                if hasattr(arr, 'slice_into'):
                    arr.slice_into(lo, hi, row)
                else:
                    row[:] = np.asarray(arr[lo:hi]) != 0

        start_ctx = end_ctx = 0
        if self.bf_drop_context:
            start_ctx, end_ctx = start_end_context_samples(ex)
        return keys.index(speaker_id), start_ctx, end_ctx, self._keep_range(ex)

    # ------------------------------------------------------------------ examples
    def enhance_example(self, ex, debug=False):
        """core.py:396-512."""
        obs, ex_array_activity, speaker_id = self._prepare_example(ex)
        x_hat = self.enhance_observation(
            obs, ex_array_activity=ex_array_activity, speaker_id=speaker_id, ex=ex,
            debug=debug)
        x_hat = self._trim_context(x_hat, ex)
        if debug:
            self.enhance_example_locals = dict(
                ex=ex, obs=obs, ex_array_activity=ex_array_activity, speaker_id=speaker_id,
                x_hat=x_hat)
        return x_hat

    def _reference_array(self, ex):
        reference_array = self.reference_array
        if reference_array is None:
            try:
                reference_array = ex['reference_array']
            except KeyError:
                raise RuntimeError(
                    'Failed to get the "reference_array" from the example.\n'
                    'Probably you tried to enhance the "train" dataset.\n'
                    'Train has no "reference_array".\n'
                    'You can set a "reference_array" with get_enhancer('
                    'reference_array="U06").\n'
                    'In case of multiarray, the reference array is used for the '
                    'projection of the human annotations.') from None
        return reference_array

    def _prepare_example(self, ex, dtype=np.float64, with_activity=True):
        """Host side of enhance_example (core.py:396-490): activity slices of the
        reference array, channel selection, arrays cut to the shortest.  ``dtype=np.int16``
        keeps the PCM samples as stored (the session driver converts on the device).
        ``with_activity=False`` (the annotation-free methods): only the audio is loaded -- no
        annotation and no target speaker is looked up -- and (obs, None, None) returned."""
        reference_array = self._reference_array(ex)
        ex_array_activity = speaker_id = None
        if with_activity:
            session_id = ex['session_id']
            speaker_id = ex['speaker_id']
            array_start = ex['start']['observation'][reference_array]
            array_end = ex['end']['observation'][reference_array]
            ex_array_activity = {
                k: arr[array_start:min(array_end, len(arr))]
                for k, arr in self.activity[session_id][reference_array].items()
            }

        def load_arrays(select):
            arrays = [
                load_audio(ex['audio_path']['observation'][array],
                           start=ex['start']['observation'][array],
                           stop=ex['end']['observation'][array], dtype=dtype)
                for array in sorted(ex['audio_path']['observation'].keys())
            ]
            # The context does not consider the end of an utterance: arrays can
            # differ in length, cut to the shortest.
            assert {v.ndim for v in arrays} == {2}, [v.shape for v in arrays]
            time_length = min(v.shape[-1] for v in arrays)
            return morph('ACN->A*CN', np.array(
                [select(v)[..., :time_length] for v in arrays]))

        if self.multiarray is True:
            obs = load_arrays(lambda v: v)
        elif self.multiarray == 'outer_array_mics':
            obs = load_arrays(lambda v: v[(0, -1), :])
        elif self.multiarray == 'first_array_mics':
            obs = load_arrays(lambda v: v[(0,), :])
        elif self.multiarray is False:
            obs = load_audio(ex['audio_path']['observation'][reference_array],
                             start=ex['start']['observation'][reference_array],
                             stop=ex['end']['observation'][reference_array], dtype=dtype)
        else:
            raise ValueError(self.multiarray)
        return obs, ex_array_activity, speaker_id

    def _trim_context(self, x_hat, ex):
        """core.py:500-505: cut the enhanced signal back to the original utterance."""
        if self.context_samples > 0:
            reference_array = self._reference_array(ex)
            start_orig = ex['start_orig']['observation'][reference_array]
            start = ex['start']['observation'][reference_array]
            start_context = start_orig - start
            num_samples_orig = ex['num_samples_orig']['observation'][reference_array]
            x_hat = x_hat[..., start_context:start_context + num_samples_orig]
        return x_hat

    # ------------------------------------------------------------------ the hot path
    def _fusable(self):
        return (
            (self.wpe_block is None or type(self.wpe_block) is WPE)
            and type(self.gss_block) is GSS and type(self.bf_block) is Beamformer
        )

    def _bf_segments(self):
        """The beamformer's segment settings (``Beamformer.segments``) or None."""
        return getattr(getattr(self, 'bf_block', None), 'segments', None)

    def _bf_null(self):
        """Whether the beamformer nulls an interferer (``Beamformer.null_interferer``)."""
        return bool(getattr(getattr(self, 'bf_block', None), 'null_interferer', False))

    def _bf_wpd(self):
        """The WPD settings of the beamformer (``Beamformer.wpd``) or None."""
        return getattr(getattr(self, 'bf_block', None), 'wpd', None)

    def _bf_online(self):
        """The online settings of the beamformer (``Beamformer.online_settings``) or None."""
        return getattr(getattr(self, 'bf_block', None), 'online_settings', None)

    def _gss_online(self):
        """The online settings of the mixture model (``GSS.online_settings``) or None."""
        return getattr(getattr(self, 'gss_block', None), 'online_settings', None)

    def _wpe_online(self):
        """The forgetting factor of an online WPE block (``WPE.online``) or None."""
        block = getattr(self, 'wpe_block', None)
        return block.alpha if getattr(block, 'online', False) else None

    # What a method that is not built for an option says: option -> (the probe or field that is
    # neither None nor False when the option is on, the sentence after "<method> with <option>: ").
    # A method names the options it refuses as a tuple of these keys, in the order in which they
    # are looked at: the first one that is on speaks.
    _REFUSALS = {
        'bf_segment_frames': ('_bf_segments',
                              'the segment-wise beamformer is built for enhance_observation only'),
        'bf_null_interferer': ('_bf_null', 'the interferer-nulling beamformer is built for '
                                           'enhance_observation only'),
        'channel_keep': ('channel_keep', 'the channel selection is built for enhance_observation '
                                         'and enhance_session only'),
        'bf=wpd': ('_bf_wpd', 'the WPD beamformer is built for enhance_observation, '
                              'enhance_example and enhance_session only'),
        'bf_online': ('_bf_online', 'the online beamformer is built for enhance_observation, '
                                    'enhance_example and enhance_session only'),
        'gss_online': ('_gss_online', 'the online mixture model is built for enhance_observation, '
                                      'enhance_example and enhance_session only'),
        'wpe_online': ('_wpe_online', 'the online WPE is built for enhance_observation, '
                       'enhance_example, enhance_session and the annotation-free methods only'),
        'wpe_per_array': ('wpe_per_array', 'the annotation-free path runs one joint WPE'),
    }
    # the posterior activity is built for the whole-window MVDR on all channels
    _NOT_WITH_ACTIVITY = ('bf_segment_frames', 'bf_null_interferer', 'channel_keep', 'bf=wpd',
                          'bf_online', 'gss_online', 'wpe_online')
    # the annotation-free path for the whole-window beamformers on all channels after one joint WPE
    _NOT_WITH_BLIND = ('bf_segment_frames', 'bf_null_interferer', 'channel_keep', 'bf=wpd',
                       'bf_online', 'gss_online', 'wpe_per_array')
    # the guided and the multi-speaker calls for the whole-window MVDR on all channels
    _NOT_WITH_GUIDED = _NOT_WITH_SPEAKERS = (
        'bf_segment_frames', 'bf=wpd', 'bf_online', 'gss_online', 'wpe_online',
        'bf_null_interferer', 'channel_keep')

    def _refuse(self, what, options):
        """NotImplementedError in the name of the method ``what`` for the first of ``options``
        (keys of `_REFUSALS`) that is on."""
        for option in options:
            probe, sentence = self._REFUSALS[option]
            on = getattr(self, probe)
            if (on() if callable(on) else on) not in (None, False):
                if option == 'bf=wpd':
                    option = f'bf={self.bf_block.type!r}'
                raise NotImplementedError(f'{what} with {option}: {sentence}')

    @staticmethod
    def _no_posterior_activity(what, posterior_activity):
        if posterior_activity:
            raise NotImplementedError(
                f'{what} with posterior_activity: the scores are built for '
                'enhance_observation_activity (one target) only')

    def interferer_candidates(self, ex_array_activity, speaker_id):
        """The classes the interferer of ``speaker_id`` is chosen from, as indices into the
        activity keys: every key but the target and the garbage tracks that
        ``Activity.garbage_class`` adds."""
        garbage = _garbage_tracks(getattr(self.activity, 'garbage_class', True))
        return [i for i, k in enumerate(ex_array_activity.keys())
                if k != speaker_id and k not in garbage]

    def stream(self, num_channels, speakers=None, target=None, *, model=None, ref_channel=0,
               fused=True, targets=None, lookahead=0):
        """A `streaming.StreamingEnhancer` with this enhancer's settings: samples in and out in
        blocks of any length, the three online stages with carried states.  ``speakers``: the
        names of the classes in activity order (``target`` one of them; `process` then also
        takes the activity as a dict of per-sample tracks) or a class count (``target`` an
        index); or ``model=`` a fitted `CACGMM` for an unguided stream (``target`` an index).
        ``targets`` in the place of ``target``: several of them, names or indices like it, all
        extracted in one pass -- `process` and `flush` then return (S, m).  ``lookahead``: the
        frames the beamformer's filter looks ahead (`StreamingEnhancer`; a stream's setting only:
        `get_enhancer` has no such keyword and the windowed path no such form).
        NotImplementedError, naming the setting, for everything the stream is not built for: it
        needs gss_online and bf_online (bf='mvdrSouden_ban'), wpe_online wherever WPE runs and
        stft_fading, and has no channel selection, segments, interferer nulling or WPD."""
        from .streaming import StreamingEnhancer

        def refuse(setting, why):
            raise NotImplementedError(f'stream with {setting}: {why}')
        if not self._fusable():
            refuse('custom blocks', 'the stream runs the library\'s own online stages')
        if self._bf_wpd() is not None:
            refuse(f'bf={self.bf_block.type!r}', 'the WPD beamformer has no online form')
        if self.bf_block.type != 'mvdrSouden_ban':
            refuse(f'bf={self.bf_block.type!r}', "only 'mvdrSouden_ban' has an online form")
        if self.channel_keep is not None:
            refuse('channel_keep', 'the selection ranks the channels of a whole window')
        if self._bf_segments() is not None:
            refuse('bf_segment_frames', 'the segment-wise beamformer needs the whole window')
        if self._bf_null():
            refuse('bf_null_interferer', 'the interferer-nulling beamformer needs the whole window')
        if not self.stft_fading:
            refuse('stft_fading=False', 'a stream is the faded STFT')
        if self._gss_online() is None:
            refuse('gss_online=False', 'the iterated EM needs the whole window')
        if self._bf_online() is None:
            refuse('bf_online=False', 'the whole-window beamformer needs the whole window')
        if self.wpe_block is not None and self._wpe_online() is None:
            refuse('wpe_online=False', 'the offline WPE needs the whole window')
        names = None
        if model is None:
            if speakers is None:
                raise ValueError('speakers: the names in activity order or a class count '
                                 '(or model=)')
            if ops._is_integer(speakers):
                num_classes = int(speakers)
            else:
                names = list(speakers)
                num_classes = len(names)
                if targets is not None:
                    if isinstance(targets, (str, bytes)) or not hasattr(targets, '__iter__'):
                        raise ValueError(f'targets={targets!r}: a sequence of names of '
                                         f'speakers={names!r}')
                    targets = list(targets)
                    for name in targets:
                        if name not in names:
                            raise ValueError(f'targets: {name!r} is not one of speakers={names!r}')
                    targets = [names.index(name) for name in targets]
                else:
                    if target not in names:
                        raise ValueError(f'target={target!r} is not one of speakers={names!r}')
                    target = names.index(target)
        else:
            if speakers is not None:
                raise ValueError('speakers with model=: the stream is unguided')
            num_classes = None
        if targets is not None and target is not None:
            raise ValueError('targets together with target: one of the two')
        if target is None and targets is None:
            raise ValueError('target: the class to extract')
        which = dict(target=target) if targets is None else dict(targets=targets)
        w, gss, bf = self.wpe_block, self._gss_online(), self._bf_online()
        return StreamingEnhancer(
            num_channels, num_classes, model=model, ref_channel=ref_channel, **which,
            stft_size=self.stft_size, stft_shift=self.stft_shift, wpe=w is not None,
            wpe_taps=w.taps if w else 10, wpe_delay=w.delay if w else 2,
            wpe_alpha=w.alpha if w else ops.WPE_ONLINE_ALPHA,
            wpe_arrays=self.wpe_arrays(None, num_channels) if w else 1,
            gss_forget=gss['forget'], gss_prior_mass=gss['prior_mass'], bf_forget=bf['forget'],
            bf_loading=bf['loading'], postfilter=self.bf_block.postfilter, fused=fused,
            speakers=names, lookahead=lookahead,
            ctx=self._ctx() if self.device_id is not None else None)

    def _params(self):
        w = self.wpe_block
        return ops.make_params(
            stft_size=self.stft_size, stft_shift=self.stft_shift,
            stft_fading=self.stft_fading, wpe=w is not None,
            wpe_taps=w.taps if w else 10, wpe_delay=w.delay if w else 2,
            wpe_iterations=w.iterations if w else 3,
            wpe_psd_context=w.psd_context if w else 0,
            bss_iterations=self.gss_block.iterations,
            bss_iterations_post=self.gss_block.iterations_post,
            bf_drop_context=self.bf_drop_context,
            # (the WPD travels in a descriptor of its own; its fused call takes the MVDR's code)
            bf='mvdrSouden_ban' if self._bf_wpd() is not None else self.bf_block.type,
            postfilter=self.bf_block.postfilter)

    def enhance_observation(self, obs, ex_array_activity, speaker_id, ex=None,
                            debug=False, fused=None, wpe_arrays=None):
        """core.py:514-571.  obs (D,N) float64, ex_array_activity dict
        speaker -> bool (N,), returns x_hat (N',) float64.  ``wpe_arrays``: the number of
        microphone arrays of a per-array WPE (None: `wpe_arrays(ex, D)`)."""
        if wpe_arrays is None:
            wpe_arrays = self.wpe_arrays(ex, np.shape(obs)[0])
        wpe_arrays = ops.check_wpe_arrays(wpe_arrays, np.shape(obs)[0])
        if fused is None:
            fused = self._fusable()
        if not fused:
            return self._enhance_observation_blocks(obs, ex_array_activity, speaker_id,
                                                    ex, debug, wpe_arrays)
        target_speaker_index = tuple(ex_array_activity.keys()).index(speaker_id)
        activity = np.array(list(ex_array_activity.values()))
        start_ctx = end_ctx = 0
        if self.bf_drop_context:
            start_ctx, end_ctx = start_end_context_samples(ex)
        params = self._params()     # raises NotImplementedError for unknown bf / postfilter
        segments = self._bf_segments()
        online = self._wpe_online()
        bf_online = self._bf_online()
        gss_online = self._gss_online()
        # (the refusals come before the context: a machine without a GPU says the same)
        if gss_online is not None and online is not None and bf_online is None:
            raise NotImplementedError(
                'gss_online with wpe_online but without bf_online in the fused call (the online '
                "WPE rides on the online MVDR's descriptor there): pass fused=False for the stage "
                'path')
        if online is not None and bf_online is None:
            # (the fused online call takes no second descriptor; the stage path combines)
            for name, on in (('bf_segment_frames', segments is not None),
                             ('bf_null_interferer', self._bf_null()),
                             ('channel_keep', self.channel_keep is not None)):
                if on:
                    raise NotImplementedError(
                        f'wpe_online with {name} in the fused call: pass fused=False for the '
                        'stage path')
        # one utterance at a time (this method is the loop body of core.py:363-392): the fused
        # call may put half of the WPE stage's frequencies on the context's second stream
        ctx = self._ctx()
        ctx.set_utterances_in_flight(1)
        select = self._channel_select()
        try:
            if gss_online is not None:
                # (every online stage in one call: the MVDR's descriptor carries the WPE's alpha)
                bf_kw = {} if bf_online is None else dict(
                    bf_online=True, bf_forget=bf_online['forget'], bf_loading=bf_online['loading'],
                    ref_channel=-1, wpe_online=online is not None,
                    wpe_alpha=ops.WPE_ONLINE_ALPHA if online is None else online)
                res = ops.enhance_observation_gss_online(
                    obs, activity, target_speaker_index, start_ctx, end_ctx, params=params,
                    debug=debug, ctx=ctx, wpe_arrays=wpe_arrays, **gss_online, **bf_kw)
            elif bf_online is not None:
                # (both online stages in one call: the descriptor carries the WPE's alpha)
                res = ops.enhance_observation_bf_online(
                    obs, activity, target_speaker_index, start_ctx, end_ctx, params=params,
                    debug=debug, ctx=ctx, wpe_arrays=wpe_arrays, ref_channel=-1,
                    wpe_online=online is not None,
                    wpe_alpha=ops.WPE_ONLINE_ALPHA if online is None else online, **bf_online)
            elif online is not None:
                res = ops.enhance_observation_wpe_online(
                    obs, activity, target_speaker_index, start_ctx, end_ctx, params=params,
                    debug=debug, ctx=ctx, wpe_arrays=wpe_arrays, alpha=online)
            elif self._bf_wpd() is not None:
                res = ops.enhance_observation_wpd(
                    obs, activity, target_speaker_index, start_ctx, end_ctx, params=params,
                    debug=debug, ctx=ctx, wpe_arrays=wpe_arrays, **self._bf_wpd())
            elif self._bf_null():
                res = ops.enhance_observation_lcmv(
                    obs, activity, target_speaker_index, start_ctx, end_ctx, params=params,
                    debug=debug, ctx=ctx, wpe_arrays=wpe_arrays,
                    candidates=self.interferer_candidates(ex_array_activity, speaker_id),
                    min_mass=self.bf_block.null_min_mass)
            elif select is not None:
                res = ops.enhance_observation_select(
                    obs, activity, target_speaker_index, start_ctx, end_ctx, params=params,
                    debug=debug, ctx=ctx, keep=select.keep, bank=select.bank,
                    floor=select.floor)
            elif segments is not None:
                res = ops.enhance_observation_segments(
                    obs, activity, target_speaker_index, start_ctx, end_ctx, params=params,
                    debug=debug, ctx=ctx, wpe_arrays=wpe_arrays, **segments)
            else:
                res = ops.enhance_observation(
                    obs, activity, target_speaker_index, start_ctx, end_ctx, params=params,
                    debug=debug, ctx=ctx, wpe_arrays=wpe_arrays)
        finally:
            ctx.set_utterances_in_flight(0)
        if not debug:
            return res
        x_hat, details = res
        Obs = details['Obs']
        if select is not None:
            selected_channels = details['selected_channels']
        acitivity_freq = details['acitivity_freq']
        target_mask = details['target_mask']
        distortion_mask = details['distortion_mask']
        if self._bf_null():
            interferer_mask = details['interferer_mask']
            interferer_index = details['interferer']
        X_hat = details['X_hat']
        masks = details['posterior'].copy()
        if self.bf_drop_context:
            start_context_frames, end_context_frames = start_end_context_frames(
                ex, self.stft_size, self.stft_shift, self.stft_fading)
            masks[:, :start_context_frames, :] = 0
            if end_context_frames > 0:
                masks[:, -end_context_frames:, :] = 0
        self.enhance_observation_locals = locals()
        return x_hat

    def enhance_observation_activity(self, obs, ex_array_activity, speaker_id, ex=None, *,
                                     freq_weights=None, fused=None, wpe_arrays=None):
        """`enhance_observation` plus what the separation learned about the annotation: returns
        (x_hat, `posterior_activity.PosteriorActivity`) -- x_hat with the bits of
        `enhance_observation`, and for every class of ``ex_array_activity`` the power-weighted
        share of each STFT frame that the posteriors (before context zeroing) give it
        (`ops.posterior_activity`; ``freq_weights`` (F,) >= 0 weighs the frequencies).  The fused
        path is one gss_enhance_observation_activity call, the block path
        `ops.posterior_activity` on the blocks' Obs and posterior.  Not with
        ``bf_segment_frames``, ``bf_null_interferer`` or ``channel_keep``
        (NotImplementedError)."""
        self._refuse('enhance_observation_activity', self._NOT_WITH_ACTIVITY)
        freq_weights = ops.check_freq_weights(freq_weights, self.stft_size // 2 + 1)
        if wpe_arrays is None:
            wpe_arrays = self.wpe_arrays(ex, np.shape(obs)[0])
        wpe_arrays = ops.check_wpe_arrays(wpe_arrays, np.shape(obs)[0])
        keys = tuple(ex_array_activity.keys())
        target_speaker_index = keys.index(speaker_id)
        start_ctx = end_ctx = 0
        if ex is not None and 'start_orig' in ex:
            start_ctx, end_ctx = start_end_context_samples(ex)
        context_frames = [ops.samples_to_stft_frames(c, self.stft_size, self.stft_shift,
                                                     fading=self.stft_fading)
                          for c in (start_ctx, end_ctx)]
        if fused is None:
            fused = self._fusable()
        if not fused:
            blocks = self._blocks_posterior(obs, ex_array_activity, False, wpe_arrays)
            scores, power = ops.posterior_activity(blocks[0], blocks[2], freq_weights,
                                                   return_power=True, ctx=self._ctx())
            # (the context frames of the posteriors are zeroed in place from here on)
            x_hat = self._enhance_observation_blocks(obs, ex_array_activity, speaker_id, ex,
                                                     False, wpe_arrays, blocks)
        else:
            activity = np.array(list(ex_array_activity.values()))
            if not self.bf_drop_context:
                start_ctx = end_ctx = 0
            params = self._params()
            ctx = self._ctx()
            ctx.set_utterances_in_flight(1)
            try:
                x_hat, scores, power = ops.enhance_observation_activity(
                    obs, activity, target_speaker_index, start_ctx, end_ctx, params=params,
                    freq_weights=freq_weights, ctx=ctx, wpe_arrays=wpe_arrays)
            finally:
                ctx.set_utterances_in_flight(0)
        return x_hat, pact.PosteriorActivity(scores, power, keys, target_speaker_index,
                                             *context_frames)

    def enhance_example_activity(self, ex, rule=None, freq_weights=None):
        """`enhance_example` plus the target speaker's refined activity: returns (x_hat,
        intervals) -- x_hat trimmed as `enhance_example` trims it, intervals
        [(start, end), ...] where `posterior_activity.decide` (``rule``: an `ActivityRule`, None:
        its defaults) finds the speaker active, restricted to the utterance's own span (the
        context is left out), in samples of the recording on the reference array's clock."""
        self._refuse('enhance_example_activity', self._NOT_WITH_ACTIVITY)
        rule = pact.ActivityRule() if rule is None else rule
        obs, ex_array_activity, speaker_id = self._prepare_example(ex)
        x_hat, act = self.enhance_observation_activity(
            obs, ex_array_activity, speaker_id, ex=ex, freq_weights=freq_weights)
        num_samples = np.shape(obs)[-1]
        active = pact.decide(act.scores, act.power, rule)[act.target_index]
        intervals = pact.frames_to_intervals(active, self.stft_size, self.stft_shift,
                                             self.stft_fading, num_samples)
        keep = self._keep_range(ex)
        if keep is not None:
            intervals = pact.clip_intervals(intervals, *keep)
        window_start, _ = self._audio_span(ex, self._reference_array(ex))
        intervals = [(window_start + a, window_start + b) for a, b in intervals]
        return self._trim_context(x_hat, ex), intervals

    def enhance_observation_blind(self, obs, num_speakers, ex=None, *, seed=0, rule=None,
                                  debug=False, method='shared_prior', fused=False):
        """Separation without an annotation, on the stage operators: stft -> WPE -> the CACGMM
        with a frequency-shared prior from `ops.blind_initialization` with K = num_speakers + 1
        classes (`ops.cacgmm_posteriors_blind`, ``gss_block.iterations`` iterations) -> for every
        class k the masks (target k, distortion = the rest; the context frames of ``ex`` dropped
        as ``bf_drop_context`` says) -> the configured beamformer -> istft.  Returns a
        `BlindSeparation`: x_hat (K,N), the prior (K,T) -- a per-frame activity estimate of every
        class --, what `posterior_activity.decide` (``rule``: an `ActivityRule`, None: its
        defaults) makes of it, and the sample intervals of every class.  Classes carry indices,
        not speaker names, and which of them is the noise class is not decided here (the class
        with the flattest prior is a usable guess).  Not with ``bf_segment_frames``,
        ``bf_null_interferer``, ``channel_keep``, the WPD beamformers or ``wpe_per_array``
        (NotImplementedError).
        ``method='aligned'``: the per-frequency CACGMM from the same start followed by the
        permutation alignment (`ops.align_posteriors` with its default plan) in place of the
        shared prior; ``prior`` is then the aligned posteriors' mean over f, and
        ``num_speakers`` is at most 7.
        ``fused=True``: the whole window in one library call (`ops.separate_observation`,
        gss_separate_observation) instead of the stage operators -- no host round trip between
        the stages, the beamformer and the iSTFT once for all classes.  Only with
        ``method='shared_prior'`` and the offline WPE (NotImplementedError otherwise), and it
        has no context frames: with ``ex`` and ``bf_drop_context`` it raises
        NotImplementedError.  The default keeps the stage path and its bits."""
        what = 'enhance_observation_blind'
        self._refuse(what, self._NOT_WITH_BLIND)
        ops.check_blind_method(method)
        if fused:
            if method != 'shared_prior':
                raise NotImplementedError(f"{what}(fused=True) with method={method!r}: the fused "
                                          "call runs the shared prior only")
            self._refuse(f'{what}(fused=True)', ('wpe_online',))
            if not self._fusable():
                raise NotImplementedError(f'{what}(fused=True) with custom blocks')
            if self.bf_drop_context and ex is not None and 'start_orig' in ex:
                raise NotImplementedError(
                    f'{what}(fused=True) with ex and bf_drop_context: the fused call has no '
                    'context frames (fused=False drops them)')
        if (isinstance(num_speakers, bool) or not isinstance(num_speakers, (int, np.integer))
                or not 1 <= num_speakers <= 18):
            raise ValueError(f'num_speakers: {num_speakers!r} is not an integer in [1, 18]')
        rule = pact.ActivityRule() if rule is None else rule
        obs = np.asarray(obs)
        if obs.ndim != 2:
            raise ValueError(f'obs: shape {obs.shape} is not (D,N)')
        K = int(num_speakers) + 1
        iterations = self.gss_block.iterations
        ops.blind_initialization(K, 1, seed)        # (argument errors before any device work)
        if method == 'aligned' and K > 8:
            raise ValueError(f'num_speakers: {num_speakers} with method=\'aligned\': the alignment '
                             'searches all K! permutations of at most 8 classes')
        ctx = self._ctx()
        if fused:
            return self._separate_fused(obs, K, seed, rule, debug, ctx)
        Obs = self._blocks_wpe(self.stft(obs), debug, 1)
        posterior, prior = ops.cacgmm_posteriors_blind(Obs, K, iterations, seed=seed,
                                                       return_prior=True, method=method, ctx=ctx)
        _, power = ops.posterior_activity(Obs, posterior, None, return_power=True, ctx=ctx)
        active = pact.decide(prior, power, rule)
        masks = posterior.copy()
        if self.bf_drop_context and ex is not None and 'start_orig' in ex:
            start_context_frames, end_context_frames = start_end_context_frames(
                ex, stft_size=self.stft_size, stft_shift=self.stft_shift,
                stft_fading=self.stft_fading)
            masks[:, :start_context_frames, :] = 0
            if end_context_frames > 0:
                masks[:, -end_context_frames:, :] = 0
        X_hat = [self.bf_block(Obs, target_mask=masks[k],
                               distortion_mask=np.sum(np.delete(masks, k, axis=0), axis=0))
                 for k in range(K)]
        x_hat = np.stack([self.istft(X) for X in X_hat])
        num_samples = obs.shape[-1]
        intervals = [pact.frames_to_intervals(active[k], self.stft_size, self.stft_shift,
                                              self.stft_fading, num_samples) for k in range(K)]
        if debug:
            self.enhance_observation_locals = locals()
        return BlindSeparation(x_hat, prior, active, intervals)

    def _blind_params(self):
        """`_params` of the annotation-free calls: one post iteration, whatever the GSS block
        says (what `ops.cacgmm_posteriors_blind` runs)."""
        params = self._params()
        params.bss_iterations_post = 1
        return params

    def _separate_fused(self, obs, K, seed, rule, debug, ctx):
        """`enhance_observation_blind(fused=True)` after its checks."""
        params = self._blind_params()
        T = ops.stft_frames(obs.shape[-1], self.stft_size, self.stft_shift, self.stft_fading)
        init = ops.blind_initialization(K, T, seed)
        ctx.set_utterances_in_flight(1)
        try:
            res = ops.separate_observation(obs, init, params=params, debug=debug, ctx=ctx)
        finally:
            ctx.set_utterances_in_flight(0)
        x_hat, prior, power = res[:3]
        active = pact.decide(prior, power, rule)
        num_samples = obs.shape[-1]
        intervals = [pact.frames_to_intervals(active[k], self.stft_size, self.stft_shift,
                                              self.stft_fading, num_samples) for k in range(K)]
        if debug:
            details = res[3]
            self.enhance_observation_locals = locals()
        return BlindSeparation(x_hat, prior, active, intervals)

    def enhance_recording_blind(self, obs, num_speakers, *, window_samples, hop_samples, seed=0,
                                start='carry', rule=None):
        """Annotation-free separation of a whole recording in linked windows: obs (D,N) ->
        `BlindRecording`.  The recording is cut into windows of ``window_samples`` every
        ``hop_samples`` (both multiples of ``stft_shift``, ``hop < window <= 2 hop``; the last
        window runs to N; `recording.window_plan`).  Every window is one fused call
        (`enhance_observation_blind(fused=True)`, K = num_speakers + 1 <= 8 classes) whose
        posteriors stay in HBM; for every window but the first one link call
        (`ops.link_posteriors`, gss_cacgmm_link) compares them with the previous window's -- in
        that window's linked numbering -- on the frames the two share, ``stft_size / stft_shift
        - 1`` frames left out on either side (a window's zero padding stands there where its
        neighbour has samples), and the window's signals, prior and posteriors take the mapping.
        ``start='fresh'``: window w starts from ``ops.blind_initialization(K, T_w, seed + w)``;
        ``'carry'``: the first columns of that table are the previous window's linked prior on
        the shared frames (`recording.start_table`), which mostly keeps the numbering by itself.
        The windows are cross-faded on the host (`recording.stitch`: the later window's weight
        rises as ``(i + 0.5) / overlap``), the prior and the frame power the same way over
        frames, and `posterior_activity.decide` (``rule``) and `frames_to_intervals` follow as
        in the window call.

        ``mappings[w, k]`` is the class of window w's own numbering that class k of the
        recording is, ``link_scores[w, k]`` the cosine similarity that link found for it.  A
        class that is silent in an overlap cannot be linked there: its score is near 0 and its
        place in the mapping is whatever the other classes leave -- read the scores before
        trusting a class across such a window.  Nothing here decides which class is the noise or
        names a speaker.  Options as `enhance_observation_blind(fused=True)`; every argument
        error is a ValueError before any device work."""
        from pb_chime5_amd import recording
        what = 'enhance_recording_blind'
        self._refuse(what, self._NOT_WITH_BLIND + ('wpe_online',))
        if not self._fusable():
            raise NotImplementedError(f'{what} with custom blocks')
        obs = np.asarray(obs)
        if obs.ndim != 2:
            raise ValueError(f'obs: shape {obs.shape} is not (D,N)')
        D, N = obs.shape
        plan = recording.check_recording(N, num_speakers, window_samples, hop_samples,
                                         self.stft_size, self.stft_shift, start, seed,
                                         self.stft_fading)
        rule = pact.ActivityRule() if rule is None else rule
        K = int(num_speakers) + 1
        params = self._blind_params()
        frames = [ops.stft_frames(e - s, self.stft_size, self.stft_shift, True)
                  for s, e in plan.windows]
        s, e = plan.windows[0]                            # (argument errors before device work)
        ops.check_separate_args(obs[:, s:e], np.empty((K, frames[0])), params)
        ctx = self._ctx()
        ops._prepare_windows(ctx, params.stft_size, params.stft_shift, None)
        F = self.stft_size // 2 + 1
        H, L = plan.hop_frames, plan.shared_frames
        # the posteriors in HBM: the window's own numbering and the linked one, reused by turns
        own_d = ctx.empty(8 * F * K * max(frames))
        linked_d = ctx.empty(8 * F * K * max(frames))
        mapping_d, scores_d = ctx.empty(max(4 * K, 16)), ctx.empty(max(8 * K * K, 16))
        n = len(plan.windows)
        mappings = np.tile(np.arange(K), (n, 1))
        link_scores = np.full((n, K), np.nan)
        x_hats, priors, powers = [], [], []
        ctx.set_utterances_in_flight(1)
        try:
            for w, ((s, e), T_w) in enumerate(zip(plan.windows, frames)):
                init = recording.start_table(K, T_w, int(seed), w, start,
                                             priors[-1] if priors else None, H, L)
                win = ops.ResidentSeparation(ctx, obs[:, s:e], init, params,
                                             gamma_d=own_d if w else linked_d)
                win.enqueue()
                if w:
                    (pb, pe), (cb, _) = plan.link_frames
                    ops.link_posteriors_device(ctx, linked_d, frames[w - 1], pb, own_d, T_w, cb,
                                               pe - pb, F, K, mapping_d, scores_d)
                    # (the previous window's table has been read: the linked one takes its place)
                    ops.link_gather_device(ctx, own_d, F, K, T_w, mapping_d, linked_d)
                x_hat, prior, power = win.result()
                if w:
                    mappings[w] = ctx.to_host(mapping_d, (K,), np.int32)
                    S = ctx.to_host(scores_d, (K, K), np.float64)
                    link_scores[w] = S[np.arange(K), mappings[w]]
                x_hats.append(x_hat[mappings[w], :e - s])
                priors.append(prior[mappings[w]])
                powers.append(power)
        finally:
            ctx.set_utterances_in_flight(0)
        starts = [s for s, _ in plan.windows]
        frame_offsets = [w * H for w in range(n)]
        T = frame_offsets[-1] + frames[-1]
        x_hat = recording.stitch(x_hats, starts, N)
        prior = recording.stitch(priors, frame_offsets, T)
        power = recording.stitch(powers, frame_offsets, T)
        active = pact.decide(prior, power, rule)
        intervals = [pact.frames_to_intervals(active[k], self.stft_size, self.stft_shift,
                                              self.stft_fading, N) for k in range(K)]
        return BlindRecording(x_hat, prior, active, intervals, list(plan.windows), mappings,
                              link_scores)

    def enhance_example_blind(self, ex, num_speakers, **kw):
        """`enhance_observation_blind` from an example: channels, context and trimming as
        `enhance_example`; the example's activity and target speaker are not looked up (a session
        without an annotation works).  The intervals are clipped to the
        utterance's own span and count samples of the recording on the reference array's
        clock."""
        self._refuse('enhance_example_blind', self._NOT_WITH_BLIND)
        obs, _, _ = self._prepare_example(ex, with_activity=False)
        out = self.enhance_observation_blind(obs, num_speakers, ex=ex, **kw)
        keep = self._keep_range(ex)
        window_start, _ = self._audio_span(ex, self._reference_array(ex))
        intervals = []
        for row in out.intervals:
            if keep is not None:
                row = pact.clip_intervals(row, *keep)
            intervals.append([(window_start + a, window_start + b) for a, b in row])
        return BlindSeparation(self._trim_context(out.x_hat, ex), out.prior, out.active, intervals)

    def enhance_observation_guided(self, obs, frame_guidance, speaker_id, ex=None, *,
                                   initialization=None, debug=False, fused=None,
                                   wpe_arrays=None):
        """`enhance_observation` guided per STFT frame.  ``frame_guidance``: dict speaker ->
        (T,) or (T,F) array over the frames of the observation's STFT, in the key order of
        ``ex_array_activity``: zero = the speaker is off, any other value the weight of the
        speaker in the initial affiliations (diarisation posteriors, annotation confidence).
        ``initialization``: optional dict of the same shape with initial affiliations used as
        given (a neural mask estimator's output).  ``fused=False`` runs the blocks."""
        self._refuse('enhance_observation_guided', self._NOT_WITH_GUIDED)
        if wpe_arrays is None:
            wpe_arrays = self.wpe_arrays(ex, np.shape(obs)[0])
        wpe_arrays = ops.check_wpe_arrays(wpe_arrays, np.shape(obs)[0])
        if fused is None:
            fused = self._fusable()
        target_speaker_index = tuple(frame_guidance.keys()).index(speaker_id)
        acitivity_freq = np.array(list(frame_guidance.values()))
        if initialization is not None:
            if tuple(initialization.keys()) != tuple(frame_guidance.keys()):
                raise ValueError('initialization and frame_guidance name different speakers: '
                                 f'{tuple(initialization)} != {tuple(frame_guidance)}')
            initialization = np.array(list(initialization.values()))
        if not fused:
            return self._enhance_guided_blocks(obs, acitivity_freq, initialization,
                                               target_speaker_index, ex, debug, wpe_arrays)
        derived, source_active_mask = ops.guidance_from_activity(acitivity_freq)
        if initialization is None:
            initialization = derived
        start_ctx = end_ctx = 0
        if self.bf_drop_context:
            start_ctx, end_ctx = start_end_context_samples(ex)
        ctx = self._ctx()
        ctx.set_utterances_in_flight(1)
        try:
            res = ops.enhance_observation_guided(
                obs, initialization, source_active_mask, target_speaker_index, start_ctx,
                end_ctx, params=self._params(), debug=debug, ctx=ctx, wpe_arrays=wpe_arrays)
        finally:
            ctx.set_utterances_in_flight(0)
        if not debug:
            return res
        x_hat, details = res
        Obs = details['Obs']
        target_mask = details['target_mask']
        distortion_mask = details['distortion_mask']
        X_hat = details['X_hat']
        masks = details['posterior'].copy()
        if self.bf_drop_context:
            start_context_frames, end_context_frames = start_end_context_frames(
                ex, self.stft_size, self.stft_shift, self.stft_fading)
            masks[:, :start_context_frames, :] = 0
            if end_context_frames > 0:
                masks[:, -end_context_frames:, :] = 0
        self.enhance_observation_locals = locals()
        return x_hat

    def _enhance_guided_blocks(self, obs, acitivity_freq, initialization,
                               target_speaker_index, ex, debug, wpe_arrays):
        """The guided call block by block: `_enhance_observation_blocks` with the frame
        guidance in the place of the converted activity."""
        Obs = self._blocks_wpe(self.stft(obs), debug, wpe_arrays)
        masks = self.gss_block(Obs, acitivity_freq, debug=debug, initialization=initialization)
        if self.bf_drop_context:
            start_context_frames, end_context_frames = start_end_context_frames(
                ex, stft_size=self.stft_size, stft_shift=self.stft_shift,
                stft_fading=self.stft_fading)
            masks[:, :start_context_frames, :] = 0
            if end_context_frames > 0:
                masks[:, -end_context_frames:, :] = 0
        target_mask = masks[target_speaker_index]
        distortion_mask = np.sum(np.delete(masks, target_speaker_index, axis=0), axis=0)
        X_hat = self.bf_block(Obs, target_mask=target_mask,
                              distortion_mask=distortion_mask, debug=debug)
        x_hat = self.istft(X_hat)
        if debug:
            self.enhance_observation_locals = locals()
        return x_hat

    def speaker_ids_of(self, ex_array_activity, speaker_ids=None):
        """The targets of `enhance_observation_speakers`: ``speaker_ids`` as a list, checked
        against the activity keys, or (None) every key but the garbage tracks that
        ``Activity.garbage_class`` adds.  ValueError for unknown, duplicate or no ids."""
        keys = list(ex_array_activity.keys())
        if speaker_ids is None:
            garbage = _garbage_tracks(getattr(self.activity, 'garbage_class', True))
            speaker_ids = [k for k in keys if k not in garbage]
        else:
            speaker_ids = list(speaker_ids)
        if not speaker_ids:
            raise ValueError('no speaker to enhance')
        unknown = [s for s in speaker_ids if s not in ex_array_activity]
        if unknown:
            raise ValueError(f'speaker ids {unknown!r} are not in the activity ({keys!r})')
        if len(set(speaker_ids)) != len(speaker_ids):
            raise ValueError(f'speaker ids {speaker_ids!r} name a speaker twice')
        return speaker_ids

    def enhance_observation_speakers(self, obs, ex_array_activity, speaker_ids=None, ex=None,
                                     debug=False, fused=None, wpe_arrays=None, *,
                                     posterior_activity=False):
        """Several speakers of one window from ONE separation: returns dict speaker_id -> x_hat
        (N',) in the order of ``speaker_ids`` (None: every speaker of the activity, the
        garbage tracks left out), each what `enhance_observation` returns for that speaker.
        STFT, WPE and GSS run once; the fused path runs the target-dependent tail of all
        speakers together (gss_enhance_observation_targets), the block path calls
        ``bf_block`` and the iSTFT once per speaker."""
        self._no_posterior_activity('enhance_observation_speakers', posterior_activity)
        self._refuse('enhance_observation_speakers', self._NOT_WITH_SPEAKERS)
        speaker_ids = self.speaker_ids_of(ex_array_activity, speaker_ids)
        if wpe_arrays is None:
            wpe_arrays = self.wpe_arrays(ex, np.shape(obs)[0])
        wpe_arrays = ops.check_wpe_arrays(wpe_arrays, np.shape(obs)[0])
        if fused is None:
            fused = self._fusable()
        if not fused:
            return self._enhance_speakers_blocks(obs, ex_array_activity, speaker_ids, ex, debug,
                                                 wpe_arrays)
        keys = tuple(ex_array_activity.keys())
        targets = [keys.index(s) for s in speaker_ids]
        activity = np.array(list(ex_array_activity.values()))
        start_ctx = end_ctx = 0
        if self.bf_drop_context:
            start_ctx, end_ctx = start_end_context_samples(ex)
        params = self._params()
        ctx = self._ctx()
        ctx.set_utterances_in_flight(1)
        try:
            res = ops.enhance_observation_targets(
                obs, activity, targets, start_ctx, end_ctx, params=params, debug=debug, ctx=ctx,
                wpe_arrays=wpe_arrays, target_names=speaker_ids)
        finally:
            ctx.set_utterances_in_flight(0)
        x_hat = res[0] if debug else res
        if debug:
            self.enhance_observation_speakers_locals = dict(details=res[1],
                                                            speaker_ids=speaker_ids)
        return dict(zip(speaker_ids, x_hat))

    def enhance_example_speakers(self, ex, speaker_ids=None, *, posterior_activity=False):
        """`enhance_example` for several speakers of the example's window at once: dict
        speaker_id -> x_hat, each trimmed like `enhance_example` trims its output."""
        self._no_posterior_activity('enhance_example_speakers', posterior_activity)
        self._refuse('enhance_example_speakers', self._NOT_WITH_SPEAKERS)
        obs, ex_array_activity, _ = self._prepare_example(ex)
        out = self.enhance_observation_speakers(obs, ex_array_activity, speaker_ids, ex=ex)
        return {k: self._trim_context(v, ex) for k, v in out.items()}

    def _enhance_speakers_blocks(self, obs, ex_array_activity, speaker_ids, ex, debug,
                                 wpe_arrays=1):
        """Block path of `enhance_observation_speakers`: one STFT / WPE / GSS, then the masks,
        ``bf_block`` and the iSTFT per speaker (`_enhance_observation_blocks` for each)."""
        Obs, acitivity_freq, masks, _, _ = self._blocks_front(obs, ex_array_activity, ex, debug,
                                                           wpe_arrays)
        keys = tuple(ex_array_activity.keys())
        out = {}
        for speaker_id in speaker_ids:
            target_speaker_index = keys.index(speaker_id)
            target_mask = masks[target_speaker_index]
            distortion_mask = np.sum(np.delete(masks, target_speaker_index, axis=0), axis=0)
            X_hat = self.bf_block(Obs, target_mask=target_mask,
                                  distortion_mask=distortion_mask, debug=debug)
            out[speaker_id] = self.istft(X_hat)
        return out

    def _blocks_wpe(self, Obs, debug, wpe_arrays):
        """The WPE block on an STFT (D,T,F): joint, per array, or none."""
        if self.wpe_block is not None and wpe_arrays > 1:
            _A = wpe_arrays
            Obs = morph('A*CTF->ACTF', Obs, A=_A)
            Obs = self.wpe_block(Obs, stack=False, debug=debug)
            Obs = morph('ACTF->A*CTF', Obs)
        elif self.wpe_block is not None:
            Obs = self.wpe_block(Obs, debug=debug)
        return Obs

    def _blocks_posterior(self, obs, ex_array_activity, debug, wpe_arrays):
        """STFT, WPE (joint or per array), activity and GSS of the block path.  Returns Obs,
        acitivity_freq, the posteriors (K,T,F) as GSS gives them and the STFT before WPE (what a
        WPD beamformer block works on)."""
        Obs = raw_obs = self.stft(obs)
        self._selected_channels = None
        if self.channel_keep is not None:
            select = self._channel_select()
            Obs, self._selected_channels = ops.select_channels(
                Obs, select.keep, bank=select.bank, floor=select.floor, ctx=self._ctx())
        Obs = self._blocks_wpe(Obs, debug, wpe_arrays)
        acitivity_freq = activity_time_to_frequency(
            np.array(list(ex_array_activity.values())),
            stft_window_length=self.stft_size, stft_shift=self.stft_shift,
            stft_fading=self.stft_fading, stft_pad=True)
        return Obs, acitivity_freq, self.gss_block(Obs, acitivity_freq, debug=debug), raw_obs

    def _blocks_front(self, obs, ex_array_activity, ex, debug, wpe_arrays, blocks=None):
        """The target-independent blocks of the block path: `_blocks_posterior` (or its result,
        ``blocks``) and the zeroed context frames.  Returns Obs, acitivity_freq, masks,
        (start_context_frames, end_context_frames) or None without bf_drop_context, and the STFT
        before WPE."""
        Obs, acitivity_freq, masks, raw_obs = blocks or self._blocks_posterior(
            obs, ex_array_activity, debug, wpe_arrays)
        if self.bf_drop_context:
            start_context_frames, end_context_frames = start_end_context_frames(
                ex, stft_size=self.stft_size, stft_shift=self.stft_shift,
                stft_fading=self.stft_fading)
            masks[:, :start_context_frames, :] = 0
            if end_context_frames > 0:
                masks[:, -end_context_frames:, :] = 0
            return (Obs, acitivity_freq, masks, (start_context_frames, end_context_frames),
                    raw_obs)
        return Obs, acitivity_freq, masks, None, raw_obs

    def _enhance_observation_blocks(self, obs, ex_array_activity, speaker_id, ex, debug,
                                    wpe_arrays=1, blocks=None):
        """Block-by-block path with the reference's control flow (one device
        round trip per block); used when a block was swapped out.  ``blocks``: the result of
        `_blocks_posterior` when the caller has run it already."""
        Obs, acitivity_freq, masks, context_frames, raw_obs = self._blocks_front(
            obs, ex_array_activity, ex, debug, wpe_arrays, blocks)
        if self._selected_channels is not None:
            selected_channels = self._selected_channels
        if context_frames is not None:
            start_context_frames, end_context_frames = context_frames
        target_speaker_index = tuple(ex_array_activity.keys()).index(speaker_id)
        target_mask = masks[target_speaker_index]
        distortion_mask = np.sum(np.delete(masks, target_speaker_index, axis=0), axis=0)
        if self._bf_null():
            # (`masks` has its context frames zeroed already; the device call zeroes them again
            # by the same rule and leaves them out of the masses, as the fused call does)
            sf, ef = context_frames if context_frames is not None else (0, 0)
            _, interferer_mask, noise_mask, interferer_index = ops.lcmv_masks_from_posteriors(
                masks, target_speaker_index, drop_context=context_frames is not None,
                start_context_frames=sf, end_context_frames=ef, ctx=self._ctx(),
                candidates=self.interferer_candidates(ex_array_activity, speaker_id))
            X_hat = self.bf_block(Obs, target_mask=target_mask, distortion_mask=distortion_mask,
                                  debug=debug, interferer_mask=interferer_mask,
                                  noise_mask=noise_mask)
        elif self._bf_wpd() is not None:
            # the raw STFT goes to the beamformer block, with the context frames gated out of its
            # statistics as the fused call gates them
            frame_gate = None
            if context_frames is not None:
                frame_gate = np.ones(Obs.shape[1], np.uint8)
                frame_gate[:start_context_frames] = 0
                if end_context_frames > 0:
                    frame_gate[-end_context_frames:] = 0
            X_hat = self.bf_block(Obs, target_mask=target_mask, distortion_mask=distortion_mask,
                                  debug=debug, raw_obs=raw_obs, frame_gate=frame_gate)
        else:
            X_hat = self.bf_block(Obs, target_mask=target_mask,
                                  distortion_mask=distortion_mask, debug=debug)
        x_hat = self.istft(X_hat)
        if debug:
            self.enhance_observation_locals = locals()
        return x_hat


def bf_block_kwargs(bf, wpe_tabs, wpe_delay, bf_wpd_taps=None, bf_wpd_delay=None,
                    bf_wpd_iterations=1, bf_wpd_power_floor=ops.WPD_POWER_FLOOR):
    """The ``wpd_*`` fields of `Beamformer` from the ``bf_wpd_*`` keywords of the
    ``get_enhancer`` functions: taps / delay None mean the WPE block's.  Settings other than the
    defaults with a ``bf`` that is no WPD type are a combination nobody reads:
    NotImplementedError."""
    if bf not in ops.WPD_BF_TYPES:
        if (bf_wpd_taps is not None or bf_wpd_delay is not None or bf_wpd_iterations != 1
                or bf_wpd_power_floor != ops.WPD_POWER_FLOOR):
            ops.check_bf_wpd(bf=bf)
        return {}
    return dict(wpd_taps=wpe_tabs if bf_wpd_taps is None else bf_wpd_taps,
                wpd_delay=wpe_delay if bf_wpd_delay is None else bf_wpd_delay,
                wpd_iterations=bf_wpd_iterations, wpd_power_floor=bf_wpd_power_floor)


def wpe_block_from(wpe, wpe_tabs, wpe_delay, wpe_iterations, wpe_psd_context, wpe_online=False,
                   wpe_alpha=ops.WPE_ONLINE_ALPHA):
    """The WPE block of the ``get_enhancer`` functions from their ``wpe*`` keywords (None
    without WPE).  NotImplementedError for the combinations nobody reads: ``wpe_online`` without
    WPE or with a PSD context, a ``wpe_alpha`` other than the default without ``wpe_online``."""
    assert wpe_online is True or wpe_online is False, wpe_online
    if wpe_online and not wpe:
        raise NotImplementedError('wpe_online with wpe=False: there is no WPE block to replace')
    if wpe_online and wpe_psd_context != 0:
        raise NotImplementedError(
            f'wpe_online with wpe_psd_context={wpe_psd_context!r}: the online WPE has no PSD '
            'context')
    if not wpe_online and wpe_alpha != ops.WPE_ONLINE_ALPHA:
        raise NotImplementedError(f'wpe_alpha={wpe_alpha!r} without wpe_online: nobody reads it')
    if not wpe:
        return None
    return WPE(taps=wpe_tabs, delay=wpe_delay, iterations=wpe_iterations,
               psd_context=wpe_psd_context, online=wpe_online, alpha=wpe_alpha)


def _enhancer_fields(
        *, multiarray, context_samples, wpe, wpe_tabs, wpe_delay, wpe_iterations, wpe_psd_context,
        activity_garbage_class, stft_size, stft_shift, stft_fading, bss_iterations,
        bss_iterations_post, bf_drop_context, bf, postfilter, device_id, wpe_per_array,
        bf_segment_frames, bf_segment_context, bf_segment_min_mass, channel_keep, channel_bands,
        bf_null_interferer, bf_null_min_mass, bf_wpd_taps, bf_wpd_delay, bf_wpd_iterations,
        bf_wpd_power_floor, wpe_online, wpe_alpha, bf_online, bf_forget, bf_loading, gss_online,
        gss_forget, gss_prior_mass):
    """What the three ``get_enhancer`` functions build alike from the keywords they share (see
    `get_enhancer` for each): the ``wpe_block``, ``gss_block``, ``bf_block`` and plain fields of
    an `Enhancer`, as the keyword arguments of its constructor.  The front door adds its own
    ``activity`` and whatever else only it has.  (``activity_garbage_class`` is shared but
    belongs to that activity: not read here.)"""
    return dict(
        multiarray=multiarray, context_samples=context_samples, bf_drop_context=bf_drop_context,
        stft_size=stft_size, stft_shift=stft_shift, stft_fading=stft_fading, device_id=device_id,
        wpe_per_array=bool(wpe_per_array), channel_keep=channel_keep, channel_bands=channel_bands,
        wpe_block=wpe_block_from(wpe, wpe_tabs, wpe_delay, wpe_iterations, wpe_psd_context,
                                 wpe_online, wpe_alpha),
        gss_block=GSS(iterations=bss_iterations, iterations_post=bss_iterations_post,
                      verbose=False, online=gss_online, forget=gss_forget,
                      prior_mass=gss_prior_mass),
        bf_block=Beamformer(type=bf, postfilter=postfilter, segment_frames=bf_segment_frames,
                            segment_context=bf_segment_context,
                            segment_min_mass=bf_segment_min_mass,
                            null_interferer=bool(bf_null_interferer),
                            null_min_mass=bf_null_min_mass,
                            online=bf_online, forget=bf_forget, loading=bf_loading,
                            **bf_block_kwargs(bf, wpe_tabs, wpe_delay, bf_wpd_taps,
                                              bf_wpd_delay, bf_wpd_iterations,
                                              bf_wpd_power_floor)))


def _shared_keywords(given):
    """The keywords of `_enhancer_fields` out of ``given``, the ``locals()`` at the head of a
    ``get_enhancer``."""
    import inspect
    return {k: given[k] for k in inspect.signature(_enhancer_fields).parameters}


def get_enhancer(
    multiarray=False,
    reference_array=None,
    context_samples=240000,

    wpe=True,
    wpe_tabs=10,
    wpe_delay=2,
    wpe_iterations=3,
    wpe_psd_context=0,

    activity_type='annotation',
    activity_path=None,
    activity_garbage_class=True,

    stft_size=1024,
    stft_shift=256,
    stft_fading=True,

    bss_iterations=20,
    bss_iterations_post=1,

    bf_drop_context=True,

    bf='mvdrSouden_ban',
    postfilter=None,

    database_path=None,

    activity_store=None,
    iterator_factory=None,
    device_id=None,
    wpe_per_array=False,
    bf_segment_frames=None,
    bf_segment_context=0,
    bf_segment_min_mass=None,
    channel_keep=None,
    channel_bands=40,
    bf_null_interferer=False,
    bf_null_min_mass=None,
    bf_wpd_taps=None,
    bf_wpd_delay=None,
    bf_wpd_iterations=1,
    bf_wpd_power_floor=ops.WPD_POWER_FLOOR,
    wpe_online=False,
    wpe_alpha=ops.WPE_ONLINE_ALPHA,
    bf_online=False,
    bf_forget=ops.BF_ONLINE_FORGET,
    bf_loading=ops.BF_ONLINE_LOADING,
    gss_online=False,
    gss_forget=ops.GSS_ONLINE_FORGET,
    gss_prior_mass=ops.GSS_ONLINE_PRIOR_MASS,
):
    """core.py:574-637 (same keyword arguments and defaults; ``activity_store``,
    ``iterator_factory``, ``device_id``, ``wpe_per_array``, ``bf_segment_*``, ``channel_*``,
    ``bf_null_*``, ``bf_wpd_*``, ``wpe_online``, ``wpe_alpha``, ``bf_online``, ``bf_forget``,
    ``bf_loading``, ``gss_online``, ``gss_forget`` and ``gss_prior_mass`` are additions).
    ``gss_online=True``: the mixture model becomes the online CACGMM (see
    `ops.cacgmm_posteriors_online`) -- the recursive EM on running sums that forget at the rate
    ``gss_forget`` (0.99: a choice, not a measurement; on the moving-speaker scene of DESIGN
    section 25 0.95 follows the movement and 0.99 shows no gain), frame t classified by the model
    of the frames before it, from a fresh state of mass ``gss_prior_mass`` (1.0: a choice, not a
    measurement) per utterance, masked by the annotation; ``bss_iterations`` and
    ``bss_iterations_post`` are not read.  With ``wpe_online=True`` and ``bf_online=True`` it
    completes the zero-look-ahead chain.  For `Enhancer.enhance_observation` / `enhance_example`
    (one fused call, or the stage path with ``fused=False``) and, one utterance at a time,
    `enhance_session`.  Not with ``bf_segment_frames``, ``bf_null_interferer``, ``channel_keep``,
    ``refined_rttm``, the WPD types, the guided, multi-speaker, activity or annotation-free
    methods, and a ``gss_forget`` / ``gss_prior_mass`` other than the default without it is a
    setting nobody reads (NotImplementedError).  Nothing here is tuned against recognition
    accuracy.
    ``bf_online=True``: 'mvdrSouden_ban' becomes the online MVDR (see
    `ops.mvdr_souden_online_from_masks`) -- running sums that forget at the rate ``bf_forget``
    (0.99, a memory of 1.6 s at the 16 ms frame shift: a choice, not a measurement), a filter per
    frame with no look-ahead, from a fresh state per utterance with the relative diagonal loading
    ``bf_loading`` (1e-2: a choice, not a measurement); the reference channel is the window's.
    For `Enhancer.enhance_observation` / `enhance_example` (one fused call, or the stage path
    with ``fused=False``) and, one utterance at a time, `enhance_session`; it combines with
    ``wpe_online=True`` and ``wpe_per_array``.  Not with another ``bf``, ``bf_segment_frames``,
    ``bf_null_interferer``, ``channel_keep``, ``refined_rttm``, the guided, multi-speaker,
    activity or annotation-free methods, and a ``bf_forget`` / ``bf_loading`` other than the
    default without it is a setting nobody reads (NotImplementedError).
    ``wpe_online=True``: the WPE block is nara_wpe's online form (see `ops.wpe_online_dtf`) -- a
    frame-recursive filter from a fresh state per utterance that forgets at the rate
    ``wpe_alpha`` (0.9999: a choice, not a measurement), the time-varying front for long windows
    with movement; ``wpe_iterations`` is not read, ``wpe_per_array`` is honoured, a
    ``wpe_psd_context`` other than 0 is NotImplementedError.  For `Enhancer.enhance_observation` /
    `enhance_example`, one utterance at a time `enhance_session`, and the annotation-free
    methods; not with the WPD types, the guided, multi-speaker or activity methods or
    ``refined_rttm``, and with ``bf_segment_frames``, ``bf_null_interferer`` or ``channel_keep``
    only on the stage path (``fused=False``) (NotImplementedError).
    ``bf='wpdSouden_ban'`` / ``'wpdSouden'``: the WPD convolutional beamformer (see
    `ops.wpd_souden_from_masks`) on the STFT BEFORE WPE -- WPE as configured still feeds the
    mixture model (``wpe_per_array`` only shapes that WPE) --, ``bf_wpd_taps`` / ``bf_wpd_delay``
    (None: the WPE block's) its tap window, ``bf_wpd_iterations`` its iterations and
    ``bf_wpd_power_floor`` (1e-3: a choice, not a measurement) the floor of the target power.  For
    `Enhancer.enhance_observation` / `enhance_example` and, one utterance at a time,
    `enhance_session` (the pipelined pcm16 path is out of scope); not with ``bf_segment_frames``,
    ``bf_null_interferer``, ``channel_keep``, the multi-speaker methods or the activity methods
    (NotImplementedError).
    ``bf_null_interferer=True``: 'mvdrSouden_ban' becomes the interferer-nulling LCMV (see
    `Beamformer`): the competing speaker with the most posterior mass in the window -- the
    garbage class is no candidate -- gets a null; where that speaker is next to silent at a
    frequency (mask sum below ``bf_null_min_mass``, None: 2 * channels) the frequency keeps the
    MVDR.  For `Enhancer.enhance_observation` / `enhance_example`; not with
    ``bf_segment_frames`` or ``channel_keep`` (NotImplementedError).
    ``channel_keep=n`` (a count) or a share in (0, 1]: keep the channels of each utterance that
    the envelope-variance measure ranks best, chosen after the STFT from a mel bank of
    ``channel_bands`` filters (see `ops.select_channels`); WPE, GSS and the beamformer run on
    those.  None: all channels.  Not with ``wpe_per_array``, ``bf='ch2'`` or
    ``bf_segment_frames`` (NotImplementedError).
    ``wpe_per_array=True``: with a multiarray mode, WPE runs on each microphone array on its
    own (the reference's ``WPE(..., stack=False)``), GSS and the beamformer on all channels;
    no effect with ``multiarray=False`` or ``wpe=False``.
    ``bf_segment_frames=L``: a time-varying 'mvdrSouden_ban' with statistics per segment of L
    STFT frames (see `Beamformer`); None: one filter per utterance."""
    given = locals()
    assert wpe is True or wpe is False, wpe
    assert activity_path is None or activity_type == 'path', (activity_path, activity_type)
    return Enhancer(
        reference_array=reference_array,
        iterator_factory=iterator_factory,
        activity=Activity(type=activity_type, garbage_class=activity_garbage_class,
                          path=activity_path, database_path=database_path,
                          store=activity_store),
        **_enhancer_fields(**_shared_keywords(given)))
