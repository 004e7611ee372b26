"""The online (frame-recursive) CACGMM with the shape of `online_mvdr.OnlineMVDR`: an object that
is fed a recording and its guidance in blocks -- or frame by frame -- and keeps its mixture model
between the calls.

    em = OnlineCACGMM(forget=0.99, prior_mass=1.0, num_classes=3, channel=4, frequency_bins=513)
    for block, mask in blocks:               # (T, F, D), (K, T) each, any T
        gamma = em.step_frames(block, mask)  # (K, T, F)

    em = OnlineCACGMM(model=fitted)          # continue a fitted `cacgmm.CACGMM`, no mask needed
    gamma = em.step_frames(block)

The state (`ops.OnlineCACGMMState`: the running sums s_k and the masses n_k) lives on the device
between the calls; feeding a recording in blocks gives the bits of feeding it at once.  The
recursion is the one of include/gss_hip.h (gss_cacgmm_online): frame t is classified by the model
of the frames before it -- causal, no look-ahead -- and then enters the sums, which forget at the
rate ``forget``.
"""
import numpy as np

from . import ops


class OnlineCACGMM:
    """``num_classes``: K; ``channel``: the channels D of a frame.  ``forget`` in (0, 1] and
    ``prior_mass`` > 0 (the defaults 0.99 and 1.0 are choices, not measurements).  Without
    ``model`` the stream starts from the fresh state, whose classes are identical: every block
    then needs a mask.  With ``model`` (a `cacgmm.CACGMM`; K, D and F are its own) it starts from
    `ops.OnlineCACGMMState.from_model` with ``prior_mass`` as the model's mass."""

    def __init__(self, forget=ops.GSS_ONLINE_FORGET, prior_mass=ops.GSS_ONLINE_PRIOR_MASS,
                 num_classes=3, channel=8, frequency_bins=257, model=None, *, ctx=None):
        if model is not None:
            if not isinstance(model, ops.CACGMM):
                raise ValueError(f'model: a CACGMM, not {type(model).__name__}')
            frequency_bins, num_classes, channel = model.shape
        if not ops._is_integer(frequency_bins) or frequency_bins < 1:
            raise ValueError(f'frequency_bins={frequency_bins!r}: a positive integer')
        self.forget, self.prior_mass = ops.check_gss_online(forget, prior_mass, num_classes, channel)
        self.num_classes, self.channel = int(num_classes), int(channel)
        self.frequency_bins = int(frequency_bins)
        self.model = model
        self._ctx = ctx
        self.state = None
        self.fallbacks = 0
        self.reset()

    def reset(self):
        """Back to the start: the fresh state, or the model the stream was built from."""
        if self.model is not None:
            self.state = ops.OnlineCACGMMState.from_model(self.model, self.prior_mass, ctx=self._ctx)
        else:
            self.state = ops.OnlineCACGMMState.fresh(self.frequency_bins, self.num_classes,
                                                     self.channel, self.prior_mass, ctx=self._ctx)
        self.fallbacks = 0

    def step_frames(self, block, source_activity_mask=None):
        """block (T,F,D), mask (K,T) / (K,T,F) or None -> the posteriors (K,T,F); the state moves
        on by T frames and ``fallbacks`` counts the (frequency, frame, class) triples that fell
        back.  A stream without a model needs the mask (ValueError)."""
        block = np.asarray(block)
        if block.ndim != 3 or block.shape[1:] != (self.frequency_bins, self.channel):
            raise ValueError(f'block: shape {block.shape} is not (T, {self.frequency_bins}, '
                             f'{self.channel})')
        if source_activity_mask is None and self.model is None:
            raise ValueError('source_activity_mask is None on a stream that started fresh: its '
                             'classes are identical and every posterior would be 1 / K; build '
                             'the stream from a model')
        gamma, fallbacks = ops.cacgmm_posteriors_online(
            block.transpose(2, 0, 1), source_activity_mask, forget=self.forget,
            prior_mass=self.prior_mass, state=self.state, return_fallbacks=True)
        self.fallbacks += fallbacks
        return gamma

    def step_frame(self, frame, source_activity_mask=None):
        """frame (F,D), mask (K,) / (K,F) or None -> (K,F): one launch per frame.  It is there for
        the interface, not for speed -- `step_frames` walks a block in one launch."""
        frame = np.asarray(frame)
        if frame.shape != (self.frequency_bins, self.channel):
            raise ValueError(f'frame: shape {frame.shape} is not ({self.frequency_bins}, '
                             f'{self.channel})')
        mask = None
        if source_activity_mask is not None:
            mask = np.asarray(source_activity_mask)[:, None]
        return self.step_frames(frame[None], mask)[:, 0]
