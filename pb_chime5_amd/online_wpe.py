"""The online (frame-recursive) WPE with the shape of nara_wpe's ``OnlineWPE``: an object that is
fed a recording in blocks -- or frame by frame -- and keeps its filter between the calls.

    wpe = OnlineWPE(taps=10, delay=2, alpha=0.9999, channel=4, frequency_bins=513)
    for block in blocks:                    # (T, F, D) each, any T
        out = wpe.step_frames(block)        # (T, F, D)

The state (`ops.OnlineWPEState`: inverse covariance, filter, the last taps + delay frames) lives on
the device between the calls; feeding a recording in blocks gives the bits of feeding it at once.
The recursion is the one of include/gss_hip.h (gss_wpe_online): every frame is filtered with the
filter as it stands before that frame updates it, and a frame whose whole buffer is digital
silence leaves the filter alone.
"""
import numpy as np

from . import ops


class OnlineWPE:
    """``channel``: the channels D of a frame; ``arrays`` = A > 1: one filter per microphone
    array of D / A consecutive channels.  ``alpha``: the forgetting factor in (0, 1] (the default
    0.9999 is a choice, not a measurement)."""

    def __init__(self, taps=10, delay=2, alpha=ops.WPE_ONLINE_ALPHA, channel=8, frequency_bins=257,
                 arrays=1, *, ctx=None):
        if not ops._is_integer(frequency_bins) or frequency_bins < 1:
            raise ValueError(f'frequency_bins={frequency_bins!r}: a positive integer')
        self.arrays, per_array = ops.check_wpe_online(taps, delay, alpha, channel, arrays)
        self.taps, self.delay, self.alpha = int(taps), int(delay), float(alpha)
        self.channel, self.frequency_bins = int(channel), int(frequency_bins)
        self._per_array = per_array
        self._ctx = ctx
        self.state = None
        self.reset()

    def reset(self):
        """Back to the fresh state: P = I, G = 0, no history."""
        self.state = ops.OnlineWPEState.fresh(self.frequency_bins, self.arrays, self._per_array,
                                              self.taps, self.delay, ctx=self._ctx)

    def step_frames(self, block):
        """block (T,F,D) -> the dereverberated frames (T,F,D); the state moves on by T frames."""
        block = np.asarray(block)
        if block.ndim != 3 or block.shape[1:] != (self.frequency_bins, self.channel):
            raise ValueError(f'block: shape {block.shape} is not (T, {self.frequency_bins}, '
                             f'{self.channel})')
        out = ops.wpe_online_dtf(block.transpose(2, 0, 1), self.taps, self.delay, self.alpha,
                                 arrays=self.arrays, state=self.state)
        return np.ascontiguousarray(out.transpose(1, 2, 0))

    def step_frame(self, frame):
        """frame (F,D) -> (F,D): one launch per frame.  It is there for the shape of nara_wpe's
        interface, not for speed -- `step_frames` walks a block in one launch."""
        frame = np.asarray(frame)
        if frame.shape != (self.frequency_bins, self.channel):
            raise ValueError(f'frame: shape {frame.shape} is not ({self.frequency_bins}, '
                             f'{self.channel})')
        return self.step_frames(frame[None])[0]
