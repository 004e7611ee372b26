"""The online (frame-recursive) MVDR with the shape of `online_wpe.OnlineWPE`: an object that is
fed a recording and its masks in blocks -- or frame by frame -- and keeps its statistics between
the calls.

    bf = OnlineMVDR(forget=0.99, loading=1e-2, channel=4, frequency_bins=513, ban=True)
    for block, mx, mn in blocks:            # (T, F, D), (T, F), (T, F) each, any T
        out = bf.step_frames(block, mx, mn) # (T, F)

The state (`ops.OnlineMVDRState`: the running sums Phi_X and Phi_N) lives on the device between the
calls; feeding a recording in blocks gives the bits of feeding it at once.  The recursion is the
one of include/gss_hip.h (gss_mvdr_online): both sums forget at the rate ``forget``, take frame t
in, and the filter of frame t is solved from them -- look-ahead L, default 0.

    bf = OnlineMVDR(channel=4, frequency_bins=513, lookahead=4)
    for block, mx, mn in blocks:
        out = bf.step_frames(block, mx, mn) # the frames RELEASED: frame g once frame g + 4 is in
    tail = bf.release()                     # the last 4, with the filter of the last frame

With ``lookahead`` = L >= 1 frame g is filtered with the filter of frame g + L (`ops.OnlineMVDRHold`
carries the L frames in between): L frames of latency for a filter that has already seen a
speaker's onset.  The sums, the filters and the fallback counts are those of L = 0.
"""
import numpy as np

from . import ops


class OnlineMVDR:
    """``channel``: the channels D of a frame; ``ref_channel``: the reference channel, one
    integer in [0, D) for the whole stream (the whole-window choice of -1 is per call, so not a
    stream's).  ``forget`` in (0, 1] and ``loading`` > 0 (the defaults 0.99 and 1e-2 are choices,
    not measurements); the fresh state is phi_n = loading * I: there are no frames yet to take a
    mean power from.  ``lookahead``: an integer in [0, 64], the frames a filter looks ahead."""

    def __init__(self, forget=ops.BF_ONLINE_FORGET, loading=ops.BF_ONLINE_LOADING, channel=8,
                 frequency_bins=257, ref_channel=0, ban=False, *, lookahead=0, ctx=None):
        if not ops._is_integer(frequency_bins) or frequency_bins < 1:
            raise ValueError(f'frequency_bins={frequency_bins!r}: a positive integer')
        self.forget, self.loading, self.ref_channel = ops.check_bf_online(
            forget, loading, ref_channel, channel)
        if self.ref_channel < 0:
            raise ValueError(f'ref_channel={ref_channel!r}: a stream names its channel, an integer '
                             f'in [0, {channel})')
        self.lookahead = ops.check_bf_lookahead(lookahead, self.ref_channel)
        self.channel, self.frequency_bins = int(channel), int(frequency_bins)
        self.ban = bool(ban)
        self._ctx = ctx
        self.state = self.hold = None
        self.fallbacks = 0
        self.reset()

    def reset(self):
        """Back to the fresh state: phi_x = 0, phi_n = loading * I, an empty delay line."""
        self.state = ops.OnlineMVDRState.fresh(self.frequency_bins, self.channel, self.loading,
                                               ctx=self._ctx)
        self.hold = (ops.OnlineMVDRHold.fresh(self.frequency_bins, self.channel, self.lookahead,
                                              ctx=self.state.ctx) if self.lookahead else None)
        self.fallbacks = 0

    def step_frames(self, block, X_mask, N_mask):
        """block (T,F,D), masks (T,F) -> the beamformed frames (T,F); the state moves on by T
        frames and ``fallbacks`` counts the (frequency, frame) pairs that fell back.  With a
        look-ahead: the frames RELEASED, max(0, held + T - lookahead) of them."""
        block = np.asarray(block)
        if block.ndim != 3 or block.shape[1:] != (self.frequency_bins, self.channel):
            raise ValueError(f'block: shape {block.shape} is not (T, {self.frequency_bins}, '
                             f'{self.channel})')
        out, fallbacks = ops.mvdr_souden_online_from_masks(
            block.transpose(2, 0, 1), X_mask, N_mask, self.ban, forget=self.forget,
            loading=self.loading, ref_channel=self.ref_channel, state=self.state,
            return_fallbacks=True, lookahead=self.lookahead, hold=self.hold)
        self.fallbacks += fallbacks
        return out

    def release(self):
        """End the delay line: the held frames (h,F), filtered with the filter of the last frame
        that entered; (0,F) with nothing held or no look-ahead.  The sums stay: a stream may go
        on, its line filling again."""
        if self.hold is None:
            return np.zeros((0, self.frequency_bins), np.complex128)
        return ops.mvdr_online_release(self.hold)

    def step_frame(self, frame, X_mask, N_mask):
        """frame (F,D), masks (F,) -> (F,): one launch per frame.  It is there for the interface,
        not for speed -- `step_frames` walks a block in one launch.  With a look-ahead: the frame
        released, or None while the line fills."""
        frame = np.asarray(frame)
        if frame.shape != (self.frequency_bins, self.channel):
            raise ValueError(f'frame: shape {frame.shape} is not ({self.frequency_bins}, '
                             f'{self.channel})')
        out = self.step_frames(frame[None], np.asarray(X_mask)[None], np.asarray(N_mask)[None])
        return out[0] if len(out) else None
