"""Samples in, samples out, in blocks of any length: the three online stages (online WPE, online
CACGMM, online MVDR) between the two ends of a stream, every state carried from block to block.

A stream is the offline path with ``stft_fading=True`` cut at arbitrary sample positions
(include/gss_hip.h, "sample-block stream"): after M samples floor(M / shift) frames exist and
max(0, floor(M / shift) * shift - (size - shift)) samples have come out, so the algorithmic
latency is below one window.  Whatever the cuts, the samples, the taps and the final states have
the bits of the stream fed as one block.  A stream has no utterance context: no frames are zeroed
in the masks, and the beamformer's reference channel is fixed by the caller.

``lookahead`` = L >= 1 gives the beamformer a filter look-ahead (include/gss_hip.h, "online MVDR
with a filter look-ahead"): frame g is filtered with the filter of frame g + L, so a block returns
the samples of the frames it RELEASES and the latency grows by L * shift samples.
"""
import numpy as np

from . import ops
from ._capi import default_context
from .cacgmm import CACGMM


class StreamingEnhancer:
    """One target of one stream, or with ``targets`` several of them from one pass.

    ``num_channels`` and ``num_classes`` (the rows of the activity handed to `process`), or
    ``model=`` a fitted `cacgmm.CACGMM`: the mixture model continues from it (mass
    ``gss_prior_mass``) and the stream is unguided -- `process` takes no activity.  ``target``:
    the class to extract; ``ref_channel``: the beamformer's reference channel.  ``wpe_arrays`` =
    A > 1: the online WPE per array of num_channels / A consecutive channels.  ``fused=False``
    runs every block through the stage operators of `ops` in the place of the one library call;
    the bits are the same.  ``speakers``: the names of the classes in activity order, for an
    activity handed to `process` as a dict.  ``targets``: a sequence of S distinct class indices
    in the place of ``target`` -- the analysis, the online WPE and the online CACGMM run once for
    all of them, `process` and `flush` return (S, m), row s with the bits of the stream of
    ``target=targets[s]``; the per-target taps of ``debug`` are stacked over S and
    ``fallbacks['mvdr_targets']`` lists the beamformer's fallback frames per target
    (``fallbacks['mvdr']`` is their sum).  ``lookahead``: an integer in [0, 64], the frames the
    beamformer's filter looks ahead (0: today's stream); `process` then returns the samples of the
    frames released, `flush` releases the rest, and with ``debug`` the 'X_hat' tap covers the frames
    released by the block while the masks, the posteriors and 'Obs' cover the block's frames.
    Nothing touches the GPU before the first block.
    """

    def __init__(self, num_channels=None, num_classes=None, *, model=None, target=0, ref_channel=0,
                 stft_size=1024, stft_shift=256, window=None, wpe=True, wpe_taps=10, wpe_delay=2,
                 wpe_alpha=ops.WPE_ONLINE_ALPHA, wpe_arrays=1,
                 gss_forget=ops.GSS_ONLINE_FORGET, gss_prior_mass=ops.GSS_ONLINE_PRIOR_MASS,
                 bf_forget=ops.BF_ONLINE_FORGET, bf_loading=ops.BF_ONLINE_LOADING,
                 postfilter=None, fused=True, speakers=None, targets=None, lookahead=0,
                 ctx=None):
        if model is not None:
            if not isinstance(model, CACGMM):
                raise ValueError(f'model: a CACGMM, not {type(model).__name__}')
            F, K, D = model.shape
            if F != stft_size // 2 + 1:
                raise ValueError(f'model: {F} frequencies, stft_size={stft_size} has '
                                 f'{stft_size // 2 + 1}')
            for name, given, has in (('num_channels', num_channels, D),
                                     ('num_classes', num_classes, K)):
                if given is not None and given != has:
                    raise ValueError(f'{name}={given!r} but the model has {has}')
            num_channels, num_classes = D, K
        for name, value in (('num_channels', num_channels), ('num_classes', num_classes)):
            if value is None:
                raise ValueError(f'{name}: needed without a model')
        if not ops._is_integer(num_classes) or num_classes < 1:
            raise ValueError(f'num_classes={num_classes!r}: a positive integer')
        D, _, size, shift = ops.check_stream(num_channels, 0, stft_size, stft_shift)
        K = int(num_classes)
        if not ops._is_integer(target) or not 0 <= target < K:
            raise ValueError(f'target={target!r}: an integer in [0, {K})')
        if targets is not None:
            if target != 0:
                raise ValueError(f'targets={targets!r} together with target={target!r}: one of '
                                 'the two')
            targets = ops.check_online_targets(targets, K)
        self.targets = targets
        if fused is not True and fused is not False:
            raise ValueError(f'fused={fused!r}: True or False')
        if wpe is not True and wpe is not False:
            raise ValueError(f'wpe={wpe!r}: True or False')
        self.wpe_arrays, self.wpe_channels = 1, D
        if wpe:
            self.wpe_arrays, self.wpe_channels = ops.check_wpe_online(wpe_taps, wpe_delay, wpe_alpha,
                                                                      D, wpe_arrays)
        self.gss_forget, self.gss_prior_mass = ops.check_gss_online(gss_forget, gss_prior_mass, K, D)
        self.bf_forget, self.bf_loading, self.ref_channel = ops.check_bf_online(
            bf_forget, bf_loading, ref_channel, D)
        if self.ref_channel < 0:
            raise ValueError(f'ref_channel={ref_channel!r}: a stream has no window to choose a '
                             f'channel over, an integer in [0, {D})')
        self.lookahead = ops.check_bf_lookahead(lookahead, self.ref_channel)
        self.params = ops.make_params(
            stft_size=size, stft_shift=shift, stft_fading=True, wpe=wpe, wpe_taps=wpe_taps,
            wpe_delay=wpe_delay, bf='mvdrSouden_ban', postfilter=postfilter,
            wpe_arrays=self.wpe_arrays if wpe else 0)
        self.D, self.K, self.F, self.size, self.shift = D, K, size // 2 + 1, size, shift
        self.target, self.wpe, self.wpe_taps, self.wpe_delay = int(target), wpe, wpe_taps, wpe_delay
        self.wpe_alpha, self.postfilter, self.fused = float(wpe_alpha), postfilter, fused
        self.model, self.window = model, window
        self.guided = model is None
        if speakers is not None:
            speakers = list(speakers)
            if len(speakers) != K or len(set(speakers)) != K:
                raise ValueError(f'speakers={speakers!r}: {K} different names')
        self.speakers = speakers
        self.ctx = ctx
        self.reset()

    # ------------------------------------------------------------------ state
    def reset(self):
        """Back to the start of a stream: fresh states (the mixture model from ``model`` again),
        the counters and the fallback counts at zero."""
        self.stream = self.wpe_state = self.em_state = self.bf_states = self.tails = None
        self.holds = None
        self.samples_in = self.samples_out = 0
        self.fallbacks = {'mvdr': 0, 'cacgmm': 0}
        if self.targets is not None:
            self.fallbacks['mvdr_targets'] = [0] * len(self.targets)
        self.flushed = False

    def _states(self):
        """The four states, made on the GPU when the first block (or a checkpoint) needs them."""
        if self.stream is not None:
            return
        self.ctx = self.ctx or default_context()
        ctx, F, D, K = self.ctx, self.F, self.D, self.K
        self.stream = ops.StreamState.fresh(D, K if self.guided else 0, self.size, self.shift,
                                            window=self.window, ctx=ctx)
        self.wpe_state = (ops.OnlineWPEState.fresh(F, self.wpe_arrays, self.wpe_channels,
                                                   self.wpe_taps, self.wpe_delay, ctx=ctx)
                          if self.wpe else None)
        self.em_state = (ops.OnlineCACGMMState.fresh(F, K, D, self.gss_prior_mass, ctx=ctx)
                         if self.guided else
                         ops.OnlineCACGMMState.from_model(self.model, self.gss_prior_mass, ctx=ctx))
        # (no frames: a stream has none yet, p_f = 1)
        self.bf_states = [ops.OnlineMVDRState.fresh(F, D, self.bf_loading, ctx=ctx)
                          for _ in self._classes()]
        if self.targets is not None or self.lookahead:
            # (a look-ahead stream synthesises through the targets entry, S = 1 included)
            self.tails = ops.StreamTails.fresh(len(self._classes()), self.size, self.shift, ctx=ctx)
        if self.lookahead:
            self.holds = [ops.OnlineMVDRHold.fresh(F, D, self.lookahead, ctx=ctx)
                          for _ in self._classes()]

    def _classes(self):
        """The classes extracted, one beamformer state each."""
        return (self.target,) if self.targets is None else self.targets

    @property
    def latency_samples(self):
        """Samples that went in and have not come out: size - shift + (samples_in mod shift),
        and lookahead * shift more once ``lookahead`` frames exist."""
        return self.samples_in - self.samples_out

    def to_host(self):
        """A checkpoint of the stream: the four states (`from_host` restores them, in any
        context) and the counters."""
        self._states()
        if self.targets is None:
            bf = {'bf': self.bf_states[0].to_host()}
        else:       # the S beamformer states stacked, the tails and whose they are
            states = [state.to_host() for state in self.bf_states]
            bf = {'bf': {k: np.stack([h[k] for h in states]) for k in states[0]},
                  'tails': self.tails.to_host()['tails'], 'targets': list(self.targets)}
        if self.lookahead:      # the delay lines, and the tails of a one-target stream
            bf.update(lookahead=self.lookahead, holds=[hold.to_host() for hold in self.holds],
                      tails=self.tails.to_host()['tails'])
        return {'stream': self.stream.to_host(), 'em': self.em_state.to_host(), **bf,
                'wpe': self.wpe_state.to_host() if self.wpe else None,
                'samples_in': self.samples_in, 'samples_out': self.samples_out,
                'fallbacks': {k: list(v) if isinstance(v, list) else v
                              for k, v in self.fallbacks.items()},
                'flushed': self.flushed}

    def from_host(self, host):
        """Continue from a checkpoint of `to_host` (of a stream with this one's settings).
        ValueError when its shapes are another stream's."""
        if ('targets' in host) != (self.targets is not None):
            raise ValueError('checkpoint: of a stream %s targets=, this stream is %s one'
                             % (('with', 'without') if 'targets' in host else ('without', 'with')))
        if self.targets is not None and tuple(host['targets']) != self.targets:
            raise ValueError(f'checkpoint: of targets={tuple(host["targets"])}, this stream has '
                             f'targets={self.targets}')
        if int(host.get('lookahead', 0)) != self.lookahead:
            raise ValueError(f'checkpoint: of lookahead={int(host.get("lookahead", 0))}, this '
                             f'stream has lookahead={self.lookahead}')
        self._states()
        ctx = self.ctx
        holds = None
        if self.lookahead:
            holds = [ops.OnlineMVDRHold.from_host(h, ctx=ctx) for h in host['holds']]
            if [hold.key for hold in holds] != [hold.key for hold in self.holds]:
                raise ValueError(f'checkpoint: delay lines built for {[h.key for h in holds]}, '
                                 f'this stream has {[h.key for h in self.holds]}')
        stream = ops.StreamState.from_host(host['stream'], ctx=ctx)
        em = ops.OnlineCACGMMState.from_host(host['em'], ctx=ctx)
        if self.targets is None:
            bfs = [ops.OnlineMVDRState.from_host(host['bf'], ctx=ctx)]
            if self.lookahead:
                tails = ops.StreamTails.from_host({'tails': host['tails']}, ctx=ctx)
                if tails.key != self.tails.key:
                    raise ValueError(f'checkpoint: tails built for ({tails._sizes}) = {tails.key}, '
                                     f'this stream has {self.tails.key}')
        else:
            S = len(self.targets)
            stacked = {k: np.asarray(v) for k, v in host['bf'].items()}
            if any(v.ndim != 4 or v.shape[0] != S for v in stacked.values()):
                raise ValueError(f'checkpoint: bf states of shapes '
                                 f'{[v.shape for v in stacked.values()]}, not (S,F,D,D) with S = {S}')
            bfs = [ops.OnlineMVDRState.from_host({k: v[s] for k, v in stacked.items()}, ctx=ctx)
                   for s in range(S)]
            tails = ops.StreamTails.from_host({'tails': host['tails']}, ctx=ctx)
            if tails.key != self.tails.key:
                raise ValueError(f'checkpoint: tails built for ({tails._sizes}) = {tails.key}, '
                                 f'this stream has {self.tails.key}')
        bf = bfs[0]
        if (host['wpe'] is not None) != self.wpe:
            raise ValueError('checkpoint: its WPE state and wpe=%r disagree' % self.wpe)
        wpe = ops.OnlineWPEState.from_host(host['wpe'], ctx=ctx) if self.wpe else None
        for name, state, key in (
                ('stream', stream, self.stream.key), ('em', em, self.em_state.key),
                ('bf', bf, (self.F, self.D)),
                ('wpe', wpe, self.wpe_state.key if self.wpe else None)):
            if state is not None and state.key != key:
                raise ValueError(f'checkpoint: {name} state built for ({state._sizes}) = '
                                 f'{state.key}, this stream has {key}')
        self.stream, self.em_state, self.wpe_state, self.bf_states = stream, em, wpe, bfs
        if self.targets is not None or self.lookahead:
            self.tails = tails
        self.holds = holds
        self.samples_in, self.samples_out = int(host['samples_in']), int(host['samples_out'])
        self.fallbacks = {k: list(v) if isinstance(v, (list, tuple)) else v
                          for k, v in host['fallbacks'].items()}
        self.flushed = bool(host['flushed'])
        return self

    # ------------------------------------------------------------------ blocks
    def _activity(self, activity, n):
        if not self.guided:
            if activity is not None:
                raise ValueError('activity: the stream continues a model and takes none')
            return None
        if activity is None:
            raise ValueError('activity: missing -- a stream started fresh has identical classes '
                             'and only the activity tells them apart (or start from model=)')
        if isinstance(activity, dict):
            if self.speakers is None:
                raise ValueError('activity: a dict needs the stream\'s speakers= names')
            if set(activity) != set(self.speakers):
                raise ValueError(f'activity: tracks of {sorted(activity)}, the stream has '
                                 f'{sorted(self.speakers)}')
            tracks = [np.asarray(activity[name]) for name in self.speakers]
            for name, track in zip(self.speakers, tracks):
                if track.shape != (n,):
                    raise ValueError(f'activity[{name!r}]: shape {track.shape} is not (n,) = ({n},)')
            activity = np.stack(tracks)
        activity = np.asarray(activity)
        if activity.shape != (self.K, n):
            raise ValueError(f'activity: shape {activity.shape} is not (K,n) = ({self.K},{n})')
        return activity != 0

    def process(self, block, activity=None, debug=False):
        """The next ``block`` (D,n) of samples, float64 or int16 PCM, with its ``activity`` (K,n)
        (or a dict of K per-sample tracks in class order) -> the samples the block finishes,
        (m,) float64 -- (S, m) with ``targets`` --; with ``debug`` (samples, details) with the
        taps over the block's frames (None when the block completes no frame).  With a
        look-ahead: the samples of the frames the block releases."""
        if self.flushed:
            raise RuntimeError('process after flush: the stream has ended, call reset()')
        block = np.asarray(block)
        if block.ndim != 2 or block.shape[0] != self.D:
            raise ValueError(f'block: shape {block.shape} is not (D,n) = ({self.D},n)')
        samples, details = self._block(block, self._activity(activity, block.shape[1]), debug)
        self.samples_in += block.shape[1]
        self.samples_out += samples.shape[-1]
        return (samples, details) if debug else samples

    def flush(self, debug=False):
        """End the stream: the zeros that complete its last frames go in (inactive), the rest
        comes out -- with a look-ahead the delay lines are released --, cut so that
        samples_out == samples_in.  `process` is an error afterwards until `reset`."""
        if self.flushed:
            raise RuntimeError('flush after flush: the stream has ended, call reset()')
        if self.samples_in == 0:        # nothing went in: nothing comes out
            self.flushed = True
            return (self._no_samples(), None) if debug else self._no_samples()
        n = ops.stream_flush_samples(self.samples_in, self.size, self.shift)
        samples, details = self._block(np.zeros((self.D, n)),
                                       np.zeros((self.K, n), bool) if self.guided else None, debug,
                                       release=True)
        samples = samples[..., :self.samples_in - self.samples_out]
        self.samples_out += samples.shape[-1]
        self.flushed = True
        return (samples, details) if debug else samples

    def _no_samples(self):
        return np.zeros(0) if self.targets is None else np.zeros((len(self.targets), 0))

    def _block(self, block, activity, debug, release=False):
        if block.shape[1] == 0:
            return self._no_samples(), None
        self._states()
        if self.lookahead:
            return self._block_lookahead(block, activity, debug, release)
        if not self.fused:
            return self._block_stages(block, activity, debug)
        Tn = ops.stream_num_frames(self.stream.received, block.shape[1], self.size, self.shift)
        shared = dict(params=self.params, stream=self.stream, em_state=self.em_state,
                      wpe_state=self.wpe_state, ref_channel=self.ref_channel,
                      wpe_alpha=self.wpe_alpha, em_forget=self.gss_forget,
                      bf_forget=self.bf_forget, window=self.window, debug=debug)
        if self.targets is not None:
            samples, details = ops.stream_block_targets(
                block, activity, bf_states=self.bf_states, tails=self.tails,
                target_indices=self.targets, **shared)
            if Tn > 0:
                self._count(self.ctx.last_mvdr_online_fallbacks_targets(len(self.targets)),
                            self.ctx.last_cacgmm_online_fallbacks())
            return samples, details
        samples, details = ops.stream_block(block, activity, bf_state=self.bf_states[0],
                                            target_index=self.target, **shared)
        if Tn > 0:
            counts = (details['fallbacks'] if details is not None else
                      (self.ctx.last_mvdr_online_fallbacks(),
                       self.ctx.last_cacgmm_online_fallbacks()))
            self._count([counts[0]], counts[1])
        return samples, details

    def _block_lookahead(self, block, activity, debug, release):
        """A block of a look-ahead stream: the one library call, or with ``fused=False`` the stage
        operators -- the front once, `ops.mvdr_souden_online_targets` with the delay lines,
        `ops.mvdr_online_release` at the end of the stream, one synthesis of the frames
        released.  A one-target stream is S = 1 of either."""
        classes, S = self._classes(), len(self._classes())
        if self.fused:
            Tn = ops.stream_num_frames(self.stream.received, block.shape[1], self.size, self.shift)
            samples, details = ops.stream_block_lookahead(
                block, activity, params=self.params, stream=self.stream, em_state=self.em_state,
                bf_states=self.bf_states, holds=self.holds, tails=self.tails,
                target_indices=classes, release=release, wpe_state=self.wpe_state,
                ref_channel=self.ref_channel, wpe_alpha=self.wpe_alpha, em_forget=self.gss_forget,
                bf_forget=self.bf_forget, window=self.window, debug=debug)
            if Tn > 0:
                self._count(self.ctx.last_mvdr_online_fallbacks_targets(S),
                            self.ctx.last_cacgmm_online_fallbacks())
        else:
            samples, details = self._lookahead_stages(block, activity, debug, release)
        if self.targets is None:
            samples = samples[0]
            if details is not None:
                details.update({k: v[0] for k, v in details.items() if k in ops._PER_TARGET})
                details.pop('fallbacks_targets', None)
        return samples, details

    def _lookahead_stages(self, block, activity, debug, release):
        classes, S = self._classes(), len(self._classes())
        Y, act_frames = ops.stft_stream(block, activity, state=self.stream, window=self.window)
        X_hat = np.zeros((S, 0, self.F), np.complex128)
        details = {}
        if Y.shape[1] > 0:
            Obs = Y
            if self.wpe:
                Obs = ops.wpe_online_dtf(Y, self.wpe_taps, self.wpe_delay, self.wpe_alpha,
                                         arrays=self.wpe_arrays, state=self.wpe_state)
            posterior, em_fallbacks = ops.cacgmm_posteriors_online(
                Obs, act_frames, forget=self.gss_forget, state=self.em_state, return_fallbacks=True)
            X_hat, bf_fallbacks = ops.mvdr_souden_online_targets(
                Obs, posterior, classes, states=self.bf_states, forget=self.bf_forget,
                ref_channel=self.ref_channel, ban=True, postfilter=self.postfilter,
                return_fallbacks=True, lookahead=self.lookahead, hold=self.holds)
            self._count(bf_fallbacks, em_fallbacks)
            if debug:
                masks = [ops.masks_from_posteriors(posterior, k, ctx=self.ctx) for k in classes]
                details = {'Obs': Obs, 'posterior': posterior,
                           'target_mask': np.stack([m[0] for m in masks]),
                           'distortion_mask': np.stack([m[1] for m in masks]),
                           'ref_channel': np.full(S, self.ref_channel),
                           'fallbacks': (sum(bf_fallbacks), em_fallbacks),
                           'fallbacks_targets': bf_fallbacks}
                if act_frames is not None:
                    details['acitivity_freq'] = act_frames
        if release:
            X_hat = np.concatenate([X_hat, ops.mvdr_online_release(
                self.holds, postfilter=self.postfilter)], axis=1)
        samples = ops.istft_stream_targets(X_hat, state=self.stream, tails=self.tails,
                                           window=self.window)
        if not debug or (Y.shape[1] == 0 and X_hat.shape[1] == 0):
            return samples, None
        details['X_hat'] = X_hat
        return samples, details

    def _count(self, bf_targets, em_fallbacks):
        self.fallbacks['mvdr'] += sum(bf_targets)
        self.fallbacks['cacgmm'] += em_fallbacks
        if self.targets is not None:
            self.fallbacks['mvdr_targets'] = [a + b for a, b in
                                              zip(self.fallbacks['mvdr_targets'], bf_targets)]

    def _block_stages(self, block, activity, debug):
        """The block through the stage operators, each with its explicit state: the front once,
        then masks, beamformer and postfilter per target through the single-target operators,
        then the synthesis of the stream (`istft_stream`, or `istft_stream_targets` with the
        tails of a stream with ``targets``)."""
        Y, act_frames = ops.stft_stream(block, activity, state=self.stream, window=self.window)
        if Y.shape[1] == 0:
            return self._no_samples(), None
        Obs = Y
        if self.wpe:
            Obs = ops.wpe_online_dtf(Y, self.wpe_taps, self.wpe_delay, self.wpe_alpha,
                                     arrays=self.wpe_arrays, state=self.wpe_state)
        posterior, em_fallbacks = ops.cacgmm_posteriors_online(
            Obs, act_frames, forget=self.gss_forget, state=self.em_state, return_fallbacks=True)
        rows = []
        for target, state in zip(self._classes(), self.bf_states):
            target_mask, distortion_mask = ops.masks_from_posteriors(posterior, target, ctx=self.ctx)
            X_hat, fallbacks = ops.mvdr_souden_online_from_masks(
                Obs, target_mask, distortion_mask, ban=True, forget=self.bf_forget,
                ref_channel=self.ref_channel, state=state, return_fallbacks=True)
            if self.postfilter == 'mask_mul':
                # (re * m, im * m as the library's postfilter, not a complex product)
                X_hat = (X_hat.view(np.float64).reshape(X_hat.shape + (2,))
                         * target_mask[..., None]).reshape(X_hat.shape[0], -1).view(np.complex128)
            rows.append((target_mask, distortion_mask, X_hat, fallbacks))
        target_mask, distortion_mask, X_hat, bf_fallbacks = (list(column) for column in zip(*rows))
        if self.targets is None:
            samples = ops.istft_stream(X_hat[0], state=self.stream, window=self.window)
            details = {'target_mask': target_mask[0], 'distortion_mask': distortion_mask[0],
                       'X_hat': X_hat[0], 'ref_channel': self.ref_channel,
                       'fallbacks': (bf_fallbacks[0], em_fallbacks)}
        else:
            X_hat = np.stack(X_hat)
            samples = ops.istft_stream_targets(X_hat, state=self.stream, tails=self.tails,
                                               window=self.window)
            details = {'target_mask': np.stack(target_mask),
                       'distortion_mask': np.stack(distortion_mask), 'X_hat': X_hat,
                       'ref_channel': np.full(len(rows), self.ref_channel),
                       'fallbacks': (sum(bf_fallbacks), em_fallbacks),
                       'fallbacks_targets': bf_fallbacks}
        self._count(bf_fallbacks, em_fallbacks)
        if not debug:
            return samples, None
        details.update(Obs=Obs, posterior=posterior)
        if act_frames is not None:
            details['acitivity_freq'] = act_frames
        return samples, details
