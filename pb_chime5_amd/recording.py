"""The arithmetic of annotation-free separation of a whole recording in linked windows
(`Enhancer.enhance_recording_blind`): the window plan, the frames two neighbours share, the start
table of a window and the cross-fade.  Host only, no device work; tests/link_reference.py holds an
independent NumPy form of each.

Windows overlap, every window is separated on its own (`ops.separate_observation`), the classes of
window w + 1 are renumbered to continue those of window w (`ops.link_posteriors` on the shared
frames), and the windows are cross-faded (Yoshioka et al., continuous speech separation)."""
from dataclasses import dataclass

import numpy as np

from . import ops

START_MODES = ('carry', 'fresh')
_LINK_MAX_CLASSES = 8                       # include/gss_hip.h: GSS_ALIGN_MAX_CLASSES


def _integer(name, value, least):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < least:
        raise ValueError(f'{name}: {value!r} is not an integer >= {least}')
    return int(value)


@dataclass(frozen=True)
class RecordingPlan:
    """Where the windows of a recording lie and what neighbours share, in samples and frames."""
    windows: tuple          # ((start, end), ...) in samples
    hop_frames: int         # H: frame t of window w + 1 is frame t + H of window w
    shared_frames: int      # L: frames two neighbours share (0 with one window)
    edge_frames: int        # E: shared frames left out of the link on either side
    overlap_samples: int    # samples two neighbours share

    @property
    def link_frames(self):
        """((begin, end) in the previous window, (begin, end) in the current one)."""
        H, L, E = self.hop_frames, self.shared_frames, self.edge_frames
        return (H + E, H + L - E), (E, L - E)


def window_plan(num_samples, window_samples, hop_samples):
    """[(start, end), ...]: ``n = max(1, (N - window) // hop + 1)`` windows, window w from
    ``w * hop``, ``window`` samples long, the last one to N (so between ``window`` and
    ``window + hop`` samples; one window of N samples when N < window)."""
    N = _integer('num_samples', num_samples, 1)
    window = _integer('window_samples', window_samples, 1)
    hop = _integer('hop_samples', hop_samples, 1)
    n = max(1, (N - window) // hop + 1)
    return [(w * hop, N if w == n - 1 else w * hop + window) for w in range(n)]


def check_recording(num_samples, num_speakers, window_samples, hop_samples, stft_size, stft_shift,
                    start='carry', seed=0, fading=True):
    """The argument rules of `Enhancer.enhance_recording_blind` -> `RecordingPlan`; ValueError.
    Both lengths are multiples of ``stft_shift`` with ``hop < window <= 2 hop`` (at most two
    windows hold any sample); ``num_speakers`` in [1, 7]; the shared frames must leave something
    to link once ``E = stft_size / stft_shift - 1`` edge frames are left out on either side."""
    if start not in START_MODES:
        raise ValueError(f'start: {start!r} is not one of {START_MODES}')
    _integer('seed', seed, 0)
    if (isinstance(num_speakers, bool) or not isinstance(num_speakers, (int, np.integer))
            or not 1 <= num_speakers <= _LINK_MAX_CLASSES - 1):
        raise ValueError(f'num_speakers: {num_speakers!r} is not an integer in '
                         f'[1, {_LINK_MAX_CLASSES - 1}] (the link searches all K! permutations of '
                         f'K = num_speakers + 1 <= {_LINK_MAX_CLASSES} classes)')
    if not fading:
        raise ValueError('stft_fading=False: the frames of neighbouring windows line up only '
                         'with the padded STFT')
    N = _integer('num_samples', num_samples, 1)
    window = _integer('window_samples', window_samples, 1)
    hop = _integer('hop_samples', hop_samples, 1)
    for name, value in (('window_samples', window), ('hop_samples', hop)):
        if value % stft_shift:
            raise ValueError(f'{name}: {value} is not a multiple of stft_shift = {stft_shift}')
    if not hop < window <= 2 * hop:
        raise ValueError(f'not hop_samples = {hop} < window_samples = {window} <= 2 hop_samples: '
                         'neighbours must overlap and at most two windows may hold a sample')
    windows = window_plan(N, window, hop)
    H = hop // stft_shift
    E = stft_size // stft_shift - 1
    if len(windows) == 1:
        return RecordingPlan(tuple(windows), H, 0, E, 0)
    L = ops.stft_frames(window, stft_size, stft_shift, True) - H
    if L - 2 * E < 1:
        raise ValueError(f'window_samples - hop_samples = {window - hop}: the {L} shared frames '
                         f'leave nothing to link without {E} edge frames on either side')
    return RecordingPlan(tuple(windows), H, L, E, window - hop)


def start_table(num_classes, num_frames, seed, window_index, start='carry', previous_prior=None,
                hop_frames=0, shared_frames=0):
    """The start of window ``window_index``'s EM, (K,T).  'fresh':
    ``ops.blind_initialization(K, T, seed + window_index)``.  'carry': the same table with its
    first ``shared_frames`` columns replaced by the previous window's linked prior on the shared
    frames (its columns from ``hop_frames``), every column then divided by its sum; window 0 (no
    ``previous_prior``) has nothing to carry."""
    if start not in START_MODES:
        raise ValueError(f'start: {start!r} is not one of {START_MODES}')
    table = ops.blind_initialization(num_classes, num_frames, seed + window_index)
    if start == 'fresh' or previous_prior is None:
        return table
    previous_prior = np.asarray(previous_prior, np.float64)
    H, L = int(hop_frames), int(shared_frames)
    if previous_prior.shape[0] != num_classes or previous_prior.shape[1] < H + L or L > num_frames:
        raise ValueError(f'previous_prior: shape {previous_prior.shape} does not hold {L} shared '
                         f'frames from frame {H} for {num_classes} classes')
    table = table.copy()
    table[:, :L] = previous_prior[:, H:H + L]
    return table / np.sum(table, axis=0, keepdims=True)


def fade_weights(overlap):
    """The weight of the LATER window on the ``overlap`` shared samples (or frames):
    ``(i + 0.5) / overlap``; the earlier window has one minus it."""
    overlap = _integer('overlap', overlap, 0)
    return (np.arange(overlap) + 0.5) / max(overlap, 1)


def stitch(pieces, offsets, total):
    """Cross-fade ``pieces`` (arrays (..., n_w) along the last axis, piece w from ``offsets[w]``)
    into one (..., total) array, window by window: on the overlap of what has been stitched so
    far with piece w the piece gets `fade_weights`, the earlier signal the rest; behind the
    overlap the piece is taken unchanged, before it the earlier signal.  The first piece starts
    at 0, the last ends at ``total``, offsets and ends ascend.  Samples are held by at most two
    windows (`check_recording`); with ``window = 2 hop`` the few frames of the STFT's padding are
    held by three, and there the earlier two share what the latest leaves, as they shared before:
    the weights always sum to one."""
    pieces = [np.asarray(p) for p in pieces]
    offsets = [int(o) for o in offsets]
    if not pieces or len(pieces) != len(offsets):
        raise ValueError(f'{len(pieces)} pieces for {len(offsets)} offsets')
    ends = [o + p.shape[-1] for o, p in zip(offsets, pieces)]
    if offsets[0] != 0 or ends[-1] != total:
        raise ValueError(f'the pieces cover [{offsets[0]}, {ends[-1]}), not [0, {total})')
    out = np.empty(pieces[0].shape[:-1] + (int(total),), np.result_type(*pieces, np.float64))
    out[..., :ends[0]] = pieces[0]
    for w in range(1, len(pieces)):
        o, O = offsets[w], ends[w - 1] - offsets[w]
        if o < offsets[w - 1] or ends[w] < ends[w - 1] or O < 0:
            raise ValueError(f'piece {w} covers [{o}, {ends[w]}): neighbours must overlap or touch '
                             'and both ends must ascend')
        r = fade_weights(O)
        out[..., o:o + O] = (1.0 - r) * out[..., o:o + O] + r * pieces[w][..., :O]
        out[..., o + O:ends[w]] = pieces[w][..., O:]
    return out
