"""From the posterior activity scores of an utterance (`ops.posterior_activity`: the
power-weighted share of every frame that the CACGMM gives each class) to a decision, sample
intervals and an RTTM file.  Everything here is host logic: the device library computes the scores
and holds no policy, as with the mel bank of the channel selection.

    x_hat, act = enhancer.enhance_observation_activity(obs, ex_array_activity, speaker_id, ex)
    active = decide(act.scores, act.power, ActivityRule())             # bool (K, T)
    intervals = frames_to_intervals(active[act.target_index], size, shift, fading, obs.shape[-1])
    write_rttm('S02.rttm', 'S02', {'P05': intervals})
"""
import decimal
import math
from dataclasses import dataclass
from pathlib import Path

import numpy as np


@dataclass(frozen=True)
class ActivityRule:
    """How `decide` reads the scores.  The defaults are choices, not measurements: a median
    over 11 frames (176 ms at shift 256 / 16 kHz) against single-frame flicker, "on" when the
    class holds half of the frame's power and "off" below about a third, gaps and bursts
    shorter than 8 frames (128 ms) closed or dropped.  Nobody has tuned them on a corpus.

    median_frames   odd, >= 1: length of the running median (1: none)
    on, off         0 < off <= on <= 1: hysteresis thresholds on the smoothed score
    min_off_frames  >= 0: an off-run shorter than this between two on-runs is filled
    min_on_frames   >= 0: an on-run shorter than this is dropped (after the filling)
    power_floor     0 <= floor < 1: frames with less than floor * max(power) score 0
    """
    median_frames: int = 11
    on: float = 0.5
    off: float = 0.35
    min_off_frames: int = 8
    min_on_frames: int = 8
    power_floor: float = 0.0

    def __post_init__(self):
        def integer(name):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f'{name}={v!r} is not an integer')
            return int(v)

        def real(name):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) \
                    or not np.isfinite(v):
                raise ValueError(f'{name}={v!r} is not a finite number')
            return float(v)

        m = integer('median_frames')
        if m < 1 or m % 2 == 0:
            raise ValueError(f'median_frames={m} is not an odd number >= 1')
        for name in ('min_off_frames', 'min_on_frames'):
            if integer(name) < 0:
                raise ValueError(f'{name}={getattr(self, name)} is negative')
        on, off, floor = real('on'), real('off'), real('power_floor')
        if not 0 < off <= on <= 1:
            raise ValueError(f'on={on}, off={off}: need 0 < off <= on <= 1')
        if not 0 <= floor < 1:
            raise ValueError(f'power_floor={floor} outside [0, 1)')


@dataclass
class PosteriorActivity:
    """What `Enhancer.enhance_observation_activity` reports about one window."""
    scores: np.ndarray             # (K, T): `ops.posterior_activity`
    power: np.ndarray              # (T,)
    keys: tuple                    # the classes, in the activity's dict order
    target_index: int              # the enhanced speaker among them
    start_context_frames: int      # frames of the window that are context, not utterance
    end_context_frames: int


def _runs(row):
    """[a, b) of every run of True in a 1-D bool array."""
    padded = np.concatenate(([False], np.asarray(row, dtype=bool), [False]))
    edges = np.flatnonzero(padded[1:] != padded[:-1])
    return [(int(a), int(b)) for a, b in zip(edges[::2], edges[1::2])]


def running_median(scores, frames):
    """Median over ``frames`` (odd) values along the last axis, the window clipped at both edges:
    np.median of what is there."""
    scores = np.asarray(scores, dtype=np.float64)
    half = int(frames) // 2
    if half == 0:
        return scores.copy()
    T = scores.shape[-1]
    out = np.empty_like(scores)
    for t in range(T):
        out[..., t] = np.median(scores[..., max(0, t - half):min(T, t + half + 1)], axis=-1)
    return out


def decide(scores, power, rule=None):
    """scores (K,T), power (T,) -> bool (K,T): which frames each class is active in.  In this
    order: scores of frames with power < rule.power_floor * max(power) become 0; running median
    (`running_median`); hysteresis (start off, on when >= rule.on, stay on while >= rule.off);
    off-runs shorter than rule.min_off_frames between two on-runs are filled; on-runs shorter
    than rule.min_on_frames are dropped."""
    rule = ActivityRule() if rule is None else rule
    scores = np.array(scores, dtype=np.float64)
    power = np.asarray(power, dtype=np.float64)
    if scores.ndim != 2:
        raise ValueError(f'scores: shape {scores.shape} is not (K,T)')
    K, T = scores.shape
    if power.shape != (T,):
        raise ValueError(f'power: shape {power.shape} is not ({T},)')
    active = np.zeros((K, T), dtype=bool)
    if T == 0:
        return active
    scores[:, power < rule.power_floor * np.max(power)] = 0.0
    smooth = running_median(scores, rule.median_frames)
    for k in range(K):
        on = False
        for t in range(T):
            on = smooth[k, t] >= (rule.off if on else rule.on)
            active[k, t] = on
        runs = _runs(active[k])
        for (_, b), (a, _) in zip(runs[:-1], runs[1:]):
            if a - b < rule.min_off_frames:
                active[k, b:a] = True
        for a, b in _runs(active[k]):
            if b - a < rule.min_on_frames:
                active[k, a:b] = False
    return active


def frames_to_intervals(active_row, size, shift, fading, num_samples):
    """The on-runs of one class as sample intervals [(start, end), ...] of the window the STFT
    was taken of.  Frame t starts at sample t * shift - pad (pad = size - shift with fading, else
    0) and has its centre at c_t = t * shift - pad + size // 2; a run of frames [a, b) becomes
    [c_a - shift // 2, c_(b-1) + shift - shift // 2), clipped to [0, num_samples); what is empty
    after that is dropped.  Adjacent runs give adjacent intervals that do not overlap."""
    row = np.asarray(active_row)
    if row.ndim != 1:
        raise ValueError(f'active_row: shape {row.shape} is not (T,)')
    size, shift, num_samples = int(size), int(shift), int(num_samples)
    pad = size - shift if fading else 0

    def centre(t):
        return t * shift - pad + size // 2

    out = []
    for a, b in _runs(row):
        start = max(centre(a) - shift // 2, 0)
        end = min(centre(b - 1) + shift - shift // 2, num_samples)
        if end > start:
            out.append((start, end))
    return out


def clip_intervals(intervals, lo, hi):
    """The parts of [(start, end), ...] inside [lo, hi)."""
    out = ((max(a, lo), min(b, hi)) for a, b in intervals)
    return [(a, b) for a, b in out if b > a]


def _seconds(samples, sample_rate):
    """samples / sample_rate as an exact decimal string."""
    samples, sample_rate = int(samples), int(sample_rate)
    # the fraction terminates when its reduced denominator has no prime factor but 2 and 5
    den = sample_rate // math.gcd(samples, sample_rate)
    for prime in (2, 5):
        while den % prime == 0:
            den //= prime
    if den != 1:
        raise ValueError(f'{samples} samples at {sample_rate} Hz have no exact decimal form')
    with decimal.localcontext() as context:
        context.prec = 100
        return format(decimal.Decimal(samples) / decimal.Decimal(sample_rate), 'f')


def write_rttm(path, file_id, intervals, sample_rate=16000):
    """Write ``{speaker: [(start, end), ...]}`` (samples) as
    ``SPEAKER <file_id> 1 <begin> <dur> <NA> <NA> <speaker> <NA> <NA>`` lines.  The seconds are
    printed exactly (decimal.Decimal(samples) / sample_rate, never through float formatting):
    `database.chime5.rttm.from_rttm` asserts that they are whole samples and reads the file back
    to the same intervals (overlapping lines are united there)."""
    lines = []
    for speaker, spans in intervals.items():
        for start, end in spans:
            start, end = int(start), int(end)
            if not 0 <= start < end:
                raise ValueError(f'{speaker}: interval ({start}, {end}) is empty or negative')
            lines.append(f'SPEAKER {file_id} 1 {_seconds(start, sample_rate)} '
                         f'{_seconds(end - start, sample_rate)} <NA> <NA> {speaker} <NA> <NA>')
    Path(path).write_text(''.join(line + '\n' for line in lines))
    return len(lines)
