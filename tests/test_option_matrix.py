"""What every option of the one-target pipeline, alone and in pairs, does to every public method
of an enhancer -- recorded once, in tests/golden/option_matrix.json, and held entry for entry.

An entry is a string: the exception class and its full message, or the marker that the call got
as far as the device (the contexts raise here, as in the ``no_context`` fixtures of the
``test_*_api.py`` modules) or as far as the session's iterator (which raises a sentinel).  The
file is written by this module, ``python tests/test_option_matrix.py --write``, from the code as
it stands: a change of a message or of the order of two refusals shows as a diff of that file.

No GPU: nothing here reaches a kernel.
"""
import contextlib
import inspect
import itertools
import json
import sys
import tempfile
from pathlib import Path
from unittest import mock

import numpy as np

GOLDEN = Path(__file__).resolve().parent / 'golden' / 'option_matrix.json'

# every single option, by the name it has in the file
OPTIONS = {
    'bf_segment_frames': dict(bf_segment_frames=64),
    'bf_null_interferer': dict(bf_null_interferer=True),
    'channel_keep': dict(channel_keep=3),
    'bf=wpdSouden_ban': dict(bf='wpdSouden_ban'),
    'bf=wpdSouden': dict(bf='wpdSouden'),
    'bf_online': dict(bf_online=True),
    'gss_online': dict(gss_online=True),
    'wpe_online': dict(wpe_online=True),
    'wpe_per_array': dict(wpe_per_array=True, multiarray=True),
    'bf=gev_ban': dict(bf='gev_ban'),
    'bf=ch2': dict(bf='ch2'),
    'bf=sum': dict(bf='sum'),
    'wpe=False': dict(wpe=False),
}

FRONT_DOORS = ('core', 'core_chime6')
SESSION, ARRAY, SPEAKERS = 'S02', 'U01', ('P05', 'P06')
D, N = 4, 4096
AT_DEVICE, AT_ITERATOR, RETURNED = '<reached the device>', '<reached the iterator>', '<returned>'


class _Device(Exception):
    pass


class _Iterator(Exception):
    pass


def configurations():
    """name -> get_enhancer keywords: the plain enhancer, every option, every unordered pair of
    options (two values of ``bf`` are no pair: one keyword holds one of them)."""
    configs = {'plain': {}}
    configs.update(OPTIONS)
    for (a, kw_a), (b, kw_b) in itertools.combinations(OPTIONS.items(), 2):
        if set(kw_a) & set(kw_b):
            continue
        configs[f'{a} + {b}'] = {**kw_a, **kw_b}
    return configs


@contextlib.contextmanager
def no_device():
    """Any attempt to create or fetch a device context raises `_Device`."""
    from pb_chime5_amd import _capi, ops

    def boom(*a, **k):
        raise _Device
    with mock.patch.object(_capi, 'default_context', boom), \
            mock.patch.object(ops, 'default_context', boom), \
            mock.patch.object(_capi.Context, '__init__', boom):
        yield


def _outcome(call, tmp):
    try:
        call()
    except _Device:
        return AT_DEVICE
    except _Iterator:
        return AT_ITERATOR
    except Exception as e:      # noqa: BLE001  (the outcome IS the exception)
        return f'{type(e).__name__}: {e}'.replace(str(tmp), '<tmp>')
    return RETURNED


def _scene(door, tmp):
    """The zero observation, its activity (two speakers and the noise track) and an example that
    loads the same from a four-channel file, in the front door's example format."""
    from pb_chime5_amd.io import dump_audio
    obs = np.zeros((D, N))
    wav = tmp / 'zeros.wav'
    if not wav.exists():
        dump_audio(obs, wav, normalize=False)
    tracks = {SPEAKERS[0]: np.ones(N, bool), SPEAKERS[1]: np.arange(N) >= N // 2,
              'Noise': np.ones(N, bool)}
    ex = dict(session_id=SESSION, speaker_id=SPEAKERS[0], example_id='zeros',
              reference_array=ARRAY, audio_path={'observation': {ARRAY: str(wav)}})
    if door == 'core':
        store = {SESSION: {ARRAY: tracks}}
        for key, value in (('start', 0), ('end', N), ('start_orig', 0), ('end_orig', N),
                           ('num_samples', N), ('num_samples_orig', N)):
            ex[key] = {'original': value, 'observation': {ARRAY: value}}
    else:
        store = {SESSION: tracks}
        ex.update(start=0, end=N, start_orig=0, end_orig=N, num_samples=N, num_samples_orig=N)
    return obs, tracks, ex, store


def _calls(enhancer, obs, tracks, ex, tmp):
    """name -> the call of every public method, in a fixed order."""
    from pb_chime5_amd import ops
    e, who = enhancer, SPEAKERS[0]
    T = ops.stft_frames(N, e.stft_size, e.stft_shift, e.stft_fading)
    guidance = {k: np.ones(T) for k in tracks}
    out = str(tmp / 'audio')
    return {
        'enhance_observation(fused=True)':
            lambda: e.enhance_observation(obs, tracks, who, ex=ex, fused=True),
        'enhance_observation(fused=False)':
            lambda: e.enhance_observation(obs, tracks, who, ex=ex, fused=False),
        'enhance_observation_activity': lambda: e.enhance_observation_activity(obs, tracks, who, ex=ex),
        'enhance_example_activity': lambda: e.enhance_example_activity(ex),
        'enhance_observation_guided': lambda: e.enhance_observation_guided(obs, guidance, who, ex=ex),
        'enhance_observation_speakers': lambda: e.enhance_observation_speakers(obs, tracks, ex=ex),
        'enhance_example_speakers': lambda: e.enhance_example_speakers(ex),
        'enhance_observation_blind': lambda: e.enhance_observation_blind(obs, 2, ex=ex),
        'enhance_recording_blind': lambda: e.enhance_recording_blind(
            obs, 2, window_samples=2048, hop_samples=1024),
        'enhance_example_blind': lambda: e.enhance_example_blind(ex, 2),
        'enhance_session': lambda: e.enhance_session(SESSION, out, audio_dir_exist_ok=True),
        'enhance_session(refined_rttm=True)': lambda: e.enhance_session(
            SESSION, out, audio_dir_exist_ok=True, refined_rttm=True),
    }


def record(tmp):
    """The whole matrix: door -> configuration -> {'constructor': outcome, 'calls': {...}}."""
    import importlib

    def iterator_factory(session_ids, context_samples):
        raise _Iterator

    matrix = {}
    with no_device():
        for door in FRONT_DOORS:
            module = importlib.import_module(f'pb_chime5_amd.{door}')
            obs, tracks, ex, store = _scene(door, tmp)
            matrix[door] = {}
            for name, kw in configurations().items():
                made = []
                entry = {'constructor': _outcome(lambda: made.append(module.get_enhancer(
                    activity_store=store, iterator_factory=iterator_factory, **kw)), tmp)}
                if made:
                    entry['calls'] = {what: _outcome(call, tmp) for what, call in
                                      _calls(made[0], obs, tracks, ex, tmp).items()}
                matrix[door][name] = entry
    return matrix


def test_every_option_and_pair_keeps_its_recorded_outcome(tmp_path):
    want = json.loads(GOLDEN.read_text())
    got = record(tmp_path)
    assert set(got) == set(want)
    for door in want:
        assert list(got[door]) == list(want[door]), door
        for name in want[door]:
            assert got[door][name] == want[door][name], (door, name)


def test_the_matrix_is_the_one_the_issue_names():
    configs = configurations()
    singles = len(OPTIONS)
    bf_values = sum('bf' in kw for kw in OPTIONS.values())
    assert len(configs) == 1 + singles + singles * (singles - 1) // 2 \
        - bf_values * (bf_values - 1) // 2
    want = json.loads(GOLDEN.read_text())
    assert all(list(want[door]) == list(configs) for door in FRONT_DOORS)
    # the file says something: constructors that refuse, calls that refuse, calls that run
    flat = [o for door in want.values() for e in door.values()
            for o in [e['constructor'], *e.get('calls', {}).values()]]
    assert AT_DEVICE in flat and AT_ITERATOR in flat
    assert sum(o.startswith('NotImplementedError: ') for o in flat) > 100


# ------------------------------------------------------------------ the three front doors
def _front_door_signatures():
    from pb_chime5_amd import core, core_chime6, core_chime6_rttm
    return {m.__name__: inspect.signature(m.get_enhancer).parameters
            for m in (core, core_chime6, core_chime6_rttm)}


def test_front_doors_share_defaults_and_the_block_keywords():
    """A keyword that more than one ``get_enhancer`` has carries one default (``multiarray``
    apart: the RTTM front door's is the reference's 'outer_array_mics'), and every keyword of the
    shared construction of the blocks is a keyword of all three."""
    from pb_chime5_amd import core
    doors = _front_door_signatures()
    shared = set.intersection(*(set(p) for p in doors.values()))
    assert len(shared) > 30
    for name in sorted(shared - {'multiarray'}):
        defaults = {door: p[name].default for door, p in doors.items()}
        assert len(set(map(repr, defaults.values()))) == 1, (name, defaults)
    blocks = inspect.signature(core._enhancer_fields).parameters
    assert len(blocks) > 30
    for name in blocks:
        assert name in shared, name


if __name__ == '__main__':
    if sys.argv[1:] != ['--write']:
        sys.exit('usage: python tests/test_option_matrix.py --write')
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    with tempfile.TemporaryDirectory() as d:
        GOLDEN.write_text(json.dumps(record(Path(d)), indent=1) + '\n')
    print(f'wrote {GOLDEN}')
