"""Every option of `Enhancer.enhance_observation` and every unordered pair of options that reaches
the device (tests/test_option_matrix.py records which), run on the GPU with ``fused=True`` and
``fused=False`` and refereed stage by stage: tests/pipeline_stage_reference.py applies the CPU
reference of each stage to the run's own input of that stage, at the stage's own bar.

* outcome: the call runs, or raises what tests/golden/option_matrix_gpu.json holds for it, entry
  for entry (`python tests/test_gpu_option_matrix.py --write` on a GPU machine writes that file
  and prints the table of tests/OPTION_MATRIX_GPU.md);
* stages: every distance of `pipeline_stage_reference.referee` below its bar, integers equal;
* the two paths: rel_err(x_hat blocks, x_hat fused) < 1e-10 where both run
  (test_gpu_pipeline.test_block_by_block_path_equals_fused); where one refuses, its message names
  the other;
* the option acts: x_hat of a pair differs by more than 1e-4 from that of each of its two single
  options on the pair's scene, but for SAME_SIGNAL;
* workspace: every pair that runs fused, on a context of this module's own in the workspace debug
  mode under both poison patterns: no guard violation, equal bits, the stage bars.

The CPU tests hold the list of configurations to the recorded matrix and re-check a sample of the
scene table.
"""
import json
import sys
import time
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import pipeline_stage_reference as psr      # noqa: E402
import test_option_matrix as om             # noqa: E402

gpu = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / 'golden' / 'option_matrix_gpu.json'
RAN = '<ran>'
PATHS = {True: 'fused=True', False: 'fused=False'}
PATHS_TOL = 1e-10       # test_gpu_pipeline.test_block_by_block_path_equals_fused
ACTS_TOL = 1e-4         # the feature modules' bar against "option silently ignored"
PATTERNS = (0x00, 0xFF)

FUSED = psr.device_configurations('fused=True')
BLOCKS = psr.device_configurations('fused=False')
CONFIGS = [name for name in om.configurations() if name in FUSED or name in BLOCKS]
PAIRS = [name for name in CONFIGS if ' + ' in name]
# (pair, the single option it equals): the other option cannot change the signal there
SAME_SIGNAL = {
    ('wpe_per_array + wpe=False', 'wpe=False'): 'without a WPE block nothing runs per array',
    ('gss_online + bf=ch2', 'bf=ch2'): 'a channel pick reads no mask',
    ('gss_online + bf=sum', 'bf=sum'): 'the channel sum reads no mask',
}


# ================================================================== CPU
def test_the_configurations_are_the_recorded_device_reaching_ones():
    """The fused cells are exactly the configurations whose recorded
    ``enhance_observation(fused=True)`` reached the device; the others of the matrix run on the
    stage path only and their recorded fused outcome is a refusal that names it."""
    recorded = json.loads(om.GOLDEN.read_text())['core']
    calls = {name: e.get('calls', {}) for name, e in recorded.items()}
    assert FUSED == [n for n in om.configurations()
                     if calls[n].get('enhance_observation(fused=True)') == om.AT_DEVICE]
    assert set(FUSED) <= set(BLOCKS) and CONFIGS == BLOCKS
    assert len(CONFIGS) == 49 and len(FUSED) == 45 and len(PAIRS) == 35
    for name in sorted(set(CONFIGS) - set(FUSED)):
        text = calls[name]['enhance_observation(fused=True)']
        assert text.startswith('NotImplementedError: ') and 'fused=False' in text, (name, text)
    assert set(psr.SCENES) == set(CONFIGS)
    held = json.loads(GOLDEN.read_text())
    assert list(held) == CONFIGS and all(list(v) == list(PATHS.values()) for v in held.values())
    for (pair, single), _ in SAME_SIGNAL.items():
        assert pair in PAIRS and single in pair.split(' + ')


def test_the_stability_sample_names_every_referee():
    kinds = {(psr.config(n).obs, psr.config(n).posterior, psr.config(n).beamformer)
             for n in psr.STABILITY_SAMPLE}
    every = {(psr.config(n).obs, psr.config(n).posterior, psr.config(n).beamformer)
             for n in CONFIGS}
    for i in range(3):
        assert {k[i] for k in kinds} == {k[i] for k in every}, i
    assert any(psr.config(n).keep for n in psr.STABILITY_SAMPLE)


@pytest.mark.parametrize('name', psr.STABILITY_SAMPLE)
def test_scenes_are_stable_for_the_referees(name):
    """The rule that keeps a scene, re-checked: every stage's referee moves STABILITY_MARGIN x
    less than the stage's bar under a last-bit change of the stage's input, and the CPU chain
    passes its own referees."""
    u = psr.scene(name)
    run = psr.cpu_chain(name, u)
    moved = psr.movements(name, u, run)
    print(f'{name}: scene {psr.SCENES[name]}, the referees move '
          + ', '.join(f'{s} {v:.1e} (bar {psr.bar(name, s):.1e})' for s, v in moved.items()))
    assert not psr.unstable(name, moved), moved
    rows = psr.referee(name, u, run)
    assert not psr.failures(rows), psr.show(rows)


# ================================================================== GPU: running a cell
def _enhancer(name):
    from pb_chime5_amd.core import get_enhancer
    return get_enhancer(**psr.keywords(name))


def _call(name, fused, scene_of=None, ctx=None):
    """-> (outcome, taps or None, seconds): configuration ``name`` on the scene of ``scene_of``."""
    scene_of = scene_of or name
    u = psr.scene(scene_of)
    enh = _enhancer(name)
    if ctx is not None:
        enh._ctx = lambda: ctx
    arrays = psr.config(scene_of).arrays if psr.config(name).per_array else None
    t0 = time.perf_counter()
    try:
        x_hat = enh.enhance_observation(u.obs, u.activity, u.speaker_id, ex=u.ex, debug=True,
                                        fused=fused, wpe_arrays=arrays)
    except Exception as e:      # noqa: BLE001  (the outcome IS the exception)
        return f'{type(e).__name__}: {e}', None, time.perf_counter() - t0
    seconds = time.perf_counter() - t0
    return RAN, _taps(name, enh, x_hat, fused), seconds


def _taps(name, enh, x_hat, fused):
    c = psr.config(name)
    loc = enh.enhance_observation_locals
    ctx = enh._ctx()
    run = {k: loc[k] for k in ('Obs', 'acitivity_freq', 'masks', 'target_mask', 'distortion_mask',
                               'X_hat')}
    run['x_hat'] = x_hat
    for k in ('selected_channels', 'interferer_index', 'interferer_mask'):
        if k in loc:
            run[k] = loc[k]
    assert ('selected_channels' in run) == (c.keep is not None)
    assert ('interferer_index' in run) == (c.beamformer == 'lcmv')
    if fused:
        run['posterior'] = loc['details']['posterior']
    if c.beamformer in ('mvdr', 'online', 'lcmv', 'segments', 'wpd'):
        run['ref_channel'] = ctx.last_ref_channel()
        if fused:
            assert loc['details']['ref_channel'] == run['ref_channel']
    run['fallbacks'] = {}
    if c.posterior == 'online':
        run['fallbacks']['posterior'] = ctx.last_cacgmm_online_fallbacks()
    counter = {'segments': ctx.last_segment_fallbacks, 'lcmv': ctx.last_lcmv_fallbacks,
               'online': ctx.last_mvdr_online_fallbacks}.get(c.beamformer)
    if counter is not None:
        run['fallbacks']['X_hat'] = counter()
    return run


_CELLS = {}


def _cell(name, fused, scene_of=None):
    """A run on the session's context, made once and shared, its arrays read-only."""
    key = (name, fused, scene_of or name)
    if key not in _CELLS:
        outcome, run, seconds = _call(name, fused, scene_of)
        for v in (run or {}).values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CELLS[key] = (outcome, run, seconds)
    return _CELLS[key]


def _refereed(name, u, run, what):
    rows = psr.referee(name, u, run)
    print(f'{what}:\n{psr.show(rows)}')
    stages = {r[0] for r in rows}
    assert stages >= set(psr.STAGES) - ({'selection'} if psr.config(name).keep is None else set())
    bad = psr.failures(rows)
    assert not bad, f'{what}:\n{psr.show(bad)}'
    return rows


# ================================================================== GPU: the tests
@gpu
@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'blocks'])
@pytest.mark.parametrize('name', CONFIGS)
def test_outcome_and_every_stage(gpu_ctx, name, fused):
    held = json.loads(GOLDEN.read_text())[name][PATHS[fused]]
    outcome, run, seconds = _cell(name, fused)
    print(f'{name} [{PATHS[fused]}]: {outcome} ({seconds:.2f} s)')
    assert outcome == held
    assert (outcome == RAN) == (name in (FUSED if fused else BLOCKS))
    if run is not None:
        _refereed(name, psr.scene(name), run, f'{name} [{PATHS[fused]}]')


@gpu
@pytest.mark.parametrize('name', CONFIGS)
def test_the_two_paths_agree(gpu_ctx, name):
    (a, fused, _), (b, blocks, _) = _cell(name, True), _cell(name, False)
    assert RAN in (a, b), (a, b)
    if fused is None:
        assert 'fused=False' in a, a
        return
    if blocks is None:
        assert 'fused=True' in b, b
        return
    err = psr.rel_err(blocks['x_hat'], fused['x_hat'])
    print(f'{name}: block path vs fused {err:.1e}')
    assert err < PATHS_TOL


@gpu
@pytest.mark.parametrize('name', PAIRS)
def test_each_option_of_a_pair_acts(gpu_ctx, name):
    """x_hat of the pair against x_hat of each of its two options alone, on the pair's scene."""
    fused = name in FUSED
    pair = _cell(name, fused)[1]['x_hat']
    for single in name.split(' + '):
        outcome, run, _ = _cell(single, fused, scene_of=name)
        assert outcome == RAN, (single, outcome)
        err = psr.rel_err(pair, run['x_hat'])
        print(f'{name} vs {single} alone: {err:.1e}')
        if (name, single) in SAME_SIGNAL:
            assert err < PATHS_TOL, SAME_SIGNAL[name, single]     # (the same signal indeed)
        else:
            assert err > ACTS_TOL, (name, single, err)


@pytest.fixture(scope='module')
def hctx():
    """The module's own context: the session's `gpu_ctx` is never put into the debug mode, and
    this one runs only this module's pairs, in parameter order."""
    from pb_chime5_amd._capi import Context
    ctx = Context(0)
    yield ctx
    ctx.close()


def _bits(value):
    if isinstance(value, np.ndarray):
        return value.dtype.str, value.shape, np.ascontiguousarray(value).tobytes()
    return value


@gpu
@pytest.mark.parametrize('name', [n for n in PAIRS if n in FUSED])
def test_workspace_hygiene_of_the_pair(hctx, name):
    """(the helper of tests/test_gpu_workspace_hygiene.py, restated as in
    tests/test_gpu_cacgmm_online.py: importing that module imports most of the suite)"""
    outs = {}
    for pattern in PATTERNS:
        hctx.debug_workspace(pattern)
        try:
            outcome, run, _ = _call(name, True, ctx=hctx)
            count, text, _ = hctx.debug_workspace_report()
        finally:
            hctx.debug_workspace(None)
        print(f'{name} [0x{pattern:02X}]: {outcome}, {count} guard violations {text}')
        assert outcome == RAN
        assert count == 0, f'{name} [0x{pattern:02X}]: {text}'
        outs[pattern] = run
    a, b = outs[0x00], outs[0xFF]
    assert sorted(a) == sorted(b)
    differ = [k for k in sorted(a) if _bits(a[k]) != _bits(b[k])]
    assert not differ, f'{name}: {differ} depend on what the workspace held'
    _refereed(name, psr.scene(name), b, f'{name} [poisoned workspace]')


# ================================================================== writing the held outcomes
def _write():
    from pb_chime5_amd._capi import default_context
    default_context(0)
    held, lines = {}, []
    t0 = time.perf_counter()
    for name in CONFIGS:
        held[name] = {}
        for fused, path in PATHS.items():
            outcome, run, seconds = _call(name, fused)
            held[name][path] = outcome
            if run is None:
                lines.append(f'| `{name}` | {path} | refused | | {1e3 * seconds:.0f} |')
                continue
            rows = psr.referee(name, psr.scene(name), run)
            worst = {}
            for stage, what, got, limit in rows:
                if isinstance(limit, float) and got >= worst.get((stage, limit), -1):
                    worst[stage, limit] = got
            bad = psr.failures(rows)
            cells = ', '.join(f'{s} {g:.1e} / {l:.1e}' if l else f'{s} bits {"equal" if g == 0 else g}'
                              for (s, l), g in worst.items())
            lines.append(f'| `{name}` | {path} | {"FAILS: " + repr(bad) if bad else "runs"} | '
                         f'{cells} | {1e3 * seconds:.0f} |')
    GOLDEN.write_text(json.dumps(held, indent=1) + '\n')
    print('| configuration | path | outcome | largest distance / bar per stage | ms |')
    print('| --- | --- | --- | --- | --- |')
    print('\n'.join(lines))
    print(f'wrote {GOLDEN} in {time.perf_counter() - t0:.1f} s')


if __name__ == '__main__':
    if sys.argv[1:] != ['--write']:
        sys.exit('usage: python tests/test_gpu_option_matrix.py --write')
    _write()
