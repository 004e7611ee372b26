"""The C-ABI library loads without a GPU and exports every symbol that
include/gss_hip.h declares (no compute calls here)."""
import re

import pytest

from conftest import REPO


def _declared_functions():
    text = (REPO / 'include' / 'gss_hip.h').read_text()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(gss_[a-z0-9_]+)\s*\(', text)))


def test_library_builds_and_exports_every_declared_symbol():
    from pb_chime5_amd import build, _capi
    build.build(verbose=False)
    lib = _capi.load_library()
    names = _declared_functions()
    assert len(names) >= 25, names
    for name in names:
        assert hasattr(lib, name), f'{name} is declared in gss_hip.h but not exported'
    # the ctypes prototypes cover exactly the declared functions
    assert sorted(_capi.SIGNATURES) == names
    assert b'gfx950' in lib.gss_version()


def test_every_fused_entry_has_a_caller_in_the_binding():
    """Each gss_enhance_observation* prototype is an entry of the binding's call table (or its
    pcm16 twin), or one of the entries with a head of their own; the table names no other."""
    from pb_chime5_amd import _capi, ops
    table = {name for entry, twin, _ in ops._FUSED_ENTRIES.values() for name in (entry, twin)
             if name is not None}
    assert table <= set(_capi.SIGNATURES), sorted(table - set(_capi.SIGNATURES))
    own_head = {'gss_enhance_observation_guided', 'gss_enhance_observation_targets',
                'gss_enhance_observation_targets_pcm16', 'gss_enhance_observation_host'}
    fused = {name for name in _capi.SIGNATURES if name.startswith('gss_enhance_observation')}
    assert fused - own_head == table, sorted((fused - own_head) ^ table)


def test_geometry_helpers_match_oracle():
    import gss_oracle as oracle
    from pb_chime5_amd import ops
    for size, shift in ((1024, 256), (512, 128), (64, 16), (4, 2)):
        for fading in (True, False):
            for n in (0, 1, 5, 255, 256, 257, 1000, 1024, 1025, 5000, 80000, 240000):
                assert ops.stft_frames(n, size, shift, fading) == \
                    oracle.stft(__import__('numpy').zeros(n), size, shift, fading=fading,
                                window=__import__('numpy').ones(size)).shape[0], (size, shift, fading, n)
            for s in (0, 1, 255, 256, 257, 16000, 240000):
                assert ops.samples_to_stft_frames(s, size, shift, fading=fading) == \
                    oracle.samples_to_stft_frames(s, size, shift, fading=fading)


def test_no_gpu_means_loud_failure():
    """The product path must not fall back to anything when no GPU is present."""
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from pb_chime5_amd import _capi
    with pytest.raises(_capi.GssError):
        _capi.Context(0)


def test_product_does_not_import_oracle():
    import ast
    pkg = REPO / 'pb_chime5_amd'
    for path in pkg.rglob('*.py'):
        tree = ast.parse(path.read_text())
        for node in ast.walk(tree):
            names = []
            if isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                names = [node.module or '']
            for n in names:
                assert 'oracle' not in n, (path, n)


def test_psd_context_is_validated_in_one_place():
    """nara_wpe accepts an int, a (left, right) tuple and np.inf; only the symmetric integer
    window is implemented -- everything else is NotImplementedError (never a silent
    truncation, never TypeError / OverflowError out of int())."""
    import numpy as np
    from pb_chime5_amd import ops
    assert ops.check_psd_context(0) == 0 and ops.check_psd_context(np.int64(3)) == 3
    assert ops.check_psd_context(2.0) == 2
    assert ops.check_psd_context(np.inf) == ops.PSD_CONTEXT_ALL == 2 ** 31 - 1
    for bad in (-np.inf, float('nan'), 1.5, (1, 2), -1, None, 'a', True):
        with pytest.raises(NotImplementedError):
            ops.check_psd_context(bad)
    assert ops.make_params(wpe_psd_context=np.inf).wpe_psd_context == 2 ** 31 - 1


def test_abi_revision_is_checked_on_load(tmp_path):
    from pb_chime5_amd import _capi
    lib = _capi.load_library()
    assert lib.gss_abi_version() == _capi.GSS_ABI_VERSION
    text = (REPO / 'include' / 'gss_hip.h').read_text()
    assert f'#define GSS_ABI_VERSION {_capi.GSS_ABI_VERSION}' in text


def test_beamformer_status_word_maps_to_the_reference_exceptions():
    """gss_last_ref_channel: -1 -> AssertionError (non-finite SNR, pb_bss
    get_optimal_reference_channel), -2 - f -> numpy.linalg.LinAlgError naming frequency f
    (scipy.linalg.eigh in get_gev_vector); channels and the "nothing ran yet" word pass."""
    import numpy as np
    from pb_chime5_amd import ops
    for ok in (0, 3, 23, -2 ** 31):
        ops._raise_for_ref_channel(ok)
    with pytest.raises(AssertionError, match='S02_U01: .*SNR is not finite'):
        ops._raise_for_ref_channel(-1, 'S02_U01')
    with pytest.raises(np.linalg.LinAlgError, match='frequency 17'):
        ops._raise_for_ref_channel(-2 - 17)
    with pytest.raises(np.linalg.LinAlgError, match='frequency 0'):
        ops._raise_for_ref_channel(-2)


def test_variant_keys_are_documented_and_used():
    """GSS_VARIANT: the keys the library accepts (csrc/gss_api.hip) are the keys INTEGRATION.md
    documents and the keys the kernels' host code asks for -- no switch without a reader, no
    reader without a switch, and no direct getenv left in the kernels' translation units."""
    import re
    csrc = REPO / 'pb_chime5_amd' / 'csrc'
    api = (csrc / 'gss_api.hip').read_text()
    table = api[api.index('kVariantKeys[] = {'):api.index('};', api.index('kVariantKeys[] = {'))]
    accepted = set(re.findall(r'"([a-z0-9_]+)"', table))
    used = set()
    for name in ('wpe.hip', 'cacgmm.hip', 'stft.hip', 'mvdr.hip'):
        text = (csrc / name).read_text()
        used |= set(re.findall(r'gss_variant(?:_set)?\("([a-z0-9_]+)"', text))
        assert 'getenv' not in text, name
    # (the fused pipeline's own switch lives in gss_api.hip, next to the one getenv of the library)
    used |= set(re.findall(r'gss_variant(?:_set)?\("([a-z0-9_]+)"', api))
    assert used == accepted, (sorted(used - accepted), sorted(accepted - used))
    doc = (REPO / 'INTEGRATION.md').read_text()
    section = doc[doc.index('## Debug switches'):doc.index('## Replacing `mpiexec')]
    documented = set(re.findall(r'`([a-z0-9_]+)(?:=[^`]*)?`', section)) & (accepted | used)
    assert documented == accepted, sorted(accepted - documented)


def test_step_flops_and_traffic_provenance(tmp_path):
    """bench.py's bookkeeping: the executed flops of a whole step (the `f64_peak_frac` of the
    line: 0.58 at the headline's 14 ms, the figure the round-5 review computed by hand as 0.59)
    and the provenance stamp of a PMC traffic file (source hashes of the dominant kernel's
    translation unit: a stale figure must not travel inside a fresh line)."""
    from pb_chime5_amd import roofline
    shape = dict(F=513, T=941, D=24, K=5, taps=10, N=240000)
    r = roofline.step_peak_frac(14.0, **shape)
    assert 600 < r['executed_gflop_per_step'] < 680 and 0.55 < r['frac'] < 0.62
    assert r['min_gflop_per_step'] < r['executed_gflop_per_step']
    # the dominant kernel dominates the count, as it dominates the step
    corr = roofline.kernel_work('wpe_corr', **shape)
    assert 0.45 < 3 * corr['executed_flops'] / (r['executed_gflop_per_step'] * 1e9) < 0.6
    # frames the correlation's MFMAs run over: whole 64-frame chunks, except that the persistent
    # 32 x 32 kernel runs a short last chunk (<= 48 frames) in groups of 16 (wpe.hip,
    # corr_item_dma); the executed count never falls below the frames that exist
    def frames(T, D):
        w = roofline.kernel_work('wpe_corr', F=1, T=T, D=D, K=5, taps=10, N=0)
        return w['executed_flops'] / roofline.kernel_work('wpe_corr', F=1, T=64, D=D, K=5, taps=10,
                                                          N=0)['executed_flops'] * 64
    assert [round(frames(T, 24)) for T in (941, 944, 945, 960, 961, 1009, 2169, 10)] == \
        [944, 944, 960, 960, 976, 1024, 2176, 16]
    assert [round(frames(T, 4)) for T in (941, 2169, 10)] == [960, 2176, 64]
    one = roofline.step_peak_frac(2.3, F=513, T=2169, D=4, K=5, taps=10, N=554490)
    assert one['frac_min_flops'] < one['frac'] < 0.35
    assert roofline.kernel_sources('wpe_corr')[0] == 'wpe.hip'
    assert roofline.kernel_sources('em_mstep')[0] == 'cacgmm.hip'
    assert roofline.kernel_sources('psd')[0] == 'mvdr.hip'
    hashes = roofline.source_hashes()
    assert {'wpe.hip', 'cacgmm.hip', 'mvdr.hip', 'stft.hip', 'gss_api.hip', 'gss_internal.h'} <= set(hashes)


def test_occupancy_budgets_of_the_resident_kernels(tmp_path):
    """Kernels whose launch shape depends on how many workgroups a CU holds, checked in the code
    objects of the in-tree build (llvm-objdump --offloading + llvm-readelf --notes):
    * em_onchip4_kernel<K> (one array: 513 workgroups on 256 CUs) must fit THREE workgroups per
      CU for every K -- LDS <= 160 KB / 3 and <= 168 VGPRs --, or the 513th workgroup runs alone
      in a second round (a 1.5 KB array added in round 6 cost K = 6 exactly that until it moved
      to global memory);
    * the single-wave / frame-splitting correlation kernels of one array fit four waves per SIMD
      (<= 128 VGPRs): at 138 the last 6 of 3078 waves ran in a second round."""
    import re
    import shutil
    import subprocess
    from pathlib import Path
    llvm = Path("/opt/rocm/lib/llvm/bin")
    lib = REPO / 'pb_chime5_amd' / 'lib'
    if not (llvm / 'llvm-readelf').exists() or not (lib / 'cacgmm.o').exists():
        pytest.skip('llvm-readelf or the per-unit objects of an in-tree build are missing')
    from pb_chime5_amd import build
    build.build(verbose=False)                      # objects of the CURRENT sources

    def kernels(unit):
        obj = tmp_path / f'{unit}.o'
        shutil.copy(lib / f'{unit}.o', obj)
        subprocess.run([str(llvm / 'llvm-objdump'), '--offloading', str(obj)], check=True,
                       capture_output=True, cwd=tmp_path)
        co = next(tmp_path.glob(f'{unit}.o.*gfx950*'))
        notes = subprocess.run([str(llvm / 'llvm-readelf'), '--notes', str(co)], check=True,
                               capture_output=True, text=True).stdout
        out = {}
        for block in notes.split('  - .agpr_count:')[1:]:
            name = re.search(r'\.name:\s+(\S+)', block).group(1)
            out[name] = {k: int(re.search(rf'\.{k}:\s+(\d+)', block).group(1))
                         for k in ('group_segment_fixed_size', 'vgpr_count', 'private_segment_fixed_size')}
        return out
    em = {n: v for n, v in kernels('cacgmm').items() if 'em_onchip4_kernel' in n}
    assert len(em) == 5, sorted(em)                 # K = 2 ... 6
    for name, meta in em.items():
        assert meta['group_segment_fixed_size'] <= 160 * 1024 // 3, (name, meta)
        assert meta['vgpr_count'] <= 168, (name, meta)
    corr = {n: v for n, v in kernels('wpe').items()
            if 'wpe_corr_ksplit_kernelILi4ELi5E' in n or 'wpe_corr_kernelILi1ELi1ELi5E' in n}
    assert len(corr) == 2, sorted(corr)
    for name, meta in corr.items():
        assert meta['vgpr_count'] <= 128 and meta['private_segment_fixed_size'] == 0, (name, meta)
