"""ctypes binding of include/gss_hip.h (libgss_hip.so).

This is the only place the Python host touches native code.  There is no CPU
fallback: if the library is missing or no GPU is visible the product path raises.
"""
import ctypes
import json
import os
from pathlib import Path

import numpy as np

_LIB = None
LIB_PATH = Path(__file__).resolve().parent / 'lib' / 'libgss_hip.so'

GSS_OK = 0
GSS_ERR_INVALID = -1
GSS_ERR_HIP = -2
GSS_ERR_NOMEM = -3
GSS_ERR_UNSUPPORTED = -4
GSS_ABI_VERSION = 7       # include/gss_hip.h revision these prototypes are written against

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_int64 = ctypes.c_int64
c_size_t = ctypes.c_size_t


class GssParams(ctypes.Structure):
    _fields_ = [(n, c_int) for n in (
        'stft_size', 'stft_shift', 'stft_fading', 'wpe', 'wpe_taps', 'wpe_delay',
        'wpe_iterations', 'bss_iterations', 'bss_iterations_post',
        'bf_drop_context', 'bf', 'postfilter', 'wpe_psd_context', 'wpe_arrays')]


class GssDebugTaps(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in (
        'Obs_ftd', 'act_frames', 'gamma', 'target_mask', 'distortion_mask',
        'Xhat', 'ref_channel')]


class GssCacgmmModel(ctypes.Structure):
    """gss_cacgmm_model: precision (F,K,D,D) complex, log_det (F,K), weight (F,K) in HBM."""
    _fields_ = [('precision_dev', c_void_p), ('log_det_dev', c_void_p), ('weight_dev', c_void_p)]


class GssAlignPlan(ctypes.Structure):
    """gss_align_plan: host arrays of `entries` int32 values each."""
    _fields_ = [('iterations', c_void_p), ('start', c_void_p), ('end', c_void_p),
                ('entries', ctypes.c_int32)]


class GssGuidance(ctypes.Structure):
    """gss_guidance: element (f, k, t) of a table at [f * f_stride + k * k_stride + t]."""
    _fields_ = [('init_dev', c_void_p), ('mask_dev', c_void_p),
                ('init_f_stride', c_int64), ('init_k_stride', c_int64),
                ('mask_f_stride', c_int64), ('mask_k_stride', c_int64)]


class GssBfSegments(ctypes.Structure):
    """gss_bf_segments: the time span of the beamformer statistics."""
    _fields_ = [('segment_frames', c_int64), ('context_segments', ctypes.c_int32),
                ('min_mass', ctypes.c_double)]


class GssBfLcmv(ctypes.Structure):
    """gss_bf_lcmv: the interferer of the LCMV beamformer and its fallback threshold."""
    _fields_ = [('interferer', ctypes.c_int32), ('candidates', ctypes.c_uint32),
                ('min_mass', ctypes.c_double)]


class GssBfWpd(ctypes.Structure):
    """gss_bf_wpd: the tap window, iterations, BAN and power floor of the WPD beamformer."""
    _fields_ = [('taps', c_int), ('delay', c_int), ('iterations', c_int), ('ban', c_int),
                ('power_floor', ctypes.c_double)]


class GssWpeOnlineState(ctypes.Structure):
    """gss_wpe_online_state: P (F,A,n,n), G (F,A,n,C) and the last taps + delay frames (F,A,L,C)
    of the online WPE, complex, in HBM."""
    _fields_ = [('inv_cov_dev', c_void_p), ('filter_dev', c_void_p), ('history_dev', c_void_p)]


class GssMvdrOnlineState(ctypes.Structure):
    """gss_mvdr_online_state: the running sums Phi_X and Phi_N (F,D,D) of the online MVDR,
    complex, in HBM."""
    _fields_ = [('phi_x', c_void_p), ('phi_n', c_void_p), ('F', ctypes.c_int32),
                ('D', ctypes.c_int32)]


class GssMvdrOnlineHold(ctypes.Structure):
    """gss_mvdr_online_hold: the delay line of the online MVDR's look-ahead -- the held frames
    (F,L,D), their target-mask values (F,L) and the last filter (F,D) in HBM, and the host counter
    `held`, which the library advances."""
    _fields_ = [('frames', c_void_p), ('mask', c_void_p), ('filter', c_void_p),
                ('F', ctypes.c_int32), ('D', ctypes.c_int32), ('L', ctypes.c_int32),
                ('held', ctypes.c_int32)]


class GssBfOnline(ctypes.Structure):
    """gss_bf_online: the online MVDR's forgetting factor, the loading of a fresh state and the
    reference channel (-1: the window's); wpe_online / wpe_alpha are read by the fused entry."""
    _fields_ = [('forget', ctypes.c_double), ('loading', ctypes.c_double),
                ('ref_channel', ctypes.c_int32), ('wpe_online', ctypes.c_int32),
                ('wpe_alpha', ctypes.c_double)]


class GssCacgmmOnlineState(ctypes.Structure):
    """gss_cacgmm_online_state: the running sums S (F,K,D,D), complex, and the masses n (F,K) of
    the online CACGMM, in HBM."""
    _fields_ = [('s', c_void_p), ('n', c_void_p), ('F', ctypes.c_int32), ('K', ctypes.c_int32),
                ('D', ctypes.c_int32)]


class GssEmOnline(ctypes.Structure):
    """gss_em_online: the online CACGMM's forgetting factor and the mass of a fresh state."""
    _fields_ = [('forget', ctypes.c_double), ('prior_mass', ctypes.c_double)]


class GssWpeOnlineCfg(ctypes.Structure):
    """gss_wpe_online_cfg: the forgetting factor of the online WPE in the fused call."""
    _fields_ = [('alpha', ctypes.c_double)]


class GssStreamState(ctypes.Structure):
    """gss_stream_state: the last `size` samples (D,size) and activity bytes (K,size) of a
    sample-block stream, the overlap-add tail (size - shift), in HBM, and the host counters."""
    _fields_ = [('x_hist', c_void_p), ('act_hist', c_void_p), ('ola_tail', c_void_p),
                ('received', c_int64), ('frames_out', c_int64), ('D', ctypes.c_int32),
                ('K', ctypes.c_int32), ('size', ctypes.c_int32), ('shift', ctypes.c_int32)]


class GssStreamCfg(ctypes.Structure):
    """gss_stream_cfg: the forgetting factors of the three online stages of a stream block and
    the beamformer's reference channel."""
    _fields_ = [('wpe_alpha', ctypes.c_double), ('em_forget', ctypes.c_double),
                ('bf_forget', ctypes.c_double), ('ref_channel', ctypes.c_int32)]


class GssChannelSelect(ctypes.Structure):
    """gss_channel_select: the band table and the settings of the envelope-variance channel
    selection."""
    _fields_ = [('bank_dev', c_void_p), ('bands', ctypes.c_int32), ('keep', ctypes.c_int32),
                ('floor', ctypes.c_double)]


_TAPS = ctypes.POINTER(GssDebugTaps)
# what the fused entries start with: ctx, params, obs_dev, D, N, act_dev, K, N_act, and of one
# target its index and the two contexts
_FUSED_HEAD = [c_void_p, ctypes.POINTER(GssParams), c_void_p, c_int, c_int64, c_void_p, c_int,
               c_int64]
_FUSED_TARGET = [c_int, c_int64, c_int64]


def _fused(*inserted, after_out=()):
    """A fused one-target entry: the head, what the entry inserts, out_dev, what it adds behind
    out_dev, the debug taps."""
    return c_int, _FUSED_HEAD + _FUSED_TARGET + list(inserted) + [c_void_p, *after_out, _TAPS]


# (S, target_index, start and end contexts of S targets)
_FUSED_TARGETS = (c_int, _FUSED_HEAD + [c_int, c_void_p, c_void_p, c_void_p, c_void_p, _TAPS])

# name -> (restype, argtypes); every symbol include/gss_hip.h declares
SIGNATURES = {
    'gss_device_count': (c_int, []),
    'gss_device_pci_bus_id': (c_int, [c_int, ctypes.c_char_p, c_int]),
    'gss_create': (c_int, [c_int, ctypes.POINTER(c_void_p)]),
    'gss_destroy': (c_int, [c_void_p]),
    'gss_last_error': (ctypes.c_char_p, [c_void_p]),
    'gss_version': (ctypes.c_char_p, []),
    'gss_abi_version': (c_int, []),
    'gss_set_stream': (c_int, [c_void_p, c_void_p]),
    'gss_set_utterances_in_flight': (c_int, [c_void_p, c_int]),
    'gss_synchronize': (c_int, [c_void_p]),
    'gss_dev_malloc': (c_int, [c_void_p, c_size_t, ctypes.POINTER(c_void_p)]),
    'gss_dev_free': (c_int, [c_void_p, c_void_p]),
    'gss_memcpy_h2d': (c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
    'gss_memcpy_d2h': (c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
    'gss_memset': (c_int, [c_void_p, c_void_p, c_int, c_size_t]),
    'gss_host_malloc': (c_int, [c_void_p, c_size_t, ctypes.POINTER(c_void_p)]),
    'gss_host_free': (c_int, [c_void_p, c_void_p]),
    'gss_memcpy_h2d_async': (c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
    'gss_memcpy_d2h_async': (c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
    'gss_profile_enable': (c_int, [c_void_p, c_int]),
    'gss_profile_filter': (c_int, [c_void_p, ctypes.c_char_p]),
    'gss_profile_reset': (c_int, [c_void_p]),
    'gss_profile_report': (c_int, [c_void_p, ctypes.c_char_p, c_size_t]),
    'gss_stft_num_frames': (c_int64, [c_int64, c_int, c_int, c_int]),
    'gss_istft_num_samples': (c_int64, [c_int64, c_int, c_int, c_int]),
    'gss_samples_to_stft_frames': (c_int64, [c_int64, c_int, c_int, c_int]),
    'gss_set_windows': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    'gss_stft': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p]),
    'gss_istft': (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    'gss_activity_time_to_frequency': (
        c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p]),
    'gss_wpe': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_int,
                        c_int, c_int, c_void_p]),
    'gss_wpe_arrays': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_int, c_int,
                               c_int, c_int, c_void_p]),
    'gss_wpe_inverse_power': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_int,
                                      c_void_p]),
    'gss_cacgmm': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p,
                           c_int, c_int, c_int, c_void_p]),
    'gss_cacgmm_guided': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int,
                                  ctypes.POINTER(GssGuidance), c_int, c_int, c_int, c_void_p]),
    'gss_cacgmm_shared_prior': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int,
                                        ctypes.POINTER(GssGuidance), c_int, c_int, c_int,
                                        c_void_p, c_void_p]),
    'gss_cacgmm_fit': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int,
                               ctypes.POINTER(GssGuidance), c_int, c_int,
                               ctypes.POINTER(GssCacgmmModel), ctypes.POINTER(GssCacgmmModel)]),
    'gss_cacgmm_predict': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int,
                                   ctypes.POINTER(GssCacgmmModel), c_int,
                                   ctypes.POINTER(GssGuidance), c_void_p, c_void_p]),
    'gss_cacgmm_align': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64,
                                 ctypes.POINTER(GssAlignPlan), c_void_p, c_void_p, c_void_p]),
    'gss_cacgmm_model_permute': (c_int, [c_void_p, ctypes.POINTER(GssCacgmmModel), c_int, c_int,
                                         c_int, c_void_p, ctypes.POINTER(GssCacgmmModel)]),
    'gss_last_align_moved': (c_int, [c_void_p, ctypes.POINTER(ctypes.c_int64)]),
    'gss_cacgmm_link': (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64,
                                c_int64, c_int, c_int, c_void_p, c_void_p]),
    'gss_cacgmm_link_gather': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p,
                                       c_void_p]),
    'gss_masks_from_posteriors': (
        c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_int, c_int, c_int64,
                c_int64, c_void_p, c_void_p]),
    'gss_mvdr_souden': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int,
                                c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'gss_mvdr_souden_ref': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int,
                                    c_void_p, c_void_p, c_int, c_int, c_void_p]),
    'gss_mvdr_souden_segments': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int,
                                         c_void_p, c_void_p, c_int, c_int,
                                         ctypes.POINTER(GssBfSegments), c_void_p, c_void_p]),
    'gss_last_segment_fallbacks': (c_int, [c_void_p, ctypes.POINTER(ctypes.c_int64)]),
    'gss_lcmv_souden': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p,
                                c_void_p, c_int, c_int, ctypes.c_double, c_void_p, c_void_p]),
    'gss_lcmv_masks_from_posteriors': (
        c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_int, ctypes.POINTER(GssBfLcmv),
                c_int, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    'gss_last_lcmv_interferer': (c_int, [c_void_p, ctypes.POINTER(ctypes.c_int32)]),
    'gss_last_lcmv_fallbacks': (c_int, [c_void_p, ctypes.POINTER(ctypes.c_int64)]),
    'gss_wpe_weighted': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_int,
                                 c_void_p, c_void_p]),
    'gss_wpd_weights': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p,
                                c_void_p, ctypes.c_double, c_void_p]),
    'gss_wpd_souden': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p,
                               ctypes.POINTER(GssBfWpd), c_int, c_void_p, c_void_p]),
    'gss_last_wpd_zero_pivots': (c_int, [c_void_p, ctypes.POINTER(ctypes.c_int64)]),
    'gss_enhance_observation_wpd': _fused(ctypes.POINTER(GssBfWpd)),
    'gss_wpe_online_init': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                                    ctypes.POINTER(GssWpeOnlineState)]),
    'gss_wpe_online': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_int, c_int,
                               ctypes.c_double, ctypes.POINTER(GssWpeOnlineState), c_void_p]),
    'gss_enhance_observation_wpe_online': _fused(ctypes.POINTER(GssWpeOnlineCfg)),
    'gss_mvdr_online_init': (c_int, [c_void_p, c_int, c_int, c_void_p, c_int64, ctypes.c_double,
                                     ctypes.POINTER(GssMvdrOnlineState)]),
    'gss_mvdr_online': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p,
                                c_int, ctypes.POINTER(GssBfOnline),
                                ctypes.POINTER(GssMvdrOnlineState), c_void_p, c_void_p]),
    'gss_last_mvdr_online_fallbacks': (c_int, [c_void_p, ctypes.POINTER(ctypes.c_int64)]),
    'gss_enhance_observation_bf_online': _fused(ctypes.POINTER(GssBfOnline)),
    'gss_cacgmm_online_init': (c_int, [c_void_p, c_int, c_int, c_int, ctypes.c_double,
                                       ctypes.POINTER(GssCacgmmModel), ctypes.c_double,
                                       ctypes.POINTER(GssCacgmmOnlineState)]),
    'gss_cacgmm_online': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int,
                                  ctypes.POINTER(GssGuidance), c_int, ctypes.POINTER(GssEmOnline),
                                  ctypes.POINTER(GssCacgmmOnlineState), c_void_p]),
    'gss_cacgmm_online_model': (c_int, [c_void_p, ctypes.POINTER(GssCacgmmOnlineState),
                                        ctypes.POINTER(GssCacgmmModel)]),
    'gss_last_cacgmm_online_fallbacks': (c_int, [c_void_p, ctypes.POINTER(ctypes.c_int64)]),
    'gss_enhance_observation_gss_online': _fused(ctypes.POINTER(GssEmOnline),
                                                 ctypes.POINTER(GssBfOnline)),
    'gss_stream_num_frames': (c_int64, [c_int64, c_int64, c_int, c_int]),
    'gss_stream_num_samples_out': (c_int64, [c_int64, c_int64, c_int, c_int]),
    'gss_stream_flush_samples': (c_int64, [c_int64, c_int, c_int]),
    'gss_stream_init': (c_int, [c_void_p, ctypes.POINTER(GssStreamState)]),
    'gss_stft_stream': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64,
                                ctypes.POINTER(GssStreamState), c_void_p, c_void_p]),
    'gss_istft_stream': (c_int, [c_void_p, c_void_p, c_int64, ctypes.POINTER(GssStreamState),
                                 c_void_p]),
    'gss_stream_block': (c_int, [c_void_p, ctypes.POINTER(GssParams), ctypes.POINTER(GssStreamCfg),
                                 ctypes.POINTER(GssStreamState), ctypes.POINTER(GssWpeOnlineState),
                                 ctypes.POINTER(GssCacgmmOnlineState),
                                 ctypes.POINTER(GssMvdrOnlineState), c_void_p, c_int, c_void_p,
                                 c_int64, c_int, c_void_p, _TAPS]),
    'gss_mvdr_online_targets': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p, c_int,
                                        ctypes.POINTER(ctypes.c_int32), c_int, c_int,
                                        ctypes.POINTER(GssBfOnline),
                                        ctypes.POINTER(GssMvdrOnlineState), c_int, c_void_p,
                                        c_void_p, c_void_p, c_void_p]),
    'gss_last_mvdr_online_fallbacks_targets': (c_int, [c_void_p, ctypes.POINTER(ctypes.c_int64),
                                                       c_int]),
    'gss_istft_stream_targets': (c_int, [c_void_p, c_void_p, c_int64, c_int,
                                         ctypes.POINTER(GssStreamState), c_void_p, c_void_p]),
    'gss_stream_block_targets': (c_int, [c_void_p, ctypes.POINTER(GssParams),
                                         ctypes.POINTER(GssStreamCfg),
                                         ctypes.POINTER(GssStreamState),
                                         ctypes.POINTER(GssWpeOnlineState),
                                         ctypes.POINTER(GssCacgmmOnlineState),
                                         ctypes.POINTER(GssMvdrOnlineState), c_void_p, c_void_p,
                                         c_int, c_void_p, c_int64, ctypes.POINTER(ctypes.c_int32),
                                         c_int, c_void_p, _TAPS]),
    'gss_mvdr_online_hold_init': (c_int, [c_void_p, ctypes.POINTER(GssMvdrOnlineHold)]),
    'gss_mvdr_online_lookahead': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p,
                                          c_void_p, c_int, ctypes.POINTER(GssBfOnline),
                                          ctypes.POINTER(GssMvdrOnlineState),
                                          ctypes.POINTER(GssMvdrOnlineHold), c_void_p, c_void_p,
                                          ctypes.POINTER(c_int64)]),
    'gss_mvdr_online_lookahead_targets': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int,
                                                  c_void_p, c_int, ctypes.POINTER(ctypes.c_int32),
                                                  c_int, c_int, ctypes.POINTER(GssBfOnline),
                                                  ctypes.POINTER(GssMvdrOnlineState),
                                                  ctypes.POINTER(GssMvdrOnlineHold), c_int,
                                                  c_void_p, c_void_p, c_void_p, c_void_p,
                                                  ctypes.POINTER(c_int64)]),
    'gss_mvdr_online_release': (c_int, [c_void_p, ctypes.POINTER(GssMvdrOnlineHold), c_int, c_int,
                                        c_void_p, c_void_p, ctypes.POINTER(c_int64)]),
    'gss_stream_block_lookahead': (c_int, [c_void_p, ctypes.POINTER(GssParams),
                                           ctypes.POINTER(GssStreamCfg),
                                           ctypes.POINTER(GssStreamState),
                                           ctypes.POINTER(GssWpeOnlineState),
                                           ctypes.POINTER(GssCacgmmOnlineState),
                                           ctypes.POINTER(GssMvdrOnlineState),
                                           ctypes.POINTER(GssMvdrOnlineHold), c_void_p, c_void_p,
                                           c_int, c_void_p, c_int64,
                                           ctypes.POINTER(ctypes.c_int32), c_int, c_int, c_void_p,
                                           ctypes.POINTER(c_int64), _TAPS]),
    'gss_last_ref_channel': (c_int, [c_void_p, ctypes.POINTER(ctypes.c_int32)]),
    'gss_last_wpe_zero_pivots': (c_int, [c_void_p, ctypes.POINTER(ctypes.c_int64)]),
    'gss_gev': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p, c_int,
                        c_void_p]),
    'gss_layout_dtf_to_ftd': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int,
                                      c_void_p]),
    'gss_layout_ftd_to_dtf': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int,
                                      c_void_p]),
    'gss_layout_permute_f64': (c_int, [c_void_p, c_void_p, c_int64, c_int64,
                                       c_int64, c_int, c_void_p]),
    'gss_enhance_observation': _fused(),
    # (the guidance in the place of act_dev, no N_act)
    'gss_enhance_observation_guided': (
        c_int, _FUSED_HEAD[:5] + [ctypes.POINTER(GssGuidance), c_int] + _FUSED_TARGET
        + [c_void_p, _TAPS]),
    'gss_enhance_observation_segments': _fused(ctypes.POINTER(GssBfSegments)),
    'gss_enhance_observation_lcmv': _fused(ctypes.POINTER(GssBfLcmv)),
    'gss_enhance_observation_pcm16': _fused(),
    'gss_enhance_observation_targets': _FUSED_TARGETS,
    'gss_enhance_observation_targets_pcm16': _FUSED_TARGETS,
    'gss_last_ref_channels': (c_int, [c_void_p, ctypes.POINTER(ctypes.c_int32), c_int]),
    'gss_channel_scores': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int,
                                   ctypes.POINTER(GssChannelSelect), c_void_p, c_void_p]),
    'gss_select_channels': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int,
                                    ctypes.POINTER(GssChannelSelect), c_void_p, c_void_p]),
    'gss_last_selected_channels': (c_int, [c_void_p, ctypes.POINTER(ctypes.c_int32), c_int]),
    'gss_enhance_observation_select': _fused(ctypes.POINTER(GssChannelSelect)),
    'gss_enhance_observation_select_pcm16': _fused(ctypes.POINTER(GssChannelSelect)),
    'gss_posterior_activity': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_int,
                                       c_void_p, c_void_p, c_void_p]),
    'gss_enhance_observation_activity': _fused(c_void_p, after_out=(c_void_p, c_void_p)),
    # (ctx, params, obs_dev, D, N, init_dev, K, out_dev, prior_dev, power_dev, gamma_dev, taps)
    'gss_separate_observation': (c_int, _FUSED_HEAD[:5] + [c_void_p, c_int, c_void_p, c_void_p,
                                                           c_void_p, c_void_p, _TAPS]),
    'gss_enhance_observation_host': (c_int, _FUSED_HEAD + _FUSED_TARGET + [c_void_p]),
    'gss_workspace_bytes': (c_size_t, [c_void_p]),
    'gss_debug_workspace': (c_int, [c_void_p, c_int]),
    'gss_debug_workspace_report': (c_int, [c_void_p, ctypes.POINTER(c_int64), ctypes.c_char_p,
                                           c_int, c_int, ctypes.POINTER(c_void_p)]),
    'gss_selftest_mfma': (c_int, [c_void_p]),
}


class GssError(RuntimeError):
    pass


def load_library(path=None):
    """Load libgss_hip.so (no GPU needed for loading) and declare prototypes."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = Path(path or os.environ.get('GSS_HIP_LIBRARY', LIB_PATH))
    if not p.exists():
        raise GssError(
            f'{p} is missing: build it with `python -m pb_chime5_amd.build` '
            '(there is no CPU fallback)')
    lib = ctypes.CDLL(str(p))
    # the prototypes below are written against one revision of include/gss_hip.h: a library
    # of another revision would read shifted arguments or a shorter gss_params
    abi = getattr(lib, 'gss_abi_version', None)
    got = None
    if abi is not None:
        abi.restype, abi.argtypes = c_int, []
        got = int(abi())
    if got != GSS_ABI_VERSION:
        raise GssError(f'{p}: ABI revision {got}, this binding needs {GSS_ABI_VERSION} '
                       '(rebuild with `python -m pb_chime5_amd.build --force`)')
    # (revision 7 gained entry points without a new revision number: a library built from an
    # older tree passes the check above and lacks them)
    missing = [name for name in SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise GssError(f'{p}: no {", ".join(missing)} in this build of revision {got} '
                       '(rebuild with `python -m pb_chime5_amd.build --force`)')
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    if path is None:
        _LIB = lib
    return lib


def _raise(lib, ctx, status, what):
    msg = lib.gss_last_error(ctx)
    msg = msg.decode() if msg else ''
    text = f'{what}: {msg}' if msg else what
    # mirror the exception types of the reference
    if status == GSS_ERR_INVALID:
        if 'assert' in msg:
            raise AssertionError(text)
        raise ValueError(text)
    if status == GSS_ERR_UNSUPPORTED:
        raise NotImplementedError(text)
    if status == GSS_ERR_NOMEM:
        raise MemoryError(text)
    raise GssError(text)


class DeviceBuffer:
    """A device allocation owned through the C ABI (gss_dev_malloc/free)."""

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        ptr = c_void_p()
        ctx._check(ctx.lib.gss_dev_malloc(ctx.handle, self.nbytes, ctypes.byref(ptr)),
                   'gss_dev_malloc')
        self.ptr = ptr.value

    def free(self):
        if self.ptr is not None and self.ctx.handle is not None:
            self.ctx.lib.gss_dev_free(self.ctx.handle, c_void_p(self.ptr))
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PinnedBuffer:
    """Page-locked host memory (gss_host_malloc/free), handed out as NumPy views."""

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = max(int(nbytes), 16)
        ptr = c_void_p()
        ctx._check(ctx.lib.gss_host_malloc(ctx.handle, self.nbytes, ctypes.byref(ptr)),
                   'gss_host_malloc')
        self.ptr = ptr.value
        self._raw = (ctypes.c_char * self.nbytes).from_address(self.ptr)

    def view(self, shape, dtype, offset=0):
        """An array of `shape` / `dtype` over the block (no copy), starting `offset` bytes in."""
        count = int(np.prod(shape, dtype=np.int64))
        assert offset + count * np.dtype(dtype).itemsize <= self.nbytes
        return np.frombuffer(self._raw, dtype=dtype, count=count, offset=offset).reshape(shape)

    def free(self):
        if self.ptr is not None and self.ctx.handle is not None:
            self._raw = None
            self.ctx.lib.gss_host_free(self.ctx.handle, c_void_p(self.ptr))
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """One per GPU (and per host thread)."""

    def __init__(self, device_id=0):
        self.lib = load_library()
        self.handle = None
        h = c_void_p()
        st = self.lib.gss_create(int(device_id), ctypes.byref(h))
        if st != GSS_OK:
            msg = self.lib.gss_last_error(None)
            raise GssError(
                f'gss_create(device {device_id}) failed: '
                f'{msg.decode() if msg else st} -- the HIP path needs an AMD GPU '
                '(there is no CPU fallback)')
        self.handle = h
        self.device_id = device_id
        self._windows = None
        self.selected_count = 0     # n of the last channel selection enqueued through `ops`

    # -- plumbing ----------------------------------------------------------
    def _check(self, status, what):
        if status != GSS_OK:
            _raise(self.lib, self.handle, status, what)

    def close(self):
        if self.handle is not None:
            self.lib.gss_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        self._check(self.lib.gss_synchronize(self.handle), 'gss_synchronize')

    def set_stream(self, stream_handle):
        self._check(self.lib.gss_set_stream(self.handle, c_void_p(stream_handle)),
                    'gss_set_stream')

    def set_utterances_in_flight(self, n):
        """How many utterances the caller keeps in flight on this GPU (0 = not said, the default).
        Exactly 1 lets a fused call use the context's internal second stream for half of the WPE
        stage's frequencies (same bits, ~1.5 % sooner); anything else keeps it on one stream."""
        self._check(self.lib.gss_set_utterances_in_flight(self.handle, int(n)),
                    'gss_set_utterances_in_flight')

    def empty(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def to_device(self, array):
        a = np.ascontiguousarray(array)
        buf = DeviceBuffer(self, max(a.nbytes, 16))
        if a.nbytes:
            self._check(self.lib.gss_memcpy_h2d(
                self.handle, c_void_p(buf.ptr), a.ctypes.data_as(c_void_p), a.nbytes),
                'gss_memcpy_h2d')
        return buf

    def upload(self, buf, array):
        a = np.ascontiguousarray(array)
        assert a.nbytes <= buf.nbytes
        self._check(self.lib.gss_memcpy_h2d(
            self.handle, c_void_p(buf.ptr), a.ctypes.data_as(c_void_p), a.nbytes),
            'gss_memcpy_h2d')

    def pinned(self, nbytes):
        return PinnedBuffer(self, nbytes)

    def upload_async(self, buf, array, offset=0):
        """H2D without waiting; `array` (C-contiguous, ideally a PinnedBuffer view) must stay
        untouched until the context was synchronised."""
        assert array.flags.c_contiguous and offset + array.nbytes <= buf.nbytes
        self._check(self.lib.gss_memcpy_h2d_async(
            self.handle, c_void_p(buf.ptr + offset), array.ctypes.data_as(c_void_p),
            array.nbytes), 'gss_memcpy_h2d_async')

    def download_async(self, array, buf, offset=0):
        """D2H into `array` without waiting (valid after synchronize())."""
        assert array.flags.c_contiguous and offset + array.nbytes <= buf.nbytes
        self._check(self.lib.gss_memcpy_d2h_async(
            self.handle, array.ctypes.data_as(c_void_p), c_void_p(buf.ptr + offset),
            array.nbytes), 'gss_memcpy_d2h_async')

    def to_host(self, buf, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= buf.nbytes, (out.nbytes, buf.nbytes)
        if out.nbytes:
            self._check(self.lib.gss_memcpy_d2h(
                self.handle, out.ctypes.data_as(c_void_p), c_void_p(buf.ptr), out.nbytes),
                'gss_memcpy_d2h')
        return out

    # -- profiling ---------------------------------------------------------
    def profile_enable(self, on=True):
        self._check(self.lib.gss_profile_enable(self.handle, int(on)), 'profile_enable')

    def profile_filter(self, kernel=None):
        self._check(self.lib.gss_profile_filter(
            self.handle, kernel.encode() if kernel else None), 'profile_filter')

    def profile_reset(self):
        self._check(self.lib.gss_profile_reset(self.handle), 'profile_reset')

    def profile_report(self):
        buf = ctypes.create_string_buffer(1 << 16)
        self._check(self.lib.gss_profile_report(self.handle, buf, len(buf)),
                    'profile_report')
        return json.loads(buf.value.decode())

    def _last(self, symbol, ctype):
        """One status word of the last call through its gss_last_* reader (synchronises)."""
        out = ctype()
        self._check(getattr(self.lib, symbol)(self.handle, ctypes.byref(out)), symbol)
        return int(out.value)

    def last_ref_channel(self):
        """Reference channel of the last MVDR run (synchronises); -1 = non-finite SNR."""
        return self._last('gss_last_ref_channel', ctypes.c_int32)

    def last_ref_channels(self, S):
        """Status words of the S targets of the last targets call (synchronises): the reference
        channel of each, or the codes of `last_ref_channel`."""
        out = (ctypes.c_int32 * int(S))()
        self._check(self.lib.gss_last_ref_channels(self.handle, out, int(S)),
                    'gss_last_ref_channels')
        return [int(v) for v in out]

    def last_selected_channels(self, n=None):
        """The channels (ascending) the last channel selection on this context kept
        (synchronises); ``n``: the first n of them (None: as many as the caller asked that
        call to keep, which the binding remembers in ``selected_count``)."""
        if n is None:
            n = self.selected_count
        out = (ctypes.c_int32 * max(int(n), 1))()
        self._check(self.lib.gss_last_selected_channels(self.handle, out, int(n)),
                    'gss_last_selected_channels')
        return [int(v) for v in out[:int(n)]]

    def last_wpe_zero_pivots(self):
        """Pivots the WPE solve of the last call zeroed (synchronises); > 0 on live channels
        means rank-deficient normal equations (T <= taps * D), see include/gss_hip.h."""
        return self._last('gss_last_wpe_zero_pivots', ctypes.c_int64)

    def last_wpd_zero_pivots(self):
        """Pivots the WPE steps of the last WPD call zeroed (synchronises); the WPE stage's own
        count stays in `last_wpe_zero_pivots`."""
        return self._last('gss_last_wpd_zero_pivots', ctypes.c_int64)

    def last_align_moved(self):
        """Frequencies whose row the last alignment on this context left off the identity
        (synchronises)."""
        return self._last('gss_last_align_moved', ctypes.c_int64)

    def last_segment_fallbacks(self):
        """(segment, frequency) pairs of the last segment-wise MVDR on this context that fell
        back to the whole-window statistics (synchronises)."""
        return self._last('gss_last_segment_fallbacks', ctypes.c_int64)

    def last_lcmv_interferer(self):
        """The interferer class of the last LCMV mask / fused call on this context, -1 when it
        had none (synchronises)."""
        return self._last('gss_last_lcmv_interferer', ctypes.c_int32)

    def last_lcmv_fallbacks(self):
        """Frequencies of the last LCMV beamformer on this context that fell back to the MVDR of
        the merged mask (synchronises)."""
        return self._last('gss_last_lcmv_fallbacks', ctypes.c_int64)

    def last_mvdr_online_fallbacks(self):
        """(frequency, frame) pairs of the last online MVDR on this context whose noise matrix had
        no Cholesky factor (synchronises)."""
        return self._last('gss_last_mvdr_online_fallbacks', ctypes.c_int64)

    def last_mvdr_online_fallbacks_targets(self, S):
        """The same per target of the last online MVDR targets call on this context, a list of S
        counts (synchronises)."""
        out = (ctypes.c_int64 * int(S))()
        self._check(self.lib.gss_last_mvdr_online_fallbacks_targets(self.handle, out, int(S)),
                    'gss_last_mvdr_online_fallbacks_targets')
        return [int(v) for v in out]

    def last_cacgmm_online_fallbacks(self):
        """(frequency, frame, class) triples of the last online CACGMM on this context whose S_k had
        no Cholesky factor (synchronises)."""
        return self._last('gss_last_cacgmm_online_fallbacks', ctypes.c_int64)

    def workspace_bytes(self):
        return int(self.lib.gss_workspace_bytes(self.handle))

    def debug_workspace(self, pattern=None):
        """The workspace debug mode (tests only; it synchronises): fill byte 0..255 = on, None = off.
        While on, workspace and `empty()` blocks start as that byte and every workspace block has
        a guard behind it (include/gss_hip.h: gss_debug_workspace)."""
        self._check(self.lib.gss_debug_workspace(self.handle, -1 if pattern is None else int(pattern)),
                    'gss_debug_workspace')

    def debug_workspace_report(self, guard_index=-1):
        """(violated guards since the mode was switched on, text naming the first, device address
        of live guard `guard_index` or None); checks the live guards (synchronises)."""
        count, addr = c_int64(), c_void_p()
        buf = ctypes.create_string_buffer(1024)
        self._check(self.lib.gss_debug_workspace_report(
            self.handle, ctypes.byref(count), buf, len(buf), int(guard_index), ctypes.byref(addr)),
            'gss_debug_workspace_report')
        return int(count.value), buf.value.decode(), addr.value

    # -- STFT tables -------------------------------------------------------
    def set_windows(self, size, shift, analysis, synthesis):
        key = (size, shift, analysis.tobytes(), synthesis.tobytes())
        if self._windows == key:
            return
        a = np.ascontiguousarray(analysis, dtype=np.float64)
        s = np.ascontiguousarray(synthesis, dtype=np.float64)
        assert a.shape == (size,) and s.shape == (size,)
        self._check(self.lib.gss_set_windows(
            self.handle, size, shift, a.ctypes.data_as(c_void_p),
            s.ctypes.data_as(c_void_p)), 'gss_set_windows')
        self._windows = key


_DEFAULT_CTX = {}


def device_count():
    return int(load_library().gss_device_count())


def device_pci_bus_id(device_id):
    """'0000:c1:00.0' -- the key of the device's sysfs entry (NUMA node, local CPUs)."""
    buf = ctypes.create_string_buffer(32)
    rc = load_library().gss_device_pci_bus_id(int(device_id), buf, len(buf))
    if rc != 0:
        raise GssError(f'gss_device_pci_bus_id({device_id}) failed with status {rc}')
    return buf.value.decode()


def pci_package(bus_id):
    """The part of a PCI address that names the physical package: 'domain:bus:device'.  The
    logical devices of a partitioned GPU (CPX / NPS modes: up to 8 per package) differ in the
    function digit at most."""
    return bus_id.lower().rsplit('.', 1)[0]


def pick_device(local_rank, bus_ids):
    """The logical device of a node-local rank: ranks go to DISTINCT physical packages first
    (round robin over the packages in device order), and only then to further logical devices
    of a package.  One logical device per package (the usual 8-GPU node): rank r -> device
    r % count, as before; a partitioned node with 64 logical devices on 8 packages: ranks 0-7
    land on 8 different GPUs instead of on the 8 partitions of the first."""
    packages = {}
    for index, bus_id in enumerate(bus_ids):
        packages.setdefault(pci_package(bus_id), []).append(index)
    groups = list(packages.values())
    if not groups:
        return 0
    mine = groups[local_rank % len(groups)]
    return mine[(local_rank // len(groups)) % len(mine)]


def default_device():
    """$GSS_DEVICE, else by LOCAL_RANK over the visible GPUs, distinct physical packages first
    (`pick_device`; ranks share devices when a node has fewer GPUs than ranks), else 0."""
    if 'GSS_DEVICE' in os.environ:
        return int(os.environ['GSS_DEVICE'])
    local_rank = int(os.environ.get('LOCAL_RANK', 0))
    if not local_rank:
        return 0
    count = max(device_count(), 1)
    try:
        return pick_device(local_rank, [device_pci_bus_id(i) for i in range(count)])
    except GssError:
        return local_rank % count


def default_context(device_id=None):
    """Process-wide context for ``device_id`` (default: ``default_device()``)."""
    if device_id is None:
        device_id = default_device()
    ctx = _DEFAULT_CTX.get(device_id)
    if ctx is None or ctx.handle is None:
        ctx = _DEFAULT_CTX[device_id] = Context(device_id)
    return ctx
