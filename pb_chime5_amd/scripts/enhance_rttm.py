"""Command line front end of the RTTM-driven path: the knobs of the reference's
``scripts/kaldi_run_rttm.py`` (:21-40, 61-89) without sacred.

    python -m pb_chime5_amd.scripts.enhance_rttm --chime6-dir CHiME6 \
        --database-rttm dev_rttm --activity-rttm dev_rttm --session-id S02 --out out

    # all GPUs of a node (utterances are sharded, no collective on the data path):
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \
        -m pb_chime5_amd.scripts.enhance_rttm ...

``--job-id / --number-of-jobs`` give the Kaldi-style static split
(``dataset_slice = slice(job_id - 1, None, number_of_jobs)``, kaldi_run_rttm.py:73).
"""
import argparse
from pathlib import Path


def _channel_keep(text):
    """'20' -> 20 channels, '0.8' -> a share of the channels."""
    try:
        return int(text)
    except ValueError:
        return float(text)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument('--chime6-dir', required=True)
    ap.add_argument('--database-rttm', required=True, nargs='+')
    ap.add_argument('--activity-rttm', nargs='+', default=None)
    ap.add_argument('--session-id', nargs='+', default=['dev'])
    ap.add_argument('--out', required=True)
    ap.add_argument('--multiarray', default='outer_array_mics')
    ap.add_argument('--context-samples', type=int, default=240000)
    ap.add_argument('--no-wpe', action='store_true')
    ap.add_argument('--wpe-tabs', type=int, default=10)
    ap.add_argument('--wpe-delay', type=int, default=2)
    ap.add_argument('--wpe-iterations', type=int, default=3)
    ap.add_argument('--wpe-per-array', action='store_true',
                    help='WPE on each microphone array on its own (get_enhancer(wpe_per_array=True))')
    ap.add_argument('--wpe-online', action='store_true',
                    help="nara_wpe's online WPE in the place of the offline one: a frame-recursive "
                         'filter that forgets, the time-varying front for long windows with '
                         'movement; --wpe-iterations is not read (get_enhancer(wpe_online=True))')
    ap.add_argument('--wpe-alpha', type=float, default=0.9999,
                    help='forgetting factor of --wpe-online, in (0, 1] (a choice, not a '
                         'measurement)')
    ap.add_argument('--bf-online', action='store_true',
                    help="the online MVDR in the place of the whole-window 'mvdrSouden_ban': running "
                         'sums that forget, a filter per frame, no look-ahead '
                         '(get_enhancer(bf_online=True))')
    ap.add_argument('--bf-forget', type=float, default=0.99,
                    help='forgetting factor of --bf-online, in (0, 1] (a choice, not a measurement)')
    ap.add_argument('--bf-loading', type=float, default=1e-2,
                    help='relative diagonal loading of the fresh state of --bf-online, > 0 (a '
                         'choice, not a measurement)')
    ap.add_argument('--gss-online', action='store_true',
                    help='the online CACGMM in the place of the iterated mixture model: the '
                         'recursive EM on running sums that forget, causal posteriors; '
                         '--bss-iterations is not read (get_enhancer(gss_online=True))')
    ap.add_argument('--gss-forget', type=float, default=0.99,
                    help='forgetting factor of --gss-online, in (0, 1] (a choice, not a measurement)')
    ap.add_argument('--gss-prior-mass', type=float, default=1.0,
                    help='mass of the fresh state of --gss-online, > 0 (a choice, not a measurement)')
    ap.add_argument('--bss-iterations', type=int, default=20)
    ap.add_argument('--bss-iterations-post', type=int, default=1)
    ap.add_argument('--bf', default='mvdrSouden_ban')
    ap.add_argument('--postfilter', default=None)
    ap.add_argument('--bf-segment-frames', type=int, default=None,
                    help='time-varying MVDR: beamformer statistics per segment of this many STFT '
                         'frames, a multiple of 64 (get_enhancer(bf_segment_frames=...))')
    ap.add_argument('--bf-segment-context', type=int, default=0,
                    help='segments either side in the statistics of a segment')
    ap.add_argument('--bf-null-interferer', action='store_true',
                    help='interferer-nulling LCMV in the place of the MVDR: a null on the '
                         'competing speaker with the most posterior mass '
                         '(get_enhancer(bf_null_interferer=True))')
    ap.add_argument('--bf-wpd-taps', type=int, default=None,
                    help="with --bf wpdSouden_ban / wpdSouden, the WPD convolutional beamformer on "
                         "the STFT before WPE: its taps (default: --wpe-tabs) "
                         "(get_enhancer(bf_wpd_taps=...))")
    ap.add_argument('--bf-wpd-delay', type=int, default=None,
                    help='delay of the WPD tap window (default: --wpe-delay)')
    ap.add_argument('--bf-wpd-iterations', type=int, default=1,
                    help='WPD iterations: the target power of iteration i > 1 is the power of '
                         'the output of iteration i - 1')
    ap.add_argument('--bf-wpd-power-floor', type=float, default=1e-3,
                    help='floor of the target power as a share of its maximum, in (0, 1]')
    ap.add_argument('--channel-keep', type=_channel_keep, default=None,
                    help='keep the channels the envelope-variance measure ranks best: a count '
                         '(20) or a share (0.8) (get_enhancer(channel_keep=...))')
    ap.add_argument('--channel-bands', type=int, default=40,
                    help='mel filters of the channel selection')
    ap.add_argument('--refined-rttm', action='store_true',
                    help='also write <example_id>.rttm next to every WAV: where inside the '
                         'segment the posteriors give the speaker the power '
                         '(enhance_session(refined_rttm=True); one utterance at a time)')
    ap.add_argument('--no-bf-drop-context', action='store_true')
    ap.add_argument('--job-id', type=int, default=1)
    ap.add_argument('--number-of-jobs', type=int, default=1)
    ap.add_argument('--test-run', action='store_true', help='first two examples only')
    args = ap.parse_args(argv)

    from pb_chime5_amd import parallel
    from pb_chime5_amd.core_chime6_rttm import get_enhancer
    parallel.init()
    multiarray = True if args.multiarray in ('True', 'true', '1') else args.multiarray
    enhancer = get_enhancer(
        database_rttm=args.database_rttm, activity_rttm=args.activity_rttm or args.database_rttm,
        chime6_dir=args.chime6_dir, multiarray=multiarray,
        context_samples=args.context_samples, wpe=not args.no_wpe, wpe_tabs=args.wpe_tabs,
        wpe_delay=args.wpe_delay, wpe_iterations=args.wpe_iterations,
        bss_iterations=args.bss_iterations, bss_iterations_post=args.bss_iterations_post,
        bf_drop_context=not args.no_bf_drop_context, bf=args.bf, postfilter=args.postfilter,
        device_id=parallel.device_index(), wpe_per_array=args.wpe_per_array,
        bf_segment_frames=args.bf_segment_frames, bf_segment_context=args.bf_segment_context,
        channel_keep=args.channel_keep, channel_bands=args.channel_bands,
        bf_null_interferer=args.bf_null_interferer, bf_wpd_taps=args.bf_wpd_taps,
        bf_wpd_delay=args.bf_wpd_delay, bf_wpd_iterations=args.bf_wpd_iterations,
        bf_wpd_power_floor=args.bf_wpd_power_floor, wpe_online=args.wpe_online,
        wpe_alpha=args.wpe_alpha, bf_online=args.bf_online, bf_forget=args.bf_forget,
        bf_loading=args.bf_loading, gss_online=args.gss_online, gss_forget=args.gss_forget,
        gss_prior_mass=args.gss_prior_mass)
    if parallel.is_master():
        Path(args.out).mkdir(parents=True, exist_ok=True)
    parallel.barrier()
    if args.test_run:
        dataset_slice = True
    elif args.number_of_jobs > 1:
        dataset_slice = slice(args.job_id - 1, None, args.number_of_jobs)
    else:
        dataset_slice = False
    extra = {'refined_rttm': True} if args.refined_rttm else {}
    enhancer.enhance_session(args.session_id, Path(args.out) / 'audio',
                             dataset_slice=dataset_slice, audio_dir_exist_ok=True, **extra)
    if parallel.is_master():
        print(f'Finished: {Path(args.out) / "audio"}')


if __name__ == '__main__':
    main()
