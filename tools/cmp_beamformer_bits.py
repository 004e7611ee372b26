"""The beamformers of two builds of libgss_hip.so: the same bits?

    python tools/cmp_beamformer_bits.py OTHER_LIBRARY          (on a GPU box)

OTHER_LIBRARY is another build of the library: the parent commit's, when a change must not move
a bit, or the one-wave solve of `bash tools/build_variant.sh mvdr_nt64 -DGSS_MVDR_NT=64`
(pb_chime5_amd/lib/variants/libgss_mvdr_nt64.so).  Every case runs once under the package's own
library and once under OTHER_LIBRARY (GSS_HIP_LIBRARY), each in a process of its own (cmp_bits.py);
outputs and reference channels are compared byte for byte.  Cases: MVDR-Souden + BAN with 4 - 29 channels and
with a dead channel (the minimum-norm path); the LCMV stage nulling, with one fallback frequency,
with a dead channel, and falling back on a dead channel; segments; three targets; GEV; the online
MVDR for one and for several targets at 4, 12, 24 and 32 channels in two unequal blocks, with
and without BAN and the postfilter, with the filters and the final sums; the stream synthesis for
one and for several signals; a fused stream of one target and of several on two cells, cut
unevenly, with every tap, the final states, the tails and the fallback counts.
Exit status 1 when an array differs."""
import sys
sys.path.insert(0, '.'); sys.path.insert(0, 'tests'); sys.path.insert(0, 'oracle')
import numpy as np
from cmp_bits import main


def cases():
    import lcmv_reference as lr
    from pb_chime5_amd import ops, synthetic
    rng = np.random.default_rng(5)
    out = {}
    for (D, T, F) in ((24, 300, 40), (20, 200, 16), (12, 150, 16), (4, 80, 9), (7, 129, 6), (29, 200, 3)):
        Y = rng.standard_normal((D, T, F)) + 1j * rng.standard_normal((D, T, F))
        Y += (rng.standard_normal((D, 1, F)) + 1j * rng.standard_normal((D, 1, F))) * (rng.standard_normal((1, T, F)) + 1j * rng.standard_normal((1, T, F))) * 3
        tm = rng.uniform(size=(T, F)); dm = rng.uniform(size=(T, F)) * (1 - tm)
        X, ref = ops.mvdr_souden_from_masks(Y, tm, dm, ban=True, return_ref_channel=True)
        out[f'mvdr X{D}'] = X; out[f'mvdr r{D}'] = np.array(ref)
        if D in (24, 7):
            out[f'gev X{D}'] = ops.gev_from_masks(Y, tm, dm, ban=True)
            X, ref, fb = ops.mvdr_souden_segments_from_masks(
                Y, tm, dm, ban=True, segment_frames=64, segment_context=1, min_mass=40.0,
                return_ref_channel=True, return_fallbacks=True)
            out[f'segments X{D}'] = X; out[f'segments r{D}'] = np.array([ref, fb])
    # a singular Phi_N (dead channel): the pseudo-inverse path
    Y = rng.standard_normal((6, 90, 5)) + 1j * rng.standard_normal((6, 90, 5)); Y[2] = 0
    tm = rng.uniform(size=(90, 5)); dm = 1 - tm
    out['mvdr dead X'] = ops.mvdr_souden_from_masks(Y, tm, dm, ban=True)

    def lcmv(name, Y, xm, im, nm, min_mass):
        for ban in (False, True):
            X, ref, fb = ops.lcmv_souden_from_masks(Y, xm, im, nm, ban=ban, min_mass=min_mass,
                                                    return_ref_channel=True, return_fallbacks=True)
            out[f'lcmv {name} X ban={ban}'] = X; out[f'lcmv {name} r ban={ban}'] = np.array([ref, fb])
    for (D, T, F) in ((5, 130, 4), (24, 200, 2), (29, 96, 2)):
        Y, xm, im, nm, _ = lr.scene(np.random.default_rng(1000 * D + T), D, T, F)
        lcmv(f'nulling {D}', Y, xm, im, nm, 0.0)
    Y, xm, im, nm, _ = lr.scene(np.random.default_rng(5130), 5, 130, 4)
    silent = im.copy()
    silent[:, 2] = 0.0
    lcmv('one fallback', Y, xm, silent, nm, 10.0)
    Y[3] = 0.0
    lcmv('dead', Y, xm, im, nm, 0.0)
    lcmv('dead, all fall back', Y, xm, np.zeros_like(im), nm, 1.0)

    u = synthetic.tiny(seed=46, num_channels=6, num_samples=19200, num_speakers=3, context=2048,
                       noise=3e-2)
    for bf in ('mvdrSouden_ban', 'gev_ban'):
        out[f'targets {bf}'] = ops.enhance_observation_targets(
            u.obs, u.activity_array, [2, 0, 1], [0, 512, 1024], 2048, wpe=True, wpe_taps=4,
            bss_iterations=5, bf=bf)
    stream_cases(out)
    return out


def stream_cases(out):
    """The online MVDR and the two stream block paths: every form NR = 1..4 of both kernels."""
    import online_mvdr_reference as mref
    import stream_reference as sr
    import stream_targets_reference as tr
    from pb_chime5_amd import ops
    from pb_chime5_amd.streaming import StreamingEnhancer
    F, T, K, targets = 5, 40, 3, (2, 0)
    for D in (4, 12, 24, 32):
        rng = np.random.default_rng([D, F, T])
        Y = mref.crandn(rng, D, T, F)
        gamma = rng.random((K, T, F)) + 0.05
        gamma /= gamma.sum(axis=0)
        for ban in (False, True):
            kw = dict(forget=0.97, ref_channel=D - 1, ban=ban, return_filters=True)
            one = ops.OnlineMVDRState.fresh(F, D, 1e-2)
            runs = {None: [ops.OnlineMVDRState.fresh(F, D, 1e-2) for _ in targets],
                    'mask_mul': [ops.OnlineMVDRState.fresh(F, D, 1e-2) for _ in targets]}
            for a, b in ((0, 13), (13, T)):
                mx, mn = ops.masks_from_posteriors(gamma[:, a:b], targets[0])
                X, W = ops.mvdr_souden_online_from_masks(Y[:, a:b], mx, mn, state=one, **kw)
                out[f'online one {D} ban={ban} X{a}'], out[f'online one {D} ban={ban} W{a}'] = X, W
                for postfilter, states in runs.items():
                    X, W = ops.mvdr_souden_online_targets(Y[:, a:b], gamma[:, a:b], targets,
                                                          states=states, postfilter=postfilter, **kw)
                    name = f'online targets {D} ban={ban} {postfilter}'
                    out[f'{name} X{a}'], out[f'{name} W{a}'] = X, W
            for name, state in [('one', one)] + [(f'targets {p} {s}', st) for p, states in runs.items()
                                                 for s, st in enumerate(states)]:
                for k, v in state.to_host().items():
                    out[f'online {name} {D} ban={ban} {k}'] = np.asarray(v)

    W, H, S, T = 64, 16, 3, 24
    X = tr.reference('a', tr.seed_of('a'))[1]['X_hat'][:S, :T]
    X = X + 1j * np.arange(1, S + 1)[:, None, None] * X
    state, tails = ops.StreamState.fresh(1, 0, W, H), ops.StreamTails.fresh(S, W, H)
    single = ops.StreamState.fresh(1, 0, W, H)
    for st in (state, single):
        ops.stft_stream(np.zeros((1, T * H)), None, state=st)
    for i, (a, b) in enumerate(sr.blocks_of(T, (1, 2, 0, 7, T - 10))):
        out[f'istft targets {i}'] = ops.istft_stream_targets(X[:, a:b], state=state, tails=tails)
        out[f'istft one {i}'] = ops.istft_stream(X[0, a:b], state=single)
    out['istft tails'] = tails.to_host()['tails']
    out['istft ola_tail'] = single.to_host()['ola_tail']

    s = tr.SETTINGS
    for cell in ('a', 'm'):
        Wc, Hc, D, A, taps, delay, K, N, wpe = tr.CELLS[cell]
        x, activity = tr.scene(cell, tr.seed_of(cell))
        for postfilter in (None, 'mask_mul'):
            for mode in (dict(target=1), dict(targets=tr.TARGETS[cell])):
                enh = StreamingEnhancer(
                    D, K, ref_channel=s['ref_channel'], stft_size=Wc, stft_shift=Hc, wpe=wpe,
                    wpe_taps=taps, wpe_delay=delay, wpe_alpha=s['wpe_alpha'], wpe_arrays=A,
                    gss_forget=s['gss_forget'], gss_prior_mass=s['gss_prior_mass'],
                    bf_forget=s['bf_forget'], bf_loading=s['bf_loading'], postfilter=postfilter,
                    **mode)
                name = f'stream {cell} {postfilter} {sorted(mode)[0]}'
                blocks = sr.blocks_of(N, tr.partitions(cell)['borders'])
                for i, (a, b) in enumerate(list(blocks) + [(None, None)]):
                    y, d = (enh.flush(debug=True) if a is None else
                            enh.process(x[:, a:b], activity[:, a:b], debug=True))
                    out[f'{name} samples {i}'] = y
                    for k, v in (d or {}).items():
                        out[f'{name} {k} {i}'] = np.asarray(v)
                host = enh.to_host()
                for stage in ('stream', 'wpe', 'em', 'bf'):
                    for k, v in (host[stage] or {}).items():
                        out[f'{name} {stage}.{k}'] = np.asarray(v)
                if 'tails' in host:
                    out[f'{name} tails'] = np.asarray(host['tails'])
                for k, v in enh.fallbacks.items():
                    out[f'{name} fallbacks {k}'] = np.asarray(v)


main(__file__, __doc__, cases)
