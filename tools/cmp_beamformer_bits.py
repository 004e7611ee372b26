"""The beamformers of two builds of libgss_hip.so: the same bits?

    python tools/cmp_beamformer_bits.py OTHER_LIBRARY          (on a GPU box)

OTHER_LIBRARY is another build of the library: the parent commit's, when a change must not move
a bit, or the one-wave solve of `bash tools/build_variant.sh mvdr_nt64 -DGSS_MVDR_NT=64`
(pb_chime5_amd/lib/variants/libgss_mvdr_nt64.so).  Every case runs once under the package's own
library and once under OTHER_LIBRARY (GSS_HIP_LIBRARY), each in a process of its own; outputs and
reference channels are compared byte for byte.  Cases: MVDR-Souden + BAN with 4 - 29 channels and
with a dead channel (the minimum-norm path); the LCMV stage nulling, with one fallback frequency,
with a dead channel, and falling back on a dead channel; segments; three targets; GEV.
Exit status 1 when an array differs."""
import os, sys, subprocess, tempfile
sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
import numpy as np


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
    return out


if len(sys.argv) == 3 and sys.argv[1] == '--run':
    np.savez(sys.argv[2], **cases())
elif len(sys.argv) == 2:
    me = os.path.abspath(__file__)
    with tempfile.TemporaryDirectory() as tmp:
        a, b = os.path.join(tmp, 'a.npz'), os.path.join(tmp, 'b.npz')
        subprocess.run([sys.executable, me, '--run', a], check=True)
        subprocess.run([sys.executable, me, '--run', b], check=True,
                       env=dict(os.environ, GSS_HIP_LIBRARY=os.path.abspath(sys.argv[1])))
        A, B = np.load(a), np.load(b)
        different = 0
        for k in A.files:
            same = A[k].tobytes() == B[k].tobytes()
            different += not same
            print(k, 'bit-identical' if same else 'DIFFERENT max %.3e' % np.nanmax(np.abs(A[k] - B[k])), 'nan' if np.isnan(A[k]).any() else '')
        print(f'{len(A.files)} arrays, {different} different')
        sys.exit(1 if different else 0)
else:
    sys.exit(__doc__)
