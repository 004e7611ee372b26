"""The online MVDR's filter look-ahead (lookahead=): the NumPy reference itself
(tests/online_mvdr_lookahead_reference.py), the onset evidence, the C surface, every argument check
and the stream's sample accounting -- none of it needs a GPU."""
import ctypes
import inspect

import numpy as np
import pytest

import online_mvdr_lookahead_reference as lr
import online_mvdr_reference as mr
from conftest import REPO
from test_mvdr_online_api import no_context  # noqa: F401  (the fixture)

SYMBOLS = ('gss_mvdr_online_hold_init', 'gss_mvdr_online_lookahead',
           'gss_mvdr_online_lookahead_targets', 'gss_mvdr_online_release',
           'gss_stream_block_lookahead')


# ------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize('blocks', lr.PARTITIONS + [(150,)], ids=lambda b: f'{len(b)} blocks')
def test_reference_block_form_equals_the_one_shot_form(blocks):
    cell = lr.PARTITION_CELL
    D, beta, loading, F, T, L = cell
    Y, mx, mn, _ = mr.scene(cell[:5], lr.seed_of(cell))
    for ban in (False, True):
        X1 = lr.reference(cell, ban, D - 1, lr.seed_of(cell))[0]
        X, counts = lr.in_blocks(Y, mx, mn, beta, D - 1, ban, loading, L, blocks)
        assert np.array_equal(X, X1) and counts == lr.released(blocks, L)


def test_reference_block_form_on_the_onset_scene():
    D, beta, loading, F, T = lr.ONSET_CELL
    Y, mx, mn, _ = lr.onset_scene()
    X1 = lr.lookahead_mvdr(Y, mx, mn, beta, 0, False, 4, loading=loading)[0]
    X, counts = lr.in_blocks(Y, mx, mn, beta, 0, False, loading, 4, lr.CPU_PARTITION)
    assert sum(lr.CPU_PARTITION) == T and np.array_equal(X, X1)
    assert counts == [0, 0, 2, 4, 5, 100, 1, 184]


def test_reference_without_a_lookahead_is_the_online_mvdr():
    for cell in lr.CELLS[:4]:
        D, beta, loading, F, T, L = cell
        Y, mx, mn, _ = mr.scene(cell[:5], lr.seed_of(cell))
        X0, W0, st0, f0 = mr.online_mvdr(Y, mx, mn, beta, 0, True, loading=loading)
        X, W, st, f = lr.lookahead_mvdr(Y, mx, mn, beta, 0, True, 0, loading=loading)
        assert np.array_equal(X, X0) and np.array_equal(W, W0) and f == f0
        assert all(np.array_equal(st[k], st0[k]) for k in st0)


def test_reference_cells_and_their_stability():
    """The cells of the issue, and the rule that keeps a seed."""
    assert lr.CELLS == [(4, .99, 1e-2, 3, 150, 4), (1, .9, 1, 1, 5, 1), (1, .9, 1, 1, 5, 8),
                        (9, .99, 1, 2, 64, 3), (17, .99, 1, 2, 64, 16), (24, .995, 1, 2, 120, 8),
                        (32, .999, 1, 1, 64, 64)]
    assert lr.PARTITIONS == [(1, 63, 64, 22), (1, 1, 1, 1, 1, 145), (3, 1, 5, 141), (1,) * 150]
    for cell in lr.CELLS:
        moved = lr.reference_movement(cell, lr.seed_of(cell))
        assert moved * mr.STABILITY_MARGIN <= mr.TOL, (cell, moved)
        assert all(lr.reference(cell, ban, ref, lr.seed_of(cell))[3] == 0
                   for ban, ref in lr.variants(cell))


def test_the_lookahead_helps_at_an_onset():
    """Onset scene, seed 0, forget 0.99: the reference's error over the 16 frames after the onset
    at L = 4 is at most ONSET_BOUND x that at L = 0 (a condition, not a measurement)."""
    e0, eL = lr.onset_errors()
    print(f'onset: error {e0:.3f} at L = 0, {eL:.3f} at L = 4, ratio {eL / e0:.3f}')
    assert (lr.ONSET_BOUND, lr.ONSET_LOOKAHEAD, lr.ONSET_SEED, lr.ONSET_CELL[1]) == (0.5, 4, 0, 0.99)
    assert eL / e0 <= lr.ONSET_BOUND


# ------------------------------------------------------------------ the C surface
def test_the_built_library_exports_the_entry_points():
    from pb_chime5_amd import _capi
    lib = _capi.load_library()
    header = (REPO / 'include' / 'gss_hip.h').read_text()
    for name in SYMBOLS:
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
        assert f'int {name}(' in header, name
    assert _capi.GSS_ABI_VERSION == 7 and lib.gss_abi_version() == 7
    assert '#define GSS_MVDR_ONLINE_MAX_LOOKAHEAD 64' in header


def test_the_hold_descriptor_is_the_header_struct():
    from pb_chime5_amd import _capi, ops
    header = (REPO / 'include' / 'gss_hip.h').read_text()
    for decl in ('gss_cplx *frames;', 'double *mask;', 'gss_cplx *filter;', 'int32_t F, D, L;',
                 'int32_t held;', '} gss_mvdr_online_hold;'):
        assert decl in header, decl
    H = _capi.GssMvdrOnlineHold
    assert [n for n, _ in H._fields_] == ['frames', 'mask', 'filter', 'F', 'D', 'L', 'held']
    assert [getattr(H, n).offset for n, _ in H._fields_] == [0, 8, 16, 24, 28, 32, 36]
    assert ctypes.sizeof(H) == 40
    # the state's layout is pinned: the line is a descriptor of its own
    assert ctypes.sizeof(_capi.GssMvdrOnlineState) == 24
    assert ops.BF_ONLINE_MAX_LOOKAHEAD == lr.MAX_LOOKAHEAD == 64


# ------------------------------------------------------------------ argument checks
def test_check_bf_lookahead(no_context):
    from pb_chime5_amd import ops
    assert ops.check_bf_lookahead() == 0 and ops.check_bf_lookahead(64) == 64
    assert ops.check_bf_lookahead(0, -1) == 0
    assert ops.check_bf_online() == (0.99, 1e-2, 0)            # its three-tuple stays
    for bad in (-1, 0.5, 4.0, 65, None, '4', True):
        with pytest.raises(ValueError, match='lookahead'):
            ops.check_bf_lookahead(bad)
    with pytest.raises(ValueError, match='ref_channel'):
        ops.check_bf_lookahead(1, -1)


def test_signature_defaults():
    from pb_chime5_amd import core, ops
    from pb_chime5_amd.online_mvdr import OnlineMVDR
    from pb_chime5_amd.streaming import StreamingEnhancer
    for fn, names in ((ops.mvdr_souden_online_from_masks, ('lookahead', 'hold')),
                      (ops.mvdr_souden_online_targets, ('lookahead', 'hold')),
                      (OnlineMVDR.__init__, ('lookahead',)),
                      (StreamingEnhancer.__init__, ('lookahead',)),
                      (core.Enhancer.stream, ('lookahead',))):
        sig = inspect.signature(fn).parameters
        assert [sig[k].default for k in names] == [0, None][:len(names)], fn
    sig = inspect.signature(ops.stream_block_lookahead).parameters
    assert sig['release'].default is False
    assert 'lookahead' not in inspect.signature(core.get_enhancer).parameters


class _Buf:
    def __init__(self, n):
        self.nbytes, self.ptr = n, 4096


class _Ctx:
    """A context that allocates nothing."""

    def empty(self, n):
        return _Buf(n)


def test_hold_shapes_and_a_mismatched_hold():
    """The buffers of a line and the rule that a call takes only the line built for it -- on a
    context that allocates nothing."""
    from pb_chime5_amd import ops
    ctx = _Ctx()
    hold = ops.OnlineMVDRHold(ctx, 5, 3, 4)
    assert hold.shapes == {'frames': (5, 4, 3), 'mask': (5, 4), 'filter': (5, 3)}
    assert hold.key == (5, 3, 4) and hold.held == 0
    assert {k: b.nbytes for k, b in hold.bufs.items()} == \
        {'frames': 16 * 60, 'mask': 8 * 20, 'filter': 16 * 15}
    s = hold.struct()
    assert (s.frames, s.mask, s.filter, s.F, s.D, s.L, s.held) == (4096, 4096, 4096, 5, 3, 4, 0)
    state = ops.OnlineMVDRState(ctx, 5, 3)
    Y, m = np.ones((3, 9, 5), complex), np.ones((9, 5))
    call = ops.mvdr_souden_online_from_masks
    for kw, word in ((dict(lookahead=3), 'hold'),                 # a line of another L
                     (dict(lookahead=0), 'hold'),                 # a line without a look-ahead
                     (dict(lookahead=4, state=None), 'state'),    # a line without its state
                     (dict(lookahead=4, ctx=_Ctx()), 'context'),
                     (dict(lookahead=4, state=ops.OnlineMVDRState(_Ctx(), 5, 3)), 'context'),
                     (dict(lookahead=4, ref_channel=-1), 'ref_channel')):
        with pytest.raises(ValueError, match=word):
            call(Y, m, m, **{'state': state, 'hold': hold, **kw})
    with pytest.raises(ValueError, match='hold'):                 # of another D, of another F
        call(np.ones((4, 9, 5), complex), m, m, state=ops.OnlineMVDRState(ctx, 5, 4), hold=hold,
             lookahead=4)
    with pytest.raises(ValueError, match='hold'):
        call(np.ones((3, 9, 6), complex), np.ones((9, 6)), np.ones((9, 6)),
             state=ops.OnlineMVDRState(ctx, 6, 3), hold=hold, lookahead=4)
    with pytest.raises(ValueError, match='hold'):
        call(Y, m, m, state=state, hold=object(), lookahead=4)
    # the posteriors form: S lines, different ones, holding equally many frames
    g = np.full((2, 9, 5), 0.5)
    states = [ops.OnlineMVDRState(ctx, 5, 3) for _ in range(2)]
    other = ops.OnlineMVDRHold(ctx, 5, 3, 4)
    targets = ops.mvdr_souden_online_targets
    for holds in ([hold], [hold, hold], [hold, ops.OnlineMVDRHold(ctx, 5, 3, 5)],
                  [hold, ops.OnlineMVDRHold(_Ctx(), 5, 3, 4)]):
        with pytest.raises(ValueError, match='hold'):
            targets(Y, g, (0, 1), states=states, lookahead=4, hold=holds)
    other.held = 2
    with pytest.raises(ValueError, match='hold'):
        targets(Y, g, (0, 1), states=states, lookahead=4, hold=[hold, other])
    with pytest.raises(ValueError, match='ref_channel'):
        targets(Y, g, (0, 1), states=states, lookahead=4, ref_channel=-1)
    with pytest.raises(ValueError, match='hold'):
        ops.mvdr_online_release([])
    with pytest.raises(ValueError, match='postfilter'):
        ops.mvdr_online_release(hold, postfilter='x')


def test_argument_errors_before_any_device_work(no_context):
    from pb_chime5_amd import core, ops
    from pb_chime5_amd.online_mvdr import OnlineMVDR
    from pb_chime5_amd.streaming import StreamingEnhancer
    Y, m = np.ones((3, 9, 5), complex), np.ones((9, 5))
    for bad in (-1, 1.5, 65):
        with pytest.raises(ValueError, match='lookahead'):
            ops.mvdr_souden_online_from_masks(Y, m, m, lookahead=bad)
        with pytest.raises(ValueError, match='lookahead'):
            OnlineMVDR(channel=3, frequency_bins=5, lookahead=bad)
        with pytest.raises(ValueError, match='lookahead'):
            StreamingEnhancer(4, 3, lookahead=bad)
        with pytest.raises(ValueError, match='lookahead'):
            ops.OnlineMVDRHold.fresh(5, 3, bad)
    with pytest.raises(ValueError, match='lookahead'):
        ops.OnlineMVDRHold.fresh(5, 3, 0)
    with pytest.raises(ValueError, match='ref_channel'):
        ops.mvdr_souden_online_from_masks(Y, m, m, lookahead=2, ref_channel=-1)
    for host, word in ((dict(frames=np.ones((5, 4)), held=0), 'frames'),
                       (dict(frames=np.ones((5, 65, 3)), held=0), 'lookahead'),
                       (dict(frames=np.ones((5, 4, 33)), held=0), 'num_channels'),
                       (dict(frames=np.ones((5, 4, 3)), held=5), 'held'),
                       (dict(frames=np.ones((5, 4, 3)), mask=np.ones((5, 3)),
                             filter=np.ones((5, 3)), held=1), 'mask')):
        with pytest.raises(ValueError, match=word):
            ops.OnlineMVDRHold.from_host(host)
    # the stream: process after flush, a checkpoint of another L
    enh = StreamingEnhancer(4, 3, stft_size=64, stft_shift=16, lookahead=3)
    assert enh.lookahead == 3 and enh.holds is None               # nothing on the GPU yet
    enh.flush()
    with pytest.raises(RuntimeError, match='flush'):
        enh.process(np.zeros((4, 16)), np.ones((3, 16), bool))
    for theirs, mine in ((0, 3), (4, 3), (3, 0)):
        host = {'lookahead': theirs} if theirs else {}
        with pytest.raises(ValueError, match='lookahead'):
            StreamingEnhancer(4, 3, stft_size=64, stft_shift=16, lookahead=mine).from_host(host)
    enhancer = core.get_enhancer(wpe_online=True, gss_online=True, bf_online=True, stft_size=64,
                                 stft_shift=16, wpe_tabs=2, wpe_delay=1)
    with pytest.raises(ValueError, match='lookahead'):
        enhancer.stream(4, 3, 0, lookahead=65)
    assert enhancer.stream(4, 3, 0, lookahead=5).lookahead == 5
    assert enhancer.stream(4, 3, 0).lookahead == 0


# ------------------------------------------------------------------ the stream's accounting
def test_stream_sample_accounting(monkeypatch):
    """The bookkeeping of `StreamingEnhancer` alone -- `samples_in`, `samples_out`, the latency and
    the cut in `flush` -- with the library call, the frame count, the flush count and the states
    replaced by their geometry: the per-block counts below are the mock's own.  The real check of
    what a block releases is tests/test_gpu_stream_lookahead.py::test_sample_accounting."""
    import stream_reference as sr
    from pb_chime5_amd import ops
    from pb_chime5_amd.streaming import StreamingEnhancer
    W, H, L, N = 64, 16, 3, 1500
    line = dict(received=0, frames=0, out=0)

    def block(block, activity=None, *, release=False, **kw):
        n = block.shape[1]
        Tn = sr.num_frames(line['received'], n, W, H)
        line['received'] += n
        line['frames'] += Tn
        rows = (line['frames'] if release else max(0, line['frames'] - L)) - line['out']
        m = sr.emitted((line['out'] + rows) * H, W, H) - sr.emitted(line['out'] * H, W, H)
        line['out'] += rows
        return np.zeros((1, m)), None
    monkeypatch.setattr(ops, 'stream_block_lookahead', block)
    monkeypatch.setattr(ops, 'stream_num_frames', sr.num_frames)
    monkeypatch.setattr(ops, 'stream_flush_samples', sr.flush_samples)
    monkeypatch.setattr(StreamingEnhancer, '_states', lambda self: None)
    enh = StreamingEnhancer(4, 3, stft_size=W, stft_shift=H, lookahead=L)
    enh.stream = type('S', (), {'received': property(lambda self: line['received'])})()
    enh.ctx = type('C', (), {'last_mvdr_online_fallbacks_targets': lambda self, S: [0] * S,
                             'last_cacgmm_online_fallbacks': lambda self: 0})()
    cuts = sr.random_cuts(N, 3)
    counts = [enh.process(np.zeros((4, n)), np.ones((3, n), bool)).shape[-1] for n in cuts]
    late = [sr.num_samples_out(a, b - a, W, H) for a, b in sr.blocks_of(N, cuts)]
    assert sum(counts) == max(0, sum(late) - L * H) and counts != late
    assert enh.latency_samples == N - sum(counts) == W - H + N % H + L * H
    tail = enh.flush()
    assert tail.shape == (N - sum(counts),) and enh.samples_out == enh.samples_in == N
    assert line['out'] == line['frames']
