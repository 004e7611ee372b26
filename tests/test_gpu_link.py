"""Cross-window class linking on the GPU (gss_cacgmm_link, gss_cacgmm_link_gather;
ops.link_posteriors and its device-resident form).

The reference for every number is tests/link_reference.py.  The mapping is asked to EQUAL the
reference's on the same input bits: every parity cell has a margin (best minus second-best total)
of at least 1e-6, ten orders above what two float64 summation orders differ by, except the two
cells that are exact ties by construction (two identical rows; one frame of one frequency with
power-of-two values), where the tie rule decides in the reference and on the device alike.  The
scores are held to 4 F L 2^-53 absolute (`link_reference.score_bound`: sums of non-negative terms
in any order, scores at most 1)."""
import ctypes

import numpy as np
import pytest

import link_reference as lr

pytestmark = pytest.mark.gpu

c_void_p = ctypes.c_void_p


def _ptr(buf):
    return c_void_p(buf.ptr if buf is not None else None)


def _link(ctx, prev, cur, pb, cb, L):
    """prev (F,K,T_prev), cur (F,K,T_cur) in the device layout -> (mapping (K,), S (K,K))."""
    from pb_chime5_amd import ops
    F, K, T_prev = prev.shape
    p_d = ctx.to_device(np.ascontiguousarray(prev, dtype=np.float64))
    c_d = ctx.to_device(np.ascontiguousarray(cur, dtype=np.float64))
    m_d, s_d = ctx.empty(max(4 * K, 16)), ctx.empty(max(8 * K * K, 16))
    ops.link_posteriors_device(ctx, p_d, T_prev, pb, c_d, cur.shape[2], cb, L, F, K, m_d, s_d)
    return ctx.to_host(m_d, (K,), np.int32), ctx.to_host(s_d, (K, K), np.float64)


# ------------------------------------------------------------------ parity with the reference
@pytest.mark.parametrize('cell', lr.CELLS, ids=lr.cell_id)
def test_link_equals_the_reference(gpu_ctx, cell):
    F, K, T_prev, T_cur, L, pb, cb, kind = cell
    prev, cur, hidden = lr.parity_input(cell)
    want, S, margin = lr.parity_reference(cell)
    if kind in ('plain', 'zero_row') and K > 1:
        assert margin >= lr.PARITY_MIN_MARGIN
    mapping, got = _link(gpu_ctx, prev, cur, pb, cb, L)
    err = float(np.max(np.abs(got - S)))
    print(f'link {lr.cell_id(cell)}: margin {margin:.1e}, scores differ by {err:.2e} '
          f'(bound {lr.score_bound(F, L):.2e}), mapping {mapping.tolist()}')
    assert sorted(mapping.tolist()) == list(range(K))
    np.testing.assert_array_equal(mapping, want)
    assert err <= lr.score_bound(F, L)
    if kind == 'tie':       # identical rows give identical bits on the device too
        h0, h1 = int(hidden[0]), int(hidden[1])
        assert got[:, h0].tobytes() == got[:, h1].tobytes()
    if kind == 'one_frame':
        assert np.all(got == 1.0)
    if kind == 'zero_row':
        assert np.all(got[:, int(hidden[1])] == 0.0)
    # the same call gives the same bits
    again_m, again_s = _link(gpu_ctx, prev, cur, pb, cb, L)
    assert again_m.tobytes() == mapping.tobytes() and again_s.tobytes() == got.tobytes()


def test_operator_layouts_and_the_gather(gpu_ctx):
    """ops.link_posteriors takes (K,T,F) host tables and frame pairs; the device gather renumbers
    a table by the mapping without a host round trip."""
    from pb_chime5_amd import ops
    ctx = gpu_ctx
    cell = lr.CELLS[5]
    F, K, T_prev, T_cur, L, pb, cb, _ = cell
    prev, cur, _ = lr.parity_input(cell)
    want, S, _ = lr.parity_reference(cell)
    mapping, scores = ops.link_posteriors(prev.transpose(1, 2, 0), cur.transpose(1, 2, 0),
                                          prev_frames=(pb, pb + L), cur_frames=(cb, cb + L), ctx=ctx)
    np.testing.assert_array_equal(mapping, want)
    assert float(np.max(np.abs(scores - S))) <= lr.score_bound(F, L)
    # whole tables: the default frames
    same = np.ascontiguousarray(cur[:, :, cb:cb + L])
    m2, s2 = ops.link_posteriors(prev[:, :, pb:pb + L].transpose(1, 2, 0), same.transpose(1, 2, 0),
                                 ctx=ctx)
    assert m2.tobytes() == mapping.tobytes() and s2.tobytes() == scores.tobytes()
    c_d, m_d, o_d = ctx.to_device(cur), ctx.to_device(mapping), ctx.empty(cur.nbytes)
    ops.link_gather_device(ctx, c_d, F, K, T_cur, m_d, o_d)
    np.testing.assert_array_equal(ctx.to_host(o_d, cur.shape, np.float64), cur[:, mapping, :])
    # an entry outside [0, K) writes NaN for that class and reads nothing
    bad = mapping.copy()
    bad[1] = K
    ops.link_gather_device(ctx, c_d, F, K, T_cur, ctx.to_device(bad), o_d)
    out = ctx.to_host(o_d, cur.shape, np.float64)
    assert np.all(np.isnan(out[:, 1, :]))
    np.testing.assert_array_equal(out[:, [0, 2], :], cur[:, mapping[[0, 2]], :])


# ------------------------------------------------------------------ hygiene
@pytest.fixture
def fresh_ctx():
    from pb_chime5_amd import _capi
    ctx = _capi.Context(0)
    yield ctx
    ctx.close()


def test_poisoned_workspace_changes_nothing(fresh_ctx):
    """Two parity cells under gss_debug_workspace in both fill patterns: no guard is touched and
    the bits are those of the plain run (a fresh context: the reserve's own term covers the
    call)."""
    ctx = fresh_ctx
    assert ctx.workspace_bytes() == 0
    for cell in (lr.CELLS[3], lr.CELLS[4]):
        F, K, T_prev, T_cur, L, pb, cb, _ = cell
        prev, cur, _ = lr.parity_input(cell)
        plain = _link(ctx, prev, cur, pb, cb, L)
        for pattern in (0x00, 0xFF):
            ctx.debug_workspace(pattern)
            try:
                got = _link(ctx, prev, cur, pb, cb, L)
                count, text, _ = ctx.debug_workspace_report()
            finally:
                ctx.debug_workspace(None)
            assert count == 0, text
            assert got[0].tobytes() == plain[0].tobytes(), (cell, pattern)
            assert got[1].tobytes() == plain[1].tobytes(), (cell, pattern)
        np.testing.assert_array_equal(plain[0], lr.parity_reference(cell)[0])
    assert ctx.workspace_bytes() > 0


# ------------------------------------------------------------------ errors
def test_link_errors_come_back_before_any_launch(gpu_ctx):
    from pb_chime5_amd import _capi
    ctx = gpu_ctx
    cell = lr.CELLS[5]
    F, K, T_prev, T_cur, L, pb, cb, _ = cell
    prev, cur, _ = lr.parity_input(cell)
    p_d, c_d = ctx.to_device(prev), ctx.to_device(cur)
    m_d, s_d = ctx.empty(64), ctx.empty(8 * 81)
    sentinel = np.full(K, -7, np.int32)

    def call(p=p_d, Tp=T_prev, pb_=pb, c=c_d, Tc=T_cur, cb_=cb, L_=L, F_=F, K_=K, m=m_d, s=s_d):
        return ctx.lib.gss_cacgmm_link(ctx.handle, _ptr(p), Tp, pb_, _ptr(c), Tc, cb_, L_, F_, K_,
                                       _ptr(m), _ptr(s))
    cases = [
        (dict(p=None), 'prev_dev is NULL'), (dict(c=None), 'cur_dev is NULL'),
        (dict(m=None), 'mapping_dev is NULL'), (dict(s=None), 'scores_dev is NULL'),
        (dict(F_=0), 'F=0'), (dict(K_=0), 'K=0'), (dict(L_=0), 'L=0'), (dict(L_=-3), 'L=-3'),
        (dict(pb_=-1), 'prev frames'), (dict(pb_=T_prev - L + 1), 'prev frames'),
        (dict(L_=T_prev + 1, pb_=0, cb_=0), 'prev frames'),
        (dict(cb_=-1), 'cur frames'), (dict(cb_=T_cur - L + 1), 'cur frames'),
        (dict(Tc=cb + L - 1), 'cur frames'), (dict(Tp=0), 'prev frames'),
        (dict(pb_=2 ** 62), 'prev frames'),
    ]
    for kw, match in cases:
        ctx.upload(m_d, sentinel)
        status = call(**kw)
        assert status == _capi.GSS_ERR_INVALID, match
        with pytest.raises(ValueError, match=match):
            ctx._check(status, 'gss_cacgmm_link')
        if kw.get('m', m_d) is not None:
            np.testing.assert_array_equal(ctx.to_host(m_d, (K,), np.int32), sentinel)
    status = call(K_=9)
    assert status == _capi.GSS_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError, match='K=9 is larger than 8'):
        ctx._check(status, 'gss_cacgmm_link')
    np.testing.assert_array_equal(ctx.to_host(m_d, (K,), np.int32), sentinel)
    # the gather's rules
    o_d = ctx.empty(cur.nbytes)

    def gather(g=c_d, F_=F, K_=K, T_=T_cur, m=m_d, o=o_d):
        return ctx.lib.gss_cacgmm_link_gather(ctx.handle, _ptr(g), F_, K_, T_, _ptr(m), _ptr(o))
    for kw, match in [(dict(g=None), 'gamma_dev is NULL'), (dict(m=None), 'mapping_dev is NULL'),
                      (dict(o=None), 'out_dev is NULL'), (dict(F_=0), 'F=0'), (dict(K_=0), 'K=0'),
                      (dict(T_=0), 'T=0'), (dict(o=c_d), 'out_dev is gamma_dev')]:
        status = gather(**kw)
        assert status == _capi.GSS_ERR_INVALID, match
        with pytest.raises(ValueError, match=match):
            ctx._check(status, 'gss_cacgmm_link_gather')
    assert gather(K_=20) == _capi.GSS_ERR_UNSUPPORTED
    # and the context is usable afterwards: the good call still gives the reference's mapping
    ctx._check(call(), 'gss_cacgmm_link')
    np.testing.assert_array_equal(ctx.to_host(m_d, (K,), np.int32), lr.parity_reference(cell)[0])


def test_profile_names_every_launch(fresh_ctx):
    ctx = fresh_ctx
    cell = lr.CELLS[2]
    F, K, T_prev, T_cur, L, pb, cb, _ = cell
    prev, cur, _ = lr.parity_input(cell)
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        _link(ctx, prev, cur, pb, cb, L)
        report = ctx.profile_report()
    finally:
        ctx.profile_enable(False)
    assert report['link_products']['calls'] == 1 and report['link_finish']['calls'] == 1
