"""dvd_track_invert_update (csrc/invert.hip), ops.invert_step and dvd_track_project_from (csrc/track.hip) on the GPU.

Everything here is exact.  The update is one fp32 subtraction per value and a max of absolute differences, so torch's fp32
`p - sf` and `(y - y_old).abs().amax()` on the device are its specification bit for bit; ops.invert_step is a hand-written
loop of SceneFlowMLPKernels.forward and ops.invert_update; a row of track_project(k0=..) is track_project of that row alone
with the shifted start frames.  Shapes: 11 x 21 (H * W odd: one value per thread), 8 x 12 (16-byte accesses), a view of the
8 x 12 case that starts 4 bytes off a 16-byte boundary (back to one value per thread), one and five images (more than one
block row), and 40 x 40 (more than one block per image on either path).
"""
import ctypes

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FX = 'tracks_b3_11x21_t4'
SHAPES = [(1, 11, 21, 0), (5, 11, 21, 0), (1, 8, 12, 0), (5, 8, 12, 0), (5, 8, 12, 1), (2, 40, 40, 0), (2, 40, 40, 3)]


def _rand(shape, seed, off=0):
    """A contiguous fp32 GPU tensor of `shape` whose first element sits 4 * off bytes past a 16-byte boundary."""
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))
    flat = torch.empty(n + 4, device=DEV)
    assert flat.data_ptr() % 16 == 0
    flat[off:off + n] = (torch.rand(n, generator=g) * 8 - 4).to(DEV)
    v = flat[off:off + n].view(shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
    return v


def _want(p, sf, y_old):
    y = p - sf
    return y, (y - y_old).abs().flatten(1).amax(1)


@pytest.mark.parametrize('B,H,W,off', SHAPES)
def test_update_and_residual_bit_for_bit(B, H, W, off):
    from dvd_hip import ops
    p, sf, y_old = (_rand((B, 3, H, W), 10 * s + B + H, off) for s in (1, 2, 3))
    want_y, want_r = _want(p, sf, y_old)
    resid = torch.zeros(B, device=DEV)
    out = _rand((B, 3, H, W), 4, off)
    got = ops.invert_update(p, sf, y_old, out=out, resid=resid)
    assert got is out and torch.equal(out, want_y) and torch.equal(resid, want_r) and bool((resid > 0).all())
    # the residual is FOLDED into what resid holds: a larger value stays
    big = torch.full((B,), 100.0, device=DEV)
    ops.invert_update(p, sf, y_old, resid=big)
    assert bool((big == 100.0).all())
    # resid=None and an output of the wrapper's own
    assert torch.equal(ops.invert_update(p, sf, y_old), want_y)


@pytest.mark.parametrize('B,H,W,off', [(5, 11, 21, 0), (5, 8, 12, 0), (5, 8, 12, 1)])
def test_y_old_may_alias_p_or_the_output(B, H, W, off):
    from dvd_hip import ops
    p, sf, y_old = (_rand((B, 3, H, W), 20 * s + H, off) for s in (1, 2, 3))
    # y_old is p: the first round of the iteration
    want_y, want_r = _want(p, sf, p)
    resid = torch.zeros(B, device=DEV)
    assert torch.equal(ops.invert_update(p, sf, p, resid=resid), want_y) and torch.equal(resid, want_r)
    # y_old is the output: every later round
    want_y, want_r = _want(p, sf, y_old)
    y = y_old.clone() if off == 0 else _rand((B, 3, H, W), 0, off).copy_(y_old)
    resid.zero_()
    assert ops.invert_update(p, sf, y, out=y, resid=resid) is y
    assert torch.equal(y, want_y) and torch.equal(resid, want_r)
    with pytest.raises(RuntimeError, match='alias'):
        ops.invert_update(p, sf, y_old, out=p)
    with pytest.raises(RuntimeError, match='sf must be'):
        ops.invert_update(p, sf[:1], y_old)
    with pytest.raises(RuntimeError, match='resid'):
        ops.invert_update(p, sf, y_old, resid=torch.zeros(B + 1, device=DEV))


@pytest.mark.parametrize('H,W', [(11, 21), (8, 12)])
def test_a_nan_is_inf_in_its_own_image_only(H, W):
    from dvd_hip import ops
    B = 3
    p, sf, y_old = (_rand((B, 3, H, W), 30 * s + W) for s in (1, 2, 3))
    want_y, want_r = _want(p, sf, y_old)
    sf = sf.clone()
    sf[1, 2, H - 1, W - 2] = float('nan')
    resid = torch.zeros(B, device=DEV)
    y = ops.invert_update(p, sf, y_old, resid=resid)
    assert resid[1].item() == float('inf') and torch.equal(resid[[0, 2]], want_r[[0, 2]])
    assert int(torch.isnan(y).sum()) == 1 and torch.equal(y[[0, 2]], want_y[[0, 2]])
    y_inf = y_old.clone()
    y_inf[2, 0, 0, 0] = float('inf')
    resid.zero_()
    ops.invert_update(p, sf, y_inf, resid=resid)
    assert resid[1].item() == float('inf') and resid[2].item() == float('inf') and resid[0] == want_r[0]


def test_caps_are_refused_before_any_launch():
    from dvd_hip import _lib, ops
    lib = _lib.load()
    buf = torch.full((64,), 7.0, device=DEV)
    ptr = ctypes.c_void_p(buf.data_ptr())
    stream = ops._stream()
    assert lib.dvd_track_invert_update(ptr, ptr, ptr, ptr, None, 65536, 4, stream) == _lib.DVD_EINVAL
    assert b'65535' in lib.dvd_last_error()
    assert lib.dvd_track_invert_update(ptr, ptr, ptr, ptr, None, 1, 1 << 30, stream) == _lib.DVD_EINVAL
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())                                   # nothing ran: p - sf would have written zeros


def _kernels(seed, time_dependent):
    from dvd_hip import ops
    from dvd_hip.networks.sceneflow_field import SceneFlowFieldNet
    net = helpers.seeded_fill_(SceneFlowFieldNet(net_width=256, n_layers=4, time_dependent=time_dependent, N_freq_xyz=16,
                                                 N_freq_t=16), seed).to(DEV)
    kern = ops.SceneFlowMLPKernels(DEV, n_freq_xyz=16, n_freq_t=16, time_dependent=time_dependent)
    kern.pack(net.parameter_list()[0::2], net.parameter_list()[1::2])
    return kern


@pytest.mark.parametrize('time_dependent,H,W', [(True, 11, 21), (False, 8, 12)])
def test_invert_step_is_the_hand_written_loop(time_dependent, H, W):
    from dvd_hip import ops
    B, n_iter = 3, 4
    kern = _kernels(5, time_dependent)
    p = _rand((B, 3, H, W), 41)
    t = (torch.tensor([1.0, 3.0, 6.0], device=DEV) / 7).view(B, 1, 1, 1).expand(B, 1, H, W).contiguous() if time_dependent else None
    resid = torch.full((B,), 9.0, device=DEV)                          # the wrapper zeroes it before the last update
    got = ops.invert_step(kern, p, t, -2.0 / 7, 0.01, n_iter=n_iter, resid=resid)
    y, sf = p, torch.empty_like(p)
    for i in range(n_iter):
        kern.forward(y, t, t_offset=-2.0 / 7, out_scale=0.01, sf_out=sf)
        want_r = torch.zeros(B, device=DEV)
        y = ops.invert_update(p, sf, y, resid=want_r)
    assert torch.equal(got, y) and torch.equal(resid, want_r)
    assert 0 < float(resid.max()) < float((got - p).abs().max())       # it moved, and the last round moved it less
    # out / scratch of the caller's own, one round, no residual
    out, scratch = torch.empty_like(p), torch.empty_like(p)
    assert ops.invert_step(kern, p, t, -2.0 / 7, 0.01, n_iter=1, out=out, scratch=scratch) is out
    kern.forward(p, t, t_offset=-2.0 / 7, out_scale=0.01, sf_out=sf)
    assert torch.equal(scratch, sf) and torch.equal(out, p - sf)
    with pytest.raises(ValueError, match='n_iter'):
        ops.invert_step(kern, p, t, 0.0, 0.01, n_iter=0)
    with pytest.raises(RuntimeError, match='three buffers'):
        ops.invert_step(kern, p, t, 0.0, 0.01, out=p)


@pytest.mark.parametrize('H,W,k0', [(11, 21, -2), (8, 12, -2), (8, 12, 1)])
def test_projection_rows_with_an_offset(H, W, k0):
    from dvd_hip import ops
    fx = helpers.load_golden(FX)
    N, start, T1 = int(fx['N']), [1, 3, 6], 5
    tabs = {k: helpers.t(fx['tab_' + k], DEV) for k in ('R', 't', 'K_T')}
    B = len(start)
    points = _rand((T1, B, 3, H, W), 51)
    depth = _rand((N, 1, H, W), 52).abs() + 0.5
    got = ops.track_project(points, start, tabs, depth_all=depth, k0=k0)
    assert set(got) == {'uv', 'z', 'inside', 'depth_at'}
    n_dead = 0
    for k in range(T1):
        for b in range(B):
            g = start[b] + k + k0
            if 0 <= g < N:
                one = ops.track_project(points[k:k + 1, b:b + 1].contiguous(), [g], tabs, depth_all=depth)
                for name, v in one.items():
                    assert torch.equal(got[name][k, b], v[0, 0]), (name, k, b)
                assert bool(got['uv'][k, b].any())
            else:
                n_dead += 1
                for name, v in got.items():
                    assert not bool(v[k, b].any()), (name, k, b)
    assert n_dead == (3 if k0 == -2 else 7)                           # frames -1, 7, 8 / 7, 8 of start 3 and all of start 6
    # k0 = 0 is the old entry, and the old entry keeps its bits
    same = ops.track_project(points, start, tabs, depth_all=depth, k0=0)
    old = ops.track_project(points, start, tabs, depth_all=depth)
    for name in old:
        assert torch.equal(same[name], old[name]), name
