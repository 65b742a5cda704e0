"""Backward-in-time advection, the host side: the plans (track_plan_back, the signed render_plan), the pins of the forwards-only
defaults, the two C entries in the header / the exports / the bindings, and the float64 specification (tests/invert_spec.py) on
the inputs the GPU tests use -- the seeded fields and points of tests/golden/tracks_b3_11x21_t4.npz with start frames [1, 3, 6]
-- so that a field on which the fixed-point iteration does not converge cannot hide behind a tolerance."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import helpers
import invert_spec as I
import tracks_spec as S

FX = 'tracks_b3_11x21_t4'
START = [1, 3, 6]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net(seed, time_dependent):
    from dvd_hip.networks.sceneflow_field import SceneFlowFieldNet
    return helpers.seeded_fill_(SceneFlowFieldNet(net_width=256, n_layers=4, time_dependent=time_dependent, N_freq_xyz=16,
                                                  N_freq_t=16), seed)


class _Ctx(object):
    pass


@pytest.fixture(scope='module')
def ctx():
    """The fixture's inputs at the start frames and both seeded fields: computed once, shared, never written to."""
    c = _Ctx()
    fx = c.fx = helpers.load_golden(FX)
    c.N, c.H, c.W = int(fx['N']), int(fx['H']), int(fx['W'])
    B = len(START)
    c.p0 = S.unproject(fx['in_depth'][START], fx['tab_R_T'][START], fx['tab_t'][START], fx['tab_K_inv_T'][START])
    c.ts = torch.from_numpy(fx['tab_ts_vali'])[START].view(B, 1, 1, 1).expand(B, 1, c.H, c.W).double()
    c.sd = {True: _net(int(fx['seed']), True).state_dict(), False: _net(int(fx['seed']) + 1, False).state_dict()}
    return c


def test_track_plan_back_counts_and_refusals():
    from dvd_hip.models.tracks import track_plan_back
    assert track_plan_back(7, START, 3) == [1, 3, 3]
    assert track_plan_back(7, [0], 4) == [0]                          # the first frame has nowhere to come from
    assert track_plan_back(7, torch.tensor([6, 2]), np.int64(9)) == [6, 2]
    assert track_plan_back(7, np.array([2.0, 2.0]), 1) == [1, 1]
    for n_frames, start, n_back in [(7, [], 2), (7, [-1], 2), (7, [7], 2), (7, [1.5], 2), (7, [True], 2), (7, [0], 0),
                                    (7, [0], -1), (7, [0], 1.5), (0, [0], 2)]:
        with pytest.raises(ValueError, match='track_plan_back'):
            track_plan_back(n_frames, start, n_back)


def test_render_plan_is_signed_only_on_request():
    from dvd_hip.models.render import render_plan
    # the pin: with its defaults a later source is still refused, with the same words
    with pytest.raises(ValueError, match='later than'):
        render_plan(7, [3], [[2, 3, 5]])
    with pytest.raises(ValueError, match='integrates forwards only'):
        render_plan(7, [3], [[5]], True)
    assert render_plan(7, [3], [[2, 3, 5]], backward=True) == ([2, 3, 5], [0, 0, 0], [1, 0, -2])
    assert render_plan(7, [3, 0], [[6], [0, 6]], backward=True) == ([6, 0, 6], [0, 1, 1], [-3, 0, -6])
    assert render_plan(7, [3], [[2, 3]], backward=True) == render_plan(7, [3], [[2, 3]])
    assert render_plan(7, [3], [[2, 5]], advect=False, backward=True) == ([2, 5], [0, 0], [0, 0])
    for target, sources in [([3], [[7]]), ([3], [[-1]]), ([7], [[1]]), ([], []), ([3], [[]]), ([3], [[1], [2]])]:
        with pytest.raises(ValueError, match='render_plan'):
            render_plan(7, target, sources, backward=True)


def test_the_two_entries_are_in_the_header_the_exports_and_the_bindings():
    from dvd_hip import _lib
    src = open(os.path.join(ROOT, 'include', 'dvd_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    lib = _lib.load()
    assert lib.dvd_abi_version() == _lib.ABI_VERSION == 8 and re.search(r'#define\s+DVD_ABI_VERSION\s+8\b', src)
    for name in ('dvd_track_invert_update', 'dvd_track_project_from'):
        assert re.search(r'\bint\s+%s\s*\(' % name, code), name
        assert name in _lib.SIGNATURES and hasattr(ctypes.CDLL(lib._name), name), name
    # dvd_track_project_from is dvd_track_project's arguments plus `int k0` in front of the stream
    old, new = _lib.SIGNATURES['dvd_track_project'], _lib.SIGNATURES['dvd_track_project_from']
    assert new[0] is old[0] and new[1] == old[1][:-1] + [ctypes.c_int, old[1][-1]]


def test_library_refuses_bad_arguments_before_any_hip_call():
    from dvd_hip import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)                                        # never dereferenced: the checks come first
    assert lib.dvd_track_invert_update(one, one, one, one, None, 65536, 4, None) == _lib.DVD_EINVAL
    assert b'65535' in lib.dvd_last_error()
    assert lib.dvd_track_invert_update(one, one, one, one, None, 0, 4, None) == _lib.DVD_EINVAL
    assert lib.dvd_track_invert_update(one, one, one, one, None, 1, 1 << 30, None) == _lib.DVD_EINVAL
    assert lib.dvd_track_invert_update(one, one, one, one, None, 1, 0, None) == _lib.DVD_EINVAL
    assert lib.dvd_track_invert_update(one, None, one, one, None, 1, 4, None) == _lib.DVD_EINVAL
    assert b'null' in lib.dvd_last_error()
    assert lib.dvd_track_project_from(None, 1, one, one, one, one, None, 3, one, 0, None, None, None, 1, 1, 4, 4, -1,
                                      None) == _lib.DVD_EINVAL
    assert lib.dvd_track_project_from(one, 1, one, one, one, one, None, 3, one, 0, None, None, None, 1, 65536, 4, 4, -1,
                                      None) == _lib.DVD_EINVAL


def test_ops_check_before_they_launch():
    from dvd_hip import ops
    p = torch.zeros(1, 3, 4, 4)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.invert_update(p, p, p)
    with pytest.raises(ValueError, match='n_iter'):
        ops.invert_step(None, p, None, 0.0, 0.01, n_iter=0)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.invert_step(None, p, None, 0.0, 0.01)
    tabs = {'R': torch.eye(3)[None], 't': torch.zeros(1, 3), 'K_T': torch.eye(3)[None]}
    with pytest.raises(RuntimeError, match='k0'):
        ops.track_project(torch.zeros(1, 1, 3, 4, 4), [0], tabs, k0=0.5)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.track_project(torch.zeros(1, 1, 3, 4, 4), [0], tabs, k0=-1)


@pytest.mark.parametrize('time_dependent', [True, False])
def test_the_iteration_contracts_on_the_test_fields(ctx, time_dependent):
    """The condition of the test inputs: every successive residual of the float64 iteration is at most a tenth of the one
    before, over the rounds the default n_iter = 4 runs (DESIGN.md 5.3.5 has 0.015 - 0.032)."""
    sd, ts = ctx.sd[time_dependent], ctx.ts if time_dependent else None
    for j in (1, 2):
        res = []
        I.invert_step(sd, ctx.p0, None if ts is None else ts - j / ctx.N, 100.0, n_iter=4, residuals=res)
        worst = [float(r.max()) for r in res]
        print('time_dependent=%s step %d residuals %s' % (time_dependent, j, ' '.join('%.3g' % r for r in worst)))
        assert 1e-4 < worst[0] < 0.1                                   # the field does move the points
        for a, b in zip(worst[:-1], worst[1:]):
            assert b <= 0.1 * a, worst
        assert worst[3] < 4.8e-7                                       # below one fp32 ulp of |p| <= 6.3


@pytest.mark.parametrize('time_dependent', [True, False])
def test_the_inverse_followed_by_a_forward_step_returns(ctx, time_dependent):
    sd, ts = ctx.sd[time_dependent], ctx.ts if time_dependent else None
    t = None if ts is None else ts - 1.0 / ctx.N
    y = I.invert_step(sd, ctx.p0, t, 100.0, n_iter=4)
    assert float((y - ctx.p0).abs().max()) > 1e-4
    back = I.forward_step(sd, y, t, 100.0)
    assert S.worst(back, ctx.p0) <= 1e-7
    assert float(ctx.p0.abs().max()) <= 6.3


def test_the_two_sided_chain_and_its_projection(ctx):
    fx, N = ctx.fx, ctx.N
    pts, resid = I.chain(ctx.sd[True], ctx.p0, ctx.ts, 1.0 / N, START, N, 3, 2, 100.0)
    assert pts.shape == (6, 3, 3, ctx.H, ctx.W) and resid.shape == (3, 3)
    # rows from the origin on are tracks_spec's forward chain
    fwd = S.integrate(ctx.sd[True], ctx.p0, ctx.ts, 1.0 / N, [2, 2, 0], 2, 1.0 / 100.0)
    assert S.worst(pts[3:], fwd) <= 1e-12
    # rows before the video and their residuals are zero; the others are not
    live = torch.tensor([[0 <= s + j - 3 < N for s in START] for j in range(6)])
    assert live.tolist() == [[False, True, True], [False, True, True], [True, True, True], [True, True, True],
                             [True, True, False], [True, True, False]]
    assert not bool(pts[~live].any()) and bool(pts[live].flatten(1).abs().sum(1).gt(0).all())
    assert bool((resid[live[:3].flip(0)] > 0).all()) and not bool(resid[~live[:3].flip(0)].any())
    # pushing a backward row forwards again returns to the row after it
    t = ctx.ts - 2.0 / N
    assert S.worst(I.forward_step(ctx.sd[True], pts[1, 1:], t[1:], 100.0), pts[2, 1:]) <= 1e-7
    # project with k0: row by row it is tracks_spec.project of that row with the shifted start
    spec = I.project(pts, START, fx['tab_R'], fx['tab_t'], fx['tab_K_T'], fx['in_depth'], k0=-3)
    assert spec['live'].tolist() == live.tolist()
    one = S.project(pts[1:2, 1:], [1, 4], fx['tab_R'], fx['tab_t'], fx['tab_K_T'], fx['in_depth'])
    for k in ('uv', 'z', 'inside', 'depth_at'):
        assert torch.equal(spec[k][1, 1:], one[k][0]) and not bool(spec[k][~live].any()), k
    same = I.project(pts[3:], START, fx['tab_R'], fx['tab_t'], fx['tab_K_T'], fx['in_depth'])
    want = S.project(pts[3:], START, fx['tab_R'], fx['tab_t'], fx['tab_K_T'], fx['in_depth'])
    for k in want:
        assert torch.equal(same[k], want[k]), k
    # `inside` of the specification alone stays within compare_inside's cap for these starts (row 3 is the frames' own)
    edge, absz = S.edge_distance(spec['uv'], spec['z'], ctx.H, ctx.W)
    skip = ((edge < 1e-3) | (absz < 1e-4)) & live[:, :, None, None]
    rest = live.clone()
    rest[3] = False
    frac = float(skip[rest].double().mean())
    print('inside: %.3f %% of the points of the rows that look into another camera are left out' % (100 * frac))
    assert frac <= 0.005 and not bool((skip[3] & ~S.border_pixels(ctx.H, ctx.W)).any())


def test_the_fp32_form_is_close_to_the_specification(ctx):
    """The yardstick has to be a yardstick: the same expressions in fp32 stay within a few ulp of the points."""
    N = ctx.N
    p64, r64 = I.chain(ctx.sd[True], ctx.p0, ctx.ts, 1.0 / N, START, N, 3, 2, 100.0)
    p32, r32 = I.chain(ctx.sd[True], ctx.p0, ctx.ts, 1.0 / N, START, N, 3, 2, 100.0, dtype=torch.float32)
    assert p32.dtype == torch.float32 and r32.dtype == torch.float32
    d = S.worst((p32.double() - p32[3].double()), (p64 - p64[3]))
    assert 0 < d < 1e-5, d
    # its projection IS the reference's: on the fixture's own points and starts it returns the fixture's fp32 results
    fx = ctx.fx
    args = (fx['ref_points'], fx['start'].tolist(), fx['tab_R'], fx['tab_t'], fx['tab_K_T'], fx['in_depth'])
    f32, f64 = I.project(*args, dtype=torch.float32), I.project(*args)
    T1, B, H, W = fx['ref_z'].shape
    live = f64['live'][:, :, None, None].expand(T1, B, H, W)
    xx, yy = S._pixel_grid(H, W)
    uv = (torch.from_numpy(fx['ref_disp']).double() + torch.stack([xx, yy], -1)) * live[..., None]
    assert S.worst(f32['uv'], uv) <= 1e-12 and S.worst(f32['z'], fx['ref_z'], live) == 0.0
    assert S.worst(f32['depth_at'], fx['ref_depth_at'], live & (f64['z'] > 0)) <= 1e-7
    assert f32['live'].tolist() == f64['live'].tolist() and not bool(f32['uv'][~f32['live']].any())
