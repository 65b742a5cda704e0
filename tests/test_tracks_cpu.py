"""Long-range tracks, the host side: the float64 restatement the GPU tests measure against (tests/tracks_spec.py) is pinned to
the fixture the real reference wrote (tests/golden/make_golden_tracks.py), and everything that is decided before a launch --
track_plan, the argument checks of project_ptcld -- is checked without a GPU."""
import numpy as np
import pytest
import torch

import helpers
import tracks_spec as S

FX = 'tracks_b3_11x21_t4'


@pytest.fixture(scope='module')
def fx():
    return helpers.load_golden(FX)


@pytest.fixture(scope='module')
def spec(fx):
    """The float64 projection of the fixture's own fp32 points (computed once, shared, never written to)."""
    return S.project(fx['ref_points'], fx['start'], fx['tab_R'], fx['tab_t'], fx['tab_K_T'], fx['in_depth'])


def _within(measured, stored):
    # the same computation as the generator's: equal up to the summation order of a float64 matmul
    return measured <= float(stored) * (1 + 1e-6) + 1e-13


def test_spec_projection_equals_the_fixture_within_the_reference_error(fx, spec):
    T1, B, H, W = fx['ref_z'].shape
    live = spec['live'][:, :, None, None].expand(T1, B, H, W)
    xx, yy = S._pixel_grid(H, W)
    coord = torch.stack([xx, yy], -1)
    assert _within(S.worst(fx['ref_disp'], spec['uv'] - coord, live[..., None].expand(T1, B, H, W, 2)), fx['ref_vs_f64_uv'])
    assert _within(S.worst(fx['ref_z'], spec['z'], live), fx['ref_vs_f64_z'])
    assert _within(S.worst(fx['ref_depth_at'], spec['depth_at'], live & (spec['z'] > 0)), fx['ref_vs_f64_depth_at'])
    # the reference's own error is at the level of fp32 rounding of the quantities' sizes (uv up to a few W, depths below 6)
    assert float(fx['ref_vs_f64_uv']) < 2e-5 and float(fx['ref_vs_f64_z']) < 5e-6 and float(fx['ref_vs_f64_depth_at']) < 5e-5


def test_spec_gradient_equals_the_fixture_within_the_reference_error(fx):
    g = S.project_grad(fx['in_up_uv'], fx['ref_points'], fx['start'], fx['tab_R'], fx['tab_t'], fx['tab_K_T'])
    assert _within(S.worst(fx['ref_g_points'], g), fx['ref_vs_f64_g_points'])
    dead = ~S.project(fx['ref_points'], fx['start'], fx['tab_R'], fx['tab_t'], fx['tab_K_T'])['live']
    assert dead.any() and not np.any(fx['ref_g_points'][dead.numpy()])


def test_spec_chain_equals_the_fixture_within_the_reference_error(fx):
    from dvd_hip.networks.sceneflow_field import SceneFlowFieldNet
    net = helpers.seeded_fill_(SceneFlowFieldNet(net_width=256, n_layers=4, time_dependent=True, N_freq_xyz=16, N_freq_t=16),
                               int(fx['seed']))
    start, N = fx['start'].tolist(), int(fx['N'])
    B, H, W = len(start), int(fx['H']), int(fx['W'])
    ts = torch.from_numpy(fx['tab_ts_vali'])[start].view(B, 1, 1, 1).expand(B, 1, H, W)
    p0 = S.unproject(fx['in_depth'][start], fx['tab_R_T'][start], fx['tab_t'][start], fx['tab_K_inv_T'][start])
    assert S.worst(fx['ref_points'][0], p0) < 2e-6               # unprojection: a few ulp of coordinates below 8
    chain = S.integrate(net.state_dict(), p0, ts, float(fx['time_step']), fx['steps_valid'].tolist(), int(fx['n_steps']),
                        1.0 / 100.0)
    ref = torch.from_numpy(fx['ref_points']).double()
    assert _within(S.worst((ref - ref[0])[1:], (chain - chain[0])[1:]), fx['ref_vs_f64_points'])
    # rows past the end of the video are zero in both
    for b, v in enumerate(fx['steps_valid'].tolist()):
        assert not np.any(fx['ref_points'][v + 1:, b]) and not bool(chain[v + 1:, b].any())
    assert float(fx['time_step']) == 1.0 / N


def test_fixture_is_well_conditioned(fx, spec):
    T1, B, H, W = fx['ref_z'].shape
    live = spec['live'][:, :, None, None].expand(T1, B, H, W)
    assert float(spec['z'].abs()[live].min()) >= 0.1
    bad, frac = S.compare_inside(spec['inside'], spec, H, W, self_rows=1)
    assert bad == 0 and frac < 0.005
    assert bool((spec['z'][live] < 0).any()) and bool(spec['inside'][live].any()) and bool((~spec['inside'][live]).any())
    assert fx['steps_valid'].tolist() == [4, 3, 1]


def test_track_plan_counts():
    from dvd_hip.models.tracks import track_plan
    assert track_plan(7, [0, 3, 5], 4) == [4, 3, 1]
    assert track_plan(7, [6], 4) == [0]                        # the last frame has nowhere to go
    assert track_plan(80, range(80), 30) == [30] * 50 + list(range(29, -1, -1))
    assert track_plan(7, np.array([2, 2]), 1) == [1, 1]        # repeated start frames are fine
    assert track_plan(7, torch.tensor([1]), np.int64(9)) == [5]
    assert track_plan(7, [3.0], 2) == [2]                      # integral floats (frame ids travel as fp32 in the items)


@pytest.mark.parametrize('n_frames,start,n_steps', [
    (7, [], 4), (7, [-1], 4), (7, [7], 4), (7, [0, 3, 70], 4), (7, [1.5], 4), (7, [float('nan')], 4), (7, ['a'], 4),
    (7, [0], 0), (7, [0], -2), (7, [0], 1.5), (7, [True], 4), (0, [0], 4)])
def test_track_plan_refuses(n_frames, start, n_steps):
    from dvd_hip.models.tracks import track_plan
    with pytest.raises(ValueError, match='track_plan'):
        track_plan(n_frames, start, n_steps)


def test_default_chunk_fits_the_slab():
    from dvd_hip.models import tracks
    c = tracks.default_chunk(30, 384, 672)
    assert c * 31 * 3 * 384 * 672 * 4 <= tracks.SLAB_BYTES < (c + 1) * 31 * 3 * 384 * 672 * 4
    assert tracks.default_chunk(10 ** 6, 384, 672) == 1
    assert tracks._runs([4, 0, 2, 3, 1], 0, 5, 1) == [(0, 1), (2, 4)] and tracks._runs([1, 1], 0, 2, 1) == []


def _cams(B):
    return torch.eye(3).repeat(B, 1, 1, 1, 1), torch.zeros(B, 1, 1, 1, 3), torch.eye(3).repeat(B, 1, 1, 1, 1)


@pytest.mark.parametrize('shape', [(2, 4, 5, 3), (2, 4, 5, 1, 2), (2, 3, 4, 5), (2, 4, 5, 3, 1)])
def test_project_ptcld_refuses_points_of_another_layout(shape):
    from dvd_hip.losses.scene_flow_projection import project_ptcld
    with pytest.raises(ValueError, match='global_p1'):
        project_ptcld()(torch.zeros(shape), *_cams(2))


def test_project_ptcld_checks_cameras_sizes_and_device():
    from dvd_hip.losses.scene_flow_projection import project_ptcld
    R, t, K = _cams(2)
    P = torch.ones(2, 4, 5, 1, 3)
    for name, args in (('R_1_T', (R[:1], t, K)), ('R_1_T', (R.view(2, 3, 3), t, K)), ('t_1', (R, t.view(2, 3), K)),
                       ('K', (R, t, K[:, 0])), ('K', (R, t, None))):
        with pytest.raises(ValueError, match=name):
            project_ptcld()(P, *args)
    with pytest.raises(ValueError, match='2 x 2'):
        project_ptcld()(torch.ones(2, 1, 5, 1, 3), R, t, K)
    with pytest.raises(ValueError, match='global_p1'):
        project_ptcld()(None, R, t, K)
    with pytest.raises(RuntimeError, match='GPU tensor'):        # no CPU path: a well-formed call off the device is an error
        project_ptcld()(P, R, t, K)
    assert project_ptcld(is_one_way=False) is not None           # the reference's constructor signature


def test_ops_check_before_they_launch():
    from dvd_hip import ops
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.track_project(torch.zeros(1, 1, 3, 4, 4), [0], {'R': torch.eye(3)[None], 't': torch.zeros(1, 3), 'K_T': torch.eye(3)[None]})
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.project_backward(torch.zeros(1, 1, 4, 4, 2), torch.zeros(1, 1, 3, 4, 4), [0],
                             {'R': torch.eye(3)[None], 't': torch.zeros(1, 3), 'K_T': torch.eye(3)[None]})


def test_library_refuses_bad_arguments_before_any_hip_call():
    import ctypes
    from dvd_hip import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)                                     # never dereferenced: the checks come first
    assert lib.dvd_track_project(None, 1, one, one, one, one, None, 3, one, 0, None, None, None, 1, 1, 4, 4, None) == _lib.DVD_EINVAL
    assert b'null' in lib.dvd_last_error()
    assert lib.dvd_track_project(one, 1, one, one, one, one, None, 3, one, 0, None, None, None, 1, 1, 1, 4, None) == _lib.DVD_EINVAL
    assert lib.dvd_track_project(one, 1, one, one, one, one, one, 3, one, 0, None, None, None, 1, 1, 4, 4, None) == _lib.DVD_EINVAL
    assert b'depth_at' in lib.dvd_last_error()
    assert lib.dvd_project_bwd(one, one, 1, one, one, one, one, 0, one, 0, 1, 1, 4, 4, None) == _lib.DVD_EINVAL
    assert lib.dvd_project_bwd(one, None, 1, one, one, one, one, 3, one, 0, 1, 1, 4, 4, None) == _lib.DVD_EINVAL
