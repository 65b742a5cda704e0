"""Query-point tracks without a GPU: the specification checks itself (tests/point_tracks_spec.py), the host helpers and every
refusal that happens before a launch (dvd_hip/models/point_tracks.py, ops.point_*, csrc/point_track.hip)."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import helpers
import point_tracks_spec as PS

FX = 'tracks_b3_11x21_t4'


def _tabs(fx):
    return {k: fx['tab_' + k] for k in ('R_T', 'R', 't', 'K_T', 'K_inv_T', 'ts_vali')}


def test_mirror_equals_the_loop_on_random_cases():
    for T1, Q, N, origin, seed, sx, sy in ((1, 1, 3, -1, 0, 1.0, 1.0), (4, 7, 5, 1, 1, 1.0, 1.0), (6, 33, 8, 2, 2, 0.5, 1.75),
                                          (3, 40, 4, 0, 3, 256 / 21.0, 256 / 11.0)):
        c = PS.score_case(T1, Q, N, origin, seed)
        args = (c['uv'], c['visible'], c['target'], origin, c['gt_uv'], c['gt_state'])
        mirror = PS.score_mirror(*args, sx=sx, sy=sy)
        loop = PS.score_loop(*args, sx=sx, sy=sy)
        assert mirror.tolist() == loop, (T1, Q, N)
        if origin >= 0:
            assert not mirror[origin].any()
    # the cases hold what they promise: every branch is taken somewhere
    c = PS.score_case(6, 257, 8, 2, 7)
    s = PS.score_mirror(c['uv'], c['visible'], c['target'], 2, c['gt_uv'], c['gt_state']).sum(0)
    assert s[0] > s[1] > 0 and 0 < s[2] < s[0] and all(s[13:18] > 0) and all(np.diff(s[3:8]) >= 0) and s[3] > 0 and s[7] < s[1]
    assert (c['target'] < 0).any() and np.isnan(c['uv']).any() and np.isinf(c['uv']).any()
    assert (c['gt_state'] == 255).any() and (c['gt_state'] == 2).any()


def test_a_distance_on_the_threshold_is_not_within_and_a_nan_never_is():
    gt_uv = np.zeros((1, 1, 2), np.float32)
    gt_state = np.zeros((1, 1), np.uint8)
    target, vis = np.zeros((1, 1), np.int32), np.ones((1, 1), np.uint8)
    for uv, want_within, err in (([4.0, 0.0], [0, 0, 0, 1, 1], 4.0), ([np.nan, 0.0], [0] * 5, 1024.0),
                                 ([0.0, 3.9999998], [0, 0, 1, 1, 1], 3.9999998), ([5000.0, 0.0], [0] * 5, 1024.0)):
        s = PS.score_mirror(np.float32([[uv]]), vis, target, -1, gt_uv, gt_state, shift=20)[0]
        assert s[:3].tolist() == [1, 1, 1] and s[3:8].tolist() == want_within and s[8:13].tolist() == want_within
        assert s[13:18].tolist() == [1 - w for w in want_within]
        e = np.float32(err)
        assert s[18] == int(round(min(float(np.sqrt(e * e)), 1024.0) * 2 ** 20))


def test_queries_first_and_strided():
    from dvd_hip.models import point_tracks as PT
    gt_uv = np.arange(3 * 6 * 2, dtype=np.float64).reshape(3, 6, 2)
    st = np.array([[1, 0, 0, 1, 0, 0], [1, 1, 1, 1, 1, 1], [0, 2, 0, 0, 0, 0]], np.uint8)
    q, track = PT.queries_first(gt_uv, st)
    assert track.tolist() == [0, 2]
    assert q.tolist() == [[1.0] + gt_uv[0, 1].tolist(), [0.0] + gt_uv[2, 0].tolist()]
    q, track = PT.queries_strided(gt_uv, st, stride=2)
    assert track.tolist() == [2, 0, 2, 0, 2]
    assert q[:, 0].tolist() == [0, 2, 2, 4, 4]
    assert q[1, 1:].tolist() == gt_uv[0, 2].tolist() and q[4, 1:].tolist() == gt_uv[2, 4].tolist()
    q, track = PT.queries_strided(gt_uv, st, stride=5)
    assert q[:, 0].tolist() == [0, 5, 5] and track.tolist() == [2, 0, 2]
    q, track = PT.queries_strided(gt_uv, np.ones_like(st))
    assert q.shape == (0, 3) and track.shape == (0,)
    for bad in (0, 1.5, True):
        with pytest.raises(ValueError, match='stride'):
            PT.queries_strided(gt_uv, st, stride=bad)
    with pytest.raises(ValueError, match='gt_uv'):
        PT.queries_first(gt_uv[..., :1], st)
    with pytest.raises(ValueError, match='gt_uv'):
        PT.queries_strided(gt_uv, st[:, :5])


def test_track_points_host_validation():
    from dvd_hip.models import point_tracks as PT
    N, H, W = 7, 11, 21
    f, xy = PT.check_queries('t', [[0, 0, 0], [6, 20, 10], [3, 1.5, 2.25]], N, H, W)
    assert f.dtype == np.int32 and f.tolist() == [0, 6, 3] and xy.dtype == np.float32 and xy[2].tolist() == [1.5, 2.25]
    for bad, word in (([], 'queries'), (np.zeros((0, 3)), 'no queries'), ([[0.5, 1, 1]], 'frames'), ([[7, 1, 1]], 'frames'),
                      ([[-1, 1, 1]], 'frames'), ([[0, 20.01, 1]], 'positions'), ([[0, 1, -0.01]], 'positions'),
                      ([[0, 1, 10.5]], 'positions'), ([[0, float('nan'), 1]], 'NaN'), ([[float('nan'), 1, 1]], 'NaN'),
                      ([[0, 1]], 'queries'), ('abc', 'queries')):
        with pytest.raises(ValueError, match=word):
            PT.check_queries('t', bad, N, H, W)
    model = SimpleNamespace(opt=SimpleNamespace(use_cnn=False))
    store = SimpleNamespace(cat=SimpleNamespace(n_frames=N), H=H, W=W)
    good = [[1, 2.5, 3.5]]
    for kw, word in ((dict(n_steps=-1), 'n_steps'), (dict(n_steps=1.5), 'n_steps'), (dict(n_back=-2), 'n_back'),
                     (dict(n_back=True), 'n_back'), (dict(n_back=1, n_iter=0), 'n_iter'), (dict(chunk=0), 'chunk'),
                     (dict(z_tol=-1.0), 'z_tol'), (dict(z_tol=float('nan')), 'z_tol'), (dict(n_steps=65535), '65535')):
        with pytest.raises(ValueError, match=word):
            PT.track_points(model, store, good, **kw)
    with pytest.raises(ValueError, match='no queries'):
        PT.track_points(model, store, np.zeros((0, 3)))
    with pytest.raises(NotImplementedError, match='use_cnn'):
        PT.track_points(SimpleNamespace(opt=SimpleNamespace(use_cnn=True)), store, good)
    with pytest.raises(ValueError, match='gt_uv'):
        PT.score_tracks(model, store, good, np.zeros((1, N + 1, 2)), np.zeros((1, N), np.uint8))
    with pytest.raises(ValueError, match='gt_uv'):
        PT.score_tracks(model, store, good, np.zeros((1, N, 2)), np.zeros((2, N), np.uint8))
    assert PT.default_chunk(61) == (8 << 30) // (61 * 12)


def test_ops_refuse_cpu_tensors_and_bad_arguments_before_a_launch():
    from dvd_hip import ops
    assert len(ops.POINT_SUMS) == 19 and len(set(ops.POINT_SUMS)) == 19 and ops.POINT_SUMS[0] == 'n_eval'
    tabs = {k: torch.zeros(2, 3, 3) for k in ('R_T', 'K_inv_T', 'R', 'K_T')}
    tabs.update(t=torch.zeros(2, 3), ts_vali=torch.zeros(2))
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.point_seed([0], torch.zeros(1, 2), torch.ones(2, 1, 4, 4), tabs)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.point_project(torch.zeros(1, 3, 1), [0], torch.zeros(1, 2), tabs, torch.ones(2, 1, 4, 4))
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.point_score(torch.zeros(1, 1, 2), torch.zeros(1, 1, dtype=torch.uint8), torch.zeros(1, 1, dtype=torch.int32),
                        torch.zeros(1, 2, 2), torch.zeros(1, 2, dtype=torch.uint8))
    assert ops.point_thr2((1, 2, 4, 8, 16)).tolist() == [1.0, 4.0, 16.0, 64.0, 256.0]
    for bad in ((1, 2, 4, 8), (1, 2, 2, 8, 16), (0, 1, 2, 4, 8), (1, 2, 4, 8, float('nan')), (1, 2, 4, 8, 1e30), 'abcde', None):
        with pytest.raises(RuntimeError, match='thresholds'):
            ops.point_thr2(bad)


def test_library_refuses_bad_arguments_before_any_hip_call():
    from dvd_hip import _lib
    lib = _lib.load()
    E = _lib.DVD_EINVAL
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    thr = (ctypes.c_float * 5)(1, 4, 16, 64, 256)

    def err():
        return lib.dvd_last_error().decode()

    def seed(frame=p, xy=p, depth=p, R=p, t=p, K=p, ts=p, N=2, points=p, t_out=p, ok=p, Q=4, H=4, W=4):
        return lib.dvd_point_seed(frame, xy, depth, R, t, K, ts, N, points, t_out, ok, Q, H, W, None)

    assert seed(frame=None) == E and 'null' in err()
    assert seed(ok=None) == E and 'null' in err()
    assert seed(ts=None) == E and 'both or none' in err()
    assert seed(t_out=None) == E and 'both or none' in err()
    for kw in (dict(Q=0), dict(Q=1 << 30), dict(N=0), dict(H=1), dict(W=1), dict(H=1 << 15, W=1 << 15)):
        assert seed(**kw) == E, kw

    def project(points=p, frame=p, xy=p, ok=p, k0=0, R=p, t=p, K=p, depth=p, N=2, z_tol=0.05, uv=p, z=p, d=p, inside=p, vis=p,
                target=p, T1=2, Q=4, H=4, W=4):
        return lib.dvd_point_project(points, frame, xy, ok, k0, R, t, K, depth, N, z_tol, uv, z, d, inside, vis, target, T1, Q,
                                     H, W, None)

    for name in ('points', 'frame', 'xy', 'R', 't', 'K', 'depth', 'uv', 'z', 'd', 'inside', 'vis', 'target'):
        assert project(**{name: None}) == E and 'null' in err(), name
    for kw in (dict(T1=0), dict(T1=65536), dict(Q=0), dict(Q=1 << 30), dict(N=0), dict(H=1), dict(k0=1 << 30), dict(k0=-(1 << 30)),
               dict(z_tol=-0.1), dict(z_tol=float('nan')), dict(z_tol=float('inf'))):
        assert project(**kw) == E, kw

    def score(uv=p, vis=p, target=p, origin=0, gt_uv=p, gt_state=p, N=2, sx=1.0, sy=1.0, thr2=thr, shift=20, sums=p, T1=2, Q=4):
        return lib.dvd_point_score(uv, vis, target, origin, gt_uv, gt_state, N, sx, sy, thr2, shift, sums, T1, Q, None)

    for name in ('uv', 'vis', 'target', 'gt_uv', 'gt_state', 'thr2', 'sums'):
        assert score(**{name: None}) == E and 'null' in err(), name
    for kw in (dict(T1=0), dict(Q=0), dict(N=0), dict(origin=2), dict(origin=-2), dict(sx=0.0), dict(sy=float('inf')),
               dict(sx=float('nan')), dict(shift=0), dict(shift=33), dict(Q=1 << 29, shift=24),
               dict(thr2=(ctypes.c_float * 5)(1, 4, 4, 64, 256)), dict(thr2=(ctypes.c_float * 5)(0, 4, 16, 64, 256)),
               dict(thr2=(ctypes.c_float * 5)(1, 4, 16, 64, float('inf')))):
        assert score(**kw) == E, kw
    assert score(Q=1 << 29, shift=24) == E and 'shift' in err()


def test_constructed_project_cases_are_clear_of_every_decision():
    fx = helpers.load_golden(FX)
    tabs, N, H, W = _tabs(fx), int(fx['N']), int(fx['H']), int(fx['W'])
    depth = PS.smooth_depth(N, H, W, 3)
    assert depth.min() > 1.5 and depth.max() < 2.5
    kinds = np.zeros(4, int)
    for T1, Q, k0, seed in ((1, 5, 0, 0), (13, 257, -6, 1), (13, 5, 0, 2)):
        pts, frame, xy = PS.constructed_project_case(tabs, depth, T1, Q, k0, seed)
        spec = PS.project(pts, frame, xy, k0, tabs['R'], tabs['t'], tabs['K_T'], depth)
        edge, absz, occ = PS.decision_margins(spec, depth, 0.05)
        # 1e-2 px, |z| >= 0.05 and 0.08 d by construction; the fp32 rounding of the stored points costs ~1e-6 of that
        assert float(edge.min()) >= 9e-3 and float(absz.min()) >= 4e-2 and float(occ.min()) >= 5e-2, (T1, Q, k0)
        live = spec['target'] >= 0
        kinds += [int((live & spec['visible']).sum()), int((live & spec['inside'] & ~spec['visible']).sum()),
                  int((live & ~spec['inside'] & (spec['z'] > 0)).sum()), int((live & (spec['z'] <= 0)).sum())]
        assert bool((~live).any()) == (T1 > 1)
    assert all(kinds > 20), kinds      # seen, occluded, outside, behind


def test_seeded_model_queries_leave_out_at_most_half_a_percent_under_the_spec():
    from dvd_hip.networks.sceneflow_field import SceneFlowFieldNet
    fx = helpers.load_golden(FX)
    N, H, W = int(fx['N']), int(fx['H']), int(fx['W'])
    net = SceneFlowFieldNet(net_width=256, n_layers=4, time_dependent=True, N_freq_xyz=16, N_freq_t=16)
    helpers.seeded_fill_(net, int(fx['seed']))
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    queries = PS.model_queries(N, H, W, 257)
    pipe = PS.pipeline(sd, _tabs(fx), fx['in_depth'], queries, 4)
    skip, frac = PS.flag_skip(pipe, fx['in_depth'], 0.05)
    live = pipe['target'] >= 0
    print('model queries: %d live rows, %d left out (%.3f %%)' % (int(live.sum()), int(skip.sum()), 100 * frac))
    assert frac <= 0.005
    assert bool(pipe['ok'].all()) and int(live.sum()) > 600 and bool((~live).any())
    assert bool(pipe['visible'][live].any()) and bool((~pipe['inside'][live]).any())
