"""Model.track / Model.video_depth on the GPU (dvd_hip/models/tracks.py).

The fixture tests/golden/tracks_b3_11x21_t4.npz holds what the real reference computes for a 7-frame video at 11 x 21, start
frames [0, 3, 5] and 4 steps (tests/golden/make_golden_tracks.py); a FrameStore is built from the fixture's own poses and
intrinsics, so its tables are the fixture's bit for bit.

Exact: step 0 is ops.unproject, every later step the stash-free MLP forward (a hand-written loop over
SceneFlowMLPKernels.forward), any `chunk` gives the same bits, rows past the end of the video are zero, steps_valid, depth_at
and inside behind the camera, video_depth against _predict_on_batch(False), `inside` under the rule of tests/tracks_spec.py
(compare_inside: step 0 projects a frame onto itself, so its border pixels sit ON an image edge and are left out by name; of
the other steps at most 0.5 % of the points may be left out).

Tolerances: the worst distance of the whole pipeline from its float64 specification (tracks_spec:
unproject, integrate, project), measured on the MI355X, x 4; the measured value must stay below 4 x the distance of the
reference's own fp32 results (the fixture) from that specification.  Against the fixture itself the bound grows by the
fixture's distance.
                        points - points[0]   uv        z         depth_at
    kernels, measured   6.3e-7               4.0e-6    1.3e-6    1.1e-5
    time-independent    6.8e-7               4.0e-6    1.1e-6    9.6e-6
    reference (fp32)    6.2e-7               4.0e-6    1.1e-6    1.1e-5     (its limit is 4 x this)
    kernels vs fixture  4.8e-7               3.8e-6    9.5e-7    8.5e-6
The bounds are 4 x the entries of MEASURED below.
"""
from types import SimpleNamespace
import warnings

import numpy as np
import pytest
import torch

import helpers
import store_spec
import tracks_spec as S

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FX = 'tracks_b3_11x21_t4'
QUANTITIES = ('points', 'uv', 'z', 'depth_at')
# worst distance from the float64 pipeline measured on the MI355X; the bound is 4 x this
MEASURED = {
    'points': 6.35e-7, 'uv': 3.97e-6, 'z': 1.32e-6, 'depth_at': 1.12e-5,
    'notime/points': 6.80e-7, 'notime/uv': 4.00e-6, 'notime/z': 1.07e-6, 'notime/depth_at': 9.59e-6,
}


def _bound(name):
    return 4.0 * MEASURED[name]


def _check(name, measured, ref_limit):
    bound = _bound(name)
    helpers.log_measured('tracks/' + name, measured, bound)
    print('measured tracks/%s %.4g (bound %.4g, reference limit %.4g)' % (name, measured, bound, ref_limit))
    assert measured <= ref_limit, (name, measured, ref_limit)
    assert measured <= bound, (name, measured, bound)


def _model(seed, **over):
    from dvd_hip.models.scene_flow_motion_field import Model
    o = dict(helpers.FULL_STEP_OPT)
    o.update(midas=False, full_logdir='/tmp')
    o.update(over)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = Model(SimpleNamespace(**o), None)
    helpers.seeded_fill_(m.net_depth, seed + 7)
    helpers.seeded_fill_(m.net_sceneflow, seed)
    m.to(torch.device(DEV))
    return m


def _store(root, fx_tree):
    from dvd_hip.datasets.frame_store import Catalogue, FrameStore
    store_spec.write_tree(root, fx_tree)
    return FrameStore(Catalogue(root, store_spec.TRACK, [1]), DEV)


class _Ctx(object):
    pass


@pytest.fixture(scope='module')
def ctx(tmp_path_factory):
    """The fixture, a store with its cameras, the model with its network, ONE track run and the float64 pipeline: computed
    once, shared by the tests below, never written to."""
    c = _Ctx()
    fx = c.fx = helpers.load_golden(FX)
    N, H, W = int(fx['N']), int(fx['H']), int(fx['W'])
    tree = store_spec.random_tree(N, H, W, [1], 5)
    tree['fr_pose_c2w'], tree['fr_intrinsics'] = fx['in_pose_c2w'], fx['in_intrinsics']
    c.store = _store(str(tmp_path_factory.mktemp('tracks')), tree)
    for k in ('R_T', 'R', 't', 'K_T', 'K_inv_T', 'ts_vali'):           # the store's tables ARE the fixture's
        assert torch.equal(c.store.tables[k].cpu(), torch.from_numpy(fx['tab_' + k])), k
    c.model = _model(int(fx['seed']))
    c.start, c.n_steps = fx['start'].tolist(), int(fx['n_steps'])
    c.depth = helpers.t(fx['in_depth'], DEV)
    c.out = c.model.track(c.store, c.start, c.n_steps, depth=c.depth)
    torch.cuda.synchronize()
    c.pipe = _pipeline(c.model.net_sceneflow, fx, time_dependent=True)
    return c


def _pipeline(net, fx, time_dependent):
    """The whole pipeline in float64 from the fixture's inputs."""
    start, N = fx['start'].tolist(), int(fx['N'])
    B, H, W = len(start), int(fx['H']), int(fx['W'])
    ts = torch.from_numpy(fx['tab_ts_vali'])[start].view(B, 1, 1, 1).expand(B, 1, H, W) if time_dependent else None
    p0 = S.unproject(fx['in_depth'][start], fx['tab_R_T'][start], fx['tab_t'][start], fx['tab_K_inv_T'][start])
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    pts = S.integrate(sd, p0, ts, 1.0 / N, fx['steps_valid'].tolist(), int(fx['n_steps']), 1.0 / 100.0)
    pipe = S.project(pts, start, fx['tab_R'], fx['tab_t'], fx['tab_K_T'], fx['in_depth'])
    pipe['points'] = pts
    return pipe


def _distances(got, pipe):
    """Worst distance of points - points[0], uv, z and depth_at (in front of the camera) from the float64 pipeline."""
    T1, B, H, W = pipe['z'].shape
    live = pipe['live'][:, :, None, None].expand(T1, B, H, W)
    pts = torch.as_tensor(got['points']).double()
    return {'points': S.worst((pts - pts[0])[1:], (pipe['points'] - pipe['points'][0])[1:]),
            'uv': S.worst(got['uv'], pipe['uv'], live[..., None].expand(T1, B, H, W, 2)),
            'z': S.worst(got['z'], pipe['z'], live),
            'depth_at': S.worst(got['depth_at'], pipe['depth_at'], live & (pipe['z'] > 0))}


def _fixture_outputs(fx):
    T1, B, H, W = fx['ref_z'].shape
    xx, yy = S._pixel_grid(H, W)
    live = torch.tensor([[v >= k for v in fx['steps_valid'].tolist()] for k in range(T1)])
    uv = (torch.from_numpy(fx['ref_disp']).double() + torch.stack([xx, yy], -1)) * live[:, :, None, None, None]
    return {'points': fx['ref_points'], 'uv': uv, 'z': fx['ref_z'], 'depth_at': fx['ref_depth_at']}


def test_step_zero_is_unproject_and_the_chain_is_the_mlp_forward(ctx):
    from dvd_hip import ops
    out, T, start = ctx.out, ctx.store.tables, ctx.start
    N, H, W = ctx.store.cat.n_frames, ctx.store.H, ctx.store.W
    B, T1 = len(start), ctx.n_steps + 1
    assert out['points'].shape == (T1, B, 3, H, W) and out['uv'].shape == (T1, B, H, W, 2)
    assert out['steps_valid'].is_cuda and out['steps_valid'].tolist() == [4, 3, 1]
    p0 = ops.unproject(ctx.depth[start], T['R_T'][start], T['t'][start], T['K_inv_T'][start], planar=True)
    assert torch.equal(out['points'][0], p0)
    net = ctx.model.net_sceneflow
    kern = ops.SceneFlowMLPKernels(DEV, n_freq_xyz=16, n_freq_t=16, time_dependent=True)      # a handle of the test's own
    kern.pack(net.parameter_list()[0::2], net.parameter_list()[1::2])
    ts = T['ts_vali'][start].view(B, 1, 1, 1).expand(B, 1, H, W).contiguous()
    valid = [4, 3, 1]
    for b in range(B):                                        # one image at a time, a buffer per step
        p = p0[b:b + 1].clone()
        for k in range(ctx.n_steps):
            if valid[b] <= k:
                assert not bool(out['points'][k + 1, b].any())
                continue
            nxt = torch.empty_like(p)
            kern.forward(p, ts[b:b + 1], t_offset=k * (1.0 / N), out_scale=1.0 / 100.0, p_next=nxt)
            assert torch.equal(out['points'][k + 1, b], nxt[0]), (b, k)
            p = nxt


def test_every_chunk_gives_the_same_bits(ctx):
    for chunk in (1, 3):
        other = ctx.model.track(ctx.store, ctx.start, ctx.n_steps, depth=ctx.depth, chunk=chunk)
        assert set(other) == set(ctx.out) == {'points', 'uv', 'z', 'depth_at', 'inside', 'steps_valid'}
        for k, v in ctx.out.items():
            assert torch.equal(other[k], v), (chunk, k)
    with pytest.raises(ValueError, match='chunk'):
        ctx.model.track(ctx.store, ctx.start, ctx.n_steps, depth=ctx.depth, chunk=0)
    with pytest.raises(ValueError, match='track_plan'):
        ctx.model.track(ctx.store, [0, 7], ctx.n_steps, depth=ctx.depth)
    with pytest.raises(ValueError, match='depth'):
        ctx.model.track(ctx.store, ctx.start, ctx.n_steps, depth=ctx.depth[:3])


def test_the_end_of_the_video_and_the_back_of_the_camera(ctx):
    got = {k: v.cpu() for k, v in ctx.out.items()}
    live = ctx.pipe['live']
    assert live.tolist() == [[v >= k for v in (4, 3, 1)] for k in range(5)]
    for k in ('points', 'uv', 'z', 'depth_at', 'inside'):
        assert not bool(got[k][~live].any()), k
    behind = (got['z'] <= 0) & live[:, :, None, None]
    assert bool(behind.any()) and bool(((ctx.pipe['z'] <= 0) == (got['z'] <= 0)).all())
    assert not bool(got['depth_at'][behind].any()) and not bool(got['inside'][behind].any())
    assert bool((got['depth_at'][~behind & live[:, :, None, None]] > 0).all())
    T1, B, H, W = got['z'].shape
    bad, frac = S.compare_inside(got['inside'], ctx.pipe, H, W, self_rows=1)
    print('inside: %d mismatches, %.3f %% of the points of steps 1.. left out' % (bad, 100 * frac))
    assert frac <= 0.005 and bad == 0
    # step 0: every pixel is in front of its own camera, and every pixel that is not on the border is inside its own image
    inner = ~S.border_pixels(H, W)
    assert bool(got['inside'][0][:, inner].all())


def test_outputs_against_the_float64_pipeline_and_the_fixture(ctx):
    got = {k: v.cpu() for k, v in ctx.out.items()}
    ref = _fixture_outputs(ctx.fx)
    d_kernel, d_ref = _distances(got, ctx.pipe), _distances(ref, ctx.pipe)
    T1, B, H, W = ctx.pipe['z'].shape
    live = ctx.pipe['live'][:, :, None, None].expand(T1, B, H, W)
    front = live & (ctx.pipe['z'] > 0)
    pts, rpts = got['points'].double(), torch.from_numpy(ref['points']).double()
    d_fix = {'points': S.worst((pts - pts[0])[1:], (rpts - rpts[0])[1:]),
             'uv': S.worst(got['uv'], ref['uv'], live[..., None].expand(T1, B, H, W, 2)),
             'z': S.worst(got['z'], ref['z'], live), 'depth_at': S.worst(got['depth_at'], ref['depth_at'], front)}
    assert abs(d_ref['points'] - float(ctx.fx['ref_vs_f64_points'])) <= 1e-9      # the same quantity the generator stored
    for q in QUANTITIES:
        print('tracks/%s: reference vs float64 %.4g, kernels vs the fixture %.4g' % (q, d_ref[q], d_fix[q]))
        _check(q, d_kernel[q], 4 * d_ref[q])
        assert d_fix[q] <= _bound(q) + d_ref[q], (q, d_fix[q])


def test_time_independent_network_against_the_float64_pipeline(ctx):
    """No fixture for this one: the specification alone, with the time-dependent fixture's reference distances as the yardstick
    of what fp32 can do on these inputs."""
    model = _model(int(ctx.fx['seed']) + 1, time_dependent=False)
    out = model.track(ctx.store, ctx.start, ctx.n_steps, depth=ctx.depth, chunk=2)
    got = {k: v.cpu() for k, v in out.items()}
    pipe = _pipeline(model.net_sceneflow, ctx.fx, time_dependent=False)
    assert not torch.equal(out['points'][1], ctx.out['points'][1])
    d_ref = _distances(_fixture_outputs(ctx.fx), ctx.pipe)
    for q, d in _distances(got, pipe).items():
        _check('notime/' + q, d, 4 * d_ref[q])
    T1, B, H, W = pipe['z'].shape
    bad, frac = S.compare_inside(got['inside'], pipe, H, W, self_rows=1)
    assert frac <= 0.005 and bad == 0
    assert out['steps_valid'].tolist() == [4, 3, 1] and not bool(got['points'][~pipe['live']].any())


def test_use_cnn_is_refused_with_a_message(ctx):
    model = _model(3, use_cnn=True)
    with pytest.raises(NotImplementedError, match='use_cnn'):
        model.track(ctx.store, ctx.start, ctx.n_steps, depth=ctx.depth)


def test_model_level_video_depth_and_track_hourglass(tmp_path):
    """The hourglass depth net at 32 x 48, 5 frames, 2 steps: video_depth is _predict_on_batch(False)['depth'] frame by frame,
    and track with its default depth is track on that depth."""
    from dvd_hip import ops
    N, H, W = 5, 32, 48
    store = _store(str(tmp_path), store_spec.random_tree(N, H, W, [1], 11))
    model = _model(21)
    depth = model.video_depth(store.frames(2))
    assert depth.shape == (N, 1, H, W) and depth.is_cuda and bool(torch.isfinite(depth).all())
    at = 0
    for batch in store.frames(2):
        model.eval()
        model.load_batch(batch)
        with torch.no_grad():
            want = model._predict_on_batch(is_train=False)['depth']
        assert torch.equal(depth[at:at + want.shape[0]], want), at
        at += want.shape[0]
    assert at == N
    whole = model.video_depth(store.frames(model._chunk()))
    out = model.track(store, [0, 2, 4], 2)
    same = model.track(store, [0, 2, 4], 2, depth=whole, chunk=1)
    for k, v in out.items():
        assert torch.equal(same[k], v), k
    assert out['steps_valid'].tolist() == [2, 2, 0]
    T = store.tables
    assert torch.equal(out['points'][0], ops.unproject(whole[[0, 2, 4]], T['R_T'][[0, 2, 4]], T['t'][[0, 2, 4]],
                                                         T['K_inv_T'][[0, 2, 4]], planar=True))
    proj = ops.track_project(out['points'], [0, 2, 4], T, depth_all=whole)
    for k in proj:
        assert torch.equal(proj[k], out[k]), k
    assert not bool(out['points'][1:, 2].any()) and bool(out['inside'][0].any())
