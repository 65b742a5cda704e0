"""Two-sided tracks on the GPU: Model.track(n_back=..) (dvd_hip/models/tracks.py, csrc/invert.hip).

The store is the one of tests/test_45_tracks_gpu.py -- the 7 frames at 11 x 21 of tests/golden/tracks_b3_11x21_t4.npz with its
seeded model -- with start frames [1, 3, 6], n_back = 3 and n_steps = 2: frame 1 has one frame before it, frame 6 none after it.

Exact: n_back = 0 is the old call, the rows from the origin on are track(n_steps=2), every backward row is a hand-written loop
of SceneFlowMLPKernels.forward and ops.invert_update, any `chunk` gives the same bits, rows before frame 0 and past the last
frame are zero and so is `resid` where there is no frame, steps_valid_back; `inside` under tracks_spec.compare_inside.

Tolerances: the rule of tests/test_45_tracks_gpu.py.  Each distance from the float64 specification
(tests/invert_spec.py) must stay below 4 x the distance of the specification's own fp32 form from it, and below 4 x the value
measured on the MI355X (MEASURED).  `cycle` pushes every backward row forwards again with the ordinary forward chain and
compares where it lands, minus the origin row, with the same quantity of the specification (there: the iteration's remainder).
                        points - points[origin]   uv        z         depth_at   resid     cycle
    kernels, measured   5.9e-7                    4.3e-6    1.1e-6    1.1e-5     4.5e-7    4.8e-7
    time-independent    6.7e-7                    5.1e-6    1.1e-6    1.3e-5     4.4e-7    4.8e-7
    fp32 form           5.9e-7                    4.1e-6    1.0e-6    1.2e-5     4.5e-7    4.8e-7     (its limit is 4 x this)
    fp32 form, t-indep. 6.7e-7                    3.6e-6    1.2e-6    9.8e-6     4.4e-7    4.8e-7
`resid` and `cycle` are at the floor of the number format: in float64 the last round moves a point by at most 6.6e-8 (1.96e-7
for the time-independent field) and the cycle returns to 7.5e-9 (2.4e-8); in fp32 both are whole ulps of the points, 2.4e-7 or
4.8e-7 for |p| <= 6.3.  The bounds are 4 x the entries of MEASURED below.
"""
from types import SimpleNamespace
import warnings

import numpy as np
import pytest
import torch

import helpers
import invert_spec as I
import store_spec
import tracks_spec as S

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FX = 'tracks_b3_11x21_t4'
START, N_BACK, N_STEPS = [1, 3, 6], 3, 2
QUANTITIES = ('points', 'uv', 'z', 'depth_at', 'resid', 'cycle')
# worst distance from the float64 specification measured on the MI355X; the bound is 4 x this
MEASURED = {
    'points': 5.91e-7, 'uv': 4.30e-6, 'z': 1.09e-6, 'depth_at': 1.12e-5, 'resid': 4.47e-7, 'cycle': 4.77e-7,
    'notime/points': 6.72e-7, 'notime/uv': 5.07e-6, 'notime/z': 1.11e-6, 'notime/depth_at': 1.27e-5, 'notime/resid': 4.38e-7,
    'notime/cycle': 4.77e-7,
}


def _check(name, measured, ref_limit):
    bound = 4.0 * MEASURED[name]
    helpers.log_measured('track_back/' + name, measured, bound)
    print('measured track_back/%s %.4g (bound %.4g, reference limit %.4g)' % (name, measured, bound, ref_limit))
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


class _Ctx(object):
    pass


@pytest.fixture(scope='module')
def ctx(tmp_path_factory):
    """The fixture, its store, the model, ONE two-sided track run and ONE one-sided: computed once, shared, never written to."""
    from dvd_hip.datasets.frame_store import Catalogue, FrameStore
    c = _Ctx()
    fx = c.fx = helpers.load_golden(FX)
    c.N, c.H, c.W = int(fx['N']), int(fx['H']), int(fx['W'])
    tree = store_spec.random_tree(c.N, c.H, c.W, [1], 5)
    tree['fr_pose_c2w'], tree['fr_intrinsics'] = fx['in_pose_c2w'], fx['in_intrinsics']
    root = str(tmp_path_factory.mktemp('track_back'))
    store_spec.write_tree(root, tree)
    c.store = FrameStore(Catalogue(root, store_spec.TRACK, [1]), DEV)
    c.model = _model(int(fx['seed']))
    c.depth = helpers.t(fx['in_depth'], DEV)
    c.out = c.model.track(c.store, START, N_STEPS, depth=c.depth, n_back=N_BACK)
    c.fwd = c.model.track(c.store, START, N_STEPS, depth=c.depth)
    torch.cuda.synchronize()
    return c


def _spec(fx, net, time_dependent, dtype):
    """The two-sided pipeline of the specification in `dtype` from the fixture's inputs, as float64 copies."""
    N, H, W, B = int(fx['N']), int(fx['H']), int(fx['W']), len(START)
    ts = torch.from_numpy(fx['tab_ts_vali'])[START].view(B, 1, 1, 1).expand(B, 1, H, W) if time_dependent else None
    p0 = S.unproject(fx['in_depth'][START], fx['tab_R_T'][START], fx['tab_t'][START], fx['tab_K_inv_T'][START])
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    pts, resid = I.chain(sd, p0, ts, 1.0 / N, START, N, N_BACK, N_STEPS, 100.0, dtype=dtype)
    pipe = I.project(pts, START, fx['tab_R'], fx['tab_t'], fx['tab_K_T'], fx['in_depth'], k0=-N_BACK, dtype=dtype)
    pipe['points'], pipe['resid'] = pts.double(), resid.double()
    # the cycle: every live backward row pushed forwards again to the origin, minus the origin row
    cyc = torch.zeros(N_BACK, B, 3, H, W, dtype=torch.float64)
    for b, s in enumerate(START):
        for j in range(1, min(N_BACK, s) + 1):
            p = pts[N_BACK - j, b:b + 1]
            for i in range(j):
                p = I.forward_step(sd, p, None if ts is None else ts[b:b + 1].to(dtype) + (i - j) * (1.0 / N), 100.0, dtype)
            cyc[j - 1, b] = p[0].double() - pts[N_BACK, b].double()
    pipe['cycle'] = cyc
    return pipe


def _cycle(model, store, out, time_dependent):
    """The kernels' cycle: row origin - j of image b, j forward steps of the MLP kernels, minus the origin row."""
    from dvd_hip import ops
    net = model.net_sceneflow
    kern = ops.SceneFlowMLPKernels(DEV, n_freq_xyz=16, n_freq_t=16, time_dependent=time_dependent)      # a handle of the test's own
    kern.pack(net.parameter_list()[0::2], net.parameter_list()[1::2])
    N, H, W, B = store.cat.n_frames, store.H, store.W, len(START)
    ts = store.tables['ts_vali'][START].view(B, 1, 1, 1).expand(B, 1, H, W).contiguous() if time_dependent else None
    pts = out['points']
    cyc = torch.zeros(N_BACK, B, 3, H, W, dtype=torch.float64)
    for b, s in enumerate(START):
        for j in range(1, min(N_BACK, s) + 1):
            p = pts[N_BACK - j, b:b + 1].clone()
            for i in range(j):
                nxt = torch.empty_like(p)
                kern.forward(p, None if ts is None else ts[b:b + 1], t_offset=(i - j) * (1.0 / N), out_scale=1.0 / 100.0, p_next=nxt)
                p = nxt
            cyc[j - 1, b] = (p[0].double() - pts[N_BACK, b].double()).cpu()
    return cyc


def _distances(got, pipe):
    """Worst distance of points - points[origin], uv, z, depth_at (in front of the camera), resid and cycle from the float64
    specification, over the rows that have a frame."""
    T1, B, H, W = pipe['z'].shape
    live = pipe['live'][:, :, None, None].expand(T1, B, H, W)
    pts, ref = torch.as_tensor(got['points']).double(), pipe['points']
    return {'points': S.worst(pts - pts[N_BACK], ref - ref[N_BACK], live[:, :, None].expand(T1, B, 3, H, W)),
            'uv': S.worst(got['uv'], pipe['uv'], live[..., None].expand(T1, B, H, W, 2)),
            'z': S.worst(got['z'], pipe['z'], live),
            'depth_at': S.worst(got['depth_at'], pipe['depth_at'], live & (pipe['z'] > 0)),
            'resid': S.worst(got['resid'], pipe['resid']),
            'cycle': S.worst(got['cycle'], pipe['cycle'])}


def _own_row_first(x):
    order = [N_BACK] + [j for j in range(N_BACK + 1 + N_STEPS) if j != N_BACK]
    return torch.as_tensor(x)[order]


def _against_the_specification(prefix, model, store, out, fx, time_dependent):
    got = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in out.items()}
    got['cycle'] = _cycle(model, store, out, time_dependent)
    p64 = _spec(fx, model.net_sceneflow, time_dependent, torch.float64)
    p32 = _spec(fx, model.net_sceneflow, time_dependent, torch.float32)
    d_kernel, d_ref = _distances(got, p64), _distances(p32, p64)
    assert float(p64['cycle'].abs().max()) < 1e-7                      # the specification itself returns
    for q in QUANTITIES:
        print('track_back/%s%s: fp32 form vs float64 %.4g' % (prefix, q, d_ref[q]))
    failed = []
    for q in QUANTITIES:
        try:
            _check(prefix + q, d_kernel[q], 4 * d_ref[q])
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, failed
    # `inside` under compare_inside, the frames' own row (the origin) first
    H, W = store.H, store.W
    spec = {k: _own_row_first(p64[k]) for k in ('uv', 'z', 'inside', 'live')}
    bad, frac = S.compare_inside(_own_row_first(got['inside']), spec, H, W, self_rows=1)
    print('inside: %d mismatches, %.3f %% of the points of the other rows left out' % (bad, 100 * frac))
    assert frac <= 0.005 and bad == 0
    assert bool(got['inside'][N_BACK][:, ~S.border_pixels(H, W)].all())
    return p64


def test_n_back_zero_is_the_old_call_and_the_forward_rows_are_the_old_rows(ctx):
    zero = ctx.model.track(ctx.store, START, N_STEPS, depth=ctx.depth, n_back=0, n_iter=1)
    assert set(zero) == set(ctx.fwd) == {'points', 'uv', 'z', 'depth_at', 'inside', 'steps_valid'}
    for k, v in ctx.fwd.items():
        assert torch.equal(zero[k], v), k
    out = ctx.out
    assert set(out) == set(ctx.fwd) | {'origin', 'steps_valid_back', 'resid'}
    B, T1 = len(START), N_BACK + 1 + N_STEPS
    assert out['origin'] == N_BACK and out['points'].shape == (T1, B, 3, ctx.H, ctx.W) and out['uv'].shape == (T1, B, ctx.H, ctx.W, 2)
    assert out['resid'].shape == (N_BACK, B) and out['resid'].dtype == torch.float32 and out['resid'].is_cuda
    for k in ('points', 'uv', 'z', 'depth_at', 'inside'):
        assert torch.equal(out[k][N_BACK:], ctx.fwd[k]), k
    assert torch.equal(out['steps_valid'], ctx.fwd['steps_valid']) and out['steps_valid'].tolist() == [2, 2, 0]
    assert out['steps_valid_back'].is_cuda and out['steps_valid_back'].dtype == torch.int32
    assert out['steps_valid_back'].tolist() == [1, 3, 3]


def test_backward_rows_are_the_hand_written_loop(ctx):
    from dvd_hip import ops
    out, T = ctx.out, ctx.store.tables
    N, H, W, B = ctx.N, ctx.H, ctx.W, len(START)
    net = ctx.model.net_sceneflow
    kern = ops.SceneFlowMLPKernels(DEV, n_freq_xyz=16, n_freq_t=16, time_dependent=True)      # a handle of the test's own
    kern.pack(net.parameter_list()[0::2], net.parameter_list()[1::2])
    ts = T['ts_vali'][START].view(B, 1, 1, 1).expand(B, 1, H, W).contiguous()
    p0 = ops.unproject(ctx.depth[START], T['R_T'][START], T['t'][START], T['K_inv_T'][START], planar=True)
    assert torch.equal(out['points'][N_BACK], p0)
    for b, s in enumerate(START):                                 # one image at a time, a buffer per round
        p = p0[b:b + 1].clone()
        for j in range(1, N_BACK + 1):
            if s - j < 0:
                assert not bool(out['points'][N_BACK - j, b].any()) and out['resid'][j - 1, b].item() == 0.0
                continue
            y, sf = p, torch.empty_like(p)
            for i in range(4):
                kern.forward(y, ts[b:b + 1], t_offset=-j * (1.0 / N), out_scale=1.0 / 100.0, sf_out=sf)
                r = torch.zeros(1, device=DEV)
                y = ops.invert_update(p, sf, y, resid=r)
            assert torch.equal(out['points'][N_BACK - j, b], y[0]), (b, j)
            assert out['resid'][j - 1, b].item() == r.item(), (b, j, r.item())
            p = y
    # n_iter is the number of rounds: one round gives other bits and a residual of the size of a step
    one = ctx.model.track(ctx.store, START, 0, depth=ctx.depth, n_back=1, n_iter=1)
    assert one['points'].shape[0] == 2 and not torch.equal(one['points'][0], out['points'][N_BACK - 1])
    assert float(one['resid'].max()) > 1e-4 and one['steps_valid'].tolist() == [0, 0, 0]


def test_every_chunk_gives_the_same_bits(ctx):
    for chunk in (1, 3):
        other = ctx.model.track(ctx.store, START, N_STEPS, depth=ctx.depth, chunk=chunk, n_back=N_BACK)
        assert set(other) == set(ctx.out)
        for k, v in ctx.out.items():
            assert torch.equal(other[k], v) if torch.is_tensor(v) else other[k] == v, (chunk, k)
    for kw in (dict(n_back=-1), dict(n_back=1.5), dict(n_back=True), dict(n_back=1, n_iter=0), dict(n_back=1, n_iter=2.0)):
        with pytest.raises(ValueError, match='n_back|n_iter'):
            ctx.model.track(ctx.store, START, N_STEPS, depth=ctx.depth, **kw)
    with pytest.raises(ValueError, match='track_plan'):
        ctx.model.track(ctx.store, START, 0, depth=ctx.depth)          # no forward rows only with backward rows
    with pytest.raises(ValueError, match='track_plan_back'):
        ctx.model.track(ctx.store, [0, 7], N_STEPS, depth=ctx.depth, n_back=1)


def test_rows_outside_the_video_are_zero(ctx):
    got = {k: v.cpu() for k, v in ctx.out.items() if torch.is_tensor(v)}
    live = torch.tensor([[0 <= s + j - N_BACK < ctx.N for s in START] for j in range(N_BACK + 1 + N_STEPS)])
    assert int((~live).sum()) == 4 and not bool(live[0, 0]) and not bool(live[1, 0]) and not bool(live[5, 2])
    for k in ('points', 'uv', 'z', 'depth_at', 'inside'):
        assert not bool(got[k][~live].any()), k
        if k in ('points', 'uv', 'z'):              # (a whole image may be behind a camera: no depth_at, not inside)
            assert bool(got[k][live].flatten(1).any(1).all()), k
    has_step = torch.tensor([[s - j >= 0 for s in START] for j in range(1, N_BACK + 1)])
    assert not bool(got['resid'][~has_step].any()) and bool((got['resid'][has_step] > 0).all())
    # four rounds end below one fp32 ulp of these points in float64 (tests/test_invert_cpu.py); in fp32 the last move is the
    # rounding of two iterates of |p| <= 6.3 (half an ulp, 2.4e-7, each) and of the field's output: 1e-5 leaves a factor of 10
    assert float(got['resid'].max()) < 1e-5


def test_outputs_against_the_float64_specification(ctx):
    _against_the_specification('', ctx.model, ctx.store, ctx.out, ctx.fx, True)


def test_time_independent_field_against_the_float64_specification(ctx):
    model = _model(int(ctx.fx['seed']) + 1, time_dependent=False)
    out = model.track(ctx.store, START, N_STEPS, depth=ctx.depth, chunk=2, n_back=N_BACK)
    assert not torch.equal(out['points'][N_BACK - 1], ctx.out['points'][N_BACK - 1])
    p64 = _against_the_specification('notime/', model, ctx.store, out, ctx.fx, False)
    assert out['steps_valid_back'].tolist() == [1, 3, 3] and not bool(out['points'].cpu()[~p64['live']].any())


def test_use_cnn_is_refused_with_a_message(ctx):
    model = _model(3, use_cnn=True)
    with pytest.raises(NotImplementedError, match='use_cnn'):
        model.track(ctx.store, START, N_STEPS, depth=ctx.depth, n_back=N_BACK)
