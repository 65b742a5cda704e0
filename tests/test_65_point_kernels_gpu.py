"""The three query-point kernels on the GPU (csrc/point_track.hip): ops.point_seed, ops.point_project, ops.point_score.

Cameras, time stamps and depth are those of the fixture tests/golden/tracks_b3_11x21_t4.npz (7 frames at 11 x 21).  Shapes: Q in
{1, 5, 257, 1000} (one thread, a part of a wave, more than one block, several blocks with a ragged last one), T1 in {1, 13}, k0
in {0, -6} (with 7 frames, 13 rows from -6 on leave the video on both sides).

Exact: the seed at integer pixels against ops.unproject, bit for bit; the projection of integer queries against
ops.track_project gathered at those pixels, bit for bit; `visible` recomputed from those bits; `target`; every flag of the
constructed sub-pixel cases (tests/point_tracks_spec.py keeps each clear of every decision by construction, so NO case is left
out); all 19 words of the score against the float32 mirror.

Tolerances: the worst distance from the float64 specification measured on the MI355X, x 4 -- the margin
tests/test_45_tracks_gpu.py uses for this chain; the measured value must also stay below 4 x the distance of the same formula
evaluated in fp32 torch (grid_sample + matmuls) from the specification.  Both distances are taken over all Q of a test: a
launch of one point has no worst case of its own to compare with.
                        seed points   uv        z         depth_at
    kernels, measured   1.0e-6        4.9e-6    6.4e-7    3.6e-7
    reference (fp32)    4.2e-6        4.9e-6    6.4e-7    3.8e-7      (its limit is 4 x this)
(the seed's direct taps are closer to float64 than grid_sample's normalise / de-normalise chain.)  The score's square root is
the compiler's correctly rounded sqrtf and agrees with numpy's float32 sqrt on every term, so word 18 is compared exactly, like
the 18 counts.  (__fsqrt_rn is the 1-ulp native square root in this toolchain: with it word 18 was off by up to one quantum of
the fp32 result per term on the MI355X, the counts exact.)
"""
import numpy as np
import pytest
import torch

import helpers
import point_tracks_spec as PS
import tracks_spec as S

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FX = 'tracks_b3_11x21_t4'
QS = (1, 5, 257, 1000)
ROWS = ((1, 0), (13, 0), (13, -6), (1, -6))        # (T1, k0)
Z_TOL = 0.05
# worst distance from the float64 specification measured on the MI355X; the bound is 4 x this
MEASURED = {'seed/points': 1.03e-6, 'project/uv': 4.89e-6, 'project/z': 6.43e-7, 'project/depth_at': 3.59e-7}


def _check(name, measured, ref_limit):
    bound = 4.0 * MEASURED[name]
    helpers.log_measured('points/' + name, measured, bound)
    print('measured points/%s %.4g (bound %.4g, reference limit %.4g)' % (name, measured, bound, ref_limit))
    assert measured <= ref_limit, (name, measured, ref_limit)
    assert measured <= bound, (name, measured, bound)


class _Ctx(object):
    pass


@pytest.fixture(scope='module')
def ctx():
    c = _Ctx()
    fx = c.fx = helpers.load_golden(FX)
    c.N, c.H, c.W = int(fx['N']), int(fx['H']), int(fx['W'])
    c.host = {k: fx['tab_' + k] for k in ('R_T', 'R', 't', 'K_T', 'K_inv_T', 'ts_vali')}
    c.tabs = {k: helpers.t(v, DEV) for k, v in c.host.items()}
    c.depth = helpers.t(fx['in_depth'], DEV)
    return c


def _grid_queries(c, frames):
    yy, xx = np.meshgrid(np.arange(c.H), np.arange(c.W), indexing='ij')
    xy = np.tile(np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float32), (len(frames), 1))
    return np.repeat(np.asarray(frames, np.int32), c.H * c.W), xy


def test_seed_at_integer_pixels_is_unproject(ctx):
    from dvd_hip import ops
    c, frames = ctx, [0, 3, 5]
    frame, xy = _grid_queries(c, frames)
    out = ops.point_seed(frame, helpers.t(xy, DEV), c.depth, c.tabs)
    T = c.tabs
    want = ops.unproject(c.depth[frames], T['R_T'][frames], T['t'][frames], T['K_inv_T'][frames], planar=True)
    assert out['points'].shape == (3, len(frame)) and out['ok'].dtype == torch.uint8
    assert torch.equal(out['points'], want.permute(1, 0, 2, 3).reshape(3, -1))
    assert torch.equal(out['t'], T['ts_vali'][torch.from_numpy(frame).long().to(DEV)])
    assert bool((out['ok'] == 1).all())
    no_t = ops.point_seed(frame, helpers.t(xy, DEV), c.depth, c.tabs, time_stamps=False)
    assert set(no_t) == {'points', 'ok'} and torch.equal(no_t['points'], out['points'])
    # into a row of a slab, and the frames as a device tensor
    slab = torch.zeros(3, 3, len(frame), device=DEV)
    ok = torch.zeros(len(frame), device=DEV, dtype=torch.uint8)
    ops.point_seed(helpers.t(frame, DEV), helpers.t(xy, DEV), c.depth, c.tabs, out={'points': slab[1], 'ok': ok}, host_frame=frame)
    assert torch.equal(slab[1], out['points']) and not bool(slab[0].any()) and not bool(slab[2].any()) and bool(ok.all())


def test_seed_refuses_a_depth_that_is_no_depth_and_a_frame_that_is_no_frame(ctx):
    from dvd_hip import ops
    c = ctx
    depth = c.depth.clone()
    bad = {(7, 4): 0.0, (8, 5): -1.0, (12, 6): float('nan'), (1, 1): float('inf')}
    for (x, y), v in bad.items():
        depth[2, 0, y, x] = v
    xy = np.float32(list(bad) + [(15, 8), (15.5, 8.5)])
    out = ops.point_seed([2] * len(xy), helpers.t(xy, DEV), depth, c.tabs)
    assert out['ok'].tolist() == [0, 0, 0, 0, 1, 1]
    assert not bool(out['points'][:, :4].any()) and bool(out['points'][:, 4:].abs().sum(0).gt(0).all())
    assert torch.equal(out['t'], c.tabs['ts_vali'][2].expand(6))
    # a frame outside the video can only arrive in a device tensor (a host list is range-checked): not ok, zeros, t = 0
    frame = torch.tensor([-1, 3, 7, 1 << 30], dtype=torch.int32, device=DEV)
    out = ops.point_seed(frame, helpers.t(np.float32([[1, 1]] * 4), DEV), c.depth, c.tabs)
    assert out['ok'].tolist() == [0, 1, 0, 0] and not bool(out['points'][:, [0, 2, 3]].any())
    assert out['t'].tolist() == [0.0, float(c.tabs['ts_vali'][3]), 0.0, 0.0]
    with pytest.raises(RuntimeError, match='ids of frame'):
        ops.point_seed([0, 7], helpers.t(np.float32([[1, 1]] * 2), DEV), c.depth, c.tabs)
    with pytest.raises(RuntimeError, match='xy'):
        ops.point_seed([0], helpers.t(np.float32([[1, 1, 1]]), DEV), c.depth, c.tabs)


def test_seed_at_subpixel_positions_against_the_float64_spec(ctx):
    from dvd_hip import ops
    c, h = ctx, ctx.host
    worst, worst_ref = 0.0, 0.0
    for Q in QS:
        frame, xy = PS.subpixel_seed_queries(c.N, c.H, c.W, Q, 40 + Q)
        out = ops.point_seed(frame, helpers.t(xy, DEV), c.depth, c.tabs)
        spec, ok = PS.seed(frame, xy, c.fx['in_depth'], h['R_T'], h['t'], h['K_inv_T'])
        assert bool(ok.all()) and out['ok'].cpu().bool().tolist() == ok.tolist()
        worst = max(worst, S.worst(out['points'].cpu(), spec))
        worst_ref = max(worst_ref, S.worst(PS.seed_fp32(frame, xy, c.fx['in_depth'], h['R_T'], h['t'], h['K_inv_T']), spec))
    _check('seed/points', worst, 4 * worst_ref)


def _dense(ctx, T1, k0):
    """A dense slab [T1,3,3,H,W] of the start frames 0, 3, 5 -- their un-projected depth, moved a little more in every row --
    and ops.track_project of it."""
    from dvd_hip import ops
    c, T, start = ctx, ctx.tabs, [0, 3, 5]
    p0 = ops.unproject(c.depth[start], T['R_T'][start], T['t'][start], T['K_inv_T'][start], planar=True)
    gen = torch.Generator().manual_seed(9 + T1)
    slab = (p0[None] + 0.05 * torch.arange(T1, device=DEV).view(T1, 1, 1, 1, 1) *
            torch.randn(T1, 3, 3, c.H, c.W, generator=gen).to(DEV)).contiguous()
    return slab, start, ops.track_project(slab, start, T, depth_all=c.depth, k0=k0)


@pytest.mark.parametrize('T1,k0', ROWS)
def test_project_at_integer_queries_is_track_project(ctx, T1, k0):
    from dvd_hip import ops
    c = ctx
    slab, start, dense = _dense(c, T1, k0)
    tol = torch.tensor(1.0, device=DEV) + torch.tensor(Z_TOL, device=DEV)            # fp32 (1 + z_tol), formed once
    for Q in QS:
        rng = np.random.RandomState(100 * T1 + Q)
        b, y, x = rng.randint(0, 3, Q), rng.randint(0, c.H, Q), rng.randint(0, c.W, Q)
        frame = np.asarray(start, np.int32)[b]
        xy = helpers.t(np.stack([x, y], 1).astype(np.float32), DEV)
        bt, yt, xt = (torch.from_numpy(v).to(DEV) for v in (b, y, x))
        points = slab.permute(0, 2, 1, 3, 4)[:, :, bt, yt, xt].contiguous()         # [T1,3,Q]
        ok = None
        if Q == 257:
            ok = torch.ones(Q, dtype=torch.uint8, device=DEV)
            ok[::5] = 0
        out = ops.point_project(points, frame, xy, c.tabs, c.depth, k0=k0, z_tol=Z_TOL, ok=ok)
        keep = torch.ones(1, Q, dtype=torch.bool, device=DEV) if ok is None else ok.bool()[None]
        g = torch.from_numpy(frame.astype(np.int64)).to(DEV)[None, :] + torch.arange(T1, device=DEV)[:, None] + k0
        live = (g >= 0) & (g < c.N) & keep
        assert torch.equal(out['target'], torch.where(live, g, torch.full_like(g, -1)).int()), (Q, T1, k0)
        for k in ('uv', 'z', 'depth_at', 'inside'):
            want = dense[k][:, bt, yt, xt]
            want = want * (keep[..., None] if k == 'uv' else keep).to(want.dtype)
            assert torch.equal(out[k], want), (k, Q, T1, k0)
            assert not bool(out[k][~live].any()), (k, Q)
        vis = out['inside'].bool() & ~(out['z'] > out['depth_at'] * tol)
        assert torch.equal(out['visible'], vis.to(torch.uint8)), (Q, T1, k0)
        if T1 == 13 and Q >= 257:
            assert bool(out['visible'].any()) and bool((out['inside'].bool() & ~vis).any()) and bool((~live).any())


def test_project_at_constructed_subpixel_cases(ctx):
    from dvd_hip import ops
    c, h = ctx, ctx.host
    depth = PS.smooth_depth(c.N, c.H, c.W, 3)
    depth_d = helpers.t(depth, DEV)
    worst = {k: 0.0 for k in ('uv', 'z', 'depth_at')}
    worst_ref = dict(worst)
    n = 0
    for T1, k0 in ROWS:
        for Q in QS:
            pts, frame, xy = PS.constructed_project_case(h, depth, T1, Q, k0, 7 * T1 + Q - k0)
            out = {k: v.cpu() for k, v in ops.point_project(helpers.t(pts, DEV), frame, helpers.t(xy, DEV), c.tabs, depth_d, k0=k0,
                                                            z_tol=Z_TOL).items()}
            spec = PS.project(pts, frame, xy, k0, h['R'], h['t'], h['K_T'], depth, Z_TOL)
            ref = PS.project_fp32(pts, frame, xy, k0, h['R'], h['t'], h['K_T'], depth, Z_TOL)
            # no case is left out: every flag of every row
            assert torch.equal(out['target'].long(), spec['target']), (T1, Q, k0)
            assert torch.equal(out['inside'].bool(), spec['inside']), (T1, Q, k0)
            assert torch.equal(out['visible'].bool(), spec['visible']), (T1, Q, k0)
            live = spec['target'] >= 0
            n += int(live.sum())
            masks = {'uv': live[..., None].expand(T1, Q, 2), 'z': live, 'depth_at': live & (spec['z'] > 0)}
            for k in worst:
                worst[k] = max(worst[k], S.worst(out[k], spec[k], masks[k]))
                worst_ref[k] = max(worst_ref[k], S.worst(ref[k], spec[k], masks[k]))
                assert not bool(out[k][~live].any())
    assert n > 10000
    for k in worst:
        _check('project/' + k, worst[k], 4 * worst_ref[k])


@pytest.mark.parametrize('T1,Q,origin', [(1, 1, -1), (13, 1, 6), (1, 257, 0), (13, 257, 6), (13, 1000, 0)])
def test_score_equals_the_mirror(ctx, T1, Q, origin):
    from dvd_hip import ops
    N = ctx.N
    case = PS.score_case(T1, Q, N, origin, 1000 + 13 * T1 + Q)
    dev = {k: helpers.t(v, DEV) for k, v in case.items()}
    for sx, sy in ((1.0, 1.0), (256.0 / ctx.W, 256.0 / ctx.H)):
        res = ops.point_score(dev['uv'], dev['visible'], dev['target'], dev['gt_uv'], dev['gt_state'], origin=origin,
                              px_scale=(sx, sy))
        assert res['shift'] == PS.eval_shift(Q) and res['sums'].shape == (T1, 19) and res['sums'].dtype == torch.int64
        want = PS.score_mirror(case['uv'], case['visible'], case['target'], origin, case['gt_uv'], case['gt_state'], sx=sx, sy=sy)
        got = res['sums'].cpu().numpy()
        assert (got[:, :18] == want[:, :18]).all(), (got - want)[:, :18]
        assert (got[:, 18] == want[:, 18]).all(), (got - want)[:, 18]
        if origin >= 0:
            assert not got[origin].any()
    if Q >= 257 and T1 == 13:
        assert want[:, 0].sum() > want[:, 1].sum() > 0 and (want[:, 13:18].sum(0) > 0).all() and want[:, 18].sum() > 0
    # accumulating into passed sums is the sum of two calls; two runs give the same bits
    again = ops.point_score(dev['uv'], dev['visible'], dev['target'], dev['gt_uv'], dev['gt_state'], origin=origin,
                            px_scale=(sx, sy), sums=res['sums'].clone())
    assert torch.equal(again['sums'], 2 * res['sums'])
    other = PS.score_case(T1, Q, N, origin, 77)
    o = {k: helpers.t(v, DEV) for k, v in other.items()}
    both = ops.point_score(o['uv'], o['visible'], o['target'], o['gt_uv'], o['gt_state'], origin=origin, px_scale=(sx, sy),
                           sums=res['sums'].clone())
    alone = ops.point_score(o['uv'], o['visible'], o['target'], o['gt_uv'], o['gt_state'], origin=origin, px_scale=(sx, sy))
    assert torch.equal(both['sums'], res['sums'] + alone['sums'])


def test_score_refusals(ctx):
    from dvd_hip import ops
    case = {k: helpers.t(v, DEV) for k, v in PS.score_case(2, 5, ctx.N, 0, 3).items()}
    args = (case['uv'], case['visible'], case['target'], case['gt_uv'], case['gt_state'])
    for kw, word in ((dict(origin=2), 'origin'), (dict(px_scale=(0.0, 1.0)), 'sx'), (dict(px_scale=(1.0, float('inf'))), 'sy'),
                     (dict(px_scale=1.0), 'px_scale'), (dict(thresholds=(1, 2, 3)), 'thresholds'),
                     (dict(sums=torch.zeros(2, 18, dtype=torch.int64, device=DEV)), 'sums')):
        with pytest.raises(RuntimeError, match=word):
            ops.point_score(*args, **kw)
    with pytest.raises(RuntimeError, match='gt_uv'):
        ops.point_score(case['uv'], case['visible'], case['target'], case['gt_uv'][:4], case['gt_state'])
    with pytest.raises(RuntimeError, match='gt_state'):
        ops.point_score(case['uv'], case['visible'], case['target'], case['gt_uv'], case['gt_state'][:, :3])
    with pytest.raises(RuntimeError, match='target'):
        ops.point_score(case['uv'], case['visible'], case['target'].long(), case['gt_uv'], case['gt_state'])
    with pytest.raises(RuntimeError, match='points hold'):
        ops.point_project(torch.zeros(2, 3, 4, device=DEV), [0] * 5, torch.zeros(5, 2, device=DEV), ctx.tabs, ctx.depth)
