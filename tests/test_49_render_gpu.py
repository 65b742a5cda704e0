"""Model.render on the GPU (dvd_hip/models/render.py) against its float64 specification (splat_spec.render).

The store is the one of tests/test_45_tracks_gpu.py: the 7 frames at 11 x 21 of tests/golden/tracks_b3_11x21_t4.npz (poses,
intrinsics, depth) with the images of store_spec.random_tree.  The cases are splat_spec.RENDER_CASES; tests/test_splat_cpu.py
asserts that at most 3 % of the target pixels of each are fragile under the specification alone.

Exact: advect=False is ops.splat of the un-projected frames, any `chunk` gives the same bits, two runs give the same bits,
`hit` agrees with the specification outside the fragile set.

Tolerances: the rule of tests/test_48_splat_gpu.py (splat_spec.compare) -- 4 x the distance of the fp32 specification from the
float64 one, plus the accumulators' quantisation, plus the rounding of an fp32 result -- and 4 x the entries of MEASURED, the
worst distances measured on the MI355X:
                          image      depth      weight
    kernels               1.4e-6     7.6e-7     5.4e-6
    fp32 specification    8.5e-7     5.2e-7     2.6e-6     (the yardstick; the limit is 4 x this per case)
The `held` case comes closest to its limit: image 1.43e-6 of 1.59e-6.
"""
from types import SimpleNamespace
import warnings

import numpy as np
import pytest
import torch

import helpers
import splat_spec as S
import store_spec

pytestmark = pytest.mark.gpu

DEV = 'cuda'
# worst distance from the float64 specification measured on the MI355X over the cases of this file; the bound is 4 x this
MEASURED = {'image': 1.43e-6, 'depth': 7.57e-7, 'weight': 5.43e-6}


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
    """The fixture, its store and the two networks: built once, shared by the tests below, never written to."""
    from dvd_hip.datasets.frame_store import Catalogue, FrameStore
    c = _Ctx()
    fx = c.fx = helpers.load_golden(S.RENDER_FX)
    c.N, c.H, c.W = int(fx['N']), int(fx['H']), int(fx['W'])
    tree = store_spec.random_tree(c.N, c.H, c.W, [1], S.RENDER_IMG_SEED)
    tree['fr_pose_c2w'], tree['fr_intrinsics'] = fx['in_pose_c2w'], fx['in_intrinsics']
    root = str(tmp_path_factory.mktemp('render'))
    store_spec.write_tree(root, tree)
    c.store = FrameStore(Catalogue(root, store_spec.TRACK, [1]), DEV)
    c.img = tree['fr_img'].transpose(0, 3, 1, 2)
    assert torch.equal(c.store.img.cpu(), torch.from_numpy(np.ascontiguousarray(c.img)))
    c.depth = helpers.t(fx['in_depth'], DEV)
    c.models = {True: _model(int(fx['seed'])), False: _model(int(fx['seed']) + 1, time_dependent=False)}
    return c


def _render(ctx, name, **kw):
    c = S.RENDER_CASES[name]
    model = ctx.models[c['time_dependent']]
    if c['novel']:
        kw.setdefault('cam_c2w', S.novel_poses(ctx.fx['in_pose_c2w'], c['target']))
    if c.get('masked'):
        kw.setdefault('valid', helpers.t(S.left_half_mask(ctx.N, ctx.H, ctx.W), DEV))
    out = model.render(ctx.store, c['target'], c['sources'], depth=ctx.depth, advect=c['advect'], **kw)
    torch.cuda.synchronize()
    return out


def _shift(ctx, name):
    from dvd_hip import ops
    c = S.RENDER_CASES[name]
    return ops.splat_shift(max(len(s) for s in c['sources']) * ctx.H * ctx.W)


@pytest.mark.parametrize('name', ['advect', 'notime', 'novel', 'held', 'masked'])
def test_against_the_specification(ctx, name):
    c = S.RENDER_CASES[name]
    out = _render(ctx, name)
    assert set(out) == {'image', 'depth', 'weight', 'hit'} and all(v.is_cuda for v in out.values())
    got = {k: v.cpu().numpy() for k, v in out.items()}
    sd = {k: v.detach().cpu() for k, v in ctx.models[c['time_dependent']].net_sceneflow.state_dict().items()}
    r64 = S.render_case(ctx.fx, ctx.img, sd, name)
    r32 = S.render_case(ctx.fx, ctx.img, sd, name, dtype=np.float32)
    S.compare('render/' + name, got, r64, r32, {}, _shift(ctx, name), MEASURED)
    assert 0.25 < got['hit'].mean() < 1.0


def test_a_novel_camera_differs_from_the_frames_own_and_K_alone_is_the_frames_pose(ctx):
    c = S.RENDER_CASES['novel']
    novel = _render(ctx, 'novel')
    own = _render(ctx, 'novel', cam_c2w=None)
    assert not torch.equal(novel['image'], own['image'])
    # the target frames' own poses and intrinsics handed in as novel cameras are the frames' cameras, bit for bit
    same = _render(ctx, 'novel', cam_c2w=ctx.fx['in_pose_c2w'][c['target']], K=ctx.fx['in_intrinsics'][c['target']])
    only_K = _render(ctx, 'novel', cam_c2w=None, K=torch.from_numpy(ctx.fx['in_intrinsics'][c['target']]))
    for k in own:
        assert torch.equal(same[k], own[k]) and torch.equal(only_K[k], own[k]), k
    with pytest.raises(ValueError, match='cam_c2w'):
        _render(ctx, 'novel', cam_c2w=np.zeros((3, 4, 4)))


def test_held_time_is_ops_splat_of_the_unprojected_frames(ctx):
    from dvd_hip import ops
    c = S.RENDER_CASES['held']
    out = _render(ctx, 'held')
    frames = [f for src in c['sources'] for f in src]
    view = [v for v, src in enumerate(c['sources']) for _ in src]
    T = ctx.store.tables
    pts = ops.unproject(ctx.depth[frames], T['R_T'][frames], T['t'][frames], T['K_inv_T'][frames], planar=True)
    tabs = {k: T[k][c['target']].contiguous() for k in ('R', 't', 'K_T')}
    want = ops.splat(pts, ctx.store.img[frames].contiguous(), view, tabs, len(c['target']))
    for k in want:
        assert torch.equal(out[k], want[k]), k
    # a source later than its target is fine when time is held, and refused when the field would have to run backwards
    with pytest.raises(ValueError, match='later than'):
        ctx.models[True].render(ctx.store, c['target'], c['sources'], depth=ctx.depth)


def test_every_chunk_and_every_run_gives_the_same_bits(ctx):
    first = _render(ctx, 'advect')
    for chunk in (None, 1, 2, 3):
        other = _render(ctx, 'advect', chunk=chunk)
        for k, v in first.items():
            assert torch.equal(other[k], v), (chunk, k)
    model = ctx.models[True]
    with pytest.raises(ValueError, match='chunk'):
        model.render(ctx.store, [3], [[1]], depth=ctx.depth, chunk=0)
    with pytest.raises(ValueError, match='render_plan'):
        model.render(ctx.store, [7], [[1]], depth=ctx.depth)
    with pytest.raises(ValueError, match='depth'):
        model.render(ctx.store, [3], [[1]], depth=ctx.depth[:3])
    with pytest.raises(TypeError, match='splat parameters'):
        model.render(ctx.store, [3], [[1]], depth=ctx.depth, z_far=3.0)


def test_a_frame_into_its_own_camera_and_time_is_its_image(ctx):
    out = _render(ctx, 'own')
    got = {k: v.cpu().numpy() for k, v in out.items()}
    r64 = S.render_case(ctx.fx, ctx.img, None, 'own')
    r32 = S.render_case(ctx.fx, ctx.img, None, 'own', dtype=np.float32)
    d = S.compare('render/own', got, r64, r32, {}, _shift(ctx, 'own'), MEASURED)
    assert got['hit'].all()
    # the image itself within the same bound: the specification returns it to 2e-6 (tests/test_splat_cpu.py)
    own = S.worst(got['image'][0], ctx.img[2])
    print('render/own: image vs store.img %.4g (vs the specification %.4g)' % (own, d['image']))
    assert own <= 4 * MEASURED['image']


def test_use_cnn_holds_time_only(ctx):
    model = _model(3, use_cnn=True)
    c = S.RENDER_CASES['held']
    with pytest.raises(NotImplementedError, match='use_cnn'):
        model.render(ctx.store, [3], [[1]], depth=ctx.depth)
    out = model.render(ctx.store, c['target'], c['sources'], depth=ctx.depth, advect=False)
    want = _render(ctx, 'held')
    for k in want:
        assert torch.equal(out[k], want[k]), k
