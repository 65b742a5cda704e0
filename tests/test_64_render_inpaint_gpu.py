"""Model.render(inpaint=True) and preprocess.triangulate_depth(densify=True) on the GPU: ops.fill_holes (csrc/fill.hip) behind the
two products that leave holes.

The render store and models are those of tests/test_49_render_gpu.py, built the same way (7 frames of 11 x 21); the cases are the
two of splat_spec.RENDER_CASES that leave holes, a novel camera and the masked one.  The triangulation store is the one of
tests/test_62_triangulate_depth_gpu.py.  Everything here is exact: inpaint=True is ops.fill_holes applied to the inpaint=False
result, bit for bit, and what the kernels compute is checked against the specification in tests/test_63_fill_kernel_gpu.py.
"""
from types import SimpleNamespace
import warnings

import numpy as np
import pytest
import torch

import helpers
import splat_spec as S
import store_spec
import triangulate_spec as T

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CASES = ('novel', 'masked')


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


def _render(c, name, **kw):
    case = S.RENDER_CASES[name]
    if case['novel']:
        kw.setdefault('cam_c2w', S.novel_poses(c.fx['in_pose_c2w'], case['target']))
    if case.get('masked'):
        kw.setdefault('valid', helpers.t(S.left_half_mask(c.N, c.H, c.W), DEV))
    out = c.model.render(c.store, case['target'], case['sources'], depth=c.depth, advect=case['advect'], **kw)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope='module')
def ctx(tmp_path_factory):
    """The fixture, its store, the network and ONE render per case with and without inpaint: shared, never written to."""
    from dvd_hip.datasets.frame_store import Catalogue, FrameStore
    c = _Ctx()
    fx = c.fx = helpers.load_golden(S.RENDER_FX)
    c.N, c.H, c.W = int(fx['N']), int(fx['H']), int(fx['W'])
    tree = store_spec.random_tree(c.N, c.H, c.W, [1], S.RENDER_IMG_SEED)
    tree['fr_pose_c2w'], tree['fr_intrinsics'] = fx['in_pose_c2w'], fx['in_intrinsics']
    root = str(tmp_path_factory.mktemp('inpaint'))
    store_spec.write_tree(root, tree)
    c.store = FrameStore(Catalogue(root, store_spec.TRACK, [1]), DEV)
    c.depth = helpers.t(fx['in_depth'], DEV)
    c.model = _model(int(fx['seed']))
    c.plain = {name: _render(c, name) for name in CASES}
    c.filled = {name: _render(c, name, inpaint=True) for name in CASES}
    return c


def _filled_by_hand(plain, power, fill=0.0):
    from dvd_hip import ops
    joint = torch.cat((plain['image'], plain['depth']), dim=1)
    out = ops.fill_holes(joint, plain['hit'], bias=plain['depth'], power=power, fill=fill)
    torch.cuda.synchronize()
    return out['values'][:, :3], out['values'][:, 3:], out['level']


@pytest.mark.parametrize('name', CASES)
def test_inpaint_is_fill_holes_of_the_plain_render(ctx, name):
    plain, filled = ctx.plain[name], ctx.filled[name]
    assert set(plain) == {'image', 'depth', 'weight', 'hit'}                     # inpaint=False: exactly today's keys
    assert set(filled) == set(plain) | {'level'}
    hit = plain['hit'] != 0
    assert 0 < int((~hit).sum()) and hit.flatten(1).any(1).all(), 'the case must leave holes, and no view empty'
    image, depth, level = _filled_by_hand(plain, 2)
    assert torch.equal(filled['image'], image) and torch.equal(filled['depth'], depth) and torch.equal(filled['level'], level)
    assert filled['image'].shape == plain['image'].shape and filled['depth'].shape == plain['depth'].shape
    assert filled['level'].dtype == torch.uint8 and filled['level'].shape == plain['hit'].shape
    # hit, weight and the hit pixels of image and depth are the plain render's bits
    assert torch.equal(filled['hit'], plain['hit']) and torch.equal(filled['weight'], plain['weight'])
    h3 = hit[:, None].expand_as(plain['image'])
    assert torch.equal(filled['image'][h3].view(torch.int32), plain['image'][h3].view(torch.int32))
    assert torch.equal(filled['depth'][hit[:, None]].view(torch.int32), plain['depth'][hit[:, None]].view(torch.int32))
    assert torch.equal(filled['level'] == 0, hit)


@pytest.mark.parametrize('name', CASES)
def test_no_hole_is_left_and_filled_depths_stay_within_the_views_range(ctx, name):
    plain, filled = ctx.plain[name], ctx.filled[name]
    hole = (filled['level'] >= 1) & (filled['level'] <= 254)
    assert torch.equal(hole, plain['hit'] == 0)
    # the plain render holds fill = 0 and depth 0 in its holes; the colours of the store are positive
    assert (plain['depth'][:, 0][hole] == 0).all() and (plain['image'].permute(0, 2, 3, 1)[hole] == 0).all()
    assert (filled['depth'][:, 0][hole] > 0).all()
    assert not (filled['image'].permute(0, 2, 3, 1)[hole] == 0).all(-1).any()
    for v in range(plain['hit'].shape[0]):
        hv = plain['hit'][v] != 0
        lo, hi = plain['depth'][v, 0][hv].min(), plain['depth'][v, 0][hv].max()
        d = filled['depth'][v, 0]
        # a weighted mean may leave the range of its terms by its roundings: a few ulp of the largest depth
        eps = 8 * float(np.spacing(np.float32(hi.item())))
        assert float(d.min()) >= float(lo) - eps and float(d.max()) <= float(hi) + eps, (v, float(lo), float(d.min()), float(hi), float(d.max()))
        for ch in range(3):
            cl, chh = plain['image'][v, ch][hv].min(), plain['image'][v, ch][hv].max()
            assert float(filled['image'][v, ch].min()) >= float(cl) - 1e-6 and float(filled['image'][v, ch].max()) <= float(chh) + 1e-6


def test_bg_power_and_fill_reach_the_kernels_and_bad_arguments_are_refused(ctx):
    plain = ctx.plain['masked']
    for power in (0, 4):
        got = _render(ctx, 'masked', inpaint=True, bg_power=power)
        image, depth, level = _filled_by_hand(plain, power)
        assert torch.equal(got['image'], image) and torch.equal(got['depth'], depth) and torch.equal(got['level'], level)
    assert not torch.equal(_filled_by_hand(plain, 0)[1], ctx.filled['masked']['depth'])
    # a view nothing reaches stays `fill`, its level 255: every pixel of every source dropped
    none = _render(ctx, 'masked', inpaint=True, fill=0.25, valid=torch.zeros(ctx.N, ctx.H, ctx.W, device=DEV, dtype=torch.uint8))
    assert (none['level'] == 255).all() and (none['image'] == 0.25).all() and (none['depth'] == 0.25).all() and not none['hit'].any()
    plain_again = _render(ctx, 'masked', inpaint=False, bg_power=3)
    assert set(plain_again) == set(plain) and all(torch.equal(plain_again[k], plain[k]) for k in plain)
    for kw in (dict(bg_power=5), dict(bg_power=-1), dict(bg_power=1.0), dict(bg_power=True), dict(inpaint=1), dict(inpaint='yes')):
        with pytest.raises(ValueError, match='bg_power|inpaint'):
            _render(ctx, 'masked', **kw)


# ---- preprocess.triangulate_depth(densify=True) ---------------------------------------------------------------------------

def test_triangulate_depth_densify(tmp_path):
    from dvd_hip import ops, preprocess
    from dvd_hip.datasets.frame_store import Catalogue, FrameStore
    H, W, N, gaps = 24, 40, 7, (1, 2, 3, 4)
    sc = T.scene(H, W, N, seed=0, noise=0.4, gaps=gaps)
    rng = np.random.default_rng(5)
    tree = {'gaps': np.array(gaps), 'fr_img': rng.random((N, H, W, 3)).astype(np.float32),
            'fr_depth_pred': (sc['depth'].astype(np.float32) * np.float32(4.0)), 'fr_depth_mvs': sc['depth'].astype(np.float32),
            'fr_pose_c2w': sc['poses'], 'fr_intrinsics': sc['intrinsics'], 'fl_ids': np.array(sc['pairs']),
            'fl_flow_1_2': sc['flow_1_2'], 'fl_flow_2_1': sc['flow_2_1'], 'fl_mask_1': sc['mask_1'], 'fl_mask_2': sc['mask_2']}
    store_spec.write_tree(str(tmp_path), tree)
    store = FrameStore(Catalogue(str(tmp_path), store_spec.TRACK, list(gaps), all_pairs=True), DEV)
    plain = preprocess.triangulate_depth(store)
    dense = preprocess.triangulate_depth(store, densify=True)
    torch.cuda.synchronize()
    assert set(dense) == set(plain) | {'depth_dense', 'dense_level'}
    for k, v in plain.items():
        same = torch.equal(dense[k], v) if torch.is_tensor(v) else np.array_equal(dense[k], v)
        assert same, k
    static = plain['static']
    assert 0 < int((~static).sum()) and static.flatten(1).any(1).all()
    assert dense['depth_dense'].shape == (N, 1, H, W) and dense['dense_level'].shape == (N, H, W)
    assert torch.equal(dense['depth_dense'][:, 0][static].view(torch.int32), plain['depth'][:, 0][static].view(torch.int32))
    assert (dense['depth_dense'] > 0).all() and torch.isfinite(dense['depth_dense']).all()
    assert torch.equal(dense['dense_level'] == 0, static) and int(dense['dense_level'].max()) < 255
    want = ops.fill_holes(plain['depth'], static.to(torch.uint8))
    assert torch.equal(dense['depth_dense'], want['values']) and torch.equal(dense['dense_level'], want['level'])
    with pytest.raises(ValueError, match='densify'):
        preprocess.triangulate_depth(store, densify='yes')
