"""Model.score_depth on the GPU (dvd_hip/models/score_depth.py).

The store and the model are those of tests/test_52_evaluate_gpu.py -- the 7 frames at 11 x 21 of
tests/golden/tracks_b3_11x21_t4.npz in a catalogue with the gaps [1, 2]; its frame files carry no motion segmentation, so a
second store adds one to the same tree.  The depth net cannot halve 11 x 21 frames, so the comparison over Model.video_depth
runs on the hourglass store of tests/test_45_tracks_gpu.py's model-level test (5 frames at 32 x 48), with a motion segmentation.

Exact: for the three alignments the result is ops.ratio_median + ops.depth_score over Model.video_depth; the derived means are
the float64 quotients of the sums; `video` is the pooled row; 'median_frame' and 'median_video' coincide on a one-frame store;
without a motion segmentation rows 1 and 2 are NaN; gt = depth with align='none' scores zero.  Against the float64 pipeline
(depth_score_spec over the same depth, with numpy's medians) the scale is equal bit for bit and the sums stay within the bounds of
tests/test_54_depth_score_gpu.py.  Model.evaluate gives the same bits before and after.
"""
from types import SimpleNamespace
import warnings

import numpy as np
import pytest
import torch

import depth_score_spec as D
import eval_spec as E
import helpers
import store_spec

pytestmark = pytest.mark.gpu

DEV = 'cuda'
MEANS = ('abs_rel', 'sq_rel', 'rmse', 'rmse_log', 'silog', 'd1', 'd2', 'd3')


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


def _store(root, tree, gaps):
    from dvd_hip.datasets.frame_store import Catalogue, FrameStore
    store_spec.write_tree(root, tree)
    return FrameStore(Catalogue(root, store_spec.TRACK, gaps), DEV)


class _Ctx(object):
    pass


@pytest.fixture(scope='module')
def ctx(tmp_path_factory):
    """The fixture, the two stores, the model and the fixture's depth: made once, shared by the tests below, never written to."""
    c = _Ctx()
    fx = c.fx = helpers.load_golden(E.PIPE_FX)
    c.tree = E.pipeline_tree(fx)
    c.store = _store(str(tmp_path_factory.mktemp('score')), c.tree, list(E.PIPE_GAPS))
    assert c.store.motion_seg is None
    N, H, W = int(fx['N']), int(fx['H']), int(fx['W'])
    c.seg = (np.random.RandomState(11).rand(N, H, W) > 0.6).astype(np.float32)
    c.store_seg = _store(str(tmp_path_factory.mktemp('score_seg')), dict(c.tree, fr_motion_seg=c.seg), list(E.PIPE_GAPS))
    assert torch.equal(c.store_seg.motion_seg.cpu(), torch.from_numpy(c.seg))
    c.model = _model(int(fx['seed']))
    c.depth = helpers.t(fx['in_depth'], DEV)
    c.gt = np.ascontiguousarray(c.tree['fr_depth_mvs'][:, None].astype(np.float32))
    assert torch.equal(c.store.depth_mvs.cpu(), torch.from_numpy(c.gt))
    return c


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(-1), b.nan_to_num(-1))


def _direct(depth, gt, align, seg=None, mask=None):
    from dvd_hip import ops
    N = depth.shape[0]
    keep = (gt > D.G_MIN)
    if mask is not None:
        keep = keep & (mask != 0)[:, None]
    keep = keep.to(torch.uint8)
    if align == 'none':
        scale = torch.ones(N, device=DEV)
    elif align == 'median_frame':
        scale = ops.ratio_median(gt.reshape(N, -1), depth.reshape(N, -1), mask=keep.reshape(N, -1))['median']
    else:
        scale = ops.ratio_median(gt.reshape(1, -1), depth.reshape(1, -1), mask=keep.reshape(1, -1))['median'].expand(N).contiguous()
    return scale, ops.depth_score(depth, gt, scale, seg=seg, mask=mask, maps=True)


@pytest.fixture(scope='module')
def hourglass(tmp_path_factory):
    """The depth net needs a size it can halve: the hourglass at 32 x 48, 5 frames with a motion segmentation (the store of
    tests/test_45_tracks_gpu.py's model-level test), and its video_depth -- made once, never written to."""
    c = _Ctx()
    c.store = _store(str(tmp_path_factory.mktemp('score_hg')), store_spec.random_tree(5, 32, 48, [1], 11, with_seg=True), [1])
    c.model = _model(21)
    c.depth = c.model.video_depth(c.store.frames(c.model._chunk()))
    return c


@pytest.mark.parametrize('align', ('none', 'median_frame', 'median_video'))
def test_score_depth_is_the_median_and_the_score_over_video_depth(hourglass, align):
    model, store, depth = hourglass.model, hourglass.store, hourglass.depth
    N, H, W = store.cat.n_frames, store.H, store.W
    assert tuple(depth.shape) == (N, 1, H, W) and store.motion_seg is not None
    out = model.score_depth(store, align=align, maps=True)
    scale, want = _direct(depth, store.depth_mvs, align, seg=store.motion_seg)
    assert out['sums'].shape == (N, 3, 9) and out['sums'].dtype == torch.int64 and out['sums'].is_cuda and out['shift'] == want['shift']
    assert torch.equal(out['scale'].isnan(), scale.isnan()) and torch.equal(out['scale'].nan_to_num(-1), scale.nan_to_num(-1))
    assert torch.equal(out['sums'], want['sums']) and torch.equal(out['maps'], want['maps']) and torch.equal(out['counted'], want['counted'])
    assert torch.equal(out['n'], out['sums'][..., 0]) and out['scale'].shape == (N,) and out['scale'].dtype == torch.float32
    bare = model.score_depth(store, align=align)
    assert 'maps' not in bare and torch.equal(bare['sums'], out['sums'])
    # a mask of the caller restricts the median and the score alike
    mask = (torch.rand(N, H, W, generator=torch.Generator().manual_seed(4)) < 0.8).to(torch.uint8).to(DEV)
    masked = model.score_depth(store, depth=depth, align=align, mask=mask)
    m_scale, m_want = _direct(depth, store.depth_mvs, align, seg=store.motion_seg, mask=mask)
    assert torch.equal(masked['sums'], m_want['sums']) and torch.equal(masked['scale'].nan_to_num(-1), m_scale.nan_to_num(-1))


def test_arguments_are_checked(ctx):
    with pytest.raises(ValueError, match='align'):
        ctx.model.score_depth(ctx.store, depth=ctx.depth, align='least_squares')
    with pytest.raises(ValueError, match='depth'):
        ctx.model.score_depth(ctx.store, depth=ctx.depth[:3])
    with pytest.raises(ValueError, match='gt'):
        ctx.model.score_depth(ctx.store, depth=ctx.depth, gt=ctx.depth[:, :, :5])
    with pytest.raises(ValueError, match='mask'):
        ctx.model.score_depth(ctx.store, depth=ctx.depth, mask=torch.ones(2, 2, dtype=torch.uint8, device=DEV))


def test_derived_means_the_pooled_row_and_nan_rows_without_a_motion_segmentation(ctx):
    for store, has_seg in ((ctx.store_seg, True), (ctx.store, False)):
        out = ctx.model.score_depth(store, depth=ctx.depth, align='median_frame')
        sums, two = out['sums'].cpu(), float(2 ** out['shift'])
        n = sums[..., 0]

        def derive(rows):
            cnt = rows[..., 0].double()
            nan = torch.full_like(cnt, float('nan'))
            mean = lambda i, unit: torch.where(cnt > 0, rows[..., i].double() / unit / cnt, nan)
            l2, l = mean(4, two), mean(5, two)
            return {'abs_rel': mean(1, two), 'sq_rel': mean(2, two), 'rmse': mean(3, two).sqrt(), 'rmse_log': l2.sqrt(),
                    'silog': l2 - l * l, 'd1': mean(6, 1.0), 'd2': mean(7, 1.0), 'd3': mean(8, 1.0)}

        want, pooled = derive(sums), derive(sums.sum(0))
        assert set(MEANS) <= set(out) and set(MEANS) <= set(out['video'])
        for k in MEANS:
            assert out[k].is_cuda and out[k].dtype == torch.float64 and out[k].shape == (sums.shape[0], 3), k
            _same(out[k].cpu(), want[k])
            assert out['video'][k].shape == (3,)
            _same(out['video'][k].cpu(), pooled[k])
            assert torch.equal(out[k].cpu().isnan(), n == 0), k
        assert torch.equal(out['video']['n'].cpu(), n.sum(0)) and bool((n[:, 0] > 0).all())
        if has_seg:
            assert bool((n[:, 1:] > 0).all()) and torch.equal(n[:, 1] + n[:, 2], n[:, 0])
            flat = ctx.model.score_depth(store, depth=ctx.depth, align='median_frame', regions=False)
            assert torch.equal(flat['sums'][:, 0], out['sums'][:, 0]) and not bool(flat['sums'][:, 1:].any())
        else:
            assert not bool(sums[:, 1:].any()) and bool(out['abs_rel'][:, 1:].isnan().all()) and bool(out['video']['d1'][1:].isnan().all())
            assert bool(out['abs_rel'][:, 0].isfinite().all())


def test_frame_and_video_medians_coincide_on_a_one_frame_store(ctx):
    from dvd_hip import ops
    depth, gt = ctx.depth[2:3], ctx.store.depth_mvs[2:3]
    keep = (gt > D.G_MIN).to(torch.uint8)
    a = ops.ratio_median(gt.reshape(1, -1), depth.reshape(1, -1), mask=keep.reshape(1, -1))['median']

    class _One(object):                      # what score_depth reads of a store (a catalogue needs two frames): frame 2 alone
        cat = SimpleNamespace(n_frames=1)
        H, W, device, motion_seg, depth_mvs = ctx.store.H, ctx.store.W, ctx.store.device, None, gt

    frame = ctx.model.score_depth(_One, depth=depth, align='median_frame')
    video = ctx.model.score_depth(_One, depth=depth, align='median_video')
    assert torch.equal(frame['scale'], video['scale']) and torch.equal(frame['scale'], a) and torch.equal(frame['sums'], video['sums'])
    assert bool(frame['scale'].isfinite().all()) and int(frame['n'][0, 0]) > 0


@pytest.mark.parametrize('align', ('none', 'median_frame', 'median_video'))
def test_against_the_float64_pipeline(ctx, align):
    depth, gt, seg = ctx.fx['in_depth'].astype(np.float32), ctx.gt, ctx.seg
    N = depth.shape[0]
    keep = (gt > np.float32(D.G_MIN)).astype(np.uint8).reshape(N, -1)
    if align == 'none':
        scale = np.ones(N, dtype=np.float32)
    elif align == 'median_frame':
        scale = D.median(gt.reshape(N, -1), depth.reshape(N, -1), keep)[0]
    else:
        scale = np.repeat(D.median(gt.reshape(1, -1), depth.reshape(1, -1), keep.reshape(1, -1))[0], N)
    out = ctx.model.score_depth(ctx.store_seg, depth=ctx.depth, align=align, maps=True)
    assert np.array_equal(out['scale'].cpu().numpy(), scale)                 # numpy's medians, bit for bit
    r64, r32 = D.score(depth, gt, scale, seg), D.score(depth, gt, scale, seg, dtype=np.float32)
    assert D.fragile_share(r64) <= D.FRAGILE_CAP and out['shift'] == r64['shift']
    sums, maps, counted = out['sums'].cpu(), out['maps'].cpu(), out['counted'].cpu().bool().numpy()
    solid = ~r64['fragile']
    assert not ((counted != r64['counted']) & solid).any()
    both = counted & r64['counted'] & r32['counted'] & solid
    bound = {}
    for q in D.TERMS:
        a, b = r64[q], r32[q].astype(np.float64)
        d_fp32 = float(np.abs(a - b)[both].max())
        bound[q] = 4.0 * d_fp32 if d_fp32 > 0 else 2.0 ** -24 * float(np.abs(a[both]).max())
        if q in D.MAPS:
            d_kernel = float(np.abs(maps[:, D.MAPS.index(q)].double().numpy() - a)[both].max())
            helpers.log_measured('score_depth/%s/%s' % (align, q), d_kernel, bound[q])
            print('measured score_depth/%s/%s %.4g (fp32 specification %.4g, bound %.4g)' % (align, q, d_kernel, d_fp32, bound[q]))
            assert d_kernel <= bound[q], (align, q, d_kernel, bound[q])
    shift = out['shift']
    two = float(2 ** shift)
    for n in range(N):
        for r in range(3):
            s_got, s_spec, n_frag = sums[n, r].tolist(), r64['sums'][n][r], r64['n_fragile'][n][r]
            for i in (0, 6, 7, 8):
                assert abs(s_got[i] - s_spec[i]) <= n_frag, (align, n, r, D.SUMS[i], s_got, s_spec)
            cnt = max(s_got[0], s_spec[0])
            for i, q in enumerate(D.TERMS, 1):
                limit = cnt * bound[q] + n_frag * D.TERM_CAPS[q] + cnt * 2.0 ** -(shift + 1)
                assert abs(s_got[i] - s_spec[i]) / two <= limit, (align, n, r, q, s_got[i] / two, s_spec[i] / two, limit)
            # ... and the reported numbers follow
            got, want = {k: float(out[k][n, r]) for k in MEANS}, D.derive(s_spec, shift)
            if s_spec[0] and n_frag == 0:
                for k in ('abs_rel', 'sq_rel', 'd1', 'd2', 'd3'):
                    lim = {'abs_rel': bound['abs_rel'], 'sq_rel': bound['sq_rel']}.get(k, 0.0) + 2.0 ** -shift
                    assert abs(got[k] - want[k]) <= lim, (align, n, r, k, got[k], want[k])


def test_the_ground_truth_scored_against_itself_is_perfect(ctx):
    out = ctx.model.score_depth(ctx.store_seg, depth=ctx.store_seg.depth_mvs, align='none')
    sums = out['sums'].cpu()
    assert bool((sums[:, 0, 0] > 0).all()) and not bool(sums[..., 1:6].any())
    for k in (6, 7, 8):
        assert torch.equal(sums[..., k], sums[..., 0])
    for k in ('abs_rel', 'sq_rel', 'rmse', 'rmse_log', 'silog'):
        assert bool((out[k][:, 0] == 0).all()) and float(out['video'][k][0]) == 0.0, k
    for k in ('d1', 'd2', 'd3'):
        assert bool((out[k][:, 0] == 1).all()) and float(out['video'][k][0]) == 1.0, k
    assert out['scale'].tolist() == [1.0] * sums.shape[0]


def test_model_evaluate_gives_the_same_bits_before_and_after(ctx):
    start, n_steps = ctx.fx['start'].tolist(), int(ctx.fx['n_steps'])
    before = ctx.model.evaluate(ctx.store, start, n_steps, depth=ctx.depth, maps=True)
    ctx.model.score_depth(ctx.store, depth=ctx.depth, maps=True)
    after = ctx.model.evaluate(ctx.store, start, n_steps, depth=ctx.depth, maps=True)
    assert torch.equal(before['sums'], after['sums']) and torch.equal(before['maps'], after['maps'])
    for k in ('depth_rel', 'photo', 'flow_epe', 'disp_mse'):
        _same(before[k], after[k])
    assert set(before) == {'sums', 'shift', 'n_inside', 'n_occluded', 'n_flow', 'depth_rel', 'photo', 'flow_epe', 'by_step',
                           'disp_mse', 'maps', 'steps_valid'}
