"""Model.evaluate on the GPU (dvd_hip/models/evaluate.py).

The store and the model are those of tests/test_45_tracks_gpu.py -- the 7 frames at 11 x 21 of
tests/golden/tracks_b3_11x21_t4.npz, start frames [0, 3, 5], 4 steps -- but the catalogue holds the gaps [1, 2], so that steps 1
and 2 find flow pairs (the writer's omitted last pairs and steps 3, 4 find none).

Exact: the sums are ops.eval_tracks over Model.track's points[1:], for every chunk; the means are the sums divided in float64;
by_step pools sums over start frames.  Against the float64 pipeline (eval_spec.pipeline_case: tracks_spec's unproject, integrate,
project) the sums stay within the bounds of tests/test_51_eval_kernel_gpu.py's third assertion, the map bound being 4 x the
distance of the fp32 run of the specification from its float64 run on these inputs.  disp_mse is _vali_on_batch's expression in
float64.  A consistent world -- one camera, one frame repeated, a field that does not move, zero flow -- scores zero.
"""
from types import SimpleNamespace
import warnings

import numpy as np
import pytest
import torch

import eval_spec as E
import helpers
import store_spec

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CAPS = {'rel': 1.0, 'photo': E.CAP, 'epe': E.CAP}


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
    """The fixture, the store, the model, ONE evaluate run with maps and the float64 pipeline: computed once, shared by the
    tests below, never written to."""
    c = _Ctx()
    fx = c.fx = helpers.load_golden(E.PIPE_FX)
    c.tree = E.pipeline_tree(fx)
    c.store = _store(str(tmp_path_factory.mktemp('evaluate')), c.tree, list(E.PIPE_GAPS))
    for k in ('R', 't', 'K_T'):
        assert torch.equal(c.store.tables[k].cpu(), torch.from_numpy(fx['tab_' + k])), k
    assert c.store.cat.pairs == E.writer_pairs(int(fx['N']), E.PIPE_GAPS)
    c.model = _model(int(fx['seed']))
    c.start, c.n_steps = fx['start'].tolist(), int(fx['n_steps'])
    c.depth = helpers.t(fx['in_depth'], DEV)
    c.out = c.model.evaluate(c.store, c.start, c.n_steps, depth=c.depth, maps=True)
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu() for k, v in c.model.net_sceneflow.state_dict().items()}
    c.case = E.pipeline_case(fx, sd)
    c.r64, c.r32 = E.run_case(c.case), E.run_case(c.case, dtype=torch.float32)
    return c


def test_sums_are_eval_tracks_over_the_tracks_for_every_chunk(ctx):
    from dvd_hip import ops
    from dvd_hip.models.evaluate import evaluate_plan
    out, store = ctx.out, ctx.store
    K, B, H, W = ctx.n_steps, len(ctx.start), store.H, store.W
    assert out['sums'].shape == (K, B, 6) and out['sums'].dtype == torch.int64 and out['sums'].is_cuda
    assert out['maps'].shape == (K, B, 3, H, W) and out['shift'] == 32 and out['steps_valid'].tolist() == [4, 3, 1]
    track = ctx.model.track(store, ctx.start, K, depth=ctx.depth)
    valid, table = evaluate_plan(store.cat, ctx.start, K)
    assert valid == [4, 3, 1] and np.array_equal(table, ctx.case['pair_row'])
    direct = ops.eval_tracks(track['points'][1:], ctx.start, store.tables, ctx.depth, store.img, k_first=1,
                             pairs=(table, store.flow_1_2, store.mask_2), maps=True)
    assert torch.equal(direct['sums'], out['sums']) and torch.equal(direct['maps'], out['maps'])
    for chunk in (1, 2, None):
        other = ctx.model.evaluate(store, ctx.start, K, depth=ctx.depth, chunk=chunk)
        assert 'maps' not in other and torch.equal(other['sums'], out['sums']), chunk
        for k in ('depth_rel', 'photo', 'flow_epe', 'disp_mse'):
            assert torch.equal(other[k].isnan(), out[k].isnan()) and torch.equal(other[k].nan_to_num(-1), out[k].nan_to_num(-1))
    with pytest.raises(ValueError, match='chunk'):
        ctx.model.evaluate(store, ctx.start, K, depth=ctx.depth, chunk=0)
    with pytest.raises(ValueError, match='track_plan'):
        ctx.model.evaluate(store, [0, 7], K, depth=ctx.depth)
    with pytest.raises(ValueError, match='depth'):
        ctx.model.evaluate(store, ctx.start, K, depth=ctx.depth[:3])
    # the steps with a flow pair have flow counts, the others none; rows past the end of the video are empty
    n_flow = out['n_flow'].cpu()
    assert bool((n_flow[torch.from_numpy(table >= 0)] > 0).all()) and not bool(n_flow[torch.from_numpy(table < 0)].any())
    assert not bool(out['sums'].cpu()[~ctx.r64['live']].any())


def test_derived_means_and_the_pooling_over_start_frames(ctx):
    out = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in ctx.out.items()}
    sums, scale = out['sums'], float(2 ** out['shift'])
    assert torch.equal(out['n_inside'], sums[..., 0]) and torch.equal(out['n_occluded'], sums[..., 1])
    assert torch.equal(out['n_flow'], sums[..., 4])

    def mean(total, count):
        want = total.double() / scale / count.double()
        return torch.where(count > 0, want, torch.full_like(want, float('nan')))

    def same(a, b):
        assert a.dtype == torch.float64 and torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(-1), b.nan_to_num(-1))

    seen = sums[..., 0] - sums[..., 1]
    same(out['depth_rel'], mean(sums[..., 2], seen))
    same(out['photo'], mean(sums[..., 3], seen))
    same(out['flow_epe'], mean(sums[..., 5], sums[..., 4]))
    # NaN exactly where nothing was counted: steps 3 and 4 have no flow pair, the rows past the end of the video have nothing
    # (and the whole of frame 5 lies behind the camera of frame 6 in this fixture)
    assert torch.equal(out['depth_rel'].isnan(), seen == 0) and torch.equal(out['flow_epe'].isnan(), sums[..., 4] == 0)
    assert bool(out['flow_epe'][2:].isnan().all()) and bool(out['depth_rel'][1:, 2].isnan().all())
    assert bool(out['depth_rel'][:2, :2].isfinite().all()) and bool(out['flow_epe'][:2, :2].isfinite().all())
    pooled = sums.sum(1)
    by = {k: v.cpu() for k, v in out['by_step'].items()}
    assert set(by) == {'depth_rel', 'photo', 'flow_epe', 'occluded'}
    p_seen = pooled[:, 0] - pooled[:, 1]
    same(by['depth_rel'], mean(pooled[:, 2], p_seen))
    same(by['photo'], mean(pooled[:, 3], p_seen))
    same(by['flow_epe'], mean(pooled[:, 5], pooled[:, 4]))
    same(by['occluded'], pooled[:, 1].double() / pooled[:, 0].double())
    for k in by:
        assert by[k].shape == (ctx.n_steps,)


def test_against_the_float64_pipeline(ctx):
    r64, r32 = ctx.r64, ctx.r32
    sums, shift = ctx.out['sums'].cpu(), ctx.out['shift']
    scale = float(2 ** shift)
    solid = ~r64['fragile']
    bound = {}
    for i, q in enumerate(('rel', 'photo', 'epe')):
        a, b = r64['maps'][:, :, i], r32['maps'][:, :, i].double()
        both = (a >= 0) & (b >= 0) & solid
        bound[q] = 4.0 * float((a - b).abs()[both].max())
        g = ctx.out['maps'][:, :, i].cpu().double()
        ours = (g >= 0) & both
        d = float((g - a).abs()[ours].max())
        helpers.log_measured('evaluate/' + q, d, bound[q])
        print('measured evaluate/%s %.4g (bound %.4g)' % (q, d, bound[q]))
        assert d <= bound[q], (q, d, bound[q])
        assert not bool((((g >= 0) != (a >= 0)) & solid).any()), q
    K, B = sums.shape[:2]
    for r in range(K):
        for b in range(B):
            s_got, s_spec, n_frag = sums[r, b].tolist(), r64['sums'][r][b], r64['n_fragile'][r][b]
            for i in (0, 1, 4):
                assert abs(s_got[i] - s_spec[i]) <= n_frag, (r, b, E.SUMS[i], s_got, s_spec, n_frag)
            n_seen, n_flow = max(s_got[0] - s_got[1], s_spec[0] - s_spec[1]), max(s_got[4], s_spec[4])
            for i, q, n in ((2, 'rel', n_seen), (3, 'photo', n_seen), (5, 'epe', n_flow)):
                limit = n * bound[q] + n_frag * CAPS[q] + n * 2.0 ** -(shift + 1)
                assert abs(s_got[i] - s_spec[i]) / scale <= limit, (r, b, q, s_got[i] / scale, s_spec[i] / scale, limit)


def test_disp_mse_is_the_validation_score_in_float64(ctx):
    depth, gt = torch.from_numpy(ctx.fx['in_depth']).double(), torch.from_numpy(ctx.tree['fr_depth_mvs']).double()[:, None]

    def disp(d):
        valid = (d > 1e-2).double()
        return (1 / (d + (1 - valid) * 1e-8)) * valid

    vali = (gt > 1e-2).double()
    want = torch.stack([torch.nn.functional.mse_loss(disp(depth[i]) * vali[i], disp(gt[i]) * vali[i]) for i in range(depth.shape[0])])
    got = ctx.out['disp_mse']
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == (int(ctx.fx['N']),)
    assert float(((got.cpu() - want).abs() / want).max()) <= 1e-9 and float(want.min()) > 0


def test_use_cnn_is_refused_with_a_message(ctx):
    model = _model(3, use_cnn=True)
    with pytest.raises(NotImplementedError, match='use_cnn'):
        model.evaluate(ctx.store, ctx.start, ctx.n_steps, depth=ctx.depth)


def test_a_consistent_world_scores_zero(tmp_path):
    """One camera, one frame repeated, a scene-flow net whose last layer is zero, zero flow with valid masks: every point lands
    on its own pixel, sees its own depth and colour, and moves as the flow says."""
    N, H, W = 5, 11, 21
    tree = store_spec.random_tree(N, H, W, [1, 2], 9)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    depth = (3.0 + 0.4 * np.sin(0.3 * xx) + 0.3 * np.cos(0.25 * yy)).astype(np.float32)
    for k in ('fr_img', 'fr_depth_pred', 'fr_depth_mvs', 'fr_pose_c2w'):
        tree[k] = np.repeat(tree[k][:1], N, 0)
    tree['fr_depth_pred'] = np.repeat(depth[None], N, 0)
    tree['fl_flow_1_2'][:], tree['fl_flow_2_1'][:], tree['fl_mask_1'][:], tree['fl_mask_2'][:] = 0, 0, 0, 0
    store = _store(str(tmp_path), tree, [1, 2])
    model = _model(13)
    with torch.no_grad():
        for p in model.net_sceneflow.parameter_list()[-2:]:
            p.zero_()
    out = model.evaluate(store, depth=store.depth_pred)
    K, B = 2, N - 1
    assert out['sums'].shape == (K, B, 6) and out['steps_valid'].tolist() == [2, 2, 2, 1]
    live = torch.tensor([[s + k < N for s in range(B)] for k in (1, 2)])
    n_inside = out['n_inside'].cpu()
    assert not bool(out['n_occluded'].any()) and bool((n_inside[live] >= (H - 2) * (W - 2)).all())
    assert not bool(n_inside[~live].any())
    for k in ('depth_rel', 'photo'):
        v = out[k].cpu()
        assert bool((v[live] < 1e-5).all()) and bool(v[~live].isnan().all()), k
    table_live = torch.tensor([[0 <= s + k < N - 1 for s in range(B)] for k in (1, 2)])      # the writer's omitted last pairs
    epe = out['flow_epe'].cpu()
    assert bool((epe[table_live] < 1e-5).all()) and bool(epe[~table_live].isnan().all())
    assert bool((out['n_flow'].cpu()[table_live] == H * W).all())
    for k, v in out['by_step'].items():
        assert bool((v.cpu() < 1e-5).all()), k
