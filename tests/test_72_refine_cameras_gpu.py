"""preprocess.refine_cameras and FrameStore.set_cameras on a FrameStore (dvd_hip/preprocess.py, csrc/pose.hip).

The store is built the way tests/test_62_triangulate_depth_gpu.py builds its own -- a tree of frame and flow files written by
tests/store_spec.py, read back by Catalogue / FrameStore -- from triangulate_spec.scene(24, 40, 7, noise=0): every pair of gaps
1 to 4, the frames' depth_pred the scene's true depth, and the frames' poses pose_spec.perturbed (frames 1 .. 6 turned by up to
1 degree per axis and moved by up to 0.03: 3.2e-2 in R, 4.4e-2 in c).  The weight is the complement of the moving disc.

Against the specification: refine_cameras is pose_spec.refine over the float64 normal_eq with the product's fp32 rounding of
the tables (`round32`) -- the same accepted steps, and poses and scales within 4 x the distance measured on the MI355X
(pose_spec.MEASURED 'refine/*').  That comparison runs both with max_iter = STEPS = 4, and this is why.  Measured on the MI355X,
the cost after every iteration (kernel, then specification):
    1.26e+04  0.8802  0.003143  1.686e-06  4.672e-08 | 4.672e-08 x 7  4.651e-08 x 3  4.618e-08 x 15
    1.26e+04  0.8802  0.003142  1.636e-06  4.618e-09 | 4e-09 x 11  3.993e-09 x 15
Four steps of quadratic convergence take the cost from 1.3e4 to its rounding floor: r = proj - x' is a difference of two fp32
numbers of up to W = 40, half an ulp of which is 1.9e-6 px, and 21 000 observations of that make a cost of about 4e-8; the
specification's own floor, 4e-9, is the fp32 rounding of the tables it shares with the product.  Past the floor whether a step
lowers the cost is decided by those roundings, in both: left to run for 30 iterations (before the loop had its stop after five
rejected steps in a row) the kernel's loop accepted 6 steps and the specification's 12 (11 and 12 with scales), all but the
first four of them changes of the cost in its second or third digit.  So the number of accepted steps means something over the
first four iterations only, and there it is asserted: four of four in both, with the cost after each of them within 10 % of
the specification's (they differ by the floor: 2e-8, 3e-6, 8e-5 and 3e-2 relative).  The default run is held against the truth,
and must end by that stop, as converged.

Against the truth every frame ends within 1 % of the perturbation, 3e-4 in R and in c: a condition, not a measurement (the
float64 reference reaches 5e-9; fp32 tables and residuals cost about 3e-7 on top).
"""
import numpy as np
import pytest
import torch

import helpers
import pose_spec as S
import store_spec
import triangulate_spec as T

pytestmark = pytest.mark.gpu

DEV = 'cuda'
H, W, N, GAPS = 24, 40, 7, (1, 2, 3, 4)
STEPS = 4                                                  # iterations above the rounding floor of the cost (see above)


def _store(tmp, sc, poses, depth):
    from dvd_hip.datasets.frame_store import Catalogue, FrameStore
    rng = np.random.default_rng(5)
    tree = {'gaps': np.array(GAPS), 'fr_img': rng.random((N, H, W, 3)).astype(np.float32), 'fr_depth_pred': depth.astype(np.float32),
            'fr_depth_mvs': sc['depth'].astype(np.float32), 'fr_pose_c2w': poses.astype(np.float32), 'fr_intrinsics': sc['intrinsics'],
            'fl_ids': np.array(sc['pairs']), 'fl_flow_1_2': sc['flow_1_2'], 'fl_flow_2_1': sc['flow_2_1'], 'fl_mask_1': sc['mask_1'],
            'fl_mask_2': sc['mask_2']}
    store_spec.write_tree(str(tmp), tree)
    return FrameStore(Catalogue(str(tmp), store_spec.TRACK, list(GAPS), all_pairs=True), DEV)


def _spec_refine(c, store, depth, scales, anchor=0):
    base = {k: v.numpy() for k, v in store.host_tables.items()}
    start = np.tile(np.eye(4), (N, 1, 1))
    start[:, :3, :3], start[:, :3, 3] = base['R'], base['t']
    ev = S.evaluator(c.sc, depth.astype(np.float32), c.static, c.rows, round32=True, base=base)
    return S.refine(ev, start, c.rows, anchor=anchor, scales=scales, max_iter=STEPS)


class _Ctx(object):
    pass


@pytest.fixture(scope='module')
def ctx(tmp_path_factory):
    """The scene, its store with perturbed cameras, the default refinement, and the one of STEPS iterations with the
    specification's: computed once, shared."""
    from dvd_hip import preprocess
    c = _Ctx()
    c.sc = T.scene(H, W, N, seed=0, noise=0.0, gaps=GAPS)
    c.rows = S.plan(c.sc['pairs'])
    c.static = (~c.sc['disc']).astype(np.float32)
    c.true = c.sc['poses'].astype(np.float64)
    c.start = S.perturbed(c.sc)
    c.store = _store(tmp_path_factory.mktemp('refine'), c.sc, c.start, c.sc['depth'])
    assert c.store.cat.pairs == c.sc['pairs']
    c.weight = helpers.t(c.static, DEV)
    c.before = {k: v.clone() for k, v in c.store.tables.items()}
    c.ref = preprocess.refine_cameras(c.store, weight=c.weight)
    c.ref5 = preprocess.refine_cameras(c.store, weight=c.weight, max_iter=STEPS)
    c.spec = _spec_refine(c, c.store, c.sc['depth'], False)
    return c


def _against_spec(ref, spec, what):
    got = ref['poses'].numpy().astype(np.float64)
    eR, ec = S.pose_errors(got, spec['poses'].astype(np.float32))
    es = float(np.abs(ref['scales'].cpu().numpy().astype(np.float64) - np.exp(spec['sigma']).astype(np.float32)).max())
    print('%s: %d iterations, %d accepted (specification %d, %d); cost %.4g -> %.4g (specification %.4g)' % (
        what, ref['iterations'], ref['accepted'], spec['iterations'], spec['accepted'], ref['cost'][0], ref['cost'][-1], spec['cost'][-1]))
    print('%s: cost %s' % (what, ' '.join('%.4g' % v for v in ref['cost'])))
    print('%s: specification %s' % (what, ' '.join('%.4g' % v for v in spec['cost'])))
    failed = []
    for key, v in (('refine/R', eR), ('refine/c', ec), ('refine/scale', es)):
        bound = 4.0 * S.MEASURED[key]
        helpers.log_measured('%s/%s' % (what, key), v, bound)
        print('measured %s/%s %.4g (bound %.4g)' % (what, key, v, bound))
        if not v <= bound:
            failed.append((key, v, bound))
    assert ref['accepted'] == spec['accepted'] == STEPS and ref['iterations'] == spec['iterations'] == STEPS, (ref['accepted'], spec['accepted'])
    assert np.allclose(ref['cost'][:STEPS], spec['cost'][:STEPS], rtol=0.1, atol=0)             # (the one after them is the floor's)
    assert not failed, failed


def test_against_the_specification_and_the_truth(ctx):
    ref = ctx.ref
    assert ref['poses'].shape == (N, 4, 4) and ref['poses'].dtype == torch.float32 and not ref['poses'].is_cuda
    assert ref['scales'].is_cuda and torch.equal(ref['scales'], torch.ones(N, device=DEV))
    assert ref['rms_before'].shape == ref['rms_after'].shape == (36,) and ref['counts'].shape == (36, 2)
    assert np.array_equal(ref['rows'], ctx.rows) and len(ref['cost']) == ref['iterations'] + 1
    _against_spec(ctx.ref5, ctx.spec, 'refine_cameras')
    print('refine_cameras with the default max_iter: %d iterations, %d accepted, converged %s, cost %s' % (
        ref['iterations'], ref['accepted'], ref['converged'], ' '.join('%.4g' % v for v in ref['cost'])))
    assert np.array_equal(ref['cost'][:STEPS + 1], ctx.ref5['cost'])       # the same launches give the same bits
    eR, ec = S.pose_errors(ref['poses'].numpy(), ctx.true)
    e0 = S.pose_errors(ctx.start, ctx.true)
    print('refine_cameras: R %.3g -> %.3g, c %.3g -> %.3g of the truth' % (e0[0], eR, e0[1], ec))
    assert eR <= 3e-4 and ec <= 3e-4
    # convergence
    assert ref['cost'][-1] < 1e-6 * ref['cost'][0] and ref['converged'] and ref['iterations'] < 30
    print('rms per row: %.3g .. %.3g px before, %.3g .. %.3g after' % (ref['rms_before'].min(), ref['rms_before'].max(),
                                                                      ref['rms_after'].min(), ref['rms_after'].max()))
    assert (ref['rms_after'] < ref['rms_before']).all() and (ref['counts'][:, 1] == 0).all() and (ref['counts'][:, 0] > 300).all()


def test_depth_scales(ctx, tmp_path):
    from dvd_hip import preprocess
    s = S.depth_scales(ctx.sc)
    depth = (ctx.sc['depth'] / s[:, None, None]).astype(np.float32)
    store = _store(tmp_path, ctx.sc, ctx.start, depth)
    ref = preprocess.refine_cameras(store, weight=ctx.weight, scales=True, max_iter=STEPS)
    _against_spec(ref, _spec_refine(ctx, store, depth, True), 'refine_cameras/scales')
    eR, ec = S.pose_errors(ref['poses'].numpy(), ctx.true)
    es = float(np.abs(ref['scales'].cpu().numpy() / s - 1).max())
    print('refine_cameras/scales: R %.3g, c %.3g, scale %.3g of the truth' % (eR, ec, es))
    assert eR <= 3e-4 and ec <= 3e-4 and es <= 3e-4 and float(ref['scales'][0]) == 1.0
    assert ref['cost'][-1] < 1e-6 * ref['cost'][0]
    store.depth_pred.mul_(ref['scales'].view(-1, 1, 1, 1))                 # the documented way to apply them
    assert float((store.depth_pred[:, 0].cpu() / torch.from_numpy(ctx.sc['depth']).float() - 1).abs().max()) <= 3e-4


def test_the_result_installs(ctx, tmp_path):
    from dvd_hip import preprocess
    ref = ctx.ref
    static = helpers.t(~ctx.sc['disc'], DEV)
    epi = []
    for tables in (None, ref['tables']):
        tri = preprocess.triangulate_depth(ctx.store, tables=tables)
        use = static & (tri['epi'][:, 0] >= 0)
        epi.append(float(tri['epi'][:, 0][use].mean()))
    print('mean epipolar distance over the static pixels: %.4g px with the perturbed cameras, %.4g with the refined' % tuple(epi))
    assert epi[1] < 0.1 * epi[0]
    assert set(ref['tables']) == set(ctx.store.tables)
    store = _store(tmp_path, ctx.sc, ctx.start, ctx.sc['depth'])           # (its own store: set_cameras changes it)
    before = {k: v.clone() for k, v in store.tables.items()}
    store.set_cameras(ref['poses'])
    for k, v in store.tables.items():
        assert v.is_cuda and torch.equal(v, ref['tables'][k]) and torch.equal(store.host_tables[k], v.cpu()), k
    for k in ('ts_train', 'ts_vali', 'K_T', 'K_inv_T'):
        assert torch.equal(store.tables[k], before[k]), k
    assert torch.equal(store.tables['cam_c2w'].cpu(), ref['poses']) and not torch.equal(store.tables['R'], before['R'])
    assert torch.equal(store.tables['R_T'], store.tables['R'].transpose(1, 2))
    K = ctx.sc['intrinsics'] * np.float32(1.5)
    store.set_cameras(ref['poses'].numpy(), intrinsics=K)
    assert torch.equal(store.tables['K_T'].cpu(), torch.from_numpy(K).transpose(1, 2)) and torch.equal(store.tables['R'], ref['tables']['R'])
    for bad in (ref['poses'][:-1], np.full((N, 4, 4), np.nan, np.float32)):
        with pytest.raises(ValueError, match='poses'):
            store.set_cameras(bad)
    with pytest.raises(ValueError, match='intrinsics'):
        store.set_cameras(ref['poses'], intrinsics=K[:-1])
    for k, v in ctx.before.items():                                        # refine_cameras itself left the shared store alone
        assert torch.equal(ctx.store.tables[k], v), k


def test_anchor_gaps_and_tables(ctx):
    from dvd_hip import preprocess
    ref = preprocess.refine_cameras(ctx.store, weight=ctx.weight, anchor=3, gaps=[1, 2], max_iter=12)
    start = ctx.store.host_tables['cam_c2w']
    assert torch.equal(ref['poses'][3], start[3]) and not torch.equal(ref['poses'][0], start[0])
    assert torch.equal(ref['tables']['R'][3], ctx.store.tables['R'][3]) and torch.equal(ref['tables']['t'][3], ctx.store.tables['t'][3])
    assert len(ref['rows']) == 2 * (6 + 5) and ref['cost'][-1] < 1e-6 * ref['cost'][0]
    assert torch.equal(ctx.ref['poses'][0], start[0])                      # (and the default anchor in the shared run)
    # started from the refined tables there is nothing left to do
    again = preprocess.refine_cameras(ctx.store, weight=ctx.weight, tables=ctx.ref['tables'], max_iter=3)
    assert again['cost'][0] == ctx.ref['cost'][-1]
    eR, ec = S.pose_errors(again['poses'].numpy(), ctx.true)
    assert eR <= 3e-4 and ec <= 3e-4
    with pytest.raises(ValueError, match='no row'):
        preprocess.refine_cameras(ctx.store, weight=ctx.weight, gaps=[9])
    with pytest.raises(RuntimeError, match='weight'):
        preprocess.refine_cameras(ctx.store, weight=ctx.weight.cpu())
