"""Model.track_points / Model.score_tracks on the GPU (dvd_hip/models/point_tracks.py).

The video, cameras, depth and network are those of tests/test_45_tracks_gpu.py: the 7-frame, 11 x 21 fixture
tests/golden/tracks_b3_11x21_t4.npz in a FrameStore, and that file's float64 pipeline and fixture distances as the yardstick of
what fp32 can do on these inputs.

Exact: integer queries on the frames 0, 3, 5 against Model.track(.., n_back=2) at those pixels, every output row, bit for bit
(the MLP's result for a point does not depend on its place in a launch); any `chunk`; the flags of the sub-pixel queries under
the rule of tests/point_tracks_spec.py (flag_skip: at most 0.5 % left out, no mismatch among the rest); score_tracks against
closed-form counts and against the float32 mirror run on the returned predictions; two runs.

Tolerances: sub-pixel queries, forward, against the float64 pipeline (spec seed -> tracks_spec.integrate on
a [1,3,1,Q] slab -> spec project): the worst distance measured on the MI355X, x 4; the measured value must stay below 4 x the
distance of fp32 torch (the seed: grid_sample + matmuls) or of the reference's own fp32 results (the fixture; the chain) from the
specification.
                        seed points   points - points[0]   uv        z         depth_at
    kernels, measured   7.5e-7        5.9e-7               3.6e-6    1.1e-6    8.6e-6
    reference (fp32)    3.1e-6        6.2e-7               4.0e-6    1.1e-6    1.1e-5     (its limit is 4 x this)
"""
import numpy as np
import pytest
import torch

import helpers
import point_tracks_spec as PS
import test_45_tracks_gpu as T45
import tracks_spec as S

pytestmark = pytest.mark.gpu

DEV = 'cuda'
Z_TOL = 0.05
KEYS = ('uv', 'z', 'depth_at', 'inside', 'visible', 'target')
# worst distance from the float64 pipeline measured on the MI355X; the bound is 4 x this
MEASURED = {'seed': 7.54e-7, 'points': 5.92e-7, 'uv': 3.57e-6, 'z': 1.10e-6, 'depth_at': 8.64e-6}


def _check(name, measured, ref_limit):
    bound = 4.0 * MEASURED[name]
    helpers.log_measured('track_points/' + name, measured, bound)
    print('measured track_points/%s %.4g (bound %.4g, reference limit %.4g)' % (name, measured, bound, ref_limit))
    assert measured <= ref_limit, (name, measured, ref_limit)
    assert measured <= bound, (name, measured, bound)


@pytest.fixture(scope='module')
def ctx(tmp_path_factory):
    """The fixture's store, model and depth as test_45 builds them, and the sub-pixel queries with ONE run of them."""
    import store_spec
    c = T45._Ctx()
    fx = c.fx = helpers.load_golden(T45.FX)
    c.N, c.H, c.W = int(fx['N']), int(fx['H']), int(fx['W'])
    tree = store_spec.random_tree(c.N, c.H, c.W, [1], 5)
    tree['fr_pose_c2w'], tree['fr_intrinsics'] = fx['in_pose_c2w'], fx['in_intrinsics']
    c.store = T45._store(str(tmp_path_factory.mktemp('point_tracks')), tree)
    c.model = T45._model(int(fx['seed']))
    c.depth = helpers.t(fx['in_depth'], DEV)
    c.host = {k: fx['tab_' + k] for k in ('R_T', 'R', 't', 'K_T', 'K_inv_T', 'ts_vali')}
    c.queries = PS.model_queries(c.N, c.H, c.W, 257)
    c.out = c.model.track_points(c.store, c.queries, n_steps=4, n_back=2, depth=c.depth)
    torch.cuda.synchronize()
    return c


def test_integer_queries_are_the_pixels_of_track(ctx):
    c, start = ctx, [0, 3, 5]
    dense = c.model.track(c.store, start, 4, depth=c.depth, n_back=2)
    yy, xx = np.meshgrid(np.arange(c.H), np.arange(c.W), indexing='ij')
    queries = np.concatenate([np.stack([np.full(c.H * c.W, f), xx.ravel(), yy.ravel()], 1) for f in start], 0).astype(np.float64)
    out = c.model.track_points(c.store, queries, n_steps=4, n_back=2, depth=c.depth)
    T1, Q = 7, 3 * c.H * c.W
    assert out['origin'] == 2 and out['points'].shape == (T1, 3, Q) and out['resid'].shape == (2,) and bool(out['ok'].all())
    assert set(out) == set(KEYS) | {'points', 'ok', 'origin', 'resid'}
    frame = torch.from_numpy(queries[:, 0].astype(np.int64)).to(DEV)
    g = frame[None, :] + torch.arange(T1, device=DEV)[:, None] - 2
    live = (g >= 0) & (g < c.N)
    assert torch.equal(out['target'], torch.where(live, g, torch.full_like(g, -1)).int())
    want = dense['points'].permute(0, 2, 1, 3, 4).reshape(T1, 3, Q)
    lp = live[:, None, :].expand(T1, 3, Q)
    assert torch.equal(out['points'][lp], want[lp])                       # (track leaves the rows without a frame zero)
    for k in ('uv', 'z', 'depth_at', 'inside'):
        assert torch.equal(out[k], dense[k].reshape((T1, Q) + tuple(dense[k].shape[4:]))), k
    tol = torch.tensor(1.0, device=DEV) + torch.tensor(Z_TOL, device=DEV)
    assert torch.equal(out['visible'], (out['inside'].bool() & ~(out['z'] > out['depth_at'] * tol)).to(torch.uint8))
    # (every query takes every backward step, frame 0's too, which track does not integrate: the residual can only be larger)
    assert bool((out['resid'] >= dense['resid'].max(1).values).all()) and bool(torch.isfinite(out['resid']).all())


def test_every_chunk_gives_the_same_bits(ctx):
    c = ctx
    for chunk in (100, 256, 1000):
        other = c.model.track_points(c.store, c.queries, n_steps=4, n_back=2, depth=c.depth, chunk=chunk)
        assert set(other) == set(c.out)
        for k, v in c.out.items():
            assert (other[k] == v) if k == 'origin' else torch.equal(other[k], v), (chunk, k)
    with pytest.raises(ValueError, match='chunk'):
        c.model.track_points(c.store, c.queries, depth=c.depth, chunk=0)
    with pytest.raises(ValueError, match='depth'):
        c.model.track_points(c.store, c.queries, depth=c.depth[:3])
    # the defaults cover the whole video on both sides of every query
    whole = c.model.track_points(c.store, c.queries, depth=c.depth)
    f = c.queries[:, 0]
    assert whole['origin'] == int(f.max()) and whole['points'].shape[0] == int(f.max()) + 1 + c.N - 1 - int(f.min())
    assert bool(((whole['target'] >= 0).sum(0) == c.N).all())


def test_subpixel_queries_against_the_float64_pipeline(ctx):
    c, fx = ctx, ctx.fx
    out = c.model.track_points(c.store, c.queries, n_steps=4, n_back=0, depth=c.depth)
    got = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in out.items()}
    assert got['origin'] == 0 and got['resid'].shape == (0,)
    assert torch.equal(out['points'], c.out['points'][2:]) and torch.equal(out['uv'], c.out['uv'][2:])
    sd = {k: v.detach().cpu() for k, v in c.model.net_sceneflow.state_dict().items()}
    pipe = PS.pipeline(sd, c.host, fx['in_depth'], c.queries, 4)
    assert bool(pipe['ok'].all()) and bool(got['ok'].all())
    live = pipe['target'] >= 0
    assert torch.equal(got['target'].long(), pipe['target'])
    skip, frac = PS.flag_skip(pipe, fx['in_depth'], Z_TOL)
    bad = sum(int(((got[k].bool() != pipe[k]) & ~skip).sum()) for k in ('inside', 'visible'))
    print('flags: %d mismatches, %.3f %% of the live rows left out' % (bad, 100 * frac))
    assert frac <= 0.005 and bad == 0
    for k in KEYS:
        assert not bool(got[k][~live].ne(-1 if k == 'target' else 0).any()), k
    # the yardstick: the reference's own fp32 results for the dense tracks of the fixture against ITS float64 pipeline
    d_ref = T45._distances(T45._fixture_outputs(fx), T45._pipeline(c.model.net_sceneflow, fx, time_dependent=True))
    frame, xy = c.queries[:, 0].astype(np.int64), c.queries[:, 1:].astype(np.float32)
    seed_ref = S.worst(PS.seed_fp32(frame, xy, fx['in_depth'], c.host['R_T'], c.host['t'], c.host['K_inv_T']), pipe['points'][0])
    pts = got['points'].double()
    T1, Q = live.shape
    _check('seed', S.worst(pts[0], pipe['points'][0]), 4 * seed_ref)
    _check('points', S.worst((pts - pts[0])[1:], (pipe['points'] - pipe['points'][0])[1:]), 4 * d_ref['points'])
    _check('uv', S.worst(got['uv'], pipe['uv'], live[..., None].expand(T1, Q, 2)), 4 * d_ref['uv'])
    _check('z', S.worst(got['z'], pipe['z'], live), 4 * d_ref['z'])
    _check('depth_at', S.worst(got['depth_at'], pipe['depth_at'], live & (pipe['z'] > 0)), 4 * d_ref['depth_at'])


SHIFTS = (0.5, 1.5, 3.0, 6.0, 12.0, 24.0)


def _made_up_ground_truth(tr, N):
    """The model's own tracks shifted by SHIFTS px in equal sixths of the annotated-visible rows; every 9th scorable row is
    annotated occluded, every 13th not annotated.  -> gt_uv [Q,N,2], gt_state [Q,N], the expected counts."""
    uv, vis, target = tr['uv'].cpu().numpy(), tr['visible'].cpu().numpy() != 0, tr['target'].cpu().numpy()
    T1, Q = target.shape
    gt_uv, gt_state = np.zeros((Q, N, 2), np.float32), np.full((Q, N), 2, np.uint8)
    cells = [(j, q) for j in range(T1) for q in range(Q)
             if target[j, q] >= 0 and j != tr['origin'] and np.all(np.abs(uv[j, q]) < 1000)]
    occ = [c for i, c in enumerate(cells) if i % 9 == 0]
    seen = [c for i, c in enumerate(cells) if i % 9 and i % 13]
    seen = seen[:len(seen) - len(seen) % 6]
    want = {'n_eval': len(occ) + len(seen), 'n_vis': len(seen), 'agree': 0, 'tp': [0] * 5, 'fp': [0] * 5,
            'by_row': np.zeros(T1, int)}
    for j, q in occ:
        gt_uv[q, target[j, q]], gt_state[q, target[j, q]] = uv[j, q], 1
        want['agree'] += not vis[j, q]
        want['by_row'][j] += 1
        for i in range(5):
            want['fp'][i] += bool(vis[j, q])
    for k, (j, q) in enumerate(seen):
        gt_uv[q, target[j, q]] = uv[j, q] + np.float32([SHIFTS[k % 6], 0.0])
        gt_state[q, target[j, q]] = 0
        want['agree'] += bool(vis[j, q])
        want['by_row'][j] += 1
        for i in range(5):
            within = k % 6 <= i
            want['tp'][i] += bool(within and vis[j, q])
            want['fp'][i] += bool(vis[j, q] and not within)
    return gt_uv, gt_state, want


def test_score_tracks_with_a_made_up_ground_truth(ctx):
    c = ctx
    gt_uv, gt_state, want = _made_up_ground_truth(c.out, c.N)
    assert want['n_vis'] > 300 and want['n_eval'] > want['n_vis'] and 0 < want['tp'][0] < want['tp'][4] and min(want['fp']) > 0
    args = dict(n_steps=4, n_back=2, depth=c.depth)
    res = c.model.score_tracks(c.store, c.queries, gt_uv, gt_state, **args)
    for k in c.out:
        assert (res['tracks'][k] == c.out[k]) if k == 'origin' else torch.equal(res['tracks'][k], c.out[k]), k
    f64 = lambda a, b: float(np.float64(a) / np.float64(b))
    assert int(res['n_eval']) == want['n_eval'] and int(res['n_gt_visible']) == want['n_vis']
    assert res['pts_within'].tolist() == [(i + 1) / 6.0 for i in range(5)]
    assert float(res['occlusion_accuracy']) == f64(want['agree'], want['n_eval'])
    assert res['jaccard'].tolist() == [f64(want['tp'][i], want['n_vis'] + want['fp'][i]) for i in range(5)]
    assert float(res['average_pts_within']) == float(res['pts_within'].mean())
    assert float(res['average_jaccard']) == float(res['jaccard'].mean())
    # the mean error: the six shifts in equal parts; a term is off by at most half an ulp of |u| + 24 < 1024 (3.1e-5) from
    # forming u + shift in fp32, plus 2^-33 from the quantisation
    assert abs(float(res['mean_err']) - sum(SHIFTS) / 6.0) <= 4e-5
    # per temporal distance: the rows pool to the totals, the origin row is empty
    by = res['by_offset']
    assert res['sums'].shape == (7, 19) and by['n_eval'].tolist() == want['by_row'].tolist() and by['n_eval'][2] == 0
    assert bool(torch.isnan(by['occlusion_accuracy'][2])) and by['pts_within'].shape == (7, 5)
    assert int(by['n_eval'].sum()) == want['n_eval']
    sums = res['sums'].cpu().numpy()
    assert sums.sum(0)[3:8].tolist() == [want['n_vis'] * (i + 1) // 6 for i in range(5)]
    assert sums.sum(0)[8:13].tolist() == want['tp'] and sums.sum(0)[13:18].tolist() == want['fp']
    # ... and everything equals the mirror run on the returned predictions
    tr = {k: res['tracks'][k].cpu().numpy() for k in ('uv', 'visible', 'target')}
    assert res['shift'] == PS.eval_shift(len(c.queries))
    assert (sums == PS.score_mirror(tr['uv'], tr['visible'], tr['target'], 2, gt_uv, gt_state)).all()
    # a benchmark's raster, device tensors for the ground truth, and a second run
    sx, sy = 256.0 / c.W, 256.0 / c.H
    scaled = c.model.score_tracks(c.store, c.queries, helpers.t(gt_uv, DEV), helpers.t(gt_state, DEV), px_scale=(sx, sy), **args)
    assert (scaled['sums'].cpu().numpy() == PS.score_mirror(tr['uv'], tr['visible'], tr['target'], 2, gt_uv, gt_state,
                                                            sx=sx, sy=sy)).all()
    assert not torch.equal(scaled['sums'], res['sums'])
    again = c.model.score_tracks(c.store, c.queries, gt_uv, gt_state, **args)
    assert torch.equal(again['sums'], res['sums'])
    # "query first": n_back = 0 evaluates later frames only
    first = c.model.score_tracks(c.store, c.queries, gt_uv, gt_state, n_steps=4, n_back=0, depth=c.depth)
    assert first['tracks']['origin'] == 0 and first['sums'].shape == (5, 19)
    assert torch.equal(first['sums'][1:], res['sums'][3:]) and not bool(first['sums'][0].any())
    assert int(first['n_eval']) == int(want['by_row'][3:].sum())


def test_refusals(ctx):
    c = ctx
    gt_uv, gt_state = np.zeros((257, c.N, 2), np.float32), np.zeros((257, c.N), np.uint8)
    for bad_uv, bad_state in ((gt_uv[:256], gt_state), (gt_uv, gt_state[:, :6]), (gt_uv[..., :1], gt_state),
                              (gt_uv.transpose(1, 0, 2), gt_state.T)):
        with pytest.raises(ValueError, match='gt_uv'):
            c.model.score_tracks(c.store, c.queries, bad_uv, bad_state, depth=c.depth)
    with pytest.raises(ValueError, match='gt_state'):
        c.model.score_tracks(c.store, c.queries, gt_uv, gt_state.astype(np.float32), depth=c.depth)
    with pytest.raises(RuntimeError, match='thresholds'):
        c.model.score_tracks(c.store, c.queries, gt_uv, gt_state, thresholds=(1, 2), depth=c.depth)
    with pytest.raises(ValueError, match='frames'):
        c.model.track_points(c.store, [[7, 1, 1]], depth=c.depth)
    with pytest.raises(ValueError, match='positions'):
        c.model.track_points(c.store, [[0, 20.5, 1]], depth=c.depth)
    model = T45._model(3, use_cnn=True)
    with pytest.raises(NotImplementedError, match='use_cnn'):
        model.track_points(c.store, c.queries, depth=c.depth)
    with pytest.raises(NotImplementedError, match='use_cnn'):
        model.score_tracks(c.store, c.queries, gt_uv, gt_state, depth=c.depth)
