"""preprocess.triangulate_depth on a FrameStore (dvd_hip/preprocess.py, csrc/triangulate.hip).

The store is built the way tests/test_60_filter_depth_gpu.py builds its own -- a tree of frame and flow files written by
tests/store_spec.py, read back by Catalogue / FrameStore -- from triangulate_spec.scene(24, 40, 7): every pair of gaps 1 to 4,
flows with 0.4 px of noise, consistency masks.  The frames' depth_pred is the scene's true depth times SCALE.

Exact: triangulate_depth is the specification's pipeline over triangulate_plan's table, bit for bit; any `chunk` gives the same
bits; tables at half scale halve the depth.  Against the float64 reference the tolerances are those of
tests/test_61_triangulate_kernel_gpu.py (MEASURED there, 4 x the measured distance).
"""
import numpy as np
import pytest
import torch

import helpers
import store_spec
import triangulate_spec as T

pytestmark = pytest.mark.gpu

DEV = 'cuda'
KEYS = ('depth', 'count', 'usable', 'epi', 'spread')
H, W, N, GAPS = 24, 40, 7, (1, 2, 3, 4)
MEASURED = T.MEASURED
SCALE = 4.0                                                # a power of two: scaling by it commutes with every rounding


def _tree(sc, seed=5):
    rng = np.random.default_rng(seed)
    return {'gaps': np.array(GAPS), 'fr_img': rng.random((N, H, W, 3)).astype(np.float32),
            'fr_depth_pred': (sc['depth'].astype(np.float32) * np.float32(SCALE)), 'fr_depth_mvs': sc['depth'].astype(np.float32),
            'fr_pose_c2w': sc['poses'], 'fr_intrinsics': sc['intrinsics'], 'fl_ids': np.array(sc['pairs']),
            'fl_flow_1_2': sc['flow_1_2'], 'fl_flow_2_1': sc['flow_2_1'], 'fl_mask_1': sc['mask_1'], 'fl_mask_2': sc['mask_2']}


def _store(tmp, sc):
    from dvd_hip.datasets.frame_store import Catalogue, FrameStore
    store_spec.write_tree(str(tmp), _tree(sc))
    return FrameStore(Catalogue(str(tmp), store_spec.TRACK, list(GAPS), all_pairs=True), DEV)


def _spec(sc, store, frames, gaps=None, mode='median', dtype=np.float32, tables=None, **params):
    tab = {k: v.numpy() for k, v in store.host_tables.items()} if tables is None else tables
    return T.pipeline(sc['flow_1_2'], sc['flow_2_1'], sc['mask_1'], sc['mask_2'], T.plan(sc['pairs'], frames, gaps), frames, tab, mode,
                      dtype, **params)


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want, what=''):
    for k in KEYS:
        assert tuple(got[k].shape) == tuple(want[k].shape), (what, k)
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, k)


class _Ctx(object):
    pass


@pytest.fixture(scope='module')
def ctx(tmp_path_factory):
    """The noisy scene, its store and ONE run per mode: computed once, shared, never written to."""
    from dvd_hip import preprocess
    c = _Ctx()
    c.sc = T.scene(H, W, N, seed=0, noise=0.4, gaps=GAPS)
    c.store = _store(tmp_path_factory.mktemp('triangulate'), c.sc)
    assert c.store.cat.pairs == c.sc['pairs']
    c.out = {mode: preprocess.triangulate_depth(c.store, mode=mode) for mode in ('median', 'mean')}
    torch.cuda.synchronize()
    return c


def test_it_is_the_specifications_pipeline(ctx):
    for mode, out in ctx.out.items():
        assert set(out) == set(KEYS) | {'frames', 'static', 'moving'}
        assert out['depth'].shape == out['epi'].shape == out['spread'].shape == (N, 1, H, W) and out['depth'].is_cuda
        assert out['count'].dtype == out['usable'].dtype == torch.uint8 and out['static'].dtype == out['moving'].dtype == torch.bool
        assert out['frames'].tolist() == list(range(N)) and out['static'].shape == out['moving'].shape == (N, H, W)
        _same(out, _spec(ctx.sc, ctx.store, range(N), mode=mode), what=mode)
        assert torch.equal(out['static'], out['count'] >= 2)
        assert torch.equal(out['moving'], (out['usable'] >= 2) & (out['count'] == 0))
        assert torch.isfinite(out['depth']).all() and torch.isfinite(out['epi']).all() and torch.isfinite(out['spread']).all()
    assert float(ctx.out['median']['static'].float().mean()) > 0.7
    assert not torch.equal(ctx.out['median']['depth'], ctx.out['mean']['depth'])
    assert not ctx.out['median']['depth'].requires_grad


def test_chunks_frames_gaps_and_parameters(ctx):
    from dvd_hip import preprocess
    for chunk in (1, 3):
        for mode in ('median', 'mean'):
            _same(preprocess.triangulate_depth(ctx.store, mode=mode, chunk=chunk), ctx.out[mode], what=(mode, chunk))
    for frames in ([0], [N - 1], [5, 2, 2]):
        got = preprocess.triangulate_depth(ctx.store, frames=frames, chunk=2)
        assert got['frames'].tolist() == frames
        _same(got, {k: ctx.out['median'][k][frames] for k in KEYS}, what=frames)
    got = preprocess.triangulate_depth(ctx.store, gaps=[2, 4], mode='mean', epi_tol=0.7, min_parallax_deg=1.0, z_near=0.5, min_count=3)
    sin2 = float(np.float32(np.sin(np.radians(1.0)) ** 2))
    _same(got, _spec(ctx.sc, ctx.store, range(N), gaps=(2, 4), mode='mean', epi_tol=0.7, sin2_min=sin2, z_near=0.5, min_count=3), what='gaps')
    assert torch.equal(got['static'], got['count'] >= 3) and int(got['usable'].max()) == 3
    for kw in (dict(chunk=0), dict(chunk=1.5), dict(min_parallax_deg=0), dict(min_parallax_deg=91), dict(frames=[N]), dict(gaps=[0])):
        with pytest.raises(ValueError, match='triangulate_depth|triangulate_plan'):
            preprocess.triangulate_depth(ctx.store, **kw)
    with pytest.raises(RuntimeError, match='mode'):
        preprocess.triangulate_depth(ctx.store, mode='max')


def test_the_wrapper_refuses_what_needs_a_device_to_tell(ctx):
    from dvd_hip import ops
    s = ctx.store
    obs, fr = T.plan(ctx.sc['pairs'], [3]), [3]
    good = dict(flow_1_2=s.flow_1_2, flow_2_1=s.flow_2_1, mask_1=s.mask_1, mask_2=s.mask_2, obs=obs, frames=fr, tables=s.tables)
    bad_pair, bad_frame, bad_dir = obs.copy(), obs.copy(), obs.copy()
    bad_pair[0, 0, 0], bad_frame[0, 1, 1], bad_dir[0, 2, 2] = len(ctx.sc['pairs']), N, 2
    for kw, word in ((dict(obs=bad_pair), 'obs names pairs'), (dict(obs=bad_frame), 'obs names frames'), (dict(obs=bad_dir), 'dir column of obs'),
                     (dict(frames=[N]), 'frames span'), (dict(flow_2_1=s.flow_2_1[:-1]), 'flow_2_1'), (dict(flow_2_1=s.flow_2_1.cpu()), 'flow_2_1'),
                     (dict(flow_1_2=s.flow_1_2.transpose(1, 2)), 'flow_1_2'), (dict(mask_1=s.mask_1.float()), 'mask_1'), (dict(mask_1=None), 'mask_1'), (dict(mask_2=None), 'mask_2'),
                     (dict(mask_2=s.mask_2[:, :, ::2]), 'mask_2'), (dict(tables={k: v for k, v in s.tables.items() if k != 'K_inv_T'}), 'K_inv_T'),
                     (dict(tables=dict(s.tables, t=s.tables['t'][:-1])), 'table t'), (dict(tables=dict(s.tables, R=s.tables['R'].cpu())), 'table R'),
                     (dict(out={'depth': torch.empty(1, H, W, device=DEV)}), r"out\['depth'\]"),
                     (dict(out={'count': torch.empty(1, H, W, device=DEV)}), r"out\['count'\]")):
        with pytest.raises(RuntimeError, match=word):
            ops.triangulate(**dict(good, **kw))
    out = {k: torch.empty((1, 1, H, W) if chan else (1, H, W), device=DEV, dtype=dt) for k, dt, chan in ops.TRI_OUT}
    res = ops.triangulate(out=out, **good)
    assert all(res[k] is out[k] for k in KEYS)
    _same(res, {k: ctx.out['median'][k][3:4] for k in KEYS}, what='out')


def test_tables_at_half_scale_halve_the_depth(ctx):
    from dvd_hip import preprocess
    half = dict(ctx.store.tables, t=ctx.store.tables['t'] * 0.5)
    for mode in ('median', 'mean'):
        got = preprocess.triangulate_depth(ctx.store, mode=mode, tables=half)
        assert torch.equal(got['depth'], ctx.out[mode]['depth'] * 0.5) and float(got['depth'].max()) > 1.0
        for k in ('count', 'usable', 'epi', 'spread', 'static', 'moving'):
            assert torch.equal(got[k], ctx.out[mode][k]), (mode, k)


def test_static_and_moving_against_the_float64_reference(ctx):
    for mode in ('median', 'mean'):
        ref = _spec(ctx.sc, ctx.store, range(N), mode=mode, dtype=np.float64)
        ok = ref['decided']
        assert float((~ok).mean()) <= 0.01
        out = {k: v.cpu().numpy() for k, v in ctx.out[mode].items() if k != 'frames'}
        assert np.array_equal(out['static'][ok], (ref['count'] >= 2)[ok])
        assert np.array_equal(out['moving'][ok], ((ref['usable'] >= 2) & (ref['count'] == 0))[ok])
        m = T.against_reference(out, ref)
        assert m['counts_equal'] and m['depth'] <= 4 * MEASURED[mode + '/depth'] and m['epi'] <= 4 * MEASURED[mode + '/epi'], m
    # the cue finds the disc and leaves the static scene alone (the noise is 0.4 px, the disc's epipolar distance 2.5 px per frame)
    moving, disc = ctx.out['median']['moving'].cpu().numpy(), ctx.sc['disc']
    assert moving[disc].mean() > 0.7 and moving[~disc].mean() < 0.01


def test_calibrate_scale_returns_the_scale_of_the_scene(ctx, tmp_path):
    """depth_pred = SCALE x the true depth, a power of two, so calibrate_scale(depth_pred, tri) is SCALE x
    calibrate_scale(true depth, tri) exactly; and with flows free of noise the triangulated depth is the true one up to fp32's
    error of s1, so that factor is 1 within the tolerance of the depth comparison (4 x MEASURED)."""
    from dvd_hip import preprocess
    sc = T.scene(H, W, N, seed=0, noise=0.0, gaps=GAPS)
    store = _store(tmp_path, sc)
    tri = preprocess.triangulate_depth(store)
    scales, s = preprocess.calibrate_scale(store.depth_pred, tri['depth'])
    ones, one = preprocess.calibrate_scale(store.depth_mvs, tri['depth'])
    assert torch.equal(scales, ones * SCALE) and s == one * np.float32(SCALE)
    tol = 4 * MEASURED['median/depth']
    print('calibrate_scale: s / SCALE - 1 = %.3g per frame at most, %.3g in the mean (tolerance %.3g)' % (
        float((scales / SCALE - 1).abs().max()), abs(float(s) / SCALE - 1), tol))
    assert float((scales / SCALE - 1).abs().max()) <= tol and abs(float(s) / SCALE - 1) <= tol
    # ... and against the true depth itself, on the pixels the triangulation vouches for
    true = helpers.t(sc['depth'].astype(np.float32), DEV)[:, None]
    static = tri['static'] & ~helpers.t(sc['disc'], DEV)
    assert float(static.float().mean()) > 0.7
    assert float((tri['depth'] / true - 1).abs()[static[:, None]].max()) <= tol


def test_score_depth_takes_the_triangulated_depth_as_ground_truth(ctx):
    """Model.score_depth(store, gt=tri['depth'], mask=tri['static']) with the depth given (no network runs): finite metrics, and
    a prediction that is SCALE x the truth is brought back to the triangulation's scale by the median alignment."""
    from dvd_hip.models.scene_flow_motion_field import Model
    tri = ctx.out['median']
    out = Model.score_depth(None, ctx.store, depth=ctx.store.depth_pred, gt=tri['depth'], mask=tri['static'])
    video = {k: v.cpu().numpy() for k, v in out['video'].items()}
    assert int(video['n'][0]) == int(tri['static'].sum())
    for k in ('abs_rel', 'sq_rel', 'rmse', 'rmse_log', 'd1'):
        assert np.isfinite(video[k][0]), k
    # (0.4 px of noise on 1.2 px of parallax per frame of gap: the fp32 contract gives abs_rel 0.09, d1 0.93, median ratio 0.96)
    assert abs(float(out['scale'][0]) * SCALE - 1) < 0.1 and video['abs_rel'][0] < 0.2 and video['d1'][0] > 0.85
