"""dvd_track_filter through ops.track_filter on the GPU (csrc/track_filter.hip).

The test makes its slabs and tables itself: the poses of tests/golden/tracks_b3_11x21_t4.npz (repeated where a case needs more
than its 7 frames), intrinsics for the case's image size, a depth video S(x, y) c_g with 3 % noise and an occluder, and seeded
points near that surface -- the start frame's own un-projection, pushed off by a random walk that grows with the row distance.

Exact: the expected value is filter_spec.fuse(dtype=np.float32) applied on the CPU to what ops.track_project(k0=..) returns for
the same slab.  depth, ratio, spread and count must match it bit for bit, in both modes, on the scalar and the 16-byte path,
for rows before frame 0 and past the last frame, at the cap of 33 rows and for a single row.

Tolerance of the static-camera property (the rule of tests/test_57_track_back_gpu.py): with one camera,
still points and depth_g = S c_g every frame must become S mean(c).  The distance max |depth / (S mean(c)) - 1| must stay below
4 x the distance of the specification's own fp32 form and below 4 x the value measured on the MI355X (MEASURED).  The image's
border pixels project ONTO the image edge, where `inside` hangs on the last bit (tracks_spec.compare_inside leaves them out for
the same reason); the property is asserted on the others.
    kernels, measured   mean 1.85e-7   median 1.80e-7      fp32 form   mean 1.85e-7   median 1.80e-7   (its limit is 4 x this)
"""
import numpy as np
import pytest
import torch

import filter_cases as C
import filter_spec as F
import helpers
import invert_spec as I
import tracks_spec as S

pytestmark = pytest.mark.gpu

DEV = 'cuda'
# worst distance of the static-camera result from S mean(c) measured on the MI355X; the bound is 4 x this
MEASURED = {'static/mean': 1.85e-7, 'static/median': 1.80e-7}

#        H   W   T1  k0   starts        N
CASES = {
    'scalar_one_block': (11, 21, 7, -3, [1, 3, 6], 7),            # rows before frame 0 and past the end
    'scalar_two_blocks': (11, 27, 5, -2, [0, 4, 6], 7),           # 297 pixels: a block and a tail
    'vector_two_blocks': (28, 40, 9, -4, [2, 5], 7),              # 1120 pixels: a block of 1024 (mean) and a tail; 5 of 256 (median)
    'vector_small': (12, 24, 9, -4, [3, 6], 7),
    'cap': (6, 8, 33, -16, [17, 3], 35),
    'single_row': (6, 8, 1, 0, [2, 0], 7),
    'one_sided': (6, 8, 4, 0, [1, 5], 7),                         # the start frame in the first row
}


def _bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _tables(fx, N, H, W):
    """fp32 tables for N frames at H x W: the fixture's poses, repeated, and a pinhole camera for the image size."""
    idx = np.arange(N) % int(fx['N'])
    K = np.array([[0.9 * W, 0.0, (W - 1) / 2.0], [0.0, 0.9 * W, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
    rep = lambda m: np.ascontiguousarray(np.broadcast_to(m.astype(np.float32), (N,) + m.shape))
    return {'R': fx['tab_R'][idx], 'R_T': fx['tab_R_T'][idx], 't': fx['tab_t'][idx], 'K_T': rep(K.T), 'K_inv_T': rep(np.linalg.inv(K).T)}


def _make(name, seed=0):
    H, W, T1, k0, starts, N = CASES[name]
    fx = helpers.load_golden(C.FX)
    rng = np.random.RandomState(100 + seed + H * W + T1)
    tabs = _tables(fx, N, H, W)
    depth, _, _ = C.static_video(N, H, W)
    depth = depth * (1.0 + 0.03 * rng.uniform(-1, 1, depth.shape)).astype(np.float32)
    depth[1::3, :, H // 3:H // 2, W // 4:W // 2] *= 0.6            # an occluder in every third frame
    depth = depth.astype(np.float32)
    B, o = len(starts), -k0
    p0 = S.unproject(depth[starts], tabs['R_T'][starts], tabs['t'][starts], tabs['K_inv_T'][starts]).numpy()
    pts = np.zeros((T1, B, 3, H, W))
    for k in range(T1):
        pts[k] = p0 + 0.02 * np.sqrt(abs(k - o)) * rng.normal(size=p0.shape)
    return dict(name=name, H=H, W=W, T1=T1, k0=k0, starts=starts, N=N, B=B, tabs=tabs, depth=depth, points=pts.astype(np.float32),
                weights=np.exp(-0.5 * ((np.arange(T1) + k0) / max(1.0, T1 / 4.0)) ** 2).astype(np.float32))


def _dev(c):
    return (helpers.t(c['points'], DEV), {k: helpers.t(c['tabs'][k], DEV) for k in ('R', 't', 'K_T')}, helpers.t(c['depth'], DEV))


def _expected(c, points, tabs, depth, mode, weights=None, tol=C.TOL, z_near=C.Z_NEAR, planar=True):
    """filter_spec.fuse in fp32 on the rows dvd_track_project_from writes for the same slab."""
    from dvd_hip import ops
    rows = ops.track_project(points, c['starts'], tabs, depth_all=depth, k0=c['k0'], planar=planar)
    exist = np.array([[0 <= s + k + c['k0'] < c['N'] for s in c['starts']] for k in range(c['T1'])])
    return F.fuse(rows['z'].cpu().numpy(), rows['depth_at'].cpu().numpy(), rows['inside'].cpu().numpy(), depth.cpu().numpy()[c['starts']],
                  exist, c['weights'] if weights is None else weights, -c['k0'], mode, tol, z_near, np.float32)


def _same(got, want, keys=('depth', 'ratio', 'spread', 'count'), what=''):
    for k in keys:
        g, w = _bits(got[k]), _bits(want[k])
        assert g.shape == w.shape and np.array_equal(g, w), (what, k, int((g != w).sum()))


@pytest.mark.parametrize('mode', ['mean', 'median'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_bit_for_bit_against_the_fp32_specification(name, mode):
    from dvd_hip import ops
    c = _make(name)
    points, tabs, depth = _dev(c)
    got = ops.track_filter(points, c['starts'], tabs, depth, c['weights'], k0=c['k0'], mode=mode, tol=C.TOL, z_near=C.Z_NEAR)
    want = _expected(c, points, tabs, depth, mode)
    assert set(got) == {'depth', 'ratio', 'count', 'spread'}
    assert got['depth'].shape == (c['B'], 1, c['H'], c['W']) and got['count'].shape == (c['B'], c['H'], c['W'])
    assert got['count'].dtype == torch.uint8 and got['ratio'].dtype == torch.float32
    _same(got, want, what=(name, mode))
    cnt = got['count'].cpu().numpy()
    live = np.array([sum(0 <= s + k + c['k0'] < c['N'] for k in range(c['T1'])) for s in c['starts']])
    assert cnt.min() >= 1 and all(cnt[b].max() <= live[b] for b in range(c['B']))
    if name == 'single_row':                                        # output equals input
        assert np.array_equal(_bits(got['depth']), _bits(c['depth'][c['starts']])) and np.all(cnt == 1)
        assert bool((got['ratio'] == 1).all()) and not bool(got['spread'].any())
    elif name == 'cap':
        assert cnt[0].max() >= 20 and cnt[1].max() <= 20              # frame 17 has all 33 rows, frame 3 only 20
    else:
        assert cnt.max() >= 3 and (cnt < live[:, None, None]).mean() > 0.02      # samples pass, and samples are gated out
    # the same launch again gives the same bits
    again = ops.track_filter(points, c['starts'], tabs, depth, c['weights'], k0=c['k0'], mode=mode, tol=C.TOL, z_near=C.Z_NEAR)
    _same(again, got, what=(name, mode, 'again'))


@pytest.mark.parametrize('mode', ['mean', 'median'])
def test_an_unaligned_output_takes_the_scalar_path_and_gives_the_same_bits(mode):
    from dvd_hip import ops
    c = _make('vector_small')
    points, tabs, depth = _dev(c)
    want = _expected(c, points, tabs, depth, mode)
    n = c['B'] * c['H'] * c['W']
    buf = torch.full((n + 8,), -7.0, device=DEV)
    off = buf[1:1 + n].view(c['B'], 1, c['H'], c['W'])
    assert off.data_ptr() % 16 == 4 and points.data_ptr() % 16 == 0
    got = ops.track_filter(points, c['starts'], tabs, depth, c['weights'], k0=c['k0'], mode=mode, out={'depth': off})
    assert got['depth'] is off
    _same(got, want, what=('offset', mode))
    assert buf[0].item() == -7.0 and bool((buf[1 + n:] == -7.0).all())            # nothing beside the slice is written
    aligned = ops.track_filter(points, c['starts'], tabs, depth, c['weights'], k0=c['k0'], mode=mode)
    _same(aligned, got, what=('aligned', mode))


@pytest.mark.parametrize('mode', ['mean', 'median'])
def test_interleaved_points_zero_and_nan_depth_zero_weight_want_and_out(mode):
    from dvd_hip import ops
    c = _make('vector_small', seed=1)
    c['depth'][c['starts'][0], 0, 2, 3] = 0.0
    c['depth'][c['starts'][1], 0, 5, 7] = np.nan
    c['depth'][c['starts'][1], 0, 5, 8] = -1.0
    c['weights'][-c['k0'] - 1] = 0.0                               # a row without weight still counts, and adds nothing to the mean
    points, tabs, depth = _dev(c)
    got = ops.track_filter(points, c['starts'], tabs, depth, c['weights'], k0=c['k0'], mode=mode)
    _same(got, _expected(c, points, tabs, depth, mode), what=mode)
    d, r, n, s = (got[k].cpu() for k in ('depth', 'ratio', 'count', 'spread'))
    assert d[0, 0, 2, 3].item() == 0.0 and bool(torch.isnan(d[1, 0, 5, 7])) and d[1, 0, 5, 8].item() == -1.0
    for b, y, x in [(0, 2, 3), (1, 5, 7), (1, 5, 8)]:
        assert r[b, 0, y, x].item() == 1.0 and n[b, y, x].item() == 0 and s[b, 0, y, x].item() == 0.0
    # (a neighbour that lands on the bad pixel reads it through the bilinear taps: D is 0 / NaN / negative there and the gate
    #  D > 0 or the ratio gates drop it -- part of the bit-for-bit comparison above)
    if mode == 'mean':
        w1 = c['weights'].copy()
        w1[-c['k0'] - 1] = 1.0
        other = ops.track_filter(points, c['starts'], tabs, depth, w1, k0=c['k0'], mode=mode)
        assert not torch.equal(other['ratio'], got['ratio']) and torch.equal(other['count'], got['count'])
    # interleaved [T1,B,H,W,3] points give the bits of the planar ones
    inter = points.permute(0, 1, 3, 4, 2).contiguous()
    _same(ops.track_filter(inter, c['starts'], tabs, depth, c['weights'], k0=c['k0'], mode=mode, planar=False), got, what='interleaved')
    c1 = _make('scalar_two_blocks')
    p1, t1, d1 = _dev(c1)
    _same(ops.track_filter(p1.permute(0, 1, 3, 4, 2).contiguous(), c1['starts'], t1, d1, c1['weights'], k0=c1['k0'], mode=mode,
                           planar=False), _expected(c1, p1, t1, d1, mode), what='interleaved scalar')
    # want=() writes only the depth; a GPU int32 start with its host copy; preallocated outputs are the ones returned
    only = ops.track_filter(points, torch.tensor(c['starts'], dtype=torch.int32, device=DEV), tabs, depth, c['weights'], k0=c['k0'],
                            mode=mode, want=(), host_start=c['starts'])
    assert set(only) == {'depth'}
    _same(only, got, keys=('depth',), what='want=()')
    pre = {'depth': torch.zeros_like(got['depth']), 'count': torch.zeros_like(got['count'])}
    res = ops.track_filter(points, c['starts'], tabs, depth, c['weights'], k0=c['k0'], mode=mode, out=pre, want=('count', 'spread'))
    assert res['depth'] is pre['depth'] and res['count'] is pre['count'] and set(res) == {'depth', 'count', 'spread'}
    _same(res, got, keys=('depth', 'count', 'spread'), what='out')
    for bad in ({'depth': torch.zeros(2, 1, 12, 25, device=DEV)}, {'count': torch.zeros(2, 12, 24, device=DEV)},
                {'ratio': torch.zeros(2, 1, 12, 24)}):
        with pytest.raises(RuntimeError, match='out'):
            ops.track_filter(points, c['starts'], tabs, depth, c['weights'], k0=c['k0'], mode=mode, out=bad)
    with pytest.raises(RuntimeError, match='weights'):
        ops.track_filter(points, c['starts'], tabs, depth, c['weights'][:-1], k0=c['k0'], mode=mode)
    with pytest.raises(RuntimeError, match='depth_all'):
        ops.track_filter(points, c['starts'], tabs, depth[:-1], c['weights'], k0=c['k0'], mode=mode)
    # the tolerance is the gate: tol = 0 lets nothing but the frame itself count (no sample hits D == z here)
    tight = ops.track_filter(points, c['starts'], tabs, depth, c['weights'], k0=c['k0'], mode=mode, tol=0.0)
    _same(tight, _expected(c, points, tabs, depth, mode, tol=0.0), what='tol=0')
    assert int(tight['count'].max()) == 1


@pytest.mark.parametrize('mode', ['mean', 'median'])
def test_static_camera_every_frame_becomes_the_mean(mode):
    """One camera, still points, depth_g = S c_g, a box window over the whole video: every frame must become S mean(c) (the
    median: S median(c))."""
    from dvd_hip import ops
    fx = helpers.load_golden(C.FX)
    n, H, W = 7, 11, 21
    radius = n - 1
    T1 = 2 * radius + 1
    tabs = {k: np.ascontiguousarray(np.broadcast_to(v[:1], v.shape)) for k, v in _tables(fx, n, H, W).items()}
    depth_np, Ssurf, c = C.static_video(n, H, W)
    starts = list(range(n))
    depth = helpers.t(depth_np, DEV)
    gt = {k: helpers.t(tabs[k], DEV) for k in tabs}
    p0 = ops.unproject(depth, gt['R_T'], gt['t'], gt['K_inv_T'], planar=True)
    points = p0[None].expand(T1, n, 3, H, W).contiguous()
    tab3 = {k: gt[k] for k in ('R', 't', 'K_T')}
    w = np.ones(T1, np.float32)
    got = ops.track_filter(points, starts, tab3, depth, w, k0=-radius, mode=mode)
    case = dict(starts=starts, k0=-radius, N=n, T1=T1, weights=w)
    _same(got, _expected(case, points, tab3, depth, mode), what=mode)
    want = Ssurf * (c.mean() if mode == 'mean' else np.median(c))
    inner = ~S.border_pixels(H, W).numpy()
    # the specification's own fp32 form: the reference's projection and sampling in fp32 (invert_spec.project), fused in fp32
    rows = I.project(points.cpu(), starts, tabs['R'], tabs['t'], tabs['K_T'], depth_np, k0=-radius, dtype=torch.float32)
    f32 = F.fuse(rows['z'], rows['depth_at'], rows['inside'], depth_np[starts], rows['live'], w, radius, mode, C.TOL, C.Z_NEAR, np.float32)
    dist = lambda d: float(np.abs(np.asarray(d, dtype=np.float64)[:, 0][:, inner] / want[inner][None] - 1.0).max())
    d_kernel, d_ref = dist(got['depth'].cpu().numpy()), dist(f32['depth'])
    bound = 4.0 * MEASURED['static/' + mode]
    helpers.log_measured('track_filter/static/' + mode, d_kernel, bound)
    print('measured track_filter/static/%s %.4g (bound %.4g, fp32 form %.4g, its limit %.4g)' % (mode, d_kernel, bound, d_ref, 4 * d_ref))
    assert bool((got['count'].cpu()[:, inner] == n).all())
    assert d_kernel <= 4.0 * d_ref, (d_kernel, d_ref)
    assert d_kernel <= bound, (d_kernel, bound)
    before = float((np.std(depth_np[:, 0].astype(np.float64), 0) / np.mean(depth_np[:, 0].astype(np.float64), 0))[inner].max())
    after = got['depth'].cpu().numpy()[:, 0].astype(np.float64)
    assert before > 2e-2 and float((np.std(after, 0) / np.mean(after, 0))[inner].max()) < 1e-6
