"""ops.triangulate (csrc/triangulate.hip) against its fp32 contract, tests/triangulate_spec.py: BIT FOR BIT on every output, in
both modes, and never a NaN or an Inf.  The largest case is 24 x 40.

Against the float64 reference on scene(24, 40, 7, noise=0.4) (the last test): count and usable are equal on every pixel whose
observations are all decided, and depth and epi are compared there.  The fp32 error of s1 grows as the parallax shrinks (den is
a difference of two numbers near A C), so the bound is 4 x the worst difference measured on the MI355X, MEASURED below -- the
margin covers other seeds' parallax:
                 depth (relative)   epi (pixels)
    median       1.212e-3           5.09e-6
    mean         1.137e-3           5.09e-6
(the kernel equals the fp32 contract bit for bit, so these are also the contract's distances, which the CPU can compute).
`decided`'s margin on sin2, 1e-3 of the threshold, is below fp32's own error of den at the default threshold (about 3e-3 there):
seed 0, the case these tests use, has no such observation; seed 2 has one.
"""
import numpy as np
import pytest
import torch

import helpers
import triangulate_spec as T

pytestmark = pytest.mark.gpu

DEV = 'cuda'
KEYS = ('depth', 'count', 'usable', 'epi', 'spread')
MODES = ('median', 'mean')
MEASURED = T.MEASURED            # worst distance from the float64 reference measured on the MI355X; the bound is 4 x this


def _gpu(sc, obs, frames, tables=None, mode='median', **params):
    from dvd_hip import ops
    tab = {k: helpers.t(v, DEV) for k, v in (sc['tables'] if tables is None else tables).items()}
    out = ops.triangulate(helpers.t(sc['flow_1_2'], DEV), helpers.t(sc['flow_2_1'], DEV), helpers.t(sc['mask_1'], DEV),
                          helpers.t(sc['mask_2'], DEV), obs, list(frames), tab, mode=mode, **params)
    return {k: out[k].cpu().numpy() for k in KEYS}


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _check(sc, obs, frames, tables=None, what='', **params):
    """Both modes of the kernel against the contract, bit for bit; -> {mode: the kernel's outputs}."""
    res = {}
    for mode in MODES:
        got = _gpu(sc, obs, frames, tables, mode, **params)
        want = T.pipeline(sc['flow_1_2'], sc['flow_2_1'], sc['mask_1'], sc['mask_2'], obs, frames,
                          sc['tables'] if tables is None else tables, mode, np.float32, **params)
        for k in KEYS:
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, mode, k, got[k].shape, want[k].shape)
            assert np.isfinite(got[k]).all(), (what, mode, k)
            same = _bits(got[k]) == _bits(want[k])
            assert same.all(), (what, mode, k, int((~same).sum()), got[k][~same][:4], want[k][~same][:4])
        res[mode] = got
    return res


@pytest.fixture(scope='module')
def noisy():
    sc = T.scene(24, 40, 7, seed=0, noise=0.4)
    return sc, T.plan(sc['pairs'], range(7))


@pytest.mark.parametrize('H,W', [(2, 2), (5, 7), (24, 40)])
def test_shapes(H, W):
    sc = T.scene(H, W, 4, seed=3, noise=0.4, gaps=(1, 2))
    res = _check(sc, T.plan(sc['pairs'], range(4)), range(4), what=(H, W))
    assert res['median']['depth'].shape == (4, 1, H, W) and res['median']['count'].shape == (4, H, W)
    if (H, W) == (24, 40):
        assert (res['median']['count'] >= 2).mean() > 0.5 and res['median']['usable'].max() == 3


@pytest.mark.parametrize('M', [0, 1, 2, 5, 32])
def test_table_lengths(noisy, M):
    sc, full = noisy
    live = full[3][full[3, :, 0] >= 0]                                   # frame 3's six observations, and frame 0's four
    rows3 = [live[i % len(live)] for i in range(M)]                     # M = 32 repeats them: equal samples (ties) in the median
    rows0 = [full[0][i % 4] for i in range(M)]
    obs = np.array([rows3, rows0], np.int32).reshape(2, M, 3)
    res = _check(sc, obs, [3, 0], what=M)
    for mode in MODES:
        assert int(res[mode]['count'].max()) == M and int(res[mode]['usable'].max()) == M
    if M == 0:
        assert (res['mean']['depth'] == 0).all() and (res['mean']['epi'] == -1).all() and (res['mean']['spread'] == 0).all()
    if M == 32:                                                          # min_count above the count: no depth anywhere
        none = _check(sc, obs[:, :6], [3, 0], what='min_count', min_count=7)
        assert (none['median']['depth'] == 0).all() and (none['median']['spread'] == 0).all() and none['median']['count'].max() == 6
        one = _check(sc, obs[:, :1], [3, 0], what='min_count 1', min_count=1)
        assert (one['median']['depth'] > 0).mean() > 0.5


def test_padding_anywhere_backward_only_and_cameras_that_differ(noisy):
    sc, full = noisy
    pad = np.full((2, 9, 3), -1, np.int32)
    pad[0, [1, 4, 5, 8]] = full[3][[0, 1, 2, 3]]                         # padding at the start, in the middle and at the end
    pad[1, [0, 2, 7]] = full[6][[0, 1, 3]]
    res = _check(sc, pad, [3, 6], what='padding')
    dense = _check(sc, np.stack([full[3][:4], np.concatenate([full[6][[0, 1, 3]], [[-1] * 3]])]), [3, 6], what='dense')
    for mode in MODES:
        for k in KEYS:
            assert np.array_equal(_bits(res[mode][k]), _bits(dense[mode][k])), (mode, k)
    back = full.copy()
    back[back[:, :, 2] == 0] = -1                                        # backward observations only (frame 0 keeps none)
    res = _check(sc, back, range(7), what='backward')
    assert res['median']['usable'][0].max() == 0 and res['median']['count'][6].max() == 4
    # two frames whose tables differ in K: frame 2 is seen through a longer lens than the flows were made with
    tab = {k: v.copy() for k, v in sc['tables'].items()}
    K = sc['intrinsics'][2].copy()
    K[0, 0] *= 1.05
    K[1, 1] *= 1.05
    tab['K_T'][2], tab['K_inv_T'][2] = K.T, np.linalg.inv(K).T
    res = _check(sc, full, range(7), tables=tab, what='K')
    plain = _check(sc, full, range(7), what='plain')
    assert not np.array_equal(res['median']['depth'][2], plain['median']['depth'][2])
    assert not np.array_equal(res['median']['epi'][1], plain['median']['epi'][1])


def test_every_gate_by_hand():
    sc = T.scene(5, 7, 3, seed=1, noise=0.0, gaps=(1, 2), masks='zero')
    H, W = 5, 7
    obs = T.plan(sc['pairs'], range(3))
    row, kw = obs[:1, :1], dict(min_count=1)                             # frame 0 against frame 1 alone: pair 0, flow_1_2 with mask_2
    assert row.tolist() == [[[0, 1, 0]]]
    base = _check(sc, row, [0], what='base', **kw)['median']
    inner = np.zeros((H, W), bool)
    inner[1:4, 1:] = True
    inner &= ~sc['disc'][0]
    assert (base['count'][0][inner] == 1).all()                          # (the camera moves: column 0 and rows 0, 4 leave the image)
    f12, m2 = sc['flow_1_2'].copy(), sc['mask_2'].copy()
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))
    m2[0, 2, 1], m2[0, 2, 2] = 1, 255                                    # masked
    f12[0, 2, 0], f12[0, 1, 0] = (-1e-45, 0), (0, 0)                     # one ulp (a denormal) past the left border, and ON it
    f12[0, 2, 6], f12[0, 1, 6] = (up(6) - np.float32(6), 0), (0, 0)      # ... the right border
    f12[0, 0, 2, 1], f12[0, 0, 3, 1] = -1e-45, 0                         # ... the top
    f12[0, 4, 2, 1], f12[0, 4, 3, 1] = up(4) - np.float32(4), 0          # ... the bottom
    f12[0, 3, 1], f12[0, 3, 2], f12[0, 3, 3] = (np.nan, 0), (0, np.inf), (1e30, -1e30)
    f12[0, 1, 1] = -3 * f12[0, 1, 1]                                     # against the parallax: a point behind both cameras
    f12[0, 1, 2, 1] += 1.5                                               # off the epipolar line: a moving point
    hand = dict(sc, flow_1_2=f12, mask_2=m2)
    assert np.float32(6) + f12[0, 2, 6, 0] == up(6) and np.float32(0) + f12[0, 2, 0, 0] < 0
    res = _check(hand, row, [0], what='gates', **kw)['median']
    for y, x in ((2, 1), (2, 2), (2, 0), (2, 6), (0, 2), (4, 2), (3, 1), (3, 2), (3, 3)):
        assert res['usable'][0, y, x] == 0 and res['epi'][0, 0, y, x] == -1 and res['depth'][0, 0, y, x] == 0, (y, x)
    for y, x in ((1, 0), (1, 6), (0, 3), (4, 3)):
        assert res['usable'][0, y, x] == 1, (y, x)
    for y, x in ((1, 1), (1, 2)):
        assert res['usable'][0, y, x] == 1 and res['count'][0, y, x] == 0 and res['depth'][0, 0, y, x] == 0, (y, x)
    assert res['epi'][0, 0, 1, 2] > 1.0 and res['epi'][0, 0, 1, 1] < 0.1
    assert T.observe(f12[0], m2[0], sc['tables'], 0, 1, np.float32)['s1'][1, 1] < 0
    # zero baseline: frame 1 stands where frame 0 stands.  With its rotation and the flow kept the rays still differ, but E = F = 0
    # puts both depths at 0, below z_near; with the same rotation and a zero flow the two rays are one, den = 0 and every quotient
    # is 0 / 0
    for same_R in (False, True):
        tab = {k: v.copy() for k, v in sc['tables'].items()}
        tab['t'][1] = tab['t'][0]
        if same_R:
            tab['R'][1] = tab['R'][0]
        z = dict(sc, flow_1_2=sc['flow_1_2'] * 0) if same_R else sc
        res = _check(z, obs[:, :1], range(3), tables=tab, what=('rotation', same_R), min_count=1)['mean']
        assert res['count'][0].max() == 0 and (res['depth'][0] == 0).all()
        if same_R:
            assert res['usable'][0].max() == 0 and (res['epi'][0] == -1).all()
        else:
            assert res['usable'][0].max() == 1
    # sin2 and e on either side of their thresholds: the thresholds are put ON a pixel's own value, and one ulp past it
    o = T.observe(sc['flow_1_2'][0], sc['mask_2'][0], sc['tables'], 0, 1, np.float32)
    noisy_flow = sc['flow_1_2'].copy()
    noisy_flow[0, 2, 5, 1] += 0.25
    on = dict(sc, flow_1_2=noisy_flow)
    e = T.observe(noisy_flow[0], sc['mask_2'][0], sc['tables'], 0, 1, np.float32)['e'][2, 5]
    s = o['sin2'][2, 5]
    assert 0.1 < e < 0.5 and s > T.SIN2_MIN
    assert _check(sc, row, [0], what='sin2 at', sin2_min=float(s), **kw)['median']['usable'][0, 2, 5] == 1
    assert _check(sc, row, [0], what='sin2 above', sin2_min=float(up(s)), **kw)['median']['usable'][0, 2, 5] == 0
    assert _check(on, row, [0], what='e at', epi_tol=float(e), **kw)['median']['count'][0, 2, 5] == 1
    below = _check(on, row, [0], what='e below', epi_tol=float(np.nextafter(e, np.float32(0))), **kw)['median']
    assert below['count'][0, 2, 5] == 0 and below['usable'][0, 2, 5] == 1
    # z_near on either side of a pixel's depth (the smaller of s1, s2 decides)
    z = min(o['s1'][2, 5], o['s2'][2, 5])
    assert _check(sc, row, [0], what='z at', z_near=float(z), **kw)['median']['count'][0, 2, 5] == 1
    assert _check(sc, row, [0], what='z above', z_near=float(up(z)), **kw)['median']['count'][0, 2, 5] == 0


def test_hostile_cameras_leave_no_nan():
    sc = T.scene(5, 7, 3, seed=1, noise=0.4, gaps=(1, 2), masks='zero')
    obs = T.plan(sc['pairs'], range(3))
    for k, v in (('t', np.nan), ('t', 1e38), ('R', np.inf), ('K_T', 0.0), ('K_inv_T', 1e30), ('K_inv_T', 0.0), ('R', 0.0)):
        tab = {q: a.copy() for q, a in sc['tables'].items()}
        tab[k][1] = v
        _check(sc, obs, range(3), tables=tab, what=(k, v), min_count=1)


def test_translations_times_two_double_the_depth_bit_for_bit(noisy):
    sc, obs = noisy
    tab = {k: v.copy() for k, v in sc['tables'].items()}
    tab['t'] = tab['t'] * np.float32(2)
    for mode in MODES:
        a, b = _gpu(sc, obs, range(7), mode=mode), _gpu(sc, obs, range(7), tables=tab, mode=mode)
        assert (a['depth'] > 0).mean() > 0.5
        assert np.array_equal(_bits(a['depth'] * np.float32(2)), _bits(b['depth'])), mode
        for k in ('count', 'usable', 'epi', 'spread'):
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (mode, k)


def test_against_the_float64_reference(noisy):
    sc, obs = noisy
    failed = []
    for mode in MODES:
        got = _gpu(sc, obs, range(7), mode=mode)
        ref = T.pipeline(sc['flow_1_2'], sc['flow_2_1'], sc['mask_1'], sc['mask_2'], obs, range(7), sc['tables'], mode, np.float64)
        m = T.against_reference(got, ref)
        print('triangulate/%s: excluded share %.4f' % (mode, m['excluded']))
        assert m['excluded'] <= 0.01                                     # no comparison leaves out more than the cap
        assert m['counts_equal'], mode
        for q in ('depth', 'epi'):
            bound = 4.0 * MEASURED[mode + '/' + q]
            helpers.log_measured('triangulate/%s/%s' % (mode, q), m[q], bound)
            print('measured triangulate/%s/%s %.4g (bound %.4g)' % (mode, q, m[q], bound))
            if not m[q] <= bound:
                failed.append((mode, q, m[q], bound))
    assert not failed, failed
