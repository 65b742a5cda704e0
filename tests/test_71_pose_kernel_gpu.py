"""ops.pose_normal_eq (csrc/pose.hip) against tests/pose_spec.py.

Per pixel the kernel is an operation-for-operation fp32 contract: `gate` equals the contract's on every decided pixel and
`resid` equals it BIT FOR BIT where gate == 1.  `decided` leaves out a pixel whose q.z lies within 1e-4 z_near of z_near in the
float64 reference; these scenes have q.z >= 2 everywhere, so it leaves out none (the cap is 0.5 %).  `counts` equals the
float64 reference exactly.

The sums are fp32 over a thread's run of 16 pixels and the wave's 64 lanes and float64 from there, so they are compared with
the float64 reference on the same fp32 inputs, per row as ||got - ref||_F / ||ref||_F over the 91 entries of J^T w J, the 13 of
J^T w r, and the cost.  The bound is 4 x the worst value measured on the MI355X over the three shapes (pose_spec.MEASURED):
                 J^T w J     J^T w r     cost        sum w |r|^2   sum w
    measured     3.038e-7    2.920e-6    8.209e-7    6.985e-7      3.595e-7
The shapes: 24 x 40 with 7 frames and all 36 rows (960 pixels: one block with a tail), 5 x 9 (45 pixels: less than a wave),
72 x 120 (8640 pixels: three blocks per row, the last one short).  The cameras are the scene's perturbed by 1 degree and 0.03,
the flows carry 0.4 px of noise, so both branches of Huber's loss are taken; the weight is the static mask times U(0.5, 1.5).
"""
import numpy as np
import pytest
import torch

import helpers
import pose_spec as S
import triangulate_spec as T

pytestmark = pytest.mark.gpu

DEV = 'cuda'
KEYS = ('sums', 'wsum', 'counts', 'resid', 'gate')
SHAPES = {'24x40': (24, 40, 7, (1, 2, 3, 4)), '5x9': (5, 9, 3, (1, 2)), '72x120': (72, 120, 3, (1, 2))}


class _Case(object):
    pass


def _case(H, W, N, gaps):
    c = _Case()
    c.sc = T.scene(H, W, N, seed=0, noise=0.4, gaps=gaps)
    c.rows = S.plan(c.sc['pairs'])
    c.tables = S.tables_from(S.perturbed(c.sc), c.sc['tables'])
    rng = np.random.default_rng(11)
    c.weight = ((~c.sc['disc']) * rng.uniform(0.5, 1.5, c.sc['disc'].shape)).astype(np.float32)
    c.depth = c.sc['depth'].astype(np.float32)
    c.log_scale = 0.05 * rng.uniform(-1, 1, N)
    return c


def _args(c, tables=None, weight='case', rows=None, log_scale='case'):
    sc = c.sc
    return dict(flow_1_2=helpers.t(sc['flow_1_2'], DEV), flow_2_1=helpers.t(sc['flow_2_1'], DEV), mask_1=helpers.t(sc['mask_1'], DEV),
                mask_2=helpers.t(sc['mask_2'], DEV), depth=helpers.t(c.depth, DEV)[:, None],
                weight=helpers.t(c.weight, DEV) if isinstance(weight, str) else weight,
                rows=c.rows if rows is None else rows, tables={k: helpers.t(v, DEV) for k, v in (c.tables if tables is None else tables).items()},
                log_scale=c.log_scale if isinstance(log_scale, str) else log_scale, huber=1.0, z_near=1e-3)


def _gpu(c, maps=True, **kw):
    from dvd_hip import ops
    out = ops.pose_normal_eq(maps=maps, **_args(c, **kw))
    return {k: v.cpu().numpy() for k, v in out.items()}


def _spec(c, dtype, tables=None, weight='case', rows=None, log_scale='case', jacobian=True):
    sc = c.sc
    return S.normal_eq(sc['flow_1_2'], sc['flow_2_1'], sc['mask_1'], sc['mask_2'], c.depth, c.weight if isinstance(weight, str) else weight,
                       c.rows if rows is None else rows, c.tables if tables is None else tables,
                       c.log_scale if isinstance(log_scale, str) else log_scale, 1.0, 1e-3, dtype, jacobian)


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else (a.view(np.int64) if a.dtype == np.float64 else a)


@pytest.fixture(scope='module')
def cases():
    """Every shape's inputs, kernel outputs, fp32 contract and float64 reference: computed once, shared, never written to."""
    out = {}
    for name, shape in SHAPES.items():
        c = _case(*shape)
        c.got, c.con, c.ref = _gpu(c), _spec(c, np.float32, jacobian=False), _spec(c, np.float64)
        out[name] = c
    return out


@pytest.mark.parametrize('name', list(SHAPES))
def test_per_pixel_contract_and_counts(cases, name):
    c = cases[name]
    H, W, N, _ = SHAPES[name]
    R = len(c.rows)
    assert c.got['sums'].shape == (R, 106) and c.got['sums'].dtype == np.float64 and c.got['wsum'].shape == (R,)
    assert c.got['counts'].shape == (R, 2) and c.got['counts'].dtype == np.int64
    assert c.got['resid'].shape == (R, H, W, 2) and c.got['gate'].shape == (R, H, W) and c.got['gate'].dtype == np.uint8
    ok = S.decided(c.ref)
    print('pose/%s: undecided share %.4f, q.z >= %.3f' % (name, float((~ok).mean()), float(c.ref['qz'].min())))
    assert float((~ok).mean()) <= 0.005
    assert np.array_equal(c.got['gate'][ok], c.con['gate'][ok]) and np.array_equal(c.con['gate'][ok], c.ref['gate'][ok])
    live = ok & (c.con['gate'] == 1)
    assert live.mean() > 0.3 and (c.got['gate'] == 0).any()
    same = _bits(c.got['resid'])[live] == _bits(c.con['resid'])[live]
    assert same.all(), (int((~same).sum()), c.got['resid'][live][~same][:4], c.con['resid'][live][~same][:4])
    assert (c.got['resid'][c.got['gate'] != 1] == 0).all()
    assert np.array_equal(c.got['counts'], c.ref['counts']) and (c.got['counts'][:, 1] == 0).all()
    nr = np.linalg.norm(c.ref['resid'], axis=-1)[c.ref['gate'] == 1]
    print('pose/%s: %.3f of the live residuals outside Huber\'s threshold' % (name, float((nr > 1.0).mean())))
    if name != '5x9':                                                           # both branches of the loss are taken (5 x 9: 2 % outside)
        assert (nr > 1.0).mean() > 0.05 and (nr < 1.0).mean() > 0.05
    assert np.isfinite(c.got['sums']).all() and np.isfinite(c.got['wsum']).all()


def test_sums_against_the_float64_reference(cases):
    worst = {'sums/JtJ': 0.0, 'sums/Jtr': 0.0, 'sums/cost': 0.0, 'sums/wr2': 0.0, 'sums/wsum': 0.0}
    for name, c in cases.items():
        m = {'sums/JtJ': S.rel_rows(c.got['sums'][:, :91], c.ref['sums'][:, :91]),
             'sums/Jtr': S.rel_rows(c.got['sums'][:, 91:104], c.ref['sums'][:, 91:104]),
             'sums/cost': S.rel_rows(c.got['sums'][:, 104:105], c.ref['sums'][:, 104:105]),
             'sums/wr2': S.rel_rows(c.got['sums'][:, 105:106], c.ref['sums'][:, 105:106]),
             'sums/wsum': S.rel_rows(c.got['wsum'][:, None], c.ref['wsum'][:, None])}
        for k, v in m.items():
            print('measured pose/%s/%s %.4g' % (name, k, v))
            worst[k] = max(worst[k], v)
    failed = []
    for k, v in worst.items():
        bound = 4.0 * S.MEASURED[k]
        helpers.log_measured('pose/' + k, v, bound)
        print('measured pose/%s %.4g (bound %.4g)' % (k, v, bound))
        if not v <= bound:
            failed.append((k, v, bound))
    assert not failed, failed


def test_behind_the_camera(cases):
    """Frame 2 turned by 180 degrees about its y axis: every observation of its rows fails the q.z gate; it adds nothing to
    the system, is counted apart, and costs the constant penalty (exactly: all-ones weight, and the penalty enters in float64)."""
    c = cases['24x40']
    tab = {k: v.copy() for k, v in c.tables.items()}
    tab['R'][2] = tab['R'][2] @ np.diag([-1, 1, -1]).astype(np.float32)
    got = _gpu(c, tables=tab, weight=None)
    ref = _spec(c, np.float64, tables=tab, weight=None)
    plain = _gpu(c, weight=None)
    turned = (c.rows[:, 1] == 2) | (c.rows[:, 2] == 2)
    assert turned.sum() == 12
    pen = float(S.params32(24, 40)[2])
    assert abs(pen - (np.hypot(40, 24) - 0.5)) < 1e-5
    assert (got['counts'][turned, 0] == 0).all() and np.array_equal(got['counts'][turned, 1], plain['counts'][turned, 0])
    assert (got['counts'][turned, 1] > 300).all() and np.array_equal(got['counts'], ref['counts'])
    assert (got['sums'][turned][:, :104] == 0).all() and (got['sums'][turned][:, 105] == 0).all() and (got['wsum'][turned] == 0).all()
    assert np.array_equal(got['sums'][turned][:, 104], got['counts'][turned, 1] * pen)
    assert np.array_equal(got['gate'][turned] == 2, plain['gate'][turned] == 1) and (got['resid'][turned] == 0).all()
    for k in KEYS:                                                           # the other rows do not notice
        assert np.array_equal(_bits(got[k][~turned]), _bits(plain[k][~turned])), k


def test_skipped_rows(cases):
    c = cases['24x40']
    P, N = len(c.sc['pairs']), 7
    rows = c.rows[:6].copy()
    rows[1, 0], rows[2, 0], rows[3, 1], rows[4, 2] = -1, P, N, -1
    got = _gpu(c, rows=rows)
    for r in (1, 2, 3, 4):
        for k in KEYS:
            assert not got[k][r].any(), (r, k)
    for r in (0, 5):
        for k in KEYS:
            assert np.array_equal(_bits(got[k][r]), _bits(cases['24x40'].got[k][r])), (r, k)


@pytest.mark.parametrize('name', ['24x40', '72x120'])
def test_reproducible_and_preallocated(cases, name):
    from dvd_hip import ops
    c = cases[name]
    H, W, N, _ = SHAPES[name]
    R = len(c.rows)
    again = _gpu(c)
    for k in KEYS:
        assert np.array_equal(_bits(again[k]), _bits(c.got[k])), k
    no_maps = _gpu(c, maps=False)
    assert set(no_maps) == {'sums', 'wsum', 'counts'}
    for k in no_maps:
        assert np.array_equal(_bits(no_maps[k]), _bits(c.got[k])), k
    out = {'sums': torch.full((R, 106), 7.0, device=DEV, dtype=torch.float64), 'wsum': torch.empty(R, device=DEV, dtype=torch.float64),
           'counts': torch.empty(R, 2, device=DEV, dtype=torch.int64), 'resid': torch.empty(R, H, W, 2, device=DEV),
           'gate': torch.empty(R, H, W, device=DEV, dtype=torch.uint8)}
    res = ops.pose_normal_eq(maps=True, out=out, **_args(c))
    for k in KEYS:
        assert res[k] is out[k] and np.array_equal(_bits(res[k].cpu().numpy()), _bits(c.got[k])), k


def test_no_weight_and_no_scale_are_ones(cases):
    c = cases['5x9']
    a = _gpu(c, weight=None, log_scale=None)
    b = _gpu(c, weight=torch.ones(3, 5, 9, device=DEV), log_scale=[0.0, 0.0, 0.0])
    ref = _spec(c, np.float64, weight=None, log_scale=None)
    for k in KEYS:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert np.array_equal(a['counts'], ref['counts'])
    assert S.rel_rows(a['sums'][:, :104], ref['sums'][:, :104]) <= 4 * S.MEASURED['sums/JtJ']


def test_the_wrapper_refuses_what_needs_a_device_to_tell(cases):
    from dvd_hip import ops
    c = cases['24x40']
    good = _args(c)
    H, W, N = 24, 40, 7
    for kw, word in ((dict(flow_2_1=good['flow_2_1'][:-1]), 'flow_2_1'), (dict(flow_1_2=good['flow_1_2'].transpose(1, 2)), 'flow_1_2'),
                     (dict(mask_1=good['mask_1'].float()), 'mask_1'), (dict(mask_2=None), 'mask_2'), (dict(depth=good['depth'][:-1]), 'depth'),
                     (dict(depth=good['depth'].double()), 'depth'), (dict(depth=good['depth'].cpu()), 'depth'),
                     (dict(weight=good['weight'][:, None]), 'weight'), (dict(weight=good['weight'].cpu()), 'weight'),
                     (dict(tables={k: v for k, v in good['tables'].items() if k != 'K_inv_T'}), 'K_inv_T'),
                     (dict(tables=dict(good['tables'], t=good['tables']['t'][:-1])), 'table t|log_scale'),
                     (dict(log_scale=[0.0] * 6), 'log_scale'), (dict(rows=np.zeros((65536, 4), np.int32)), 'rows'),
                     (dict(out={'sums': torch.empty(36, 106, device=DEV)}), r"out\['sums'\]"),
                     (dict(out={'counts': torch.empty(36, 2, device=DEV, dtype=torch.int32)}), r"out\['counts'\]")):
        with pytest.raises(RuntimeError, match=word):
            ops.pose_normal_eq(**dict(good, **kw))
    with pytest.raises(RuntimeError, match=r"out\['gate'\]"):
        ops.pose_normal_eq(maps=True, out={'gate': torch.empty(36, H, W, device=DEV)}, **good)
