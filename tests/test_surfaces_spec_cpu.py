"""tests/surfaces_spec.py kept honest without a GPU: its cases satisfy the condition its comparisons rest on, its tolerance table
is held to the reference's own error from both sides, its float64 oracle agrees with an independent NumPy restatement, and the
shape arithmetic of the wrapper checks (dvd_hip/ops.py: _shape_is, _images, _image_size, pack_cameras) refuses on the host."""
import numpy as np
import pytest
import torch

import surfaces_spec as S
from dvd_hip import ops


@pytest.mark.parametrize('name', list(S.CASES))
def test_fp32_and_float64_oracle_take_the_same_decisions(name):
    S.decisions_agree(name)


@pytest.fixture(scope='module')
def measured():
    return S.measure()


def test_tolerances_are_no_tighter_than_the_reference_and_not_quietly_loosened(measured):
    """TOL = factor x (largest fp32-oracle error), rounded up to one digit: the fp32 oracle stays within TOL / factor in every
    case, and its largest error is not below TOL / 16."""
    assert set(S.TOL) == set(measured) == set(S.TOL_FACTOR)
    for key, per in measured.items():
        worst = max(per.values())
        print('%-20s measured %.3e  TOL %.0e' % (key, worst, S.TOL[key]))
        assert worst <= S.TOL[key] / S.TOL_FACTOR[key], (key, per)
        assert worst >= S.TOL[key] / 16.0, (key, per)


def _numpy_surfaces(c):
    """The pinhole formulas and the border-clamped bilinear warp, restated in NumPy float64 with nothing shared with the oracle."""
    a = {k: v.double().numpy() for k, v in c.items()}
    B, _, H, W = a['depth_1'].shape
    m = {k: a[k].reshape(B, 1, 1, -1, 3) for k in S.CAM_KEYS}
    xy1 = np.stack(list(np.meshgrid(np.arange(W), np.arange(H))) + [np.ones((H, W))], -1)[None].astype(np.float64)       # [1,H,W,3]
    mul = lambda p, M: np.einsum('bhwi,bhwij->bhwj', p, np.broadcast_to(M, (B, H, W, 3, 3)))
    ray = mul(np.broadcast_to(xy1, (B, H, W, 3)), m['K_inv'])
    pc1, pc2 = a['depth_1'][:, 0, :, :, None] * ray, a['depth_2'][:, 0, :, :, None] * ray
    P1, P2 = mul(pc1, m['R_1']) + m['t_1'][:, 0], mul(pc2, m['R_2']) + m['t_2'][:, 0]
    out = {'global_p1': P1}
    for key_q, key_f, s in (('p1_camera_2', 'dflow_1_2', a['sflow_1_2'][:, :, :, 0]), (None, 'staticflow_1_2', 0.0)):
        q = mul(P1 + s - m['t_2'][:, 0], m['R_2_T'])
        img = mul(q, m['K'])
        z = img[..., 2:]
        out[key_f] = np.where(z < 1e-3, 0.0, img[..., :2] / (z + 1e-8) - xy1[..., :2])
        if key_q:
            out[key_q], out['depth_image_1_2'] = q, z[..., 0][:, None]
    tx = np.clip(xy1[..., 0] + a['flow_1_2'][..., 0], 0, W - 1)
    ty = np.clip(xy1[..., 1] + a['flow_1_2'][..., 1], 0, H - 1)
    x0, y0 = np.floor(tx).astype(int), np.floor(ty).astype(int)
    x1, y1, wx, wy = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1), (tx - x0)[..., None], (ty - y0)[..., None]
    bi = np.arange(B)[:, None, None]
    warp = lambda v: ((1 - wy) * ((1 - wx) * v[bi, y0, x0] + wx * v[bi, y0, x1]) + wy * ((1 - wx) * v[bi, y1, x0] + wx * v[bi, y1, x1]))
    out['warped_p2_camera_2'], out['warped_global_p2'] = warp(pc2), warp(P2)
    out['sf_by_depth'] = out['warped_global_p2'] - P1
    out['depth_warp_1_2'] = warp(a['depth_2'][:, 0, :, :, None])[..., 0][:, None]
    return out


def test_float64_oracle_equals_an_independent_numpy_restatement():
    name = 'b3_7x9'
    got, want = S.surfaces(name, torch.float64), _numpy_surfaces(S.case(name))
    assert set(want) == set(S.SURFACES)
    for k in S.SURFACES:
        w = torch.from_numpy(np.ascontiguousarray(want[k])).reshape(got[k].shape)
        e = S.rel_err(got[k], w)
        print(k, e)
        assert e <= 1e-12, (k, e)


def test_rel_err_is_per_image_and_per_component():
    want = torch.zeros(2, 3, 4, 1, 3, dtype=torch.float64)
    want[0, ..., 0], want[0, ..., 1], want[1, ..., 0] = 150.0, 0.2, 1.0
    got = want.clone()
    assert S.rel_err(got, want) == 0.0
    got[0, 1, 2, 0, 1] += 0.02                                        # 10 % of the small component; 1e-4 of the tensor's maximum
    assert S.rel_err(got, want) == pytest.approx(0.1)
    got = want.clone()
    got[1, 0, 0, 0, 2] = 1e-30                                        # an all-zero component must be matched exactly
    assert S.rel_err(got, want) == float('inf')
    got[1, 0, 0, 0, 2] = float('nan')
    assert S.rel_err(got, want) != S.rel_err(got, want)
    planar = torch.ones(2, 1, 3, 4)
    assert S.rel_err(planar * 1.5, planar) == pytest.approx(0.5)


# -- the wrapper checks, as far as they are host arithmetic ----------------------------------------------------------------
@pytest.fixture
def no_launch(monkeypatch):
    def load():
        raise AssertionError('a refused call reached the library')
    monkeypatch.setattr(ops._lib, 'load', load)


def _inputs(B=2, H=4, W=6):
    cams = {k: torch.zeros((B, 1, 1, 1, 3) if k.startswith('t_') else (B, 1, 1, 3, 3)) for k in ops.CAM_KEYS}
    return dict(depth_1=torch.ones(B, 1, H, W), depth_2=torch.ones(B, 1, H, W), flow_1_2=torch.zeros(B, H, W, 2), cams=cams)


def test_shared_shape_checks_name_the_argument(no_launch):
    assert ops._image_size('unit', 'depth', torch.ones(2, 1, 4, 6)) == (2, 4, 6)
    for bad in (torch.ones(2, 4, 6), torch.ones(2, 2, 4, 6), torch.ones(0, 1, 4, 6), None, 3.0):
        with pytest.raises(RuntimeError, match=r'unit: depth must be a tensor \[B,1,H,W\]'):
            ops._image_size('unit', 'depth', bad)
    ok = torch.ones(2, 4, 6, 2)
    assert ops._shape_is('unit', 'flow', ok, ((2, 4, 6, 2),)) is ok
    for bad in (torch.ones(2, 6, 4, 2), torch.ones(1, 4, 6, 2), torch.ones(2, 4, 6), torch.ones(2, 4, 6, 2, 1), None, [1.0]):
        with pytest.raises(RuntimeError, match='unit: flow must be a tensor'):
            ops._shape_is('unit', 'flow', bad, ((2, 4, 6, 2),))
    # every shape is looked at before any device: a wrong shape late in the list wins over the CPU tensor before it
    with pytest.raises(RuntimeError, match='unit: b must be'):
        ops._images('unit', [('a', torch.ones(2, 3), ((2, 3),)), ('b', torch.ones(2, 4), ((2, 3), (3, 2))), ('c', None, ((1,),))])
    with pytest.raises(RuntimeError, match='unit: a must be a GPU tensor'):
        ops._images('unit', [('a', torch.ones(2, 3), ((2, 3),)), ('c', None, ((1,),))])
    assert ops._camera_shapes(3, 9) == ((3, 1, 1, 3, 3), (3, 3, 3), (3, 9)) and ops._camera_shapes(3, 3) == ((3, 1, 1, 1, 3), (3, 3))


def test_pack_cameras_checks_every_table_against_B(no_launch):
    cams = _inputs()['cams']
    for k in ops.CAM_KEYS:
        per = 3 if k.startswith('t_') else 9
        for bad in (cams[k][:1], torch.zeros(3, *cams[k].shape[1:]), torch.zeros(2, 1, 1, per), torch.zeros(2 * per),
                    torch.zeros(2, 1, 1, 3, 3) if per == 3 else torch.zeros(2, 1, 1, 1, 3), torch.zeros(2, 1, 1, 4, 4)):
            with pytest.raises(RuntimeError, match='unit: %s must be' % k):
                ops.pack_cameras(dict(cams, **{k: bad}), 2, 'unit')
        with pytest.raises(RuntimeError, match='cams must hold'):
            ops.pack_cameras({j: v for j, v in cams.items() if j != k}, 2, 'unit')
    flat = {k: v.reshape(2, -1) if k.startswith('t_') else v.reshape(2, 3, 3) for k, v in cams.items()}
    for good in (cams, flat, dict(flat, K=cams['K'].reshape(2, 9))):       # the shapes pass; the CPU tensor is what is left
        with pytest.raises(RuntimeError, match='unit: R_1 must be a GPU tensor'):
            ops.pack_cameras(good, 2, 'unit')


def test_wrappers_refuse_tensors_of_another_image_on_the_host(no_launch):
    a = _inputs()
    B, H, W = 2, 4, 6
    others = {'depth_2': [(1, 1, H, W), (B, 1, H + 1, W), (B, 1, H, W - 1), (B, H, W)],
              'flow_1_2': [(3, H, W, 2), (B, W, H, 2), (B, H, W, 3), (B, 2, H, W)]}
    for fn, extra in ((ops.warp_surfaces, {}), (ops.warp_surfaces_backward, {'grads': {}})):
        for name, shapes in others.items():
            for sh in shapes:
                with pytest.raises(RuntimeError, match='%s: %s must be' % (fn.__name__, name)):
                    fn(**dict(a, **{name: torch.zeros(sh)}), **extra)
        for sh in ((B, H, W, 3), (B, H, W, 1, 2), (1, H, W, 1, 3), (B, W, H, 1, 3)):
            with pytest.raises(RuntimeError, match='%s: sflow_1_2 must be' % fn.__name__):
                fn(sflow_1_2=torch.zeros(sh), **a, **extra)
        with pytest.raises(RuntimeError, match='%s: K_inv must be' % fn.__name__):
            fn(**dict(a, cams=dict(a['cams'], K_inv=torch.zeros(3, 1, 1, 3, 3))), **extra)
        with pytest.raises(RuntimeError, match='%s: depth_1 must be a tensor' % fn.__name__):
            fn(**dict(a, depth_1=torch.ones(B, H, W)), **extra)
        with pytest.raises(RuntimeError, match='depth_1 must be a GPU tensor'):
            fn(**a, **extra)
    with pytest.raises(RuntimeError, match='warp_surfaces: want holds'):
        ops.warp_surfaces(want=('global_p1', 'global_p2'), **a)
    with pytest.raises(RuntimeError, match='warp_surfaces_backward: grads holds'):
        ops.warp_surfaces_backward(grads={'dflow': torch.zeros(B, H, W, 2)}, **a)
    for k in S.SURFACES:
        good = ops._surface_shape(k, B, H, W)
        for sh in ((1,) + good[1:], good[:-1] + (good[-1] + 1,), ops._surface_shape(k, B, W, H)):
            with pytest.raises(RuntimeError, match='warp_surfaces_backward: the gradient of %s must be' % k):
                ops.warp_surfaces_backward(grads={k: torch.zeros(sh)}, **a)
    for fn, name in ((ops.flow_warp, 'buffer'), (ops.flow_warp_backward, 'g_out')):
        for sh in ((1, H, W, 2), (B, H, W + 1, 2), (B, W, H, 2), (B, H, W), (B, 2, H, W)):
            with pytest.raises(RuntimeError, match='%s: flow_1_2 must be' % fn.__name__):
                fn(torch.zeros(B, 3, H, W), torch.zeros(sh))
        with pytest.raises(RuntimeError, match=r'%s: %s must be a tensor \[B,C,H,W\]' % (fn.__name__, name)):
            fn(torch.zeros(B, H, W), torch.zeros(B, H, W, 2))
        with pytest.raises(RuntimeError, match='%s: %s must be a GPU tensor' % (fn.__name__, name)):
            fn(torch.zeros(B, 3, H, W), torch.zeros(B, H, W, 2))
    R, t = torch.zeros(B, 3, 3), torch.zeros(B, 3)
    for args, name in (((torch.ones(B, H, W), R, t, R), 'depth'), ((torch.ones(B, 1, H, W), R[:1], t, R), 'R'),
                       ((torch.ones(B, 1, H, W), R, torch.zeros(B, 4), R), 't'), ((torch.ones(B, 1, H, W), R, t, torch.zeros(B, 3)), 'K_inv')):
        with pytest.raises(RuntimeError, match='unproject: %s must be' % name):
            ops.unproject(*args)
    for planar, g in ((True, torch.zeros(B, 3, H, W)), (False, torch.zeros(B, H, W, 1, 3)), (False, torch.zeros(B, H, W, 3))):
        for kw, name in ((dict(R=R[:1], K_inv=R), 'R'), (dict(R=R, K_inv=torch.zeros(3, 3, 3)), 'K_inv'),
                         (dict(R=R, K_inv=R, scale=torch.ones(2)), 'scale')):
            with pytest.raises(RuntimeError, match='unproject_backward: %s must be' % name):
                ops.unproject_backward(g, planar, **kw)
        with pytest.raises(RuntimeError, match='unproject_backward: g_points must be a GPU tensor'):
            ops.unproject_backward(g, planar, R, R)
    for planar, g in ((True, torch.zeros(B, 2, H, W)), (False, torch.zeros(B, H, W, 2)), (True, torch.zeros(B, H, W))):
        with pytest.raises(RuntimeError, match='unproject_backward: g_points must be'):
            ops.unproject_backward(g, planar, R, R)
