"""CPU-only checks of the forward splat (csrc/splat.hip) and of Model.render's host half (models/render.py): the C entries
exist and refuse bad arguments before any HIP call, the workspace size, render_plan, the fixed-point shift, and the float64
specification (tests/splat_spec.py) checked against cases whose answer is known -- plus the condition every GPU comparison
rests on: under the specification alone, at most 3 % of the target pixels of every input set the GPU tests use are fragile."""
import ctypes

import numpy as np
import pytest
import torch

import helpers
import splat_spec as S
import store_spec


def _lib():
    from dvd_hip import _lib
    return _lib, _lib.load()


def _err(lib):
    return lib.dvd_last_error().decode()


P = ctypes.c_void_p(64)      # a non-null pointer that is never followed: every call below is refused before any HIP call


def _zmin(lib, **over):
    a = dict(points=P, planar=1, values=P, valid=None, view=P, R=P, t=P, K_T=P, V=2, zbuf=P, S=3, C=3, H=11, W=21, z_near=1e-3,
             w_tap=1.0 / 64)
    a.update(over)
    return lib.dvd_splat_zmin(a['points'], a['planar'], a['values'], a['valid'], a['view'], a['R'], a['t'], a['K_T'], a['V'],
                              a['zbuf'], a['S'], a['C'], a['H'], a['W'], a['z_near'], a['w_tap'], None)


def _acc(lib, **over):
    a = dict(points=P, planar=1, values=P, valid=None, view=P, R=P, t=P, K_T=P, V=2, zbuf=P, acc=P, S=3, C=3, H=11, W=21,
             z_near=1e-3, z_tol=0.05, w_tap=1.0 / 64, value_bound=1.0, shift=40, n_max=3 * 11 * 21)
    a.update(over)
    return lib.dvd_splat_accumulate(a['points'], a['planar'], a['values'], a['valid'], a['view'], a['R'], a['t'], a['K_T'],
                                    a['V'], a['zbuf'], a['acc'], a['S'], a['C'], a['H'], a['W'], a['z_near'], a['z_tol'],
                                    a['w_tap'], a['value_bound'], a['shift'], a['n_max'], None)


def _res(lib, **over):
    a = dict(zbuf=P, acc=P, V=2, C=3, H=11, W=21, shift=40, w_min=0.25, value_bound=1.0, fill=0.0, image=P, depth=P, weight=P,
             hit=P)
    a.update(over)
    return lib.dvd_splat_resolve(a['zbuf'], a['acc'], a['V'], a['C'], a['H'], a['W'], a['shift'], a['w_min'], a['value_bound'],
                                 a['fill'], a['image'], a['depth'], a['weight'], a['hit'], None)


def test_the_four_symbols_exist_and_refuse_bad_arguments():
    _l, lib = _lib()
    for name in ('dvd_splat_workspace_bytes', 'dvd_splat_zmin', 'dvd_splat_accumulate', 'dvd_splat_resolve'):
        assert name in _l.SIGNATURES and hasattr(lib, name), name
    nan = float('nan')
    bad_zmin = [dict(points=None), dict(values=None), dict(view=None), dict(R=None), dict(t=None), dict(K_T=None),
                dict(zbuf=None), dict(C=0), dict(C=9), dict(H=1), dict(W=1), dict(z_near=-1e-3), dict(z_near=nan),
                dict(w_tap=0.0), dict(w_tap=0.26), dict(w_tap=-0.1), dict(w_tap=nan), dict(S=0), dict(V=0)]
    for over in bad_zmin:
        assert _zmin(lib, **over) == _l.DVD_EINVAL, over
        assert 'splat_zmin' in _err(lib), over
    assert _zmin(lib, points=None) == _l.DVD_EINVAL and 'null' in _err(lib)
    bad_acc = bad_zmin[:6] + [dict(zbuf=None), dict(acc=None), dict(C=0), dict(C=9), dict(H=1), dict(W=1), dict(z_near=-1.0),
                              dict(z_tol=-0.01), dict(z_tol=nan), dict(w_tap=0.0), dict(w_tap=0.5), dict(value_bound=0.0),
                              dict(value_bound=-1.0), dict(value_bound=nan), dict(shift=0), dict(shift=41), dict(shift=-3),
                              dict(n_max=0), dict(shift=40, n_max=(1 << 22) + 1), dict(shift=30, n_max=(1 << 32) + 1)]
    for over in bad_acc:
        assert _acc(lib, **over) == _l.DVD_EINVAL, over
        assert 'splat_accumulate' in _err(lib), over
    bad_res = [dict(zbuf=None), dict(acc=None), dict(image=None), dict(depth=None), dict(weight=None), dict(hit=None), dict(C=0),
               dict(C=9), dict(H=1), dict(W=1), dict(shift=0), dict(shift=41), dict(w_min=0.0), dict(w_min=-1.0), dict(w_min=nan),
               dict(value_bound=0.0), dict(value_bound=-2.0)]
    for over in bad_res:
        assert _res(lib, **over) == _l.DVD_EINVAL, over
        assert 'splat_resolve' in _err(lib), over


def test_workspace_bytes():
    _l, lib = _lib()
    ws = lib.dvd_splat_workspace_bytes
    assert ws(1, 1, 2, 2) == 4 * (4 + 2 * 8)
    assert ws(2, 3, 11, 21) == 2 * 11 * 21 * (4 + 4 * 8)
    assert ws(8, 3, 384, 672) == 8 * 384 * 672 * 36
    assert ws(1, 8, 12, 20) == 12 * 20 * (4 + 9 * 8)
    assert ws(65535, 8, 4096, 4096) == 65535 * 4096 * 4096 * 76      # beyond 32 bits
    for bad in ((0, 3, 11, 21), (-1, 3, 11, 21), (2, 0, 11, 21), (2, 9, 11, 21), (2, 3, 1, 21), (2, 3, 11, 1)):
        assert ws(*bad) == 0, bad


def test_ops_splat_refuses_cpu_tensors_and_bad_parameters():
    from dvd_hip import ops
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.splat(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), [0], {}, 1)
    with pytest.raises(RuntimeError, match='w_tap'):
        ops._splat_params('splat', w_tap=0.3)
    with pytest.raises(RuntimeError, match='z_near'):
        ops._splat_params('splat', z_near=-1.0)
    assert set(ops.BYTE_CLASS_KERNELS['geometry']) >= {'splat_zmin_kernel', 'splat_accumulate_kernel', 'splat_resolve_kernel'}


def test_shift_formula_keeps_n_unit_taps_below_2_to_62():
    from dvd_hip import ops
    for n in (1, 2, 3, 4, 5, 231, 4 * 384 * 672, 1 << 22, (1 << 22) + 1, 1 << 23, (1 << 30) - 1, 1 << 30, 65535 * (1 << 30)):
        shift = ops.splat_shift(n)
        ceil_log2 = 0
        while (1 << ceil_log2) < n:
            ceil_log2 += 1
        assert shift == min(40, 62 - ceil_log2), n
        assert 1 <= shift <= 40
        assert n * (1 << shift) <= 1 << 62, n      # n taps of magnitude 1: exact Python integers
        _l, lib = _lib()
        # the kernel entry accepts exactly this shift for this n_max (it is refused for a later reason: the stream of this
        # call is never reached) and refuses the next larger one where the formula, not the cap of 40, is the limit
        if shift < 40:
            assert _acc(lib, shift=shift + 1, n_max=n) == _l.DVD_EINVAL and 'overflows' in _err(lib)
    assert ops.splat_shift(4 * 384 * 672) == 40 and ops.splat_shift((1 << 22) + 1) == 39
    with pytest.raises(RuntimeError):
        ops.splat_shift(0)


def test_render_plan():
    from dvd_hip.models.render import render_plan
    assert render_plan(7, [3, 5], [[1, 2, 3], [5]]) == ([1, 2, 3, 5], [0, 0, 0, 1], [2, 1, 0, 0])
    assert render_plan(7, [3, 5], [[1, 2, 3], [5]], advect=False) == ([1, 2, 3, 5], [0, 0, 0, 1], [0, 0, 0, 0])
    assert render_plan(7, [2], [[6, 0]], advect=False) == ([6, 0], [0, 0], [0, 0])
    assert render_plan(7, np.array([6]), [np.array([0, 6])]) == ([0, 6], [0, 0], [6, 0])
    assert render_plan(7, torch.tensor([1]), [torch.tensor([1.0])]) == ([1], [0], [0])
    for args, msg in ((([], []), 'no target'), (([3], []), 'source lists'), (([3, 4], [[1]]), 'source lists'),
                      (([3], [[]]), 'no source'), (([3], [[1.5]]), 'not an integer'), (([3.5], [[1]]), 'not an integer'),
                      (([3], [['a']]), 'not an integer'), (([3], [[True]]), 'not an integer'), (([7], [[1]]), 'outside'),
                      (([3], [[-1]]), 'outside'), (([3], [[7]]), 'outside'), (([3], [[4]]), 'later than'),
                      (([3], [3]), 'must be a list'), (([3], [[float('nan')]]), 'not an integer')):
        with pytest.raises(ValueError, match=msg):
            render_plan(7, *args)
    with pytest.raises(ValueError, match='outside'):
        render_plan(7, [3], [[7]], advect=False)
    with pytest.raises(ValueError, match='n_frames'):
        render_plan(0, [0], [[0]])


def test_spec_a_frame_into_its_own_camera_returns_its_image():
    """Points un-projected from a camera and splatted back land on their own pixels: weight 1, hit everywhere."""
    fx = helpers.load_golden(S.RENDER_FX)
    N, H, W = int(fx['N']), int(fx['H']), int(fx['W'])
    img = store_spec.random_tree(N, H, W, [1], S.RENDER_IMG_SEED)['fr_img'].transpose(0, 3, 1, 2)
    res = S.render_case(fx, img, None, 'own')
    assert res['hit'].all() and S.fragile_share(res) == 0.0
    np.testing.assert_allclose(res['image'][0], img[2], atol=2e-6)
    np.testing.assert_allclose(res['weight'], 1.0, atol=1e-5)
    np.testing.assert_allclose(res['depth'][0], fx['in_depth'][2], rtol=1e-6)


def test_spec_two_planes():
    case = S.two_planes()
    near = S.run(case, z_tol=0.05)
    assert near['hit'].all()
    np.testing.assert_allclose(near['image'], 0.25, atol=1e-6)
    np.testing.assert_allclose(near['depth'], 2.0, atol=1e-6)
    np.testing.assert_allclose(near['weight'], 1.0, atol=1e-5)
    both = S.run(case, z_tol=1.5)
    np.testing.assert_allclose(both['image'], 0.5, atol=1e-6)
    np.testing.assert_allclose(both['depth'], 2.0, atol=1e-6)
    np.testing.assert_allclose(both['weight'], 2.0, atol=1e-5)
    far_only = dict(case, view=[-1, 0])
    np.testing.assert_allclose(S.run(far_only)['image'], 0.75, atol=1e-6)
    assert not S.run(dict(case, view=[-1, 1]))['hit'].any() and (S.run(dict(case, view=[-1, 1]), fill=0.5)['image'] == 0.5).all()


def test_spec_drops_hostile_points_and_clamps():
    case = S.CASES['hostile'][0]()
    res = S.run(case)
    alone = S.run(dict(case, view=[0, 0, 0, -1]))
    assert np.array_equal(res['image'][0], alone['image'][0]) and np.array_equal(res['hit'][0], alone['hit'][0])
    assert np.isfinite(res['image']).all() and np.isfinite(res['weight']).all() and not alone['hit'][1].any()
    clamped, par = S.CASES['clamped']
    res = S.run(clamped(), **par)
    assert np.abs(res['image']).max() <= 1.0 and (np.abs(res['image']) == 1.0).any()


@pytest.mark.parametrize('name', sorted(S.CASES))
def test_fragile_share_of_the_splat_cases_is_within_the_cap(name):
    make, params = S.CASES[name]
    case = make()
    r64, r32 = S.run(case, **params), S.run(case, dtype=np.float32, **params)
    share = S.fragile_share(r64)
    print('%s: %.2f %% fragile, %.0f %% hit' % (name, 100 * share, 100 * r64['hit'].mean()))
    assert share <= S.FRAGILE_CAP
    assert r64['hit'].mean() > 0.4      # the case draws something
    # outside the fragile set fp32 and float64 agree about `hit`: the yardstick of the GPU tests is defined
    assert not ((r64['hit'] != r32['hit']) & ~S.fragile(r64)).any()


def _sd(fx, time_dependent):
    from dvd_hip.networks.sceneflow_field import SceneFlowFieldNet
    net = SceneFlowFieldNet(net_width=256, n_layers=4, time_dependent=time_dependent, N_freq_xyz=16, N_freq_t=16)
    helpers.seeded_fill_(net, int(fx['seed']) + (0 if time_dependent else 1))      # the networks of tests/test_49
    return {k: v.detach() for k, v in net.state_dict().items()}


@pytest.mark.parametrize('name', sorted(S.RENDER_CASES))
def test_fragile_share_of_the_render_cases_is_within_the_cap(name):
    fx = helpers.load_golden(S.RENDER_FX)
    N, H, W = int(fx['N']), int(fx['H']), int(fx['W'])
    img = store_spec.random_tree(N, H, W, [1], S.RENDER_IMG_SEED)['fr_img'].transpose(0, 3, 1, 2)
    sd = _sd(fx, S.RENDER_CASES[name]['time_dependent'])
    r64 = S.render_case(fx, img, sd, name)
    r32 = S.render_case(fx, img, sd, name, dtype=np.float32)
    share = S.fragile_share(r64)
    print('%s: %.2f %% fragile, %.0f %% hit' % (name, 100 * share, 100 * r64['hit'].mean()))
    assert share <= S.FRAGILE_CAP and r64['hit'].mean() > 0.25
    assert not ((r64['hit'] != r32['hit']) & ~S.fragile(r64)).any()
