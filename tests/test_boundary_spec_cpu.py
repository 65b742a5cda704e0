"""The premises of tests/test_51_beyond_the_grid_gpu.py, checked on the CPU for every one of its cases: the shape exceeds the
launch cap it is meant to cross, the float64 reference survives a round trip through the kernel's storage format unchanged,
and the absolute terms of every accumulated quantity sum to less than 2^24 -- so fp32 arithmetic is exact in any order and
"equal bit for bit" is what a correct kernel gives.  Also: the references of tests/boundary_spec.py against independent
formulations of the same operations, and its two loss-scale models at hand-computed points."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import boundary_spec as S
import test_51_beyond_the_grid_gpu as T51


def _exact(t, *dtypes):
    return all(S.survives(t, d) for d in (torch.float32,) + dtypes)


@pytest.mark.parametrize('relu_in', [True, False])
def test_head1x1_case_crosses_the_cap_and_is_exact_in_fp32_and_fp16(relu_in):
    x, w, b, gy = S.head1x1_exact_inputs()
    N, C, H, W = x.shape
    items = N * (H * W // 4)
    assert H * W % 4 == 0 and T51.A16_CAP_ITEMS < items < 2 * T51.A16_CAP_ITEMS          # a second, ragged trip
    assert (items - T51.A16_CAP_ITEMS) % T51.A16_BLOCK and T51.A16_CAP_ITEMS // (H * W // 4) == N - 1   # ... inside the last image
    assert float(w.abs().max()) == 2 and float(gy.abs().max()) == 2
    assert S.gscale_begin_ref(2.0, 2.0, 4.0) == 2.0
    ref = S.head1x1_ref(x, w, b, gy, relu_in, S=2.0)
    assert _exact(x, torch.float16) and _exact(gy) and _exact(w) and _exact(ref['y'])
    assert _exact(ref['gx'], torch.float16) and _exact(ref['gw']) and _exact(ref['gb'])
    for k in ('y_abs', 'gw_abs', 'gb_abs'):
        assert float(ref[k].max()) < S.EXACT_LIMIT, k
    assert float(ref['gx'].abs().max()) == 8.0                          # a +-2 of w meets a +-2 of gy on a live pixel
    # the definition, from autograd
    xd, wd, bd = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.conv2d(F.relu(xd) if relu_in else xd, wd.view(1, C, 1, 1), bd)
    y.backward(gy)
    assert torch.equal(y.detach(), ref['y']) and torch.equal(2.0 * xd.grad, ref['gx'])
    assert torch.equal(wd.grad, ref['gw']) and torch.equal(bd.grad, ref['gb'])


def test_head3x3_case_crosses_both_caps_and_is_exact():
    x, w, b, gy = S.head3x3_exact_inputs()
    N, C, H, W = x.shape
    total = N * H * W
    assert T51.A16_CAP_ITEMS < total < 2 * T51.A16_CAP_ITEMS and (total - T51.A16_CAP_ITEMS) % T51.A16_BLOCK
    assert T51.A16_CAP_ITEMS // (H * W) == N - 1
    assert total > T51.H3_WGRAD_CAP_PIXELS and S.head3x3_chunk(total) > T51.H3_WGRAD_CHUNK_PIXELS
    assert (H * W) % S.head3x3_chunk(total) and C % 8                   # chunks straddle the images; a partial channel group
    assert float(w.abs().max()) == 2 and float(gy.abs().max()) == 2
    ref = S.head3x3_ref(x, w, b, gy, S=2.0)
    assert _exact(x, torch.float16) and _exact(ref['y']) and _exact(ref['gx'], torch.float16)
    assert _exact(ref['gw']) and _exact(ref['gb'])
    for k in ('y_abs', 'gx_abs', 'gw_abs', 'gb_abs'):
        assert float(ref[k].max()) < S.EXACT_LIMIT, k
    # the definition written out tap by tap at a few pixels, the corners included
    xp = F.pad(x, (1, 1, 1, 1))
    for n, r, c in [(0, 0, 0), (N - 1, H - 1, W - 1), (1, 0, W - 1), (2, 137, 411)]:
        assert float(ref['y'][n, 0, r, c]) == float((xp[n, :, r:r + 3, c:c + 3] * w[0]).sum() + b[0])


@pytest.mark.parametrize('n', [S.ADD_F16_VEC_N, S.ADD_F16_SCALAR_N])
def test_add_f16_cases_cross_the_cap_and_are_exact_in_fp16(n):
    a, b = S.add_f16_exact_inputs(n)
    items = n // 4 if n % 4 == 0 else n
    assert T51.A16_CAP_ITEMS < items < 2 * T51.A16_CAP_ITEMS and (items - T51.A16_CAP_ITEMS) % T51.A16_BLOCK
    assert n > T51.A16_CAP_ITEMS                       # the misaligned views take the scalar path at the vector case's n
    assert _exact(a, torch.float16) and _exact(b, torch.float16) and _exact(a + b, torch.float16)
    assert float((a.abs() + b.abs()).max()) < 2048


def test_to_half_cases():
    n4, n3 = S.TO_HALF_N
    assert n4 % 4 == 0 and n3 % 4 != 0 and n4 // 4 > T51.A16_CAP_ITEMS and (n4 // 4 - T51.A16_CAP_ITEMS) % T51.A16_BLOCK
    g = S.small_ints((n4,), 41, -1000, 1000)
    assert _exact(g, torch.float16) and _exact(g * 0.125)


def test_subsample_case_crosses_the_cap_and_is_exact():
    shape, out_shape = S.SUBSAMPLE_SHAPE, S.subsample_out_shape(S.SUBSAMPLE_SHAPE)
    N, C, H, W = shape
    assert H % 2 and W % 2
    fwd, bwd = int(np.prod(out_shape)), N * C * H * ((W + 1) // 2)
    for items in (fwd, bwd):
        assert items > T51.SUBSAMPLE_CAP_ITEMS and items % T51.SUBSAMPLE_CAP_ITEMS % 256
    x, gy = S.pool_exact_inputs(shape, out_shape, 1, 1024, 51)
    assert _exact(x.double(), torch.float16) and _exact(gy.double(), torch.float16)
    y, gx = S.subsample_ref(x, gy)
    assert y.shape == out_shape and torch.equal(y, x.double()[:, :, ::2, ::2])
    assert float(gx.sum()) == float(gy.double().sum()) and torch.equal(gx[:, :, ::2, ::2], gy.double())


@pytest.mark.parametrize('k,st,pad', S.AVGPOOL_CFGS)
def test_avgpool_cases_cross_the_cap_and_are_exact(k, st, pad):
    shape = S.AVGPOOL_SHAPE
    out_shape = S.avgpool_out_shape(shape, k, st, pad)
    for items in (int(np.prod(out_shape)), int(np.prod(shape))):
        assert items > T51.AVGPOOL_CAP_ITEMS and items % T51.AVGPOOL_CAP_ITEMS % 256
    x, gy = S.pool_exact_inputs(shape, out_shape, 36, 3, 61)
    assert _exact(x.double(), torch.float16) and _exact(gy.double(), torch.float16)
    y, gx = S.avgpool_ref(x, k, st, pad, gy)
    assert y.shape == out_shape and _exact(y, torch.float16) and _exact(gx, torch.float16)
    assert torch.equal(y, y.round()) and torch.equal(gx, gx.round())           # whole numbers: no division ever rounds
    # window sums of absolute values (forward) and of |gy| / k^2 (backward) stay far below 2^24, and below fp16's 2048
    assert float(F.avg_pool2d(x.double().abs(), k, st, pad).max()) * k * k < 2048
    assert float(gy.abs().max()) / (k * k) * 4 < 2048
    assert float(y.abs().max()) > 0 and float(gx.abs().max()) > 0


def test_gather_cases_cross_the_tile_cap():
    t1, t2 = S.gather_tiles(S.GATHER_LAUNCH_1), S.gather_tiles(S.GATHER_LAUNCH_2)
    assert t1 == [(855, 16), (1, 4), (1, 1), (1, 4)] and t2 == [(977, 4)]
    assert S.GATHER_B * t1[0][0] == 4275 > T51.GATHER_MAX_TILES       # every tile of the small tensors: second trip only
    assert S.GATHER_B * t2[0][0] > T51.GATHER_MAX_TILES
    for launch in (S.GATHER_LAUNCH_1, S.GATHER_LAUNCH_2):
        for t, (shape, dtype) in zip(S.gather_inputs(launch, 71), launch):
            assert t.shape == shape and t.dtype == dtype and not bool(torch.isnan(t.double()).any())


def test_loss_scale_models_at_hand_computed_points():
    # begin: max|g| max|w| = f 2^e, f in [0.5, 1): S = 2^(target - e)
    assert S.gscale_begin_ref(2.0, 2.0, 4.0) == 2.0                    # 4 = 0.5 * 2^3
    assert S.gscale_begin_ref(1.0, 1.0, 4.0) == 8.0                    # 1 = 0.5 * 2^1
    assert S.gscale_begin_ref(1.5, 1.0, 4.0) == 8.0
    assert S.gscale_begin_ref(1e-38, 1.0, 14.0) == 2.0 ** 120 and S.gscale_begin_ref(1e38, 1.0, -24.0) == 2.0 ** -120
    for m in (0.0, float('inf'), float('nan'), 3.2e38):
        assert S.gscale_begin_ref(m, 1.0, 4.0) == 1.0
    assert S.gscale_begin_ref(1e30, 1e30, 4.0) == 1.0                  # the fp32 product overflows
    # end: the transitions tests/test_10_act_fp16_gpu.py pins on the kernel
    st = [1.0, 1.0, 4.0] + [0.0] * 13
    for obs, fwd, want in [(10000.0, 0.0, [4.0, 0.0, 0.0, 0.0]), (1000.0, 0.0, [7.0, 0.0, 0.0, 0.0]),
                           (1.0, 0.0, [11.0, 0.0, 0.0, 0.0]), (40000.0, 0.0, [9.0, 0.0, 0.0, 0.0]),
                           (2.0 ** 20, 0.0, [2.0, 0.0, 1.0, 1.0]), (float('inf'), 0.0, [-6.0, 0.0, 1.0, 2.0]),
                           (8192.0, 0.0, [-6.0, 0.0, 0.0, 2.0]), (8192.0, 70000.0, [-6.0, 0.0, 1.0, 3.0])]:
        st[3], st[6] = obs, fwd
        st = S.gscale_end_model(st)
        assert st[2:6] == want and st[6] == 0.0
    assert st[8:11] == [1.0, 1.0, 1.0]


def test_loss_scale_models_at_the_edges_the_gpu_tests_use():
    """What the two models say at the cases of tests/test_50_fp16_boundary_gpu.py, written out by hand."""
    got = [S.gscale_begin_ref(f * 2.0 ** k / 2.0, 2.0, 4.0) for k in (-20, 0, 10) for f in (1.0, 1.5)]
    assert got == [2.0 ** 23, 2.0 ** 23, 8.0, 8.0, 2.0 ** -7, 2.0 ** -7]
    assert S.gscale_begin_ref(3.0, 1.0, 4.0) == 4.0 and S.gscale_begin_ref(1.0, 8.0, 4.0) == 1.0
    K = S.GS_OVERFLOW

    def end(target, obs, fwd=0.0):
        s = S.gscale_end_model([2.0, 0.5, target, obs, 1.0, 3.0, fwd, 0.0, 1.0, 2.0, 1.0] + [0.0] * 5)
        assert s[:2] == [2.0, 0.5] and s[3] == 0.0 and s[6] == 0.0
        return s[2], s[4], s[5], s[8], s[9], s[10]
    assert end(4.0, 0.0) == (4.0, 0.0, 3.0, 0.0, 2.0, 0.0) and end(4.0, 2.0 ** 13) == (4.0, 0.0, 3.0, 0.0, 2.0, 0.0)
    assert end(4.0, float(np.nextafter(K, np.float32(0)))) == (2.0, 0.0, 3.0, 0.0, 2.0, 0.0)
    assert end(4.0, float(K)) == (1.0, 1.0, 4.0, 0.0, 2.0, 0.0)
    assert end(4.0, float(np.nextafter(K, np.float32(1e9)))) == (1.0, 1.0, 4.0, 0.0, 2.0, 0.0)
    assert end(12.0, 1.0)[0] == 14.0 and end(13.0, 2.0 ** 11)[0] == 14.0 and end(14.0, 1000.0)[0] == 14.0
    assert end(-20.0, float('inf'))[0] == -24.0 and end(-22.0, 2.0 ** 20)[0] == -24.0 and end(-24.0, 2.0 ** 16)[0] == -24.0
    assert end(4.0, float('nan')) == (-4.0, 1.0, 4.0, 0.0, 2.0, 0.0)
    assert end(4.0, 2.0 ** 13, 65504.0) == (4.0, 1.0, 4.0, 1.0, 3.0, 2.0)
    assert end(4.0, 2.0 ** 13, 65472.0) == (4.0, 0.0, 3.0, 0.0, 2.0, 0.0)
