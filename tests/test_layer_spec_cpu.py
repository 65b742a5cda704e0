"""tests/layer_spec.py held to ATen on the CPU, and the case tables of tests/test_68_layer_kernels_gpu.py held to the path
predicates: every row must reach the path it names, so a table cannot drift when someone edits a threshold in the host code
(the predicates quote the lines they restate)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layer_spec as S


# -- BatchNorm + residual + ReLU ------------------------------------------------------------------------------------------------
def _bn_autograd(t, relu, dtype):
    """relu(batch_norm(x) (+ r)) by autograd in `dtype` -> y, gx, gr, ggamma, gbeta (eps as the kernels see it)."""
    c = {k: (None if v is None else v.to(dtype)) for k, v in t.items()}
    x, gamma, beta = c['x'].clone().requires_grad_(True), c['gamma'].clone().requires_grad_(True), c['beta'].clone().requires_grad_(True)
    r = None if c['r'] is None else c['r'].clone().requires_grad_(True)
    y = F.batch_norm(x, c['mean'], c['var'], gamma, beta, False, 0.0, S.bn_eps32())
    if r is not None:
        y = y + r
    if relu:
        y = y.relu()
    y.backward(c['gy'])
    return dict(y=y.detach(), gx=x.grad, gr=None if r is None else r.grad, ggamma=gamma.grad, gbeta=beta.grad)


@pytest.mark.parametrize('case', S.BN_CASES, ids=S.bn_case_id)
def test_bn_spec_is_float64_autograd(case):
    """The specification against float64 autograd of the ATen composition: only the association differs (x s + b against
    (x - mean) rstd gamma + beta), so a handful of float64 roundings of M."""
    (N, C, H, W), res, relu, affine, _, _ = case
    t = S.bn_inputs(case)
    ref = _bn_autograd(t, relu, torch.float64)
    y, pre, M = S.bn_forward(t['x'], t['r'], t['gamma'], t['beta'], t['mean'], t['var'], relu)
    assert np.all(np.abs(y - ref['y'].numpy()) <= 16 * 2.0 ** -53 * M)
    assert np.all(M >= np.abs(pre) * (1 - 1e-12))
    mask = (ref['y'].numpy() > 0) if relu else None
    b = S.bn_backward(t['gy'], mask, t['x'], t['gamma'], t['mean'], t['var'])
    assert np.all(np.abs(b['gx'] - ref['gx'].numpy()) <= 16 * 2.0 ** -53 * b['M_gx'])
    if res:
        assert np.array_equal(b['gr'], ref['gr'].numpy())
    n = N * H * W
    assert np.all(np.abs(b['gbeta'] - ref['gbeta'].numpy()) <= n * 2.0 ** -53 * b['M_gbeta'])
    assert np.all(np.abs(b['ggamma'] - ref['ggamma'].numpy()) <= (n + 16) * 2.0 ** -53 * b['M_ggamma'])
    if C >= 3 and relu and affine:
        assert not y[:, 0].any() and b['gbeta'][0] == 0.0 and b['ggamma'][0] == 0.0      # the fully masked channel
    if C >= 3:
        assert b['gbeta'][C - 1] == 0.0 and b['ggamma'][C - 1] == 0.0                    # the channel with gy == 0
    assert float(t['var'].min()) == pytest.approx(0.05) and bool((t['gamma'] < 0).any()) == affine


@pytest.mark.parametrize('case', [c for c in S.BN_CASES if c[2]], ids=S.bn_case_id)
def test_bn_spec_alone_leaves_few_signs_undecided(case):
    """The GPU test asserts the kernel's [y > 0] wherever |pre| of the specification exceeds the bound: on these inputs (and on
    their fp16-rounded copies) that must be all but 1 % of the elements -- leaving out the channel masked on purpose would
    only lower the share, so it is counted."""
    (N, C, H, W), res, relu, _, _, _ = case
    for f in (lambda v: v, S.rounded_to_half):
        t = S.bn_inputs(case)
        _, pre, M = S.bn_forward(f(t['x']), f(t['r']), t['gamma'], t['beta'], t['mean'], t['var'], relu)
        undecided = np.abs(pre) <= S.bn_c_y(res) * S.U * M
        assert undecided.mean() < 0.01, undecided.mean()


@pytest.mark.parametrize('shape', list(S.BN_PATHS))
def test_bn_table_rows_reach_their_paths(shape):
    N, C, H, W = shape
    want = S.BN_PATHS[shape]
    got = dict(npb=S.bn_bwd_npb(N, C, H * W), records=S.bn_records(N, C, H * W), vec=S.bn_vec(H * W), chunks=S.bn_chunks(H * W),
               last=S.bn_last_chunk(H * W))
    assert got == want
    assert {c[0] for c in S.BN_CASES} == set(S.BN_PATHS)


def test_bn_tables_cover_what_they_claim():
    P = S.BN_PATHS
    npb = [s for s, p in P.items() if p['npb'] > 1]
    assert any(P[s]['vec'] for s in npb) and any(not P[s]['vec'] for s in npb)                # npb > 1 on both loops
    assert any(P[s]['npb'] == s[0] and P[s]['records'] == 1 for s in npb)                     # npb = N
    assert any(s[0] % P[s]['npb'] == 1 for s in npb if P[s]['npb'] < s[0])                    # a last block of one image
    assert any(p['chunks'] > 1 and p['vec'] and p['last'] < 256 for p in P.values())          # a short last chunk, 16-byte loop
    assert any(p['chunks'] > 1 and not p['vec'] and p['last'] == 1 for p in P.values())
    assert any(p['chunks'] == 1 and p['last'] == S.K_BN_CHUNK for p in P.values())
    # every option both ways; relu=False and a missing gx on an npb > 1 shape
    for i in range(1, 6):
        assert {c[i] for c in S.BN_CASES} == {True, False}, i
    assert any(not c[2] and c[0] in npb for c in S.BN_CASES) and any(not c[4] and c[0] in npb for c in S.BN_CASES)
    # the rounding counts grow with the chain they count
    assert S.bn_c_gbeta(5, 512, 16) == 2 + 3 + 8 + 1 and S.bn_c_ggamma(5, 512, 16) == 1 + 16 + 8 + 1
    assert S.bn_c_gbeta(1, 2, 4097) == 15 + 8 + 1 and S.bn_c_ggamma(1, 2, 4097) == 1 + 16 + 8 + 1


# -- bilinear resize ------------------------------------------------------------------------------------------------------------
X2_SHAPES = list(S.UP_X2) + [(1, 2, 12, 21), (1, 1, 24, 42), (1, 2, 70, 150)]


@pytest.mark.parametrize('align', [False, True])
@pytest.mark.parametrize('shape', X2_SHAPES)
def test_resize_spec_against_aten_fp32_for_x2(shape, align):
    """fp32 ATen forms the same fp32 coordinate for x2 and blends in fp32 with the roundings counted for the kernel (8 forward;
    the backward scatters one product per tap), so it must stay within those counts of the specification."""
    N, C, H, W = shape
    x, gy = S.up_inputs(shape, (2 * H, 2 * W), H * 100 + W)
    xr = x.clone().requires_grad_(True)
    yr = F.interpolate(xr, scale_factor=2, mode='bilinear', align_corners=align)
    yr.backward(gy)
    y, M = S.up_forward(x, (2 * H, 2 * W), align)
    assert S.ratio(yr.detach().numpy(), y, M, S.UP_C_FWD) <= 1.0
    gx, Mg = S.up_backward(gy, (H, W), align)
    assert S.ratio(xr.grad.numpy(), gx, Mg, S.up_c_bwd((H, W), (2 * H, 2 * W), align)) <= 1.0


@pytest.mark.parametrize('planes,in_hw,out_hw,align,route', S.UP_DIRECT)
def test_resize_spec_against_aten_float64(planes, in_hw, out_hw, align, route):
    """Any size: float64 ATen differs from the specification only through the fp32 coordinate -- at most three fp32 roundings of a
    coordinate below n_in, times the largest step between neighbours."""
    x, _ = S.up_inputs((planes,) + in_hw, out_hw, out_hw[0])
    y, _ = S.up_forward(x, out_hw, align)
    ref = F.interpolate(x.double()[None], size=out_hw, mode='bilinear', align_corners=align)[0].numpy()
    step = 2.0 * float(x.abs().max())
    assert np.abs(y - ref).max() <= 2 * 3 * S.U * max(in_hw) * step
    for n_in, n_out in zip(in_hw, out_hw):
        m = S.up_matrix(n_in, n_out, align)
        assert np.allclose(m.sum(1), 1.0, rtol=0, atol=2e-16) and (m >= 0).all()


@pytest.mark.parametrize('shape', list(S.UP_X2))
def test_resize_x2_rows_reach_their_paths(shape):
    N, C, H, W = shape
    want = S.UP_X2[shape]
    for k, align in enumerate((False, True)):
        assert S.up_bwd_route((H, W), (2 * H, 2 * W), align) == want['route'][k], align
        if 'window' in want:
            win = S.up_fwd_window(W, 2 * W, align)
            assert {'all': all(win), 'none': not any(win)}[want['window']], (align, win)
    assert S.up_fwd_vec(2 * W) == want['vec']
    if 'segs' in want:
        assert S.up_bwd_segments(H) == want['segs']
    if 'yscale_align' in want:
        assert float(S.up_scale(H, 2 * H, True)) == want['yscale_align']


@pytest.mark.parametrize('planes,in_hw,out_hw,align,route', S.UP_DIRECT)
def test_resize_direct_rows_reach_their_paths(planes, in_hw, out_hw, align, route):
    assert S.up_bwd_route(in_hw, out_hw, align) == route


def test_resize_tables_cover_what_they_claim():
    X = S.UP_X2
    assert [X[s]['yscale_align'] for s in ((1, 3, 1, 4), (1, 3, 2, 4), (1, 3, 3, 6))] == [0.0, float(np.float32(1) / np.float32(3)),
                                                                                       float(np.float32(0.4))]
    assert X[(2, 2, 17, 4)]['segs'] == 2 and 17 % 16 == 1 and 34 % 8 != 0            # row groups of 8 straddle the planes
    assert any(not v['vec'] for v in X.values()) and any(v.get('window') == 'none' and v['vec'] for v in X.values())
    # the decoder's maps read windows; the routes of the direct table are all there, refusal included
    assert all(S.up_fwd_window(84, 168, a) for a in (False, True)) == True  # noqa: E712
    assert {r[4] for r in S.UP_DIRECT} == {'gather6', 'gather8', 'refused'}
    assert any(r[4] == 'gather8' and r[2][0] <= 8 and float(S.up_scale(r[1][0], r[2][0], r[3])) < float(S.THIRD) for r in S.UP_DIRECT)
    # the rounding count of the backward follows the taps: x2 without align_corners reads an inner source index from four outputs
    assert S.up_taps(33, 66, False) == 4 and S.up_taps(1, 2, True) <= 4


# -- max-pool -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', S.MAXPOOL_SIZES)
def test_maxpool_spec_is_aten(hw):
    x, gy = S.maxpool_inputs(hw)
    y, pos = S.maxpool_forward(x.numpy())
    yr, ir = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    assert np.array_equal(y, yr.numpy(), equal_nan=True)
    assert np.array_equal(S.maxpool_flat_index(pos, hw), ir.numpy())
    xr = x.double().requires_grad_(True)
    F.max_pool2d(xr, 3, 2, 1).backward(gy.double())
    assert np.array_equal(S.maxpool_backward(gy, pos, hw), xr.grad.numpy())
    # the data is what the GPU test says it is
    assert bool((x[0, 1] < 0).all()) and bool(torch.isinf(x[0, 2]).all()) and int(torch.isnan(x).sum()) == 2
    assert int(np.isnan(y[0, 3]).sum()) >= 1 and bool((y[0, 1] < 0).all()) and bool((x[0, 0] > 0).any() or hw == (1, 1))
    # small integers: every routed sum (at most 4 terms of |gy| <= 8, times 1/8) is exact in fp16 and fp32
    assert float(gy.abs().max()) <= 8 and bool((gy == gy.round()).all())
    if hw[0] * hw[1] >= 24:
        assert bool((pos[0, 4] != 4).any()) and bool((pos[1] != pos[1, :, :1, :1]).any())      # ties decided by the scan order


# -- grouped convolution -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', list(S.GCONV_CASES))
def test_gconv_rows_reach_their_paths(shape):
    N, C, H, W = shape
    want = S.GCONV_CASES[shape]
    assert dict(fwd=S.gconv_fwd_tile(W), wg=S.gconv_wgrad_tile(W), vec=S.gconv_vec(W), grid=S.gconv_fwd_grid(H, W)) == want
    assert C % 8 == 0


def test_gconv_tables_cover_what_they_claim():
    G = S.GCONV_CASES
    for s in ((2, 16, 13, 84), (1, 8, 17, 67), (2, 24, 9, 56), (1, 16, 8, 168)):      # tests/test_42_gconv_bn_site_gpu.py SHAPES
        assert s in G
    both = {(v['fwd'], v['vec']) for v in G.values()}
    assert ((84, 12), True) in both and ((64, 16), True) in both and ((64, 16), False) in both
    assert {v['wg'] for v in G.values()} == {56, 64}
    assert G[(1, 8, 12, 84)]['grid'] == (1, 1, 84, 12)                                 # one exact tile
    assert G[(1, 8, 13, 168)]['grid'][1:] == (2, 84, 1) and S.gconv_wgrad_grid(13, 168) == (3, 2)
    assert G[(1, 8, 8, 60)]['vec'] and G[(1, 8, 8, 60)]['grid'][2] < 64               # 16-byte staging, partial tile
    assert S.gconv_c_gw(1, 13, 168) == 168 + 7 + 1 + 2 and S.gconv_c_gw(2, 13, 84) == 84 + 7 + 0 + 2


def test_gconv_spec_norm_dominates():
    x, w, gy = S.gconv_inputs((1, 16, 3, 5))
    r = S.gconv_spec(x, w, gy)
    for k in ('y', 'gx', 'gw'):
        assert np.all(r['M_' + k] >= np.abs(r[k]) * (1 - 1e-12)) and r[k].shape == r['M_' + k].shape
    ref = F.conv2d(x, w, None, 1, 1, 1, 2).numpy()
    assert S.ratio(ref, r['y'], r['M_y'], S.GCONV_C_FWD) <= 1.0
