"""The layer kernels between the matrix kernels of a depth-net step -- csrc/bnrelu.hip, csrc/upsample.hip, csrc/pool.hip
maxpool3s2_* and the plain 8-per-group 3x3 of csrc/gconv.hip -- through their wrappers in dvd_hip/conv.py, one code path at a
time against the float64 specification of tests/layer_spec.py.

Cases: the tables of layer_spec (BN_CASES / BN_PATHS, UP_X2, UP_DIRECT, MAXPOOL_SIZES, GCONV_CASES); every row names the path
it is there for and tests/test_layer_spec_cpu.py holds the rows to the host code's predicates.

Norm: element-wise |got - spec| <= c * 2^-24 * M, M the specification evaluated on absolute values and c the number of fp32
roundings on the longest path to one output, counted from the kernel's source in each test's docstring.  Nothing is measured
on the code under test.  Every comparison is logged (helpers.log_measured, the ratio against a bound of 1.0) next to fp32
ATen's ratio in the same norm on the same inputs (bound None).  Max-pool is exact.

Every fp32 case runs again with fp16 storage on inputs rounded to fp16 first: activations and data gradients must be the fp32
kernel's rounded once (torch.equal(out16, out32.half())), the fp32 parameter gradients are held to the specification with the
same norm.  Every backward runs twice and must give the same bits."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layer_spec as S
from helpers import log_measured

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(autouse=True)
def state():
    """A fresh loss-scale state for the fp16 gradients: S = 1 / S = 1."""
    from dvd_hip import conv as C, ops
    st = ops.gscale_new(torch.device(DEV))
    C.set_grad_scale_state(st)
    yield st
    C.set_grad_scale_state(None)


def _np(t):
    return t.detach().float().cpu().numpy()


def _check(figures):
    """figures: (name, ratio measured against the bound, 1.0 | None).  Logs and prints every one, then asserts the bounded."""
    bad = []
    for name, value, bound in figures:
        log_measured('test_68_' + name, value, bound)
        print('%-72s %.3f%s' % (name, value, '' if bound is not None else '  (fp32 ATen, not asserted)'))
        if bound is not None and not value <= bound:
            bad.append('%s: %.3f of the bound' % (name, value))
    assert not bad, '\n'.join(bad)


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    if not torch.equal(a, b):
        bad = (a != b).reshape(-1).nonzero().reshape(-1)
        raise AssertionError('%s: %d of %d elements differ, the first at flat index %d: %r against %r' % (
            what, bad.numel(), a.numel(), int(bad[0]), float(a.reshape(-1)[bad[0]]), float(b.reshape(-1)[bad[0]])))


# ================================================================================================================================
# bnrelu
# ================================================================================================================================
def _bn_run(case, t, half):
    """One forward and two backwards of conv.bn_eval_relu -> dict of results (None where a gradient is not requested)."""
    from dvd_hip import conv as C
    from dvd_hip.ops import known_amax
    (N, Cc, H, W), res, relu, affine, xgrad, frozen = case
    dtype = torch.float16 if half else torch.float32
    bn = torch.nn.BatchNorm2d(Cc, eps=S.BN_EPS, affine=affine).to(DEV).eval()
    with torch.no_grad():
        if affine:
            bn.weight.copy_(t['gamma'])
            bn.bias.copy_(t['beta'])
        bn.running_mean.copy_(t['mean'])
        bn.running_var.copy_(t['var'])
    if affine and frozen:
        bn.weight.requires_grad_(False)
        bn.bias.requires_grad_(False)
    x = t['x'].to(dtype).to(DEV).requires_grad_(xgrad)
    r = t['r'].to(dtype).to(DEV).requires_grad_(True) if res else None
    y = C.bn_eval_relu(bn, x, residual=r, relu=relu)
    assert type(y.grad_fn).__name__.startswith('_BnRelu') and y.dtype == dtype
    if not half:              # the attached max|y| is the tensor's maximum, not a bound
        assert known_amax(y) is not None and float(known_amax(y)) == float(y.detach().abs().max())
    seen = {}
    if xgrad:
        x.register_hook(lambda g: seen.__setitem__('gx', (known_amax(g), float(g.detach().abs().max()))))
    if res:
        r.register_hook(lambda g: seen.__setitem__('gr', (known_amax(g), float(g.detach().abs().max()))))
    gy = t['gy'].to(dtype).to(DEV)
    passes = []
    for _ in range(2):
        x.grad = None
        if res:
            r.grad = None
        bn.zero_grad(set_to_none=True)
        seen.clear()
        y.backward(gy, retain_graph=True)
        if not half:          # max|gx| and max|g_residual| ride on the gradients the pass hands on
            assert set(seen) == ({'gx'} if xgrad else set()) | ({'gr'} if res else set())
            for k, (am, true_max) in seen.items():
                assert am is not None and float(am) == true_max, k
        passes.append(dict(gx=x.grad, gr=r.grad if res else None, ggamma=bn.weight.grad if affine else None,
                           gbeta=bn.bias.grad if affine else None))
    for k in passes[0]:
        a, b = passes[0][k], passes[1][k]
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), k
    wants = dict(gx=xgrad, gr=res, ggamma=affine and not frozen, gbeta=affine and not frozen)
    for k, w in wants.items():
        assert (passes[0][k] is not None) == w, k
    return dict(passes[0], y=y.detach())


def _bn_aten(t, relu):
    c = {k: v for k, v in t.items()}
    x, gamma, beta = c['x'].clone().requires_grad_(True), c['gamma'].clone().requires_grad_(True), c['beta'].clone().requires_grad_(True)
    r = None if c['r'] is None else c['r'].clone().requires_grad_(True)
    y = F.batch_norm(x, c['mean'], c['var'], gamma, beta, False, 0.0, S.BN_EPS)
    if r is not None:
        y = y + r
    if relu:
        y = y.relu()
    y.backward(c['gy'])
    return dict(y=y.detach(), gx=x.grad, ggamma=gamma.grad, gbeta=beta.grad)


def _bn_figures(case, t, got, tag, with_y=True):
    """The results of a run against the specification on the inputs `t` -> figures; the exact parts are asserted here."""
    (N, Cc, H, W), res, relu, affine, xgrad, frozen = case
    y_got = _np(got['y'])
    y, pre, M = S.bn_forward(t['x'], t['r'], t['gamma'], t['beta'], t['mean'], t['var'], relu)
    figs = []
    name = 'bnrelu_%s_%s_' % (S.bn_case_id(case), tag)
    if with_y:
        figs.append((name + 'y', S.ratio(y_got, y, M, S.bn_c_y(res)), 1.0))
        if relu:              # the sign of every element the specification decides
            decided = np.abs(pre) > S.bn_c_y(res) * S.U * M
            assert decided.mean() > 0.99 and np.array_equal((y_got > 0)[decided], (pre > 0)[decided])
    mask = (y_got > 0) if relu else None
    b = S.bn_backward(t['gy'], mask, t['x'], t['gamma'], t['mean'], t['var'])
    if got['gr'] is not None and with_y:
        assert np.array_equal(_np(got['gr']), b['gr'].astype(np.float32)), 'gr is gy under the mask, exactly'
    if got['gx'] is not None and with_y:
        figs.append((name + 'gx', S.ratio(_np(got['gx']), b['gx'], b['M_gx'], S.BN_C_GX), 1.0))
    if got['gbeta'] is not None:
        figs.append((name + 'gbeta', S.ratio(_np(got['gbeta']), b['gbeta'], b['M_gbeta'], S.bn_c_gbeta(N, Cc, H * W)), 1.0))
        figs.append((name + 'ggamma', S.ratio(_np(got['ggamma']), b['ggamma'], b['M_ggamma'], S.bn_c_ggamma(N, Cc, H * W)), 1.0))
        if Cc >= 3:           # gy == 0 in the last channel, and channel 0 fully masked behind a ReLU: sums of zeros
            zero = [Cc - 1] + ([0] if relu else [])
            assert not _np(got['gbeta'])[zero].any() and not _np(got['ggamma'])[zero].any()
    if Cc >= 3 and relu and affine:
        assert not y_got[:, 0].any()
    return figs


@pytest.mark.parametrize('case', S.BN_CASES, ids=S.bn_case_id)
def test_bnrelu_against_float64(case):
    """conv.bn_eval_relu, forward and backward.  Roundings (csrc/bnrelu.hip):
      y       s = gamma / sqrtf(var + eps): 3 (:35);  b = beta - mean * s: 2, a product and a difference (:36; 1 if the compiler
              contracts them);  fmaf(x, s, b): 1 (:43);  + r: 1 (:49)                                    -> 7, 6 without a residual
      gx      s: 3 (:111);  g * s: 1 (:135, :148)                                                             -> 4
      gr      g itself                                                                                  -> exact
      gbeta   a thread's chain `sg += (g.x + g.y) + (g.z + g.w)` (:127): 2 inside the quad and one per trip after the first (the
              first adds to 0.0), or `sg += g` (:141): one per trip after the first;  wave_sum: 6 (:156);  the four waves as
              (a + b) + (c + d): 2 (:169);  the records in double: 0 (:189);  the store: 1 (:195)
                                                                   -> 2 + (trips - 1) + 9 on the 16-byte loop, (trips - 1) + 9 scalar
      ggamma  x - mean: 1 (:131);  four nested fmaf per quad trip (:131-132) or one per element trip (:143);  then as gbeta,
              rstd applied in double (:196)                                                              -> 1 + 4 trips + 9, 1 + trips + 9
    trips = layer_spec.bn_thread_trips: the images of an npb block times the quads (elements) of thread 0.
    The backward specification is given the kernel's own [y > 0]; where the specification decides the sign of y the kernel must
    agree (all but < 1 % of the elements: tests/test_layer_spec_cpu.py)."""
    (N, Cc, H, W), res, relu, affine, xgrad, frozen = case
    t = S.bn_inputs(case)
    got = _bn_run(case, t, half=False)
    figs = _bn_figures(case, t, got, 'f32')
    # fp32 ATen on the CPU in the same norm, against the specification under ATen's own mask
    a = _bn_aten(t, relu)
    ya = _np(a['y'])
    y, pre, M = S.bn_forward(t['x'], t['r'], t['gamma'], t['beta'], t['mean'], t['var'], relu)
    b = S.bn_backward(t['gy'], (ya > 0) if relu else None, t['x'], t['gamma'], t['mean'], t['var'])
    name = 'bnrelu_%s_aten_' % S.bn_case_id(case)
    figs += [(name + 'y', S.ratio(ya, y, M, S.bn_c_y(res)), None), (name + 'gx', S.ratio(_np(a['gx']), b['gx'], b['M_gx'], S.BN_C_GX), None),
             (name + 'gbeta', S.ratio(_np(a['gbeta']), b['gbeta'], b['M_gbeta'], S.bn_c_gbeta(N, Cc, H * W)), None),
             (name + 'ggamma', S.ratio(_np(a['ggamma']), b['ggamma'], b['M_ggamma'], S.bn_c_ggamma(N, Cc, H * W)), None)]
    # fp16 storage: the fp32 kernel's values rounded once; the parameter gradients against the specification
    t16 = {k: (S.rounded_to_half(v) if k in ('x', 'r', 'gy') else v) for k, v in t.items()}
    g32, g16 = _bn_run(case, t16, half=False), _bn_run(case, t16, half=True)
    for k in ('y', 'gx', 'gr'):
        if g32[k] is not None:
            _same(g16[k], g32[k].half(), k + ' with fp16 storage')
    figs += _bn_figures(case, t16, dict(g16, y=g16['y']), 'f16', with_y=False)
    _check(figs)


# ================================================================================================================================
# upsample
# ================================================================================================================================
def _up_run(x, gy, align, half):
    from dvd_hip import conv as C
    dtype = torch.float16 if half else torch.float32
    xg = x.to(dtype).to(DEV).requires_grad_(True)
    y = C.upsample_bilinear2x(xg, align)
    assert type(y.grad_fn).__name__.startswith('_UpsampleBilinear') and y.dtype == dtype
    grads = []
    for _ in range(2):
        xg.grad = None
        y.backward(gy.to(dtype).to(DEV), retain_graph=True)
        grads.append(xg.grad)
    _same(grads[0], grads[1], 'gx of two backward passes')
    return y.detach(), grads[0]


UP_DOC = """Roundings (csrc/upsample.hip, built with -ffp-contract=off).  The specification has the kernel's fp32 coordinate,
    i0, i1 and w1 = s - i0 (exact); what rounds is
      forward   per axis w0 = 1.0f - w1: 1 (:40) and the blend w0 * a + w1 * b: two products and a sum, 3 (:101 / :105, :135) -> 8
      backward  per axis the weight: w0 = 1 - w1, and w0 + w1 where both taps land on the last index: 2 (:40, :172 / :249);  one
                fmaf per candidate, a candidate of weight 0 adding exactly nothing (:211-212, :294-304): the non-zero taps that land
                on one input index (layer_spec.up_taps)                                        -> (2 + taps_x) + (2 + taps_y)"""


@pytest.mark.parametrize('align', [False, True], ids=['half_pixel', 'align_corners'])
@pytest.mark.parametrize('shape', list(S.UP_X2), ids=lambda s: 'x'.join(map(str, s)))
def test_upsample_x2_against_float64(shape, align):
    N, Cc, H, W = shape
    out_hw = (2 * H, 2 * W)
    x, gy = S.up_inputs(shape, out_hw, H * 100 + W)
    y, gx = _up_run(x, gy, align, half=False)
    assert tuple(y.shape) == (N, Cc) + out_hw
    ys, M = S.up_forward(x, out_hw, align)
    gs, Mg = S.up_backward(gy, (H, W), align)
    cb = S.up_c_bwd((H, W), out_hw, align)
    xr = x.clone().requires_grad_(True)
    yr = F.interpolate(xr, scale_factor=2, mode='bilinear', align_corners=align)
    yr.backward(gy)
    name = 'upsample_%s_%s_%s_' % ('x'.join(map(str, shape)), 'align' if align else 'half', S.UP_X2[shape]['route'][int(align)])
    figs = [(name + 'y', S.ratio(_np(y), ys, M, S.UP_C_FWD), 1.0), (name + 'gx', S.ratio(_np(gx), gs, Mg, cb), 1.0),
            (name + 'y_aten', S.ratio(_np(yr), ys, M, S.UP_C_FWD), None), (name + 'gx_aten', S.ratio(_np(xr.grad), gs, Mg, cb), None)]
    x16, gy16 = S.rounded_to_half(x), S.rounded_to_half(gy)
    (y32, gx32), (y16, gx16) = _up_run(x16, gy16, align, half=False), _up_run(x16, gy16, align, half=True)
    _same(y16, y32.half(), 'y with fp16 storage')
    _same(gx16, gx32.half(), 'gx with fp16 storage')
    _check(figs)


test_upsample_x2_against_float64.__doc__ = 'conv.upsample_bilinear2x, both flavours, forward and backward.  ' + UP_DOC

SENTINEL = -777.0


def _up_direct(x, gy, in_hw, out_hw, align, half):
    """The C entry points on [planes, H, W] -> (y, gx of the first call, gx of the second, status of the backward, message)."""
    from dvd_hip import _lib
    from dvd_hip.ops import _p, _stream
    lib = _lib.load()
    dtype = torch.float16 if half else torch.float32
    xd, gd = x.to(dtype).to(DEV).contiguous(), gy.to(dtype).to(DEV).contiguous()
    planes = x.shape[0]
    y = torch.full((planes,) + tuple(out_hw), SENTINEL, device=DEV, dtype=dtype)
    _lib.check(lib.dvd_upsample_bilinear_fwd_t(_p(xd), _p(y), int(half), ctypes.c_longlong(planes), in_hw[0], in_hw[1], out_hw[0],
                                               out_hw[1], int(align), _stream()), 'dvd_upsample_bilinear_fwd_t')
    gxs, status, msg = [], None, ''
    for _ in range(2):
        gx = torch.full((planes,) + tuple(in_hw), SENTINEL, device=DEV, dtype=dtype)
        status = lib.dvd_upsample_bilinear_bwd_t(_p(gd), _p(gx), int(half), ctypes.c_longlong(planes), in_hw[0], in_hw[1], out_hw[0],
                                                 out_hw[1], int(align), _stream())
        if status != _lib.DVD_OK:
            msg = (lib.dvd_last_error() or b'').decode('utf-8', 'replace')
        gxs.append(gx)
    torch.cuda.synchronize()
    return y, gxs[0], gxs[1], status, msg


@pytest.mark.parametrize('planes,in_hw,out_hw,align,route', S.UP_DIRECT,
                         ids=['%dx%d_to_%dx%d_%s_%s' % (r[1] + r[2] + ('align' if r[3] else 'half', r[4])) for r in S.UP_DIRECT])
def test_upsample_other_sizes_through_the_c_entry_points(planes, in_hw, out_hw, align, route):
    from dvd_hip import _lib
    x, gy = S.up_inputs((planes,) + in_hw, out_hw, 10 * out_hw[0] + int(align))
    y, gx, gx2, status, msg = _up_direct(x, gy, in_hw, out_hw, align, half=False)
    ys, M = S.up_forward(x, out_hw, align)
    name = 'upsample_%dx%d_to_%dx%d_%s_%s_' % (in_hw + out_hw + ('align' if align else 'half', route))
    figs = [(name + 'y', S.ratio(_np(y), ys, M, S.UP_C_FWD), 1.0)]
    x16, gy16 = S.rounded_to_half(x), S.rounded_to_half(gy)
    y32, g32, _, _, _ = _up_direct(x16, gy16, in_hw, out_hw, align, half=False)
    y16, g16, _, status16, msg16 = _up_direct(x16, gy16, in_hw, out_hw, align, half=True)
    _same(y16, y32.half(), 'y with fp16 storage')
    if route == 'refused':      # an error, the message, and not one element written
        for st, m, g in ((status, msg, gx), (status, msg, gx2), (status16, msg16, g16)):
            assert st != _lib.DVD_OK and S.REFUSED_MESSAGE in m, (st, m)
            assert bool((g == SENTINEL).all())
    else:
        assert status == _lib.DVD_OK and status16 == _lib.DVD_OK, (msg, msg16)
        _same(gx, gx2, 'gx of two backward launches')
        gs, Mg = S.up_backward(gy, in_hw, align)
        figs.append((name + 'gx', S.ratio(_np(gx), gs, Mg, S.up_c_bwd(in_hw, out_hw, align)), 1.0))
        _same(g16, g32.half(), 'gx with fp16 storage')
    _check(figs)


test_upsample_other_sizes_through_the_c_entry_points.__doc__ = (
    'dvd_upsample_bilinear_{fwd,bwd}_t at sizes that are not x2: upsample_bilinear_bwd_kernel<8>, the n_out <= 8 admission and the '
    'refusal of factors above 3 (the only thing compared is the specification: fp32 ATen forms another coordinate here).  ' + UP_DOC)


# ================================================================================================================================
# maxpool
# ================================================================================================================================
@pytest.mark.parametrize('hw', S.MAXPOOL_SIZES, ids=lambda s: '%dx%d' % s)
def test_maxpool_is_the_specification_exactly(hw, state):
    """conv.maxpool3s2 on signed data with an all-negative plane (a padding of 0 would win every border window), a plane of
    -inf, NaNs and a plateau: the fp32 and the fp16 (to_half) forward equal the specification's values; the backward routes every
    gy to the first maximum of its window -- gy are small integers, so the at most four routed terms add exactly in fp32, and in
    the fp16-gradient form times 1 / S = 1 / 8 as well."""
    from dvd_hip import conv as C
    x, gy = S.maxpool_inputs(hw)
    ys, pos = S.maxpool_forward(x.numpy())
    gs = S.maxpool_backward(gy, pos, hw)
    xg = x.to(DEV).requires_grad_(True)
    y = C.maxpool3s2(xg)
    assert type(y.grad_fn).__name__.startswith('_MaxPool3s2') and y.dtype == torch.float32
    assert np.array_equal(_np(y), ys, equal_nan=True), 'fp32 forward'
    grads = []
    for _ in range(2):
        xg.grad = None
        y.backward(gy.to(DEV), retain_graph=True)
        grads.append(xg.grad)
    _same(grads[0], grads[1], 'gx of two backward passes')
    assert np.array_equal(_np(grads[0]), gs.astype(np.float32)), 'fp32 backward'
    # the fp32 / fp16 boundary fused into the pooling, and the fp16 gradient times 1 / S
    state[1] = 0.125
    xh = x.to(DEV).requires_grad_(True)
    yh = C.maxpool3s2(xh, to_half=True)
    assert yh.dtype == torch.float16
    with np.errstate(over='ignore'):
        want16 = ys.astype(np.float16)
    assert np.array_equal(yh.detach().cpu().numpy(), want16, equal_nan=True), 'fp16 forward'
    grads = []
    for _ in range(2):
        xh.grad = None
        yh.backward(gy.half().to(DEV), retain_graph=True)
        grads.append(xh.grad)
    _same(grads[0], grads[1], 'gx of two fp16 backward passes')
    assert grads[0].dtype == torch.float32
    assert np.array_equal(_np(grads[0]), S.maxpool_backward(gy, pos, hw, 0.125).astype(np.float32)), 'fp16 backward'


# ================================================================================================================================
# gconv c8
# ================================================================================================================================
def _gconv_run(x, w, gy, half):
    from dvd_hip import conv as C
    dtype = torch.float16 if half else torch.float32
    xg = x.to(dtype).to(DEV).requires_grad_(True)
    wg = w.to(DEV).requires_grad_(True)
    y = C.gconv3x3_c8(xg, wg)
    assert type(y.grad_fn).__name__.startswith('_GConv3x3C8') and y.dtype == dtype
    grads = []
    for _ in range(2):
        xg.grad = wg.grad = None
        y.backward(gy.to(dtype).to(DEV), retain_graph=True)
        grads.append((xg.grad, wg.grad))
    _same(grads[0][0], grads[1][0], 'gx of two backward passes')
    _same(grads[0][1], grads[1][1], 'gw of two backward passes')
    return y.detach(), grads[0][0], grads[0][1]


@pytest.mark.parametrize('shape', list(S.GCONV_CASES), ids=lambda s: 'x'.join(map(str, s)))
def test_gconv_c8_against_float64(shape):
    """conv.gconv3x3_c8 (no BatchNorm site), forward, backward-data and backward-weight.  Roundings (csrc/gconv.hip):
      y, gx   one fma per source channel and tap into the accumulator, 8 x 9 (:165-181)                            -> 72
      gw      a lane's chain of one fma per pixel of its row, tile after tile (:428-443; staged zeros add exactly nothing): W;
              the 8 rows of a band (:456-458): 7;  gconv_wgrad_reduce_kernel: the records of a residue class mod 4 in order, the
              first to 0.0, the tail behind class 0 (:531-533): records / 4 + records % 4 - 1;  the classes as (0 + 1) + (2 + 3)
              (:538): 2;  out_scale is 1 here                                  -> W + 7 + (records / 4 + records % 4 - 1) + 2
    M is the same convolution of absolute values."""
    N, Cc, H, W = shape
    x, w, gy = S.gconv_inputs(shape)
    y, gx, gw = _gconv_run(x, w, gy, half=False)
    r = S.gconv_spec(x, w, gy)
    cw = S.gconv_c_gw(N, H, W)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yr = F.conv2d(xr, wr, None, 1, 1, 1, Cc // 8)
    yr.backward(gy)
    name = 'gconv_c8_%s_' % 'x'.join(map(str, shape))
    figs = [(name + 'y', S.ratio(_np(y), r['y'], r['M_y'], S.GCONV_C_FWD), 1.0),
            (name + 'gx', S.ratio(_np(gx), r['gx'], r['M_gx'], S.GCONV_C_FWD), 1.0),
            (name + 'gw', S.ratio(_np(gw), r['gw'], r['M_gw'], cw), 1.0),
            (name + 'y_aten', S.ratio(_np(yr), r['y'], r['M_y'], S.GCONV_C_FWD), None),
            (name + 'gx_aten', S.ratio(_np(xr.grad), r['gx'], r['M_gx'], S.GCONV_C_FWD), None),
            (name + 'gw_aten', S.ratio(_np(wr.grad), r['gw'], r['M_gw'], cw), None)]
    x16, gy16 = S.rounded_to_half(x), S.rounded_to_half(gy)
    (y32, gx32, _), (y16, gx16, gw16) = _gconv_run(x16, w, gy16, half=False), _gconv_run(x16, w, gy16, half=True)
    _same(y16, y32.half(), 'y with fp16 storage')
    _same(gx16, gx32.half(), 'gx with fp16 storage')
    r16 = S.gconv_spec(x16, w, gy16)
    figs.append((name + 'gw_f16', S.ratio(_np(gw16), r16['gw'], r16['M_gw'], cw), 1.0))
    _check(figs)
