"""The max|x| operand scales that producers hand to the fp32 matrix kernels (csrc/xconv.hip, csrc/xwgrad3.hip).

Every fp32 operand of those kernels is scaled by ONE power of two taken from a device scalar, "max|x| or an upper bound"
(csrc/dvd_split.h pow2_scale).  The scalar is a side channel: a kernel's epilogue writes it, conv.py passes it on by reasoning
("a convex combination never exceeds the largest input"), autograd nodes hand it over (conv._Site).  A scalar 2^k too large
costs k of the 22 operand bits and stays inside every parity tolerance of the suite; one too small by 4x or more turns into
Inf, but only for data that reaches the headroom; a stale one survives a HIP-graph replay of the batch it was captured with.

All comparisons here are exact (== on floats, torch.equal) or inequalities: a scalar a kernel computes IS max|t| of what it
stored, a scalar passed on IS the input's scalar (or ka + kb) and bounds the tensor.  fp32 storage only (fp16 activations carry
no operand scale).

Measured, not asserted (test_every_consumed_scalar_bounds_its_operand_*; MI355X, profiles/operand_scales_measured.jsonl): the
loosest scalar / max|t| among the operands a matrix kernel consumed is 1.54 in MiDaS at 1x3x64x96 (1.87 in the second pass of
the process, input / 16) and 1.45 in the hourglass at 2x3x32x48 (second pass 1.11): less than one of the 22 operand bits."""
import inspect
import math

import pytest
import torch
import torch.nn.functional as F

import helpers

pytestmark = pytest.mark.gpu

PLANT = -1003.0        # the planted extreme: negative, far above anything the random data produces


def _true(t):
    return float(t.detach().abs().max())


def _scalar(t, what=''):
    from dvd_hip.ops import known_amax
    k = known_amax(t)
    assert k is not None, 'no max|.| scalar attached %s' % what
    return float(k)


def _assert_exact(t, what):
    s, m = _scalar(t, what), _true(t)
    assert s == m, '%s: attached scalar %r, max|t| %r' % (what, s, m)
    return s


def _positions(shape):
    N, C, H, W = shape
    return {'first': (0, 0, 0, 0), 'last': (N - 1, C - 1, H - 1, W - 1), 'row_end': (0, C // 2, H // 2, W - 1)}


def _planted(shape, pos, device='cuda'):
    t = torch.zeros(shape, device=device)
    t[pos] = PLANT
    return t


def _grad_probe(t, seen, key):
    """What a tensor's gradient carries when autograd hands it on: (attached scalar | None, a copy of the gradient)."""
    from dvd_hip.ops import known_amax

    def hook(g):
        k = known_amax(g)
        seen[key] = (None if k is None else float(k), g.detach().clone())
    t.register_hook(hook)


def _assert_grad_exact(seen, key):
    assert key in seen, 'no gradient reached %s' % key
    k, g = seen[key]
    assert k is not None, '%s: the gradient carries no scalar' % key
    assert k == _true(g), '%s: attached scalar %r, max|g| %r' % (key, k, _true(g))
    return k, g


# ---- 1. scalars a kernel computes: exact, and taken after the whole epilogue ----------------------------------------------

FWD_CASES = [
    # N, Cin, Cout, H, W, k, groups, bias
    (2, 20, 40, 11, 19, 3, 1, True),
    (1, 32, 1, 17, 29, 1, 1, False),
    (1, 48, 64, 19, 23, 5, 1, False),
    (1, 32, 32, 9, 12, 11, 1, False),
    (2, 96, 96, 9, 14, 3, 3, False),
]


def _forward_options(C, conv, x, label=''):
    """Every epilogue option combination of the forward kernel -> {option: scalar}; asserts each scalar on the way."""
    N, _, H, W = x.shape
    out_shape = (N, conv.out_channels, H, W)
    got = {}
    got['module'] = _assert_exact(conv(x), label + ' module')
    got['plain'] = _assert_exact(C.xconv2d(conv, x), label + ' plain')
    assert got['module'] == got['plain']
    got['relu_in'] = _assert_exact(C.xconv2d(conv, x, relu_in=True), label + ' relu_in')
    for name, pos in _positions(out_shape).items():
        res = _planted(out_shape, pos)
        for relu_in in (False, True):
            what = '%s residual at %s%s' % (label, name, ' relu_in' if relu_in else '')
            y = C.xconv2d(conv, x, relu_in=relu_in, residual=res)
            s = _assert_exact(y, what)
            assert s == abs(float(y[pos])) and s > 0.9 * abs(PLANT), what      # the planted element IS the maximum
            got['residual/%s/%d' % (name, relu_in)] = s
        what = '%s relu(residual) at %s' % (label, name)
        y = C.xconv2d(conv, x, residual=res, res_relu=True)
        s = _assert_exact(y, what)
        assert s < 0.5 * abs(PLANT), what + ': the rectified value must not reach the scalar'
        got['res_relu/%s' % name] = s
    return got


@pytest.mark.parametrize('N,Cin,Cout,H,W,k,groups,bias', FWD_CASES)
def test_forward_scalar_is_exact_after_the_whole_epilogue(N, Cin, Cout, H, W, k, groups, bias):
    from dvd_hip import conv as C
    torch.manual_seed(Cin + Cout + k)
    conv = C.XConv2d(Cin, Cout, k, padding=k // 2, groups=groups, bias=bias).cuda()
    x = torch.randn(N, Cin, H, W, device='cuda')
    with torch.no_grad():
        _forward_options(C, conv, x)


@pytest.mark.parametrize('k', [1, 3])
def test_forward_scalar_is_the_same_float_under_every_block_shape(k):
    from dvd_hip import _lib, conv as C
    torch.manual_seed(50 + k)
    conv = C.XConv2d(256, 256, k, padding=k // 2).cuda()
    x = torch.randn(1, 256, 12, 20, device='cuda')
    lib = _lib.load()
    per_shape = []
    try:
        for cfg in range(8):
            _lib.check(lib.dvd_xconv_select(cfg), 'dvd_xconv_select')
            with torch.no_grad():
                per_shape.append(_forward_options(C, conv, x, 'block shape %d' % cfg))
    finally:
        _lib.check(lib.dvd_xconv_select(0), 'dvd_xconv_select')
    for cfg, got in enumerate(per_shape[1:], start=1):
        assert got == per_shape[0], 'block shape %d: %r' % (cfg, {o: (v, per_shape[0][o]) for o, v in got.items()
                                                                   if v != per_shape[0][o]})


BWD_CASES = [(2, 20, 40, 11, 19, 3, 1), (1, 32, 1, 17, 29, 1, 1), (1, 48, 64, 19, 23, 5, 1), (2, 96, 96, 9, 14, 3, 3),
             (1, 256, 256, 12, 20, 1, 1), (1, 256, 256, 12, 20, 3, 1)]


@pytest.mark.parametrize('N,Cin,Cout,H,W,k,groups', BWD_CASES)
def test_backward_data_scalar_plain_masked_and_after_the_alias_add(N, Cin, Cout, H, W, k, groups):
    from dvd_hip import conv as C
    torch.manual_seed(Cin + Cout + k + 1)
    conv = C.XConv2d(Cin, Cout, k, padding=k // 2, groups=groups).cuda()
    x = torch.randn(N, Cin, H, W, device='cuda')
    gy = torch.randn(N, Cout, H, W, device='cuda')
    seen = {}
    # plain
    xg = x.clone().requires_grad_(True)
    _grad_probe(xg, seen, 'plain')
    C.xconv2d(conv, xg).backward(gy)
    unmasked_max, g_plain = _assert_grad_exact(seen, 'plain')
    # relu_in: the element where the unmasked gradient is largest is masked away; the scalar is the masked tensor's maximum
    worst = tuple(int(i) for i in (g_plain.abs() == g_plain.abs().max()).nonzero()[0])
    xm = x.clone()
    xm[worst] = -1.0
    xm = xm.requires_grad_(True)
    _grad_probe(xm, seen, 'masked')
    C.xconv2d(conv, xm, relu_in=True).backward(gy)
    k_masked, g_masked = _assert_grad_exact(seen, 'masked')
    assert float(g_masked[worst]) == 0.0 and k_masked < unmasked_max
    # alias=True and a second consumer: its gradient is added in the epilogue, the scalar is taken after the add
    for name, pos in _positions(x.shape).items():
        for relu_in in (False, True):
            xa_in = x.clone()
            if relu_in:
                xa_in[pos] = 1.0                    # (the planted element must survive the mask)
            xa_in = xa_in.requires_grad_(True)
            key = 'alias/%s/%d' % (name, relu_in)
            _grad_probe(xa_in, seen, key)
            y, xa = C.xconv2d(conv, xa_in, relu_in=relu_in, alias=True)
            torch.autograd.backward([y, xa], [gy, _planted(x.shape, pos)])
            k_alias, g_alias = _assert_grad_exact(seen, key)
            assert k_alias == abs(float(g_alias[pos])) and k_alias > 0.9 * abs(PLANT), key


@pytest.mark.parametrize('N,Cc,G,H,W', [(1, 256, 1, 21, 30), (1, 64, 2, 13, 23)])
def test_stride_two_forward_and_backward_data_scalars(N, Cc, G, H, W):
    from dvd_hip import conv as C
    torch.manual_seed(Cc + G)
    conv = C.XConv2d(Cc, Cc, 3, stride=2, padding=1, groups=G, bias=True).cuda()
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    for name, pos in [('random', None)] + list(_positions((N, Cc, H, W)).items()):
        x = torch.randn(N, Cc, H, W, device='cuda')
        gy = torch.randn(N, Cc, Ho, Wo, device='cuda')
        if pos is not None:                 # an extreme input / gradient element at the tensor's edges
            x[pos] = PLANT
            gy[pos[0], pos[1], min(pos[2], Ho - 1), min(pos[3], Wo - 1)] = PLANT
        xg = x.requires_grad_(True)
        seen = {}
        _grad_probe(xg, seen, 'gx ' + name)
        y = conv(xg)
        # (the kernel's own output: the stride-1 kernel's would come through _Subsample2)
        assert C.xconv_s2_supported(conv, xg) and type(y.grad_fn).__name__ == '_XConvBackward', 'the strided kernels must be taken'
        _assert_exact(y, 'stride 2 forward, ' + name)
        y.backward(gy)
        _assert_grad_exact(seen, 'gx ' + name)


def _bn_case():
    from test_06_xconv_gpu import BN_CASES
    assert len(BN_CASES) == 5
    return BN_CASES


@pytest.mark.parametrize('case', range(5))
def test_conv_bn_act_scalars(case):
    from dvd_hip import conv as C
    Cin, Cout, k, groups, stride, affine, cbias, with_res, relu, H, W = _bn_case()[case]
    torch.manual_seed(Cin + Cout + k)
    N = 2
    conv = C.XConv2d(Cin, Cout, k, stride=stride, padding=0 if stride > 1 else k // 2, groups=groups, bias=cbias).cuda()
    bn = torch.nn.BatchNorm2d(Cout, affine=affine).cuda().eval()
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.5)
        bn.running_var.uniform_(0.3, 2.0)
        if affine:
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0, 0.3)
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    plants = [None] + (list(_positions((N, Cout, Ho, Wo)).values()) if with_res else [])
    for pos in plants:
        x = torch.randn(N, Cin, H, W, device='cuda').requires_grad_(True)
        res = None
        if with_res:
            res = torch.randn(N, Cout, Ho, Wo, device='cuda')
            if pos is not None:
                res[pos] = PLANT
            res = res.requires_grad_(True)
        gy = torch.randn(N, Cout, Ho, Wo, device='cuda')
        seen = {}
        _grad_probe(x, seen, 'gx')
        if with_res:
            _grad_probe(res, seen, 'gres')
        y = C.conv_bn_act(conv, bn, x, residual=res, relu=relu)
        assert 'XConvBn' in type(y.grad_fn).__name__, 'the fused path must be taken'
        s = _assert_exact(y, 'conv_bn_act %d %s' % (case, pos))
        if pos is not None and relu:
            assert s < 0.5 * abs(PLANT)           # rectified: the planted value must not reach the scalar
        y.backward(gy)
        _assert_grad_exact(seen, 'gx')
        if with_res:
            assert 'gres' in seen
            if seen['gres'][0] is not None:       # the masked gradient handed to the residual branch: exact where attached
                _assert_grad_exact(seen, 'gres')


def test_stem_scalar():
    from dvd_hip import conv as C
    torch.manual_seed(3)
    conv = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False).cuda()
    bn = torch.nn.BatchNorm2d(64).cuda().eval()
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.5)
        bn.running_var.uniform_(0.3, 2.0)
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0, 0.3)
    x = torch.randn(2, 3, 33, 51, device='cuda')
    y = C.stem_conv_bn_relu(conv, bn, x)
    assert tuple(y.shape) == (2, 64, 17, 26)
    _assert_exact(y, 'stem')
    x[1, 2, 32, 50] = PLANT                   # an extreme pixel in the last (odd) row and column
    _assert_exact(C.stem_conv_bn_relu(conv, bn, x), 'stem, extreme last pixel')


# ---- 2. scalars passed on by reasoning: bounds, and the documented ones ----------------------------------------------------

PASS_SHAPES = [(2, 5, 7, 9), (1, 3, 12, 21)]


class _Tagged(torch.autograd.Function):
    """Identity whose backward hands on a copy of the gradient with `factor * max|g|` attached, the way a producing kernel
    attaches its scalar to the gradient it writes."""

    attached = []          # the scalars handed on, in order

    @staticmethod
    def forward(ctx, x, factor):
        ctx.factor = factor
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        from dvd_hip.ops import amax, set_amax
        g = g.clone()
        k = amax(g) * ctx.factor
        _Tagged.attached.append(float(k))
        return set_amax(g, k), None


def _tag(x, factor):
    from dvd_hip.ops import amax, set_amax
    x = x.cuda()
    k = amax(x) * factor
    return set_amax(x.requires_grad_(True), k), float(k)


def _passes_on(op, x_cpu, gy_of=None, backward=True, slack=0.0):
    """op's output (and, if backward, its input gradient) carries EXACTLY the scalar of its input, as a bound.
    Run with the exact maximum and with a 3x looser one (so that a recomputed maximum is not mistaken for the passed-on one).
    slack: relative excess over the bound that the op's own fp32 roundings may cause (0: the arithmetic is exact or monotone).
    -> (max|y|, max|gx| | None, scalar of gy) of the run with the exact scalars."""
    out = None
    for factor in (3.0, 1.0):
        x, kx = _tag(x_cpu, factor)
        seen = {}
        _grad_probe(x, seen, 'gx')
        y = op(x)
        ky = _scalar(y, 'output')
        assert ky == kx, 'output scalar %r is not the input scalar %r' % (ky, kx)
        assert _true(y) <= ky * (1.0 + slack)
        out = (_true(y), None, None)
        if backward:
            gy = torch.randn(y.shape, device='cuda') if gy_of is None else gy_of(y)
            _Tagged.apply(y, factor).backward(gy)
            kg, gx = seen['gx']
            assert kg is not None, 'the input gradient carries no scalar'
            assert kg == _Tagged.attached[-1], 'gradient scalar %r is not the output gradient\'s %r' % (kg, _Tagged.attached[-1])
            assert kg >= _true(gy)
            assert _true(gx) <= kg * (1.0 + slack)
            out = (_true(y), _true(gx), kg)
    return out


@pytest.mark.parametrize('shape', PASS_SHAPES)
@pytest.mark.parametrize('align', [False, True])
def test_upsample_passes_the_input_scalar_on(shape, align):
    from dvd_hip import conv as C
    torch.manual_seed(1)
    x = torch.randn(shape)
    _passes_on(lambda t: C.upsample_bilinear2x(t, align), x, backward=False)
    for corner in ((0, 0, 0, 0), (shape[0] - 1, shape[1] - 1, shape[2] - 1, shape[3] - 1)):
        xc = x.clone()
        xc[corner] = -7.5                      # a corner sample is copied: the bound is attained
        ymax, _, _ = _passes_on(lambda t: C.upsample_bilinear2x(t, align), xc, backward=False)
        assert ymax == 7.5


@pytest.mark.parametrize('shape', PASS_SHAPES)
def test_maxpool_passes_the_input_scalar_on(shape):
    from dvd_hip import conv as C
    torch.manual_seed(2)
    x = torch.randn(shape)
    _passes_on(C.maxpool3s2, x, backward=False)
    xc = x.clone()
    xc[-1, -1, -1, -1] = 7.5                   # a positive extreme in the last window: attained
    assert _passes_on(C.maxpool3s2, xc, backward=False)[0] == 7.5
    xc[-1, -1, -1, -1] = -7.5                  # a negative one is never selected: a bound all the same
    assert _passes_on(C.maxpool3s2, xc, backward=False)[0] < 7.5


@pytest.mark.parametrize('shape', PASS_SHAPES)
def test_subsample_passes_scalars_on_both_ways(shape):
    from dvd_hip import conv as C
    torch.manual_seed(3)
    x = torch.randn(shape)
    _passes_on(lambda t: C._subsample(t, 2), x)
    xc = x.clone()
    xc[0, 0, 0, 0] = -7.5                      # a kept sample; a constant gradient: both bounds attained
    ymax, gmax, kg = _passes_on(lambda t: C._subsample(t, 2), xc, gy_of=lambda y: torch.full_like(y, -9.0))
    assert ymax == 7.5 and gmax == 9.0 == kg


@pytest.mark.parametrize('shape', PASS_SHAPES)
@pytest.mark.parametrize('k,stride,pad', [(2, 2, 0), (3, 2, 1), (3, 1, 1), (5, 2, 2)])
def test_avgpool_passes_scalars_on_both_ways(shape, k, stride, pad):
    from dvd_hip import conv as C
    torch.manual_seed(4)
    pool = C.AvgPool2d(k, stride, pad)
    x = torch.randn(shape)

    def op(t):
        y = pool(t)
        assert 'AvgPool' in type(y.grad_fn).__name__ and 'Backward' in type(y.grad_fn).__name__      # csrc/pool.hip, not ATen
        return y
    _passes_on(op, x)
    # a constant input: every window without padding averages to the constant; a constant gradient: a pixel under
    # ceil(k / stride)^2 windows of weight 1 / k^2 receives that share of it (the whole of it for stride 1)
    ymax, gmax, kg = _passes_on(op, torch.full(shape, -2.0), gy_of=lambda y: torch.full_like(y, 9.0))
    assert ymax == 2.0
    share = math.ceil(k / stride) ** 2 / float(k * k)
    assert kg == 9.0 and gmax <= 9.0 and abs(gmax - 9.0 * share) <= 1e-5, (gmax, share)
    if stride == 1:
        assert gmax == 9.0
    # a constant that k * k does not divide: the window sum (forward) and the sum of the quotients gy / k^2 (backward, stride
    # 1) round k * k times, each by at most 2^-24 of the running value, and may carry the result past the constant by ulps --
    # (1 + 2^-24)^(k k + 1) <= 1 + k k 2^-23.  That is the bound such a tensor has; pow2_scale leaves two bits of headroom
    _passes_on(op, torch.full(shape, 1.7), gy_of=lambda y: torch.full_like(y, -1.7), slack=k * k * 2.0 ** -23)


@pytest.mark.parametrize('shape', PASS_SHAPES)
def test_add_bounded_attaches_the_sum_of_the_bounds(shape):
    from dvd_hip import conv as C
    from dvd_hip.ops import known_amax
    torch.manual_seed(5)
    for attained in (False, True):
        a, b = torch.randn(shape), torch.randn(shape)
        if attained:                           # equal-sign maxima at the same place
            a[-1, -1, -1, -1], b[-1, -1, -1, -1] = -7.5, -6.25
        for factor in (3.0, 1.0):
            (ta, ka), (tb, kb) = _tag(a, factor), _tag(b, factor)
            y = C.add_bounded(ta, tb)
            want = float(known_amax(ta) + known_amax(tb))
            assert _scalar(y) == want and abs(want - (ka + kb)) <= 1e-6 * want
            assert _true(y) <= want
            if attained and factor == 1.0:
                assert _true(y) == want == 13.75
    # one operand without a scalar: nothing to attach
    y = C.add_bounded(_tag(a, 1.0)[0], b.cuda())
    assert known_amax(y) is None


@pytest.mark.parametrize('shape', PASS_SHAPES)
def test_alias_output_carries_the_input_scalar(shape):
    from dvd_hip import conv as C
    torch.manual_seed(6)
    N, Cc, H, W = shape
    conv = C.XConv2d(Cc, 8, 3, padding=1).cuda()
    bn = torch.nn.BatchNorm2d(8).cuda().eval()
    x_cpu = torch.randn(shape)
    for factor in (3.0, 1.0):
        x, kx = _tag(x_cpu, factor)
        y, xa = C.xconv2d(conv, x, alias=True)
        assert _scalar(xa, 'alias') == kx and _true(xa) <= kx and torch.equal(xa.detach(), x.detach())
        x, kx = _tag(x_cpu, factor)
        y, xa = C.conv_bn_act(conv, bn, x, alias=True)
        assert 'XConvBn' in type(y.grad_fn).__name__
        assert _scalar(xa, 'alias of conv_bn_act') == kx and _true(xa) <= kx and torch.equal(xa.detach(), x.detach())
        if factor == 1.0:
            assert _true(xa) == kx             # attained: the alias IS the input


# ---- 3. every scalar a matrix kernel consumes, in the real networks ---------------------------------------------------------

def _install_audit(monkeypatch, C, records):
    """Wrap the two host functions through which every fp32 operand scale reaches a kernel; records
    (wrapper, operand, scalar, true max of the operand as the kernel consumes it).  A 3x3 weight gradient that is handed a
    rowsum tensor (the entry point that also sums the gradient's rows) is recorded as 'xconv_wgrad3_rowsum'.  With stride=2
    the audited gy is the compact gradient: its maximum is the zero-interleaved copy's that the kernel consumes."""
    from dvd_hip.ops import amax_of
    real_run, real_wgrad = C._xconv_run, C.xconv_wgrad
    sig_run, sig_wgrad = inspect.signature(real_run), inspect.signature(real_wgrad)

    def note(wrapper, operand, t, k, relu=False):
        v = t.detach()
        records.append((wrapper, operand, float(k), float((v.relu() if relu else v).abs().max())))

    def run(*args, **kw):
        ba = sig_run.bind(*args, **kw)
        a = ba.arguments
        if a['x'].dtype == torch.float32:
            if a.get('x_amax') is None:
                a['x_amax'] = amax_of(a['x'])
            note('_xconv_run', 'x', a['x'], a['x_amax'], relu=bool(a.get('relu_in', False)))
        return real_run(*ba.args, **ba.kwargs)

    def wgrad(*args, **kw):
        ba = sig_wgrad.bind(*args, **kw)
        a = ba.arguments
        if a['gy'].dtype == torch.float32 and a['x'].dtype == torch.float32:
            if a.get('x_amax') is None:
                a['x_amax'] = amax_of(a['x'])
            if a.get('g_amax') is None:
                a['g_amax'] = amax_of(a['gy'])
            name = 'xconv_wgrad3_rowsum' if (a.get('rowsum') is not None and a['wshape'][2] == 3) else 'xconv_wgrad'
            note(name, 'x', a['x'], a['x_amax'], relu=bool(a['relu_in']))
            note(name, 'gy', a['gy'], a['g_amax'])
        return real_wgrad(*ba.args, **ba.kwargs)

    monkeypatch.setattr(C, '_xconv_run', run)
    monkeypatch.setattr(C, 'xconv_wgrad', wgrad)


def _audit_network(monkeypatch, name, net, shape, wrappers):
    from dvd_hip import conv as C
    records = []
    _install_audit(monkeypatch, C, records)
    g = torch.Generator().manual_seed(41)
    x0 = torch.rand(shape, generator=g).cuda()
    sites0 = C.STATS['sites_premasked'] + C.STATS['sites_no_pass']
    for rep, scale in enumerate((1.0, 1.0 / 16.0)):
        # the second pass in the same process: a smaller input and another upstream gradient -- a scalar that survived from
        # the first pass (a reused buffer, an attribute left on a tensor object) shows up as looseness, or as a bound too small
        start = len(records)
        net.zero_grad(set_to_none=True)
        out = net(x0 * scale)
        gy = torch.randn(out.shape, generator=g).cuda() * (1.0 if rep == 0 else 1e-3)
        out.backward(gy)
        rec = records[start:]
        assert rec
        worst = {}
        for wrapper, operand, k, m in rec:
            assert math.isfinite(k), '%s pass %d: %s %s scalar %r' % (name, rep, wrapper, operand, k)
            assert k >= m, '%s pass %d: %s %s scalar %r below max|t| %r' % (name, rep, wrapper, operand, k, m)
            if m > 0.0:
                worst[wrapper] = max(worst.get(wrapper, 1.0), k / m)
        for wrapper in wrappers:
            assert any(r[0] == wrapper for r in rec), '%s pass %d never reached %s' % (name, rep, wrapper)
        for wrapper, ratio in sorted(worst.items()):      # measured, not asserted: pass-through bounds are legitimately loose
            print('%s pass %d %s: %d operands, loosest scalar / max|t| = %.4g' %
                  (name, rep, wrapper, sum(r[0] == wrapper for r in rec), ratio))
            helpers.log_measured('operand_scales/%s/pass%d/%s/scalar_over_max' % (name, rep, wrapper), ratio, None)
    assert C.STATS['sites_premasked'] + C.STATS['sites_no_pass'] > sites0, 'no BatchNorm+ReLU site took the hand-over'


def test_every_consumed_scalar_bounds_its_operand_midas(monkeypatch):
    from dvd_hip.third_party.MiDaS import MidasNet
    net = MidasNet(path=None, non_negative=True, normalize_input=True)
    helpers.seeded_fill_(net, 7)
    with torch.no_grad():                      # (the synthetic head calibration of tests/test_30_full_step_gpu.py)
        net.scratch.output_conv[4].weight.mul_(30.0)
        net.scratch.output_conv[4].bias.fill_(2000.0)
    net = net.cuda().eval()
    _audit_network(monkeypatch, 'midas_1x3x64x96', net, (1, 3, 64, 96),
                   ('_xconv_run', 'xconv_wgrad', 'xconv_wgrad3_rowsum'))


def test_every_consumed_scalar_bounds_its_operand_hourglass(monkeypatch):
    from dvd_hip.third_party.hourglass import HourglassModel_Embed
    net = HourglassModel_Embed(noexp=False, use_embedding=False)
    helpers.seeded_fill_(net, 7)
    net = net.cuda().eval()
    _audit_network(monkeypatch, 'hourglass_2x3x32x48', net, (2, 3, 32, 48), ('_xconv_run', 'xconv_wgrad'))


# ---- 4. HIP-graph replay with shrinking magnitudes ----------------------------------------------------------------------------

def test_graph_replay_recomputes_every_scalar_for_the_replayed_data():
    """atomicMax never goes down: a scalar whose zero fill is not part of the graph keeps the largest value it ever saw.
    Replays with x0 * 64, x0 / 64 and a fresh tensor: every scalar of the capture is the maximum of THIS replay's tensor, and
    the results are the bits of an eager run."""
    from dvd_hip import conv as C, ops
    torch.manual_seed(41)
    c1, c2 = C.XConv2d(32, 64, 3, padding=1).cuda(), C.XConv2d(64, 256, 1).cuda()
    c3, c4 = C.XConv2d(256, 256, 1).cuda(), C.XConv2d(256, 32, 3, padding=1).cuda()
    bns = [torch.nn.BatchNorm2d(c).cuda().eval() for c in (64, 256, 256)]
    with torch.no_grad():
        for bn in bns:
            bn.running_mean.normal_(0, 0.5)
            bn.running_var.uniform_(0.3, 2.0)
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0, 0.3)
    params = [p for m in (c1, c2, c3, c4) + tuple(bns) for p in m.parameters()]

    def run(x, gy):
        acts = [C.xconv2d(c1, x)]
        acts.append(C.bn_eval_relu(bns[0], acts[-1]))
        acts.append(C.conv_bn_act(c2, bns[1], acts[-1], relu=False))
        acts.append(C.conv_bn_act(c3, bns[2], acts[-1]))
        acts.append(C.xconv2d(c4, acts[-1]))
        grads = {}
        for i, t in enumerate([x] + acts[:-1]):
            t.register_hook(lambda g, i=i: grads.__setitem__(i, g))
        acts[-1].backward(gy)
        return acts, [grads[i] for i in sorted(grads)]

    def fresh_grads():
        for p in params:
            p.grad = None

    x0 = torch.randn(1, 32, 16, 16, device='cuda')
    gy = torch.randn(1, 32, 16, 16, device='cuda')
    inputs = [('x0 * 64', x0 * 64.0), ('x0 / 64', x0 / 64.0), ('fresh', torch.randn(1, 32, 16, 16, device='cuda'))]
    # the eager results first: they are the warm-up pass the project's capture sites run before a capture, and no eager
    # autograd graph is alive while (or after) the graph is captured
    want = {}
    for label, value in [('x0', x0)] + inputs:
        fresh_grads()
        xe = value.clone().requires_grad_(True)
        e_acts, _ = run(xe, gy)
        want[label] = [e_acts[-1].detach().clone(), xe.grad.clone()] + [p.grad.clone() for p in params]
        del e_acts, xe
    fresh_grads()
    x_static = x0.clone().requires_grad_(True)
    gy_static = gy.clone()
    torch.cuda.synchronize()
    C.PACK_PLAN.extend()
    sites0 = C.STATS['sites_premasked'] + C.STATS['sites_no_pass']
    ops.begin_capture()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        acts, grads = run(x_static, gy_static)
    assert C.STATS['sites_premasked'] + C.STATS['sites_no_pass'] > sites0, 'the site hand-over was not captured'
    static_pgrads = [p.grad for p in params]
    assert all(g is not None for g in static_pgrads) and x_static.grad is not None and len(grads) == 5
    static_xgrad = x_static.grad
    tagged = [('act%d' % i, t) for i, t in enumerate(acts)] + [('grad%d' % i, t) for i, t in enumerate(grads)]
    tagged += [('x', x_static), ('gy', gy_static)]
    tagged = [(n, t) for n, t in tagged if getattr(t, '_dvd_amax', None) is not None]
    names = set(n for n, _ in tagged)
    assert names >= set(['act%d' % i for i in range(5)] + ['grad%d' % i for i in range(5)]), names
    for n, t in tagged:
        assert ops.known_amax(t) is None       # (a capture's scalar is not served outside it, by design)
    for label, value in inputs:
        with torch.no_grad():
            x_static.copy_(value)
        C.PACK_PLAN.ensure_current()
        graph.replay()
        for n, t in tagged:
            s, m = float(t._dvd_amax[1]), _true(t)
            assert s == m, 'replay with %s: scalar of %s is %r, max|t| is %r' % (label, n, s, m)
        got = [acts[-1].detach(), static_xgrad] + static_pgrads
        for i, (a, b) in enumerate(zip(got, want[label])):
            assert torch.equal(a, b), 'replay with %s: result %d differs from the eager run' % (label, i)
    fresh_grads()


# ---- 5. what the scale must not change ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('N,Cin,Cout,H,W,k', [(1, 64, 32, 20, 36, 3), (2, 256, 320, 12, 20, 1)])
def test_power_of_two_equivariance_is_bitwise(N, Cin, Cout, H, W, k):
    """x -> x * 2^e selects the same split terms and an unscale factor that is an exact power of two: y * 2^e, gx unchanged,
    gw * 2^e, bit for bit; likewise for gy -> gy * 2^e."""
    from dvd_hip import conv as C
    torch.manual_seed(Cin + k)
    conv = C.XConv2d(Cin, Cout, k, padding=k // 2, bias=False).cuda()
    x = torch.randn(N, Cin, H, W, device='cuda')
    gy = torch.randn(N, Cout, H, W, device='cuda')

    def run(xv, gv):
        xg = xv.clone().requires_grad_(True)
        conv.weight.grad = None
        y = C.xconv2d(conv, xg)
        y.backward(gv)
        return y.detach(), xg.grad, conv.weight.grad.clone()
    y0, gx0, gw0 = run(x, gy)
    for e in (-40, -7, 9, 40):
        s = 2.0 ** e
        y, gx, gw = run(x * s, gy)
        assert torch.equal(y, y0 * s), 'x * 2^%d: y' % e
        assert torch.equal(gx, gx0), 'x * 2^%d: gx' % e
        assert torch.equal(gw, gw0 * s), 'x * 2^%d: gw' % e
        y, gx, gw = run(x, gy * s)
        assert torch.equal(y, y0), 'gy * 2^%d: y' % e
        assert torch.equal(gx, gx0 * s), 'gy * 2^%d: gx' % e
        assert torch.equal(gw, gw0 * s), 'gy * 2^%d: gw' % e
    conv.weight.grad = None


def test_all_zero_input_gives_the_bias_exactly():
    from dvd_hip import conv as C
    torch.manual_seed(8)
    conv = C.XConv2d(32, 48, 3, padding=1).cuda()
    x = torch.zeros(2, 32, 9, 13, device='cuda')
    y = C.xconv2d(conv, x)
    assert torch.equal(y.detach(), conv.bias.detach().view(1, -1, 1, 1).expand_as(y))
    assert _scalar(y) == _true(conv.bias)


def test_an_entirely_rectified_site_feeds_zero_and_finite_gradients():
    from dvd_hip import conv as C
    torch.manual_seed(9)
    c1, c2 = C.XConv2d(32, 64, 1).cuda(), C.XConv2d(64, 48, 3, padding=1).cuda()
    bn = torch.nn.BatchNorm2d(64).cuda().eval()
    with torch.no_grad():
        bn.bias.fill_(-1000.0)                 # relu(bn(conv(x))) == 0 everywhere
    x = torch.randn(2, 32, 9, 13, device='cuda').requires_grad_(True)
    y1 = C.conv_bn_act(c1, bn, x)
    assert 'XConvBn' in type(y1.grad_fn).__name__
    assert _true(y1) == 0.0 and _scalar(y1) == 0.0
    y2 = C.xconv2d(c2, y1)
    assert torch.equal(y2.detach(), c2.bias.detach().view(1, -1, 1, 1).expand_as(y2))
    assert _scalar(y2) == _true(c2.bias)
    y2.backward(torch.randn_like(y2))
    grads = [x.grad] + [p.grad for m in (c1, c2, bn) for p in m.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)


@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
@pytest.mark.parametrize('k', [1, 3])
def test_non_finite_input_reaches_the_scalar_as_inf(bad, k):
    from dvd_hip import conv as C
    torch.manual_seed(10)
    conv = C.XConv2d(32, 48, k, padding=k // 2).cuda()
    x = torch.randn(1, 32, 13, 17)
    x[0, 5, 6, 7] = bad
    with torch.no_grad():
        y = C.xconv2d(conv, x.cuda())
        ref = F.conv2d(x.double(), conv.weight.detach().double().cpu(), conv.bias.detach().double().cpu(), padding=k // 2)
    s = _scalar(y)
    assert s == float('inf'), 'forward scalar %r' % s
    assert torch.equal(~torch.isfinite(y.cpu()), ~torch.isfinite(ref))
    assert int((~torch.isfinite(ref)).sum()) == 48 * k * k
