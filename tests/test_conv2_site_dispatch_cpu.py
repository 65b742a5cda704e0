"""Host logic of the fused `conv2` + BatchNorm + ReLU sites on the CPU (conv.conv_bn_act -> conv._conv2_site_kind, conv._GConvBn,
the stride-2 form of conv._XConvBn): which of the ResNeXt `conv2` kinds takes which path (fp32 fused; fp16 and CPU tensors on the
composition), pre-masked against self-masked sites, and where dbeta comes from (the weight-gradient call, or the fallback pass over
the COMPACT gradient).  The library is a stand-in that computes every entry point's contract in float64 and records the calls; a
tensor subclass reports is_cuda.  Gradients are compared with autograd on the float64 ATen expression: the stand-ins round to the
fp32 tensors they are handed, so 1e-5 of the value (+ 1e-6) -- a wiring error is an O(1) difference.  The kernels:
tests/test_42_gconv_bn_site_gpu.py, tests/test_43_conv2_bn_sites_gpu.py."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn


class _Gpu(torch.Tensor):
    @property
    def is_cuda(self):
        return True


def _plain(t):
    return None if t is None else t.detach().as_subclass(torch.Tensor)


class _Lib(object):
    def __init__(self):
        self.calls = []
        self.in_kernel = 1

    def _rec(self, name, **kw):
        self.calls.append((name, kw))
        return 0

    def names(self):
        return [n for n, _ in self.calls]

    def dvd_bnrelu_bwd_workspace_bytes(self, N, C, HW):
        return 16

    def dvd_gconv3x3_c8_bn_wgrad_workspace_bytes(self, N, C, H, W):
        return 16

    def dvd_xwgrad3_workspace_bytes(self, *dims):
        return 16

    def dvd_xwgrad_rowsum_in_kernel(self, N, Cin, Cout, H, W, KS, groups):
        self._rec('in_kernel?', hw=(H, W))
        return self.in_kernel

    def dvd_gconv3x3_c8_bn_fwd(self, x, w, gamma, beta, mean, var, eps, y, y_amax, N, C, H, W, stream):
        x, w, gamma, beta = _plain(x), _plain(w), _plain(gamma), _plain(beta)
        s = gamma.double() / torch.sqrt(var.double() + eps)
        z = F.conv2d(x.double(), w.double(), padding=1, groups=C // 8)
        out = (z * s.reshape(1, -1, 1, 1) + (beta.double() - mean.double() * s).reshape(1, -1, 1, 1)).relu()
        _plain(y).copy_(out)
        y_amax.fill_(float(out.abs().max()))
        return self._rec('dvd_gconv3x3_c8_bn_fwd')

    def dvd_gconv3x3_c8_bn_bwd_data(self, g, w, gamma, var, eps, mask_src, gx, gx_amax, N, C, H, W, stream):
        s = _plain(gamma).double() / torch.sqrt(var.double() + eps)
        out = F.conv_transpose2d(_plain(g).double() * s.reshape(1, -1, 1, 1), _plain(w).double(), padding=1, groups=C // 8)
        if mask_src is not None:
            out = out * (_plain(mask_src) > 0)
        _plain(gx).copy_(out)
        gx_amax.fill_(float(out.abs().max()))
        return self._rec('dvd_gconv3x3_c8_bn_bwd_data', masked=mask_src is not None)

    def dvd_gconv3x3_c8_bn_bwd_weight(self, x, g, gw, chansum, ws, ws_bytes, N, C, H, W, stream):
        x, g = _plain(x).double(), _plain(g).double()
        _plain(gw).copy_(torch.nn.grad.conv2d_weight(x, gw.shape, g, padding=1, groups=C // 8))
        chansum.copy_(g.sum((0, 2, 3)))
        return self._rec('dvd_gconv3x3_c8_bn_bwd_weight')

    def dvd_bnrelu_bwd_t(self, gy, y, x, gamma, mean, var, eps, gx, gres, ggamma, gbeta, ws, ws_bytes, f16, out_scale, N, C, HW,
                         relu, g_amax, stream):
        gy = _plain(gy)
        g = gy.double() * (_plain(y) > 0) if relu else gy.double()
        if gres is not None:
            _plain(gres).copy_(g)
        if gbeta is not None:
            gbeta.copy_(g.sum((0, 2, 3)))
        if g_amax is not None:
            g_amax.fill_(float(g.abs().max()))
        return self._rec('dvd_bnrelu_bwd_t', relu=bool(relu), sums=gbeta is not None, hw=HW)

    def dvd_subsample2_bwd(self, gy, gyf, f16, planes, H, W, stream):
        out = _plain(gyf)
        out.zero_()
        out[:, :, ::2, ::2] = _plain(gy)
        return self._rec('dvd_subsample2_bwd', hw=(H, W))

    def _wgrad(self, name, x, gy, gw, rowsum, groups):
        x, gy = _plain(x).double(), _plain(gy).double()
        _plain(gw).copy_(torch.nn.grad.conv2d_weight(x, gw.shape, gy, padding=1, groups=groups))
        if rowsum is not None:
            rowsum.copy_(gy.sum((0, 2, 3)))
        return self._rec(name, hw=tuple(gy.shape[2:]))

    def dvd_xwgrad3_rowsum(self, x, x_amax, gy, g_amax, gw, rowsum, ws, ws_bytes, N, Cin, Cout, H, W, groups, relu_in, stream):
        assert x_amax is not None and g_amax is not None and rowsum is not None and not relu_in
        return self._wgrad('dvd_xwgrad3_rowsum', x, gy, gw, rowsum, groups)

    def dvd_xwgrad3(self, x, x_amax, gy, g_amax, gw, ws, ws_bytes, N, Cin, Cout, H, W, groups, relu_in, stream):
        assert x_amax is not None and g_amax is not None and not relu_in
        return self._wgrad('dvd_xwgrad3', x, gy, gw, None, groups)

    def dvd_convbn_finalize(self, W, dW, dbeta, gamma, mean, var, eps, cbias, Cout, K, dgamma, dcbias, stream):
        W, dW, gamma = _plain(W), _plain(dW), _plain(gamma)
        assert K == W[0].numel() and cbias is None
        rstd = 1.0 / torch.sqrt(var.double() + eps)
        acc = (W.double().reshape(Cout, -1) * dW.double().reshape(Cout, -1)).sum(1)
        dgamma.copy_(rstd * (acc - mean.double() * dbeta.double()))
        dW.copy_(dW.double() * (gamma.double() * rstd).reshape(-1, 1, 1, 1))
        return self._rec('dvd_convbn_finalize')


@pytest.fixture
def stand_in(monkeypatch):
    from dvd_hip import conv as C
    lib = _Lib()

    def run(x, packed, Cout, KS, bias=None, residual=None, mask_src=None, relu_in=False, relu_out=False, res_relu=False,
            groups=1, bn=None, x_amax=None, y_amax=None, stride=1, out_hw=None):
        w, transposed = packed
        assert transposed == (stride == -2 or (stride == 1 and bn is None))
        xin = _plain(x).double()
        if stride == 2:
            y = F.conv2d(xin, w.double(), padding=1, groups=groups, stride=2)
        elif stride == -2:
            op = (out_hw[0] - 1 - 2 * (xin.shape[2] - 1), out_hw[1] - 1 - 2 * (xin.shape[3] - 1))
            y = F.conv_transpose2d(xin, w.double(), padding=1, groups=groups, stride=2, output_padding=op)
        else:
            y = (F.conv_transpose2d if transposed else F.conv2d)(xin, w.double(), padding=KS // 2, groups=groups)
        if bn is not None:
            g, b, m, v, eps = bn
            s = _plain(g).double() / torch.sqrt(v.double() + eps)
            y = y * s.reshape(1, -1, 1, 1) + (_plain(b).double() - m.double() * s).reshape(1, -1, 1, 1)
        if mask_src is not None:
            y = y * (_plain(mask_src) > 0)
        if relu_out:
            y = y.relu()
        if y_amax is not None:
            y_amax.fill_(float(y.abs().max()))
        lib._rec('_xconv_run', stride=stride, groups=groups, bn=bn is not None, masked=mask_src is not None)
        return y.to(x.dtype).contiguous().as_subclass(_Gpu)

    def scaled(weight, groups, gamma, var, eps):
        return (_plain(weight).double() * (_plain(gamma).double() / torch.sqrt(var.double() + eps)).reshape(-1, 1, 1, 1), True)

    monkeypatch.setattr(C, '_xconv_run', run)
    monkeypatch.setattr(C, 'xconv_packed', lambda weight, transposed, groups=1: (_plain(weight), bool(transposed)))
    monkeypatch.setattr(C, 'xconv_packed_scaled', scaled)
    monkeypatch.setattr(C, 'amax_of', lambda t: _plain(t).abs().max().reshape(1))
    monkeypatch.setattr(C, 'new_scalar', lambda device: torch.zeros(1))
    monkeypatch.setattr(C, 'set_amax', lambda t, am: t)
    monkeypatch.setattr(C, 'known_amax', lambda t: None)
    monkeypatch.setattr(C, '_p', lambda t: t)
    monkeypatch.setattr(C, '_stream', lambda: 0)
    monkeypatch.setattr(C, '_workspace', lambda nbytes, device: torch.empty(int(nbytes), dtype=torch.uint8))
    monkeypatch.setattr(C._lib, 'load', lambda: lib)
    monkeypatch.setattr(C._lib, 'check', lambda rc, name: None)
    for k in C.STATS:
        C.STATS[k] = 0
    assert not any(C.AB.values())
    return C, lib


class _Consumer(torch.autograd.Function):
    """A convolution-like consumer of a site's output: its backward masks the gradient and tells the site (see conv._Site)."""

    @staticmethod
    def forward(ctx, y, site):
        ctx.site = site
        ctx.save_for_backward(y)
        return y * 2.0

    @staticmethod
    def backward(ctx, gy):
        y, = ctx.saved_tensors
        g = (2.0 * gy * (y > 0)).contiguous()
        ctx.site.wrote(g, g.abs().max().reshape(1))
        return g, None


def _layer(C, kind):
    g = torch.Generator().manual_seed(len(kind) + 7)
    if kind == 'c8':
        conv = C.GroupedConv3x3C8(16)
    elif kind == 'c16':
        conv = C.GroupedConv3x3C16(64)
    elif kind == 'c16s2':
        conv = C.GroupedConv3x3C16(64, stride=2)
    else:
        conv = C.XConv2d(64, 64, 3, stride=2, padding=1, groups=2, bias=False)
    ch = conv.in_channels
    bn = nn.BatchNorm2d(ch).eval()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.2)
        bn.weight.copy_(1.0 + 0.3 * torch.randn(ch, generator=g))
        bn.weight[1::3].neg_()
        bn.bias.copy_(0.1 * torch.randn(ch, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(ch, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(ch, generator=g))
    x = torch.randn(2, ch, 5, 7, generator=g).relu()
    return conv, bn, x, g


def _reference(conv, bn, x, gy, consumed):
    w, ga, be = [t.detach().double().requires_grad_(True) for t in (conv.weight, bn.weight, bn.bias)]
    xx = x.double().requires_grad_(True)
    h = xx.relu()                    # the input is a site's output: the layer masks its input gradient for that site
    z = F.conv2d(h, w, None, conv.stride, 1, 1, conv.groups)
    y = F.batch_norm(z, bn.running_mean.double(), bn.running_var.double(), ga, be, False, 0.0, bn.eps).relu()
    (y * 2.0 if consumed else y).backward(gy.double())
    return [h.grad if False else xx.grad, w.grad, ga.grad, be.grad]


def _fused(C, conv, bn, x, gy, consumed):
    for p in list(conv.parameters()) + list(bn.parameters()):
        p.grad = None
    leaf = x.clone().requires_grad_(True)
    xin = (leaf * 1.0).as_subclass(_Gpu)
    xin._dvd_site = C._Site()        # x is a BatchNorm+ReLU site's output
    y = C.conv_bn_act(conv, bn, xin)
    assert getattr(y, '_dvd_site', None) is not None
    out = _Consumer.apply(y, y._dvd_site) if consumed else y
    out.backward(gy)
    return [leaf.grad, conv.weight.grad, bn.weight.grad, bn.bias.grad], xin._dvd_site


def _close(got, want):
    for i, (a, b) in enumerate(zip(got, want)):
        a = _plain(a)
        assert a.dtype == torch.float32 and torch.allclose(a.double(), b, rtol=1e-5, atol=1e-6), (i, float((a.double() - b).abs().max()))


@pytest.mark.parametrize('consumed', [True, False])
def test_eight_per_group_site(stand_in, consumed):
    C, lib = stand_in
    conv, bn, x, g = _layer(C, 'c8')
    gy = torch.randn(2, 16, 5, 7, generator=g)
    got, in_site = _fused(C, conv, bn, x, gy, consumed)
    # x > 0 exactly where relu(x) keeps it: the reference's input ReLU is the mask the epilogue applies for the site in front
    _close(got, _reference(conv, bn, x, gy, consumed))
    assert lib.names().count('dvd_gconv3x3_c8_bn_fwd') == 1 and '_xconv_run' not in lib.names()
    passes = [kw for n, kw in lib.calls if n == 'dvd_bnrelu_bwd_t']
    assert passes == ([] if consumed else [{'relu': True, 'sums': False, 'hw': 35}]), passes
    assert ('dvd_gconv3x3_c8_bn_bwd_data', {'masked': True}) in lib.calls and 'dvd_gconv3x3_c8_bn_bwd_weight' in lib.names()
    assert in_site.amax is not None and in_site.ref is not None         # the hand-over to the site in front, with max|gx|
    assert C.STATS == {'sites_premasked': int(consumed), 'sites_masked': int(not consumed), 'sites_no_pass': 0}, C.STATS


def test_no_maskfuse_keeps_the_mask_out_of_the_epilogue(stand_in):
    C, lib = stand_in
    conv, bn, x, g = _layer(C, 'c8')
    gy = torch.randn(2, 16, 5, 7, generator=g)
    C.AB['no_maskfuse'] = True
    try:
        _fused(C, conv, bn, x, gy, True)
    finally:
        C.AB['no_maskfuse'] = False
    assert ('dvd_gconv3x3_c8_bn_bwd_data', {'masked': False}) in lib.calls
    assert [kw['relu'] for n, kw in lib.calls if n == 'dvd_bnrelu_bwd_t'] == [True]
    assert C.STATS['sites_masked'] == 1 and C.STATS['sites_premasked'] == 0


@pytest.mark.parametrize('kind,in_kernel', [('c16', 1), ('c16', 0), ('c16s2', 1), ('c16s2', 0), ('s2', 1), ('s2', 0)])
def test_xconv_family_sites(stand_in, kind, in_kernel):
    C, lib = stand_in
    lib.in_kernel = in_kernel
    conv, bn, x, g = _layer(C, kind)
    s2 = kind != 'c16'
    ch = conv.in_channels
    gy = torch.randn(2, ch, 3 if s2 else 5, 4 if s2 else 7, generator=g)
    got, in_site = _fused(C, conv, bn, x, gy, True)
    _close(got, _reference(conv, bn, x, gy, True))
    groups = conv.groups // 2 if kind != 's2' else conv.groups
    runs = [kw for n, kw in lib.calls if n == '_xconv_run']
    assert runs == [{'stride': 2 if s2 else 1, 'groups': groups, 'bn': True, 'masked': False},
                    {'stride': -2 if s2 else 1, 'groups': groups, 'bn': False, 'masked': True}], runs
    assert 'dvd_gconv3x3_c8_bn_fwd' not in lib.names()
    assert ('in_kernel?', {'hw': (5, 7)}) in lib.calls                 # asked for the resolution the weight gradient runs at
    assert (('dvd_subsample2_bwd', {'hw': (5, 7)}) in lib.calls) == s2
    passes = [kw for n, kw in lib.calls if n == 'dvd_bnrelu_bwd_t']
    if in_kernel:                      # pre-masked, sums from the kernel, max|g| from the consumer: no pass
        assert passes == [] and ('dvd_xwgrad3_rowsum', {'hw': (5, 7)}) in lib.calls and 'dvd_xwgrad3' not in lib.names()
    else:                              # the sum pass, over the COMPACT gradient
        assert passes == [{'relu': False, 'sums': True, 'hw': gy.shape[2] * gy.shape[3]}], passes
        assert ('dvd_xwgrad3', {'hw': (5, 7)}) in lib.calls and 'dvd_xwgrad3_rowsum' not in lib.names()
    assert C.STATS['sites_premasked'] == 1 and C.STATS['sites_masked'] == 0


def test_fp16_and_cpu_tensors_keep_the_composition(stand_in, monkeypatch):
    C, lib = stand_in
    seen = []
    monkeypatch.setattr(C, 'bn_eval_relu', lambda bn, z, residual=None, relu=True: seen.append(z.dtype) or z)
    for kind in ('c8', 'c16', 'c16s2', 's2'):
        conv, bn, x, g = _layer(C, kind)
        monkeypatch.setattr(conv, 'forward', lambda t: t)
        assert C._conv2_site_kind(conv, bn, x.as_subclass(_Gpu), None, True) == {'c16s2': 's2'}.get(kind, kind)
        assert C._conv2_site_kind(conv, bn, x.half().as_subclass(_Gpu), None, True) is None
        C.conv_bn_act(conv, bn, x.half().as_subclass(_Gpu))
        C.conv_bn_act(conv, bn, x)                                     # a CPU tensor
    assert seen == [torch.float16, torch.float32] * 4 and lib.calls == []
    # not a ReLU site, a residual, a BatchNorm without affine parameters: the composition
    conv, bn, x, g = _layer(C, 'c8')
    xg = x.as_subclass(_Gpu)
    assert C._conv2_site_kind(conv, bn, xg, None, False) is None and C._conv2_site_kind(conv, bn, xg, xg, True) is None
    assert C._conv2_site_kind(conv, nn.BatchNorm2d(16, affine=False).eval(), xg, None, True) is None
