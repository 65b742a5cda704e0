"""Host logic of conv._XConvBn.backward on the CPU: under default switches an fp32 BatchNorm+ReLU site whose consumer has
applied the ReLU mask runs NO pass of its own over the gradient -- the per-channel sums (dbeta) come from the weight-gradient
call (dvd_xwgrad1s_rowsum for the dense 1x1, dvd_xwgrad3_rowsum for the grouped 3x3 convolutions of torchvision's Bottleneck
behind third_party/midas_blocks.py:35-50), max|g| from the consumer's epilogue -- and a site that masks for itself takes its
sums from the same call.  The library is a stand-in that computes every entry point's contract in float64 and records the
calls; conv.xconv_wgrad itself runs.  The gradients are compared with autograd on the float64
ATen expression: the stand-ins round their results to the fp32 tensors they are handed, so 1e-5 of the value (+ 1e-6) -- a
wiring error is an O(1) difference.  The kernels: tests/test_40_wgrad_rowsum_gpu.py."""
import pytest
import torch
import torch.nn.functional as F


class _Lib(object):
    def __init__(self):
        self.calls = []
        self.in_kernel = 1

    def dvd_xwgrad_rowsum_in_kernel(self, N, Cin, Cout, H, W, KS, groups):
        assert (N, H, W) == (2, 5, 7) and Cout == 8 and (Cin, KS, groups) in ((6, 1, 1), (8, 3, 2))
        return self.in_kernel

    def _rec(self, name, **kw):
        self.calls.append((name, kw))
        return 0

    def names(self):
        return [n for n, _ in self.calls]

    def dvd_bnrelu_bwd_workspace_bytes(self, N, C, HW):
        return 16

    def dvd_xwgrad1s_workspace_bytes(self, *dims):
        return 16

    def dvd_xwgrad3_workspace_bytes(self, *dims):
        return 16

    def dvd_bnrelu_bwd_t(self, gy, y, x, gamma, mean, var, eps, gx, gres, ggamma, gbeta, ws, ws_bytes, f16, out_scale, N, C, HW,
                         relu, g_amax, stream):
        g = gy.double() * (y > 0) if relu else gy.double()
        if gres is not None:
            gres.copy_(g)
        if gbeta is not None:
            gbeta.copy_(g.sum((0, 2, 3)))
        if g_amax is not None:
            g_amax.fill_(float(g.abs().max()))
        return self._rec('dvd_bnrelu_bwd_t', relu=bool(relu))

    def _wgrad(self, name, x, gy, gw, rowsum, groups):
        gw.copy_(torch.nn.grad.conv2d_weight(x.double(), gw.shape, gy.double(), padding=gw.shape[2] // 2, groups=groups))
        if rowsum is not None:
            rowsum.copy_(gy.double().sum((0, 2, 3)))
        return self._rec(name, rowsum=rowsum is not None)

    def dvd_xwgrad1s_rowsum(self, x, x_amax, gy, g_amax, gw, rowsum, ws, ws_bytes, N, Cin, Cout, H, W, relu_in, stream):
        assert x_amax is not None and g_amax is not None and not relu_in
        return self._wgrad('dvd_xwgrad1s_rowsum', x, gy, gw, rowsum, 1)

    def dvd_xwgrad3_rowsum(self, x, x_amax, gy, g_amax, gw, rowsum, ws, ws_bytes, N, Cin, Cout, H, W, groups, relu_in, stream):
        assert x_amax is not None and g_amax is not None and not relu_in and rowsum is not None
        return self._wgrad('dvd_xwgrad3_rowsum', x, gy, gw, rowsum, groups)

    def dvd_xwgrad3(self, x, x_amax, gy, g_amax, gw, ws, ws_bytes, N, Cin, Cout, H, W, groups, relu_in, stream):
        return self._wgrad('dvd_xwgrad3', x.relu() if relu_in else x, gy, gw, None, groups)

    def dvd_convbn_finalize(self, W, dW, dbeta, gamma, mean, var, eps, cbias, Cout, K, dgamma, dcbias, stream):
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
            groups=1, bn=None, x_amax=None, y_amax=None):
        w, transposed = packed
        xin = (x.relu() if relu_in else x).double()
        y = (F.conv_transpose2d if transposed else F.conv2d)(xin, w.double(), padding=KS // 2, groups=groups)
        if bn is not None:
            g, b, m, v, eps = bn
            s = g.double() / torch.sqrt(v.double() + eps)
            y = y * s.reshape(1, -1, 1, 1) + (b.double() - m.double() * s).reshape(1, -1, 1, 1)
        if residual is not None:
            y = y + residual.double()
        if mask_src is not None:
            y = y * (mask_src > 0)
        if relu_out:
            y = y.relu()
        if y_amax is not None:
            y_amax.fill_(float(y.abs().max()))
        return y.to(x.dtype).contiguous()

    def scaled(weight, groups, gamma, var, eps):
        return (weight.detach().double() * (gamma.double() / torch.sqrt(var.double() + eps)).reshape(-1, 1, 1, 1), True)

    monkeypatch.setattr(C, '_xconv_run', run)
    monkeypatch.setattr(C, 'xconv_packed', lambda weight, transposed, groups=1: (weight.detach(), bool(transposed)))
    monkeypatch.setattr(C, 'xconv_packed_scaled', scaled)
    monkeypatch.setattr(C, 'amax_of', lambda t: t.detach().abs().max().reshape(1))
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


def _bn(c, g):
    return [1.0 + 0.1 * torch.randn(c, generator=g), 0.05 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g),
            0.5 + torch.rand(c, generator=g)]


def _site(C, x, w, bn, groups=1, eps=1e-5):
    gamma, beta, mean, var = bn
    out_site = C._Site()
    out = C._XConvBn.apply(x, C.amax_of(x), w, None, gamma, beta, mean, var, eps, None, True, groups, False,
                           getattr(x, '_dvd_site', None), out_site)
    out[0]._dvd_site = out_site
    return out[0]


def _ref_site(x, w, bn, groups=1, eps=1e-5):
    gamma, beta, mean, var = bn
    return F.batch_norm(F.conv2d(x, w, padding=w.shape[2] // 2, groups=groups), mean, var, gamma, beta, False, 0.0, eps).relu()


@pytest.mark.parametrize('consumed', [True, False])
def test_premasked_sites_take_their_sums_from_the_weight_gradient_call(stand_in, consumed):
    """conv1 (dense 1x1) -> conv2 (grouped 3x3) -> a plain convolution: both sites find their mask applied by their consumer.
    consumed=False: nobody consumes conv2's output, so that site masks for itself (one mask pass) and still takes the sums of
    the masked gradient from the weight-gradient call."""
    C, lib = stand_in
    g = torch.Generator().manual_seed(11)
    ws = [torch.randn(8, 6, 1, 1, generator=g) * 0.4, torch.randn(8, 4, 3, 3, generator=g) * 0.2, torch.randn(5, 8, 1, 1, generator=g) * 0.4]
    bns = [_bn(8, g), _bn(8, g)]
    x0 = torch.randn(2, 6, 5, 7, generator=g)
    gy = torch.randn(2, 5 if consumed else 8, 5, 7, generator=g)

    def leaves(dtype):
        return ([w.to(dtype).clone().requires_grad_(True) for w in ws],
                [[t.to(dtype).clone().requires_grad_(i < 2) for i, t in enumerate(bn)] for bn in bns], x0.to(dtype).clone().requires_grad_(True))

    W, B, x = leaves(torch.float64)
    h = _ref_site(_ref_site(x, W[0], B[0]), W[1], B[1], groups=2)
    (F.conv2d(h, W[2]) if consumed else h).backward(gy.double())
    want = [x.grad] + [w.grad for w in W[:2 + consumed]] + [t.grad for bn in B for t in bn[:2]]

    W, B, x = leaves(torch.float32)
    h = _site(C, _site(C, x, W[0], B[0]), W[1], B[1], groups=2)
    (C._xconv(h, W[2], None, None, False, False) if consumed else h).backward(gy)
    got = [x.grad] + [w.grad for w in W[:2 + consumed]] + [t.grad for bn in B for t in bn[:2]]
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == torch.float32 and torch.allclose(a.double(), b, rtol=1e-5, atol=1e-6), (i, float((a.double() - b).abs().max()))

    passes = [kw for n, kw in lib.calls if n.startswith('dvd_bnrelu_bwd')]
    assert passes == ([] if consumed else [{'relu': True}]), passes
    # both sites hand dbeta to their weight-gradient call, the grouped one through the 3x3 entry point that sums
    assert ('dvd_xwgrad1s_rowsum', {'rowsum': True}) in lib.calls and ('dvd_xwgrad3_rowsum', {'rowsum': True}) in lib.calls
    assert 'dvd_xwgrad3' not in lib.names()
    assert C.STATS == {'sites_premasked': 1 + consumed, 'sites_masked': 1 - consumed, 'sites_no_pass': 0}, C.STATS


def test_shapes_the_kernels_do_not_sum_keep_the_sites_own_pass(stand_in):
    """Where the weight-gradient kernel of the shape has no summing form, the entry point would add a pass over gy that is
    slower than the site's own: the site keeps its sum pass and hands no sums tensor on."""
    C, lib = stand_in
    lib.in_kernel = 0
    g = torch.Generator().manual_seed(13)
    w = (torch.randn(8, 6, 1, 1, generator=g) * 0.4).requires_grad_(True)
    wc = (torch.randn(5, 8, 3, 3, generator=g) * 0.2).requires_grad_(True)
    x = torch.randn(2, 6, 5, 7, generator=g).requires_grad_(True)
    C._xconv(_site(C, x, w, _bn(8, g)), wc, None, None, False, False).sum().backward()
    assert [kw for n, kw in lib.calls if n.startswith('dvd_bnrelu_bwd')] == [{'relu': False}]
    assert ('dvd_xwgrad1s_rowsum', {'rowsum': False}) in lib.calls and ('dvd_xwgrad1s_rowsum', {'rowsum': True}) not in lib.calls
    assert C.STATS == {'sites_premasked': 1, 'sites_masked': 0, 'sites_no_pass': 0}


def test_other_dtypes_keep_the_sites_own_pass(stand_in):
    """Only fp32 sites skip the pass (float64 here stands for 'not fp32': the fp16 forms need the GPU)."""
    C, lib = stand_in
    g = torch.Generator().manual_seed(12)
    w = (torch.randn(8, 6, 1, 1, generator=g) * 0.4).double().requires_grad_(True)
    wc = (torch.randn(5, 8, 3, 3, generator=g) * 0.2).double().requires_grad_(True)
    bn = [t.double() for t in _bn(8, g)]
    x = torch.randn(2, 6, 5, 7, generator=g).double().requires_grad_(True)
    lib.dvd_xwgrad1s_rowsum = lambda x, xa, gy, ga, gw, rowsum, *rest: lib._wgrad('dvd_xwgrad1s_rowsum', x, gy, gw, rowsum, 1)
    C._xconv(_site(C, x, w, bn), wc, None, None, False, False).sum().backward()
    assert [kw for n, kw in lib.calls if n.startswith('dvd_bnrelu_bwd')] == [{'relu': False}]
    assert ('dvd_xwgrad1s_rowsum', {'rowsum': False}) in lib.calls
    assert C.STATS == {'sites_premasked': 1, 'sites_masked': 0, 'sites_no_pass': 0}
