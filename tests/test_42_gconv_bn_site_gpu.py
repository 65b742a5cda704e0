"""The BatchNorm+ReLU site of the 8-per-group 3x3 convolution inside the kernels of csrc/gconv.hip (dvd_gconv3x3_c8_bn_*,
conv._GConvBn) against the composition it replaces, `bn_eval_relu(bn, gconv3x3_c8(x, w))`, and against float64 autograd of
relu(batch_norm(conv2d)) on the CPU.

Shapes (N, C, H, W), the smallest that reach every code path of the three kernels:
  (2, 16, 13, 84)   84x12 tile, a last tile row of one line, 56-wide weight-gradient tiles with a partial band
  (1,  8, 17, 67)   64x16 tile, scalar load / store path, partial tiles on both edges
  (2, 24,  9, 56)   16-byte path on the 64-wide tile, 56-wide weight-gradient tile
  (1, 16,  8, 168)  two tiles per row, exactly one band
BatchNorm parameters are random with some negative gamma and var in [0.3, 3]; channel 0 has a beta so low that its whole output is
masked; the input is a ReLU output (exact zeros).

Bounds.  Forward, backward-data and the masking epilogue form the composition's values with the composition's roundings (same
accumulators, same fmaf, the same product g * s): bit-identical.  dW, dgamma and dbeta are s * sum(g x) instead of
sum((g s) x) and sums in another order: only the order of roundings changes, so their error against float64 may be at most
twice the error of the composition on the same inputs against the same reference (both are measured here)."""
import pytest
import torch
import torch.nn.functional as F

from helpers import log_measured

pytestmark = pytest.mark.gpu

SHAPES = [(2, 16, 13, 84), (1, 8, 17, 67), (2, 24, 9, 56), (1, 16, 8, 168)]
EPS = 1e-5
_CACHE = {}


def _inputs(shape):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(1000 * C + H + W)
    x = torch.randn(N, C, H, W, generator=g).relu()
    w = torch.randn(C, 8, 3, 3, generator=g) * 0.2
    gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
    gamma[1::3] = -gamma[1::3]                             # some negative scales
    beta = 0.2 * torch.randn(C, generator=g)
    beta[0] = -100.0                                       # channel 0: everything masked
    mean = 0.2 * torch.randn(C, generator=g)
    var = 0.3 + 2.7 * torch.rand(C, generator=g)
    gy = torch.randn(N, C, H, W, generator=g)
    return x, w, gamma, beta, mean, var, gy


def _bn(C, gamma, beta, mean, var, device, dtype):
    bn = torch.nn.BatchNorm2d(C, eps=EPS).to(device=device, dtype=dtype).eval()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(mean)
        bn.running_var.copy_(var)
    return bn


class _Consumer(torch.autograd.Function):
    """Stand-in for the convolution that consumes a site's output: identity forward; its backward masks the gradient with
    [y > 0] in a tensor of its own and tells the site so (what a backward-data epilogue with mask_src does)."""

    @staticmethod
    def forward(ctx, y, site):
        ctx.site = site
        ctx.save_for_backward(y)
        return y.clone()

    @staticmethod
    def backward(ctx, gy):
        y, = ctx.saved_tensors
        g = gy * (y > 0).to(gy.dtype)
        ctx.site.wrote(g)
        return g, None


def _site_run(C, t, premask, in_site=None):
    """One forward + backward of the fused site -> dict of results."""
    x = t['x'].clone().requires_grad_(True)
    w = t['w'].clone().requires_grad_(True)
    gamma = t['gamma'].clone().requires_grad_(True)
    beta = t['beta'].clone().requires_grad_(True)
    out_site = C._Site()
    for k in C.STATS:
        C.STATS[k] = 0
    seen = {}
    x.register_hook(lambda g: seen.__setitem__('gx', g))       # the tensor the kernel wrote, with the scalar attached to it
    y, y_amax = C._GConvBn.apply(x, w, gamma, beta, t['mean'], t['var'], EPS, in_site, out_site)
    (_Consumer.apply(y, out_site) if premask else y).backward(t['gy'])
    assert C.STATS['sites_premasked'] == int(premask) and C.STATS['sites_masked'] == int(not premask), C.STATS
    return dict(y=y.detach(), y_amax=y_amax, gx=x.grad, gw=w.grad, ggamma=gamma.grad, gbeta=beta.grad,
                gx_amax=float(seen['gx']._dvd_amax[1]), site_saw_gx=in_site is not None and in_site.is_exactly(seen['gx']))


def _results(shape):
    """Everything the tests of one shape compare, computed once."""
    if shape in _CACHE:
        return _CACHE[shape]
    from dvd_hip import conv as C
    N, Cc, H, W = shape
    cpu = dict(zip(('x', 'w', 'gamma', 'beta', 'mean', 'var', 'gy'), _inputs(shape)))
    t = {k: v.cuda() for k, v in cpu.items()}
    # the composition (the parent's path): stand-alone convolution, then the BatchNorm+ReLU kernel
    bn = _bn(Cc, t['gamma'], t['beta'], t['mean'], t['var'], 'cuda', torch.float32)
    xc = t['x'].clone().requires_grad_(True)
    wc = t['w'].clone().requires_grad_(True)
    yc = C.bn_eval_relu(bn, C.gconv3x3_c8(xc, wc))
    yc.backward(t['gy'])
    comp = dict(y=yc.detach(), gx=xc.grad, gw=wc.grad, ggamma=bn.weight.grad, gbeta=bn.bias.grad)
    # float64 autograd on the CPU
    x64, w64 = cpu['x'].double().requires_grad_(True), cpu['w'].double().requires_grad_(True)
    g64, b64 = cpu['gamma'].double().requires_grad_(True), cpu['beta'].double().requires_grad_(True)
    y64 = F.batch_norm(F.conv2d(x64, w64, padding=1, groups=Cc // 8), cpu['mean'].double(), cpu['var'].double(), g64, b64, False, 0.0,
                       EPS).relu()
    y64.backward(cpu['gy'].double())
    ref = dict(gw=w64.grad, ggamma=g64.grad, gbeta=b64.grad)
    own = _site_run(C, t, premask=False)
    pre = _site_run(C, t, premask=True)
    in_site = C._Site()
    msk = _site_run(C, t, premask=True, in_site=in_site)
    msk['in_site'] = in_site
    again = _site_run(C, t, premask=True)
    _CACHE[shape] = dict(t=t, comp=comp, ref=ref, own=own, pre=pre, msk=msk, again=again)
    return _CACHE[shape]


@pytest.mark.parametrize('shape', SHAPES)
def test_a1_forward_is_the_composition_bit_for_bit(shape):
    r = _results(shape)
    y = r['own']['y']
    assert torch.equal(y, r['comp']['y'])
    assert float(y[:, 0].abs().max()) == 0.0 and float(y.max()) > 0.0          # the fully masked channel, and not everything
    for k in ('own', 'pre', 'msk'):
        assert torch.equal(r[k]['y'], y)
        assert float(r[k]['y_amax']) == float(y.abs().max())


@pytest.mark.parametrize('shape', SHAPES)
def test_a2_backward_data_is_the_composition_bit_for_bit(shape):
    r = _results(shape)
    assert float(r['comp']['gx'].abs().max()) > 0.0
    assert torch.equal(r['pre']['gx'], r['comp']['gx'])          # mask pre-applied by the consumer
    assert torch.equal(r['own']['gx'], r['comp']['gx'])          # the site masks for itself


@pytest.mark.parametrize('shape', SHAPES)
def test_a3_masking_epilogue_and_its_maximum(shape):
    r = _results(shape)
    want = r['comp']['gx'] * (r['t']['x'] > 0).to(torch.float32)
    got, site = r['msk']['gx'], r['msk']['in_site']
    assert torch.equal(got, want)
    assert float((want != r['comp']['gx']).sum()) > 0            # the mask removed something
    assert r['msk']['site_saw_gx'] and site.amax is not None
    assert float(site.amax) == float(want.abs().max()) == r['msk']['gx_amax']
    # without a mask the scalar is max|gx| of the unmasked result
    assert r['pre']['gx_amax'] == float(r['comp']['gx'].abs().max())


def _err(a, b):
    return float((a.double().cpu() - b).abs().max() / b.abs().max())


@pytest.mark.parametrize('shape', SHAPES)
def test_a4_parameter_gradients_against_float64(shape):
    r = _results(shape)
    failed = []
    for k in ('gw', 'ggamma', 'gbeta'):
        e_site, e_comp = _err(r['pre'][k], r['ref'][k]), _err(r['comp'][k], r['ref'][k])
        print('%s %s: site %.3e, composition %.3e of max against float64' % (shape, k, e_site, e_comp))
        log_measured('test_42_a4_%s_%s_site' % ('x'.join(map(str, shape)), k), e_site, 2.0 * e_comp)
        log_measured('test_42_a4_%s_%s_composition' % ('x'.join(map(str, shape)), k), e_comp, None)
        if not e_site <= 2.0 * e_comp:
            failed.append('%s: site %.3e > 2 x composition %.3e' % (k, e_site, e_comp))
        # the same bits however the mask was obtained
        assert torch.equal(r['pre'][k], r['own'][k]), k
    assert not failed, failed


@pytest.mark.parametrize('shape', SHAPES)
def test_a5_backward_is_deterministic(shape):
    r = _results(shape)
    for k in ('gx', 'gw', 'ggamma', 'gbeta'):
        assert torch.equal(r['pre'][k], r['again'][k]), k
