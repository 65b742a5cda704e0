"""Dense positions in the k x k tiles of csrc/xconv.hip (csrc/xconv_tile.h): a GEMM column of a block is an OUTPUT of its
tile, (q / TC, q % TC), and reads the LDS cell (q / TC) * P + q % TC of the haloed tile -- the halo columns of a tile row are
no longer computed and dropped.  dvd_xconv_select(8) keeps the earlier mapping (the column is the cell) and its tile choice.

Two properties per case:
  * the mapping changes which lane computes an output, never the products or the order of its K sum: forward and
    backward-data are BITWISE equal between hook 0 and hook 8, with every epilogue option the public path reaches (bias,
    residual with and without ReLU, input ReLU, mask, fused eval BatchNorm, the BatchNorm-scaled backward packing, fp16
    activation storage), and so is the max|y| scalar the epilogue folds;
  * against F.conv2d in float64 on the CPU, which knows neither mapping: the bounds of tests/test_06_xconv_gpu.py,
    4e-6 of max|y| for forward and input gradient, 2e-5 for the weight gradient.

Shapes are the smallest at which the mapping can go wrong: one block with most lanes idle, TR * TC equal to the block's
positions, ragged last tile rows / columns / channel blocks, 128-position blocks, one-row and one-column images, the direct
staging of the wide halos, grouped layers, the stride-2 forward (phase planes, pitch TC + 1) and its backward-data (virtual
zero-interleaved input), and one 1x1 case, whose tile and code path are the same under both hooks."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL, TOL_W = 4e-6, 2e-5

CASES = [
    # N, Cin, Cout, H, W, k, groups, stride
    (2, 32, 32, 5, 7, 3, 1, 1),           # one block, most lanes idle
    (1, 32, 32, 16, 16, 3, 1, 1),         # TR * TC = 256 positions exactly, no idle lane
    (1, 256, 256, 12, 21, 3, 1, 1),       # 252 of 256 positions, the 512-thread shape
    (1, 256, 256, 13, 45, 3, 1, 1),       # ragged last tile row and column
    (2, 272, 288, 9, 14, 3, 1, 1),        # ... and a ragged channel block
    (1, 256, 128, 20, 36, 3, 1, 1),       # 128-position blocks
    (1, 32, 32, 1, 40, 3, 1, 1),          # one-row image
    (1, 32, 32, 40, 1, 3, 1, 1),          # one-column image
    (1, 16, 64, 12, 20, 5, 1, 1),         # wide halos, direct staging
    (1, 32, 32, 9, 12, 11, 1, 1),
    (1, 64, 256, 11, 17, 5, 1, 1),
    (2, 64, 64, 9, 23, 3, 2, 1),          # grouped, 32 per group
    (1, 128, 128, 7, 10, 3, 2, 1),        # grouped, 64 per group
    (1, 64, 64, 10, 14, 3, 2, 2),         # stride 2: S2 forward, ZI backward-data
    (1, 64, 64, 11, 15, 3, 2, 2),         # ... odd image
    (1, 64, 256, 6, 10, 1, 1, 1),         # 1x1: must not change
]


def _err(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


def _make(N, Cin, Cout, H, W, k, groups, stride):
    g = torch.Generator().manual_seed(1000 * Cin + 10 * H + W + k)
    conv = torch.nn.Conv2d(Cin, Cout, k, stride=stride, padding=k // 2, groups=groups, bias=True)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.1)
        conv.bias.copy_(torch.randn(Cout, generator=g))
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    x = torch.randn(N, Cin, H, W, generator=g)
    gy = torch.randn(N, Cout, Ho, Wo, generator=g)
    return conv, x, gy, (Ho, Wo), g


@pytest.mark.parametrize('N,Cin,Cout,H,W,k,groups,stride', CASES)
def test_bitwise_equal_to_haloed_positions(N, Cin, Cout, H, W, k, groups, stride):
    from dvd_hip import _lib, conv as C
    from dvd_hip.ops import amax_of, new_scalar
    conv, x, gy, (Ho, Wo), g = _make(N, Cin, Cout, H, W, k, groups, stride)
    dev = torch.device('cuda')
    conv = conv.to(dev)
    x, gy = x.to(dev), gy.to(dev)
    res = torch.randn(N, Cout, Ho, Wo, generator=g).to(dev)          # forward residual
    galias = torch.randn(N, Cin, H, W, generator=g).to(dev)          # backward: gradient of the input's other consumers
    gamma, beta = (torch.rand(Cout, generator=g) + 0.5).to(dev), torch.randn(Cout, generator=g).to(dev)
    mean, var = torch.randn(Cout, generator=g).to(dev), (torch.rand(Cout, generator=g) + 0.5).to(dev)
    bn = (gamma, beta, mean, var, 1e-5)
    w = conv.weight
    pk, pkT = C.xconv_packed(w, False, groups), C.xconv_packed(w, True, groups)
    pkTs = C.xconv_packed_scaled(w, groups, gamma, var, 1e-5)
    fs = {'stride': 2} if stride == 2 else {}
    bs = {'stride': -2, 'out_hw': (H, W)} if stride == 2 else {}
    strided = stride == 2       # (the public strided path has bias and the fused BatchNorm, no residual or input ReLU)

    def runs(half):
        cast = (lambda t: t.half()) if half else (lambda t: t)
        xx, gg, rr, ga = cast(x), cast(gy), cast(res), cast(galias)
        xa, ga_amax = (None, None) if half else (amax_of(xx), amax_of(gg))
        out = []

        def fwd(name, **kw):
            ya = new_scalar(dev)
            y = C._xconv_run(xx, pk, Cout, k, groups=groups, x_amax=xa, y_amax=ya, **fs, **kw)
            out.append(('fwd ' + name, y, ya))

        def bwd(name, packed=pkT, **kw):
            ya = new_scalar(dev)
            y = C._xconv_run(gg, packed, Cin, k, groups=groups, x_amax=ga_amax, y_amax=ya, **bs, **kw)
            out.append(('bwd ' + name, y, ya))
        fwd('plain')
        fwd('bias', bias=conv.bias)
        fwd('bn relu', bias=conv.bias, bn=bn, relu_out=True)
        if not strided:
            fwd('bias residual', bias=conv.bias, residual=rr)
            fwd('relu_in bias relu(residual)', bias=conv.bias, residual=rr, res_relu=True, relu_in=True)
            fwd('bn residual relu', bn=bn, residual=rr, relu_out=True)
        bwd('plain')
        bwd('mask', mask_src=xx)
        bwd('bn-scaled mask', packed=pkTs, mask_src=xx)
        if not strided:
            bwd('alias mask', mask_src=xx, residual=ga)
        return out

    lib = _lib.load()
    cpg_in, cpg_out = Cin // groups, Cout // groups
    halves = (False, True) if (cpg_in % 16 == 0 and cpg_out % 16 == 0) else (False,)
    got = {}
    try:
        for sel in (0, 8):
            _lib.check(lib.dvd_xconv_select(sel), 'dvd_xconv_select')
            got[sel] = [(half, r) for half in halves for r in runs(half)]
    finally:
        _lib.check(lib.dvd_xconv_select(0), 'dvd_xconv_select')
    torch.cuda.synchronize()
    assert len(got[0]) == len(got[8])
    for (half, (name, y0, a0)), (_, (_, y8, a8)) in zip(got[0], got[8]):
        what = '%s%s' % (name, ' fp16' if half else '')
        assert torch.isfinite(y0.float()).all(), what
        assert torch.equal(y0, y8), '%s: %d of %d outputs differ from the haloed mapping' % (
            what, int((y0 != y8).sum()), y0.numel())
        assert float(a0) == float(a8) and float(a0) > 0.0, '%s: max|y| %r != %r' % (what, float(a0), float(a8))


@pytest.mark.parametrize('N,Cin,Cout,H,W,k,groups,stride', CASES)
def test_against_float64(N, Cin, Cout, H, W, k, groups, stride):
    from dvd_hip import conv as C
    conv, x, gy, _, _ = _make(N, Cin, Cout, H, W, k, groups, stride)
    xd = x.double().requires_grad_(True)
    wd = conv.weight.detach().double().requires_grad_(True)
    yd = F.conv2d(xd, wd, conv.bias.detach().double(), stride=stride, padding=k // 2, groups=groups)
    yd.backward(gy.double())
    cg = conv.cuda()
    xg = x.cuda().requires_grad_(True)
    if stride == 2:
        assert C.xconv_s2_supported(cg, xg)
        y = C._xconv(xg, cg.weight, cg.bias, None, False, False, groups, stride=2)
    else:
        assert C.xconv_supported(cg, xg)
        y = C.xconv2d(cg, xg)
    y.backward(gy.cuda())
    e = _err(y.detach(), yd.detach())
    print('fwd err %.2e of max|y|' % e)
    assert e < TOL, 'forward'
    e = _err(xg.grad, xd.grad)
    print('dgrad err %.2e' % e)
    assert e < TOL, 'input gradient'
    e = _err(cg.weight.grad, wd.grad)
    print('wgrad err %.2e' % e)
    assert e < TOL_W, 'weight gradient'
