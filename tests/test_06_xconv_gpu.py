"""Dense convolutions on the split-operand MFMA kernels (csrc/xconv.hip, csrc/xwgrad3.hip) against F.conv2d on the
CPU in float64 (the reference's nn.Conv2d arithmetic, third_party/midas_blocks.py:102-168, MiDaS.py:186-195,
hourglass.py:21-57).

Tolerance: fp32 class.  Every operand is scaled by a power of two and split into two fp16 terms (22 bits), a product is
three partial products with fp32 accumulation (csrc/dvd_split.h; round 2: three bf16 terms / six products), so the error
against the float64 result must be of the size of an fp32 convolution's own rounding error:
  * max |err| <= 4e-6 * max |y| on zero-mean data (an fp32 CPU convolution of the same data measures 1-2e-6 on these
    shapes; a plain fp16 / bf16 product would be 5e-4 / 4e-3), weight gradients 2e-5 (K = N*H*W up to 4e4 terms);
  * ELEMENT-WISE relative error on a well-conditioned case (all operands positive: no cancellation, every output is
    as large as the sum of its terms' magnitudes) <= 4e-6: measured on MI355X 2.1e-6 for sums of 2 304 products (432
    sequential fp32 accumulations of a growing positive sum -- a sequential fp32 multiply-add chain over the same data
    measures 1.4e-6, the CPU's blocked fp32 convolution 3.3e-7), 2.5e-7 .. 9.6e-7 for every other case
    (test_elementwise_relative_error_without_cancellation; values in profiles/r03_parity_measured.jsonl)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 4e-6


def _ref(x, w, b, relu_in=False, res=None, res_relu=False):
    xd = x.double()
    if relu_in:
        xd = xd.relu()
    y = F.conv2d(xd, w.double(), None if b is None else b.double(), padding=w.shape[-1] // 2)
    if res is not None:
        y = y + (res.double().relu() if res_relu else res.double())
    return y


def _err(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


def _where(got, want, names):
    d = (got.double().cpu() - want).abs()
    i = np.unravel_index(int(d.argmax()), d.shape)
    bad = (d > TOL * float(want.abs().max())).sum().item()
    return 'worst at %s=%s, %d of %d elements off' % (names, tuple(int(v) for v in i), bad, d.numel())


def test_identity_weights_copy_the_input():
    """W = centre-tap identity: the output IS the input to the 22 bits one product carries (two fp16 terms per operand,
    csrc/dvd_split.h: |err| <= 2^-22 |x|) -- isolates the staging layout and the output mapping."""
    from dvd_hip import conv as C
    torch.manual_seed(0)
    for KS in (1, 3):
        for (N, Cc, H, W) in ((1, 32, 7, 40), (2, 160, 13, 21)):
            x = torch.randn(N, Cc, H, W)
            conv = torch.nn.Conv2d(Cc, Cc, KS, padding=KS // 2, bias=False)
            with torch.no_grad():
                conv.weight.zero_()
                conv.weight[torch.arange(Cc), torch.arange(Cc), KS // 2, KS // 2] = 1.0
            conv = conv.cuda()
            y = C.xconv2d(conv, x.cuda())
            assert _err(y, x.double()) < 2.5e-7, 'KS=%d %s: %s' % (KS, (N, Cc, H, W), _where(y, x.double(), 'n,c,y,x'))


@pytest.mark.parametrize('tap', [0, 2, 4, 6, 8])
def test_single_tap_shifts_the_input(tap):
    """Only one tap non-zero: the output is the input shifted by that tap (zero padded) -- isolates the tap offsets."""
    from dvd_hip import conv as C
    torch.manual_seed(1)
    N, Cc, H, W = 1, 32, 9, 37
    x = torch.randn(N, Cc, H, W)
    conv = torch.nn.Conv2d(Cc, Cc, 3, padding=1, bias=False)
    with torch.no_grad():
        conv.weight.zero_()
        conv.weight[torch.arange(Cc), torch.arange(Cc), tap // 3, tap % 3] = 1.0
    want = _ref(x, conv.weight.detach(), None)
    y = C.xconv2d(conv.cuda(), x.cuda())
    assert _err(y, want) < 2.5e-7, _where(y, want, 'n,c,y,x')


CASES = [
    # N, Cin, Cout, H, W, KS
    (2, 256, 256, 24, 42, 3),        # the MiDaS decoder convolution (refinenet3 level)
    (1, 256, 256, 48, 84, 3),
    (2, 64, 256, 24, 42, 1),         # ResNeXt bottleneck 1x1
    (1, 1024, 256, 12, 21, 3),       # scratch.layer3_rn
    (1, 256, 128, 20, 36, 3),        # output_conv[0]
    (1, 128, 32, 30, 70, 3),         # output_conv[2]: 32 output channels
    (1, 32, 1, 17, 29, 1),           # output_conv[4]: one output channel
    (2, 20, 40, 11, 19, 3),          # channel counts that are multiples of nothing
    (1, 48, 64, 19, 23, 5),          # hourglass inception branches
    (1, 32, 32, 21, 33, 7),
    (1, 32, 32, 24, 40, 11),
    (1, 3, 64, 16, 24, 7),           # 3 input channels
    (1, 512, 512, 13, 22, 1),        # >= 256 output channels: the 256-channel block shapes (1x1: 256 x 128 positions)
    (1, 256, 512, 10, 15, 3),        # (k >= 3: 256 x 256 positions, one 512-thread block per CU)
    (2, 272, 288, 9, 14, 3),         # 256-channel blocks with a ragged last block, Cin a multiple of 16 only
    (2, 256, 320, 12, 20, 1),        # 1x1 weight gradient on 256 x 256-channel workgroups (H * W a multiple of 4), ragged
    (3, 512, 256, 8, 18, 1),         # ... two input-channel blocks, 9 chunks per image
    (1, 64, 256, 11, 17, 5),         # 256-row block shape with the direct activation staging of the large kernels (k >= 5)
    (1, 256, 64, 10, 13, 7),         # ... reached by the backward-data pass (M = Cin = 256): hourglass 7x7 / 11x11 branches
    (1, 256, 32, 9, 12, 11),
    (1, 16, 256, 7, 9, 3),           # a single 16-channel chunk: the pipeline's prologue covers the whole K loop of a tap row
    (1, 32, 256, 6, 10, 1),          # 1x1 with two K steps only
    (2, 256, 256, 96, 128, 1),       # wide 1x1 weight gradient with six 16-pixel chunks per workgroup (its chunk pipeline in steady state)
]


@pytest.mark.parametrize('N,Cin,Cout,H,W,KS', CASES)
def test_forward_and_input_gradient(N, Cin, Cout, H, W, KS):
    from dvd_hip import conv as C
    torch.manual_seed(Cin + Cout + KS)
    x = torch.randn(N, Cin, H, W)
    conv = torch.nn.Conv2d(Cin, Cout, KS, padding=KS // 2, bias=True)
    want = _ref(x, conv.weight.detach(), conv.bias.detach())
    xg = x.cuda().requires_grad_(True)
    cg = torch.nn.Conv2d(Cin, Cout, KS, padding=KS // 2, bias=True).cuda()
    cg.load_state_dict(conv.state_dict())
    y = C.xconv2d(cg, xg)
    e = _err(y.detach(), want)
    e32 = _err(conv(x).detach(), want)
    print('fwd err %.2e of max|y| (fp32 CPU conv: %.2e)' % (e, e32))
    assert e < TOL, _where(y.detach(), want, 'n,co,y,x')
    # backward: input gradient, weight gradient, bias gradient against float64 autograd
    gy = torch.randn(N, Cout, H, W)
    xd = x.double().requires_grad_(True)
    wd = conv.weight.detach().double().requires_grad_(True)
    bd = conv.bias.detach().double().requires_grad_(True)
    F.conv2d(xd, wd, bd, padding=KS // 2).backward(gy.double())
    y.backward(gy.cuda())
    e = _err(xg.grad, xd.grad)
    print('dgrad err %.2e' % e)
    assert e < TOL, 'dgrad: ' + _where(xg.grad, xd.grad, 'n,ci,y,x')
    e = _err(cg.weight.grad, wd.grad)
    print('wgrad err %.2e' % e)
    assert e < 2e-5, 'wgrad: ' + _where(cg.weight.grad, wd.grad, 'co,ci,ky,kx')
    assert _err(cg.bias.grad, bd.grad) < 1e-5


@pytest.mark.parametrize('N,Cin,Cout,H,W,KS', [(2, 256, 256, 24, 40, 3), (2, 512, 256, 16, 24, 1), (1, 64, 32, 20, 36, 3)])
def test_elementwise_relative_error_without_cancellation(N, Cin, Cout, H, W, KS):
    """All inputs, weights and output gradients in [0.5, 1.5]: nothing cancels, so max |err| / |y| PER ELEMENT measures the
    arithmetic itself (22-bit operands, dropped low x low partial product, fp32 accumulation) and not the conditioning of
    the data.  Bound 4e-6 = 2x the worst value measured on MI355X (2.1e-6, forward of the 3x3 256 -> 256 case: 2 304 products
    = 432 sequential fp32 accumulations of a growing positive sum, the worst case for accumulation rounding; a sequential fp32
    multiply-add chain over such data measures 1.4e-6, tests/test_split_bf16_cpu.py); every other row measures below 1e-6.
    The fp32 CPU convolution's own element-wise error (blocked summation: 3e-7) is printed beside it."""
    from dvd_hip import conv as C
    from helpers import log_measured
    g = torch.Generator().manual_seed(7 * Cin + KS)
    x = torch.rand(N, Cin, H, W, generator=g) + 0.5
    conv = torch.nn.Conv2d(Cin, Cout, KS, padding=KS // 2, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.rand(conv.weight.shape, generator=g) + 0.5)
    gy = torch.rand(N, Cout, H, W, generator=g) + 0.5
    xd = x.double().requires_grad_(True)
    wd = conv.weight.detach().double().requires_grad_(True)
    yd = F.conv2d(xd, wd, None, padding=KS // 2)
    yd.backward(gy.double())
    x32 = x.clone().requires_grad_(True)
    y32 = conv(x32)
    y32.backward(gy)
    xg = x.cuda().requires_grad_(True)
    cg = torch.nn.Conv2d(Cin, Cout, KS, padding=KS // 2, bias=False).cuda()
    cg.load_state_dict(conv.state_dict())
    y = C.xconv2d(cg, xg)
    y.backward(gy.cuda())

    def rel(got, want):
        return float(((got.double().cpu() - want).abs() / want.abs()).max())
    rows = {'fwd': (rel(y.detach(), yd.detach()), rel(y32.detach(), yd.detach())),
            'dgrad': (rel(xg.grad, xd.grad), rel(x32.grad, xd.grad)),
            'wgrad': (rel(cg.weight.grad, wd.grad), rel(conv.weight.grad, wd.grad))}
    for k, (e, e32) in rows.items():
        print('%s element-wise rel err %.2e (fp32 CPU convolution: %.2e)' % (k, e, e32))
        log_measured('xconv_elementwise_%s_%dx%dx%d' % (k, Cin, Cout, KS), e, 4e-6)
        assert e < 4e-6, k


@pytest.mark.parametrize('KS', [1, 3])
def test_block_shapes_give_identical_results(KS):
    """dvd_xconv_select: the block shape / addressing mode changes which workgroup computes a product, never the product
    or the order of a pixel's K sum -- outputs are bitwise equal, forward and backward-data, with every epilogue option."""
    from dvd_hip import _lib, conv as C
    torch.manual_seed(40 + KS)
    N, Cin, Cout, H, W = 2, 256, 256, 24, 42
    x, res = torch.randn(N, Cin, H, W).cuda(), torch.randn(N, Cout, H, W).cuda()
    conv = torch.nn.Conv2d(Cin, Cout, KS, padding=KS // 2).cuda()
    gy = torch.randn(N, Cout, H, W).cuda()
    lib = _lib.load()
    outs = []
    try:
        for cfg in (0, 1, 2, 3, 4, 5, 6, 7):     # 6 / 7: the 1x1 kernels without their two-chunk loop / wide epilogue
            _lib.check(lib.dvd_xconv_select(cfg), 'dvd_xconv_select')
            xg = x.clone().requires_grad_(True)
            y = C.xconv2d(conv, xg, relu_in=True, residual=res, res_relu=True)
            y.backward(gy)
            outs.append((y.detach().clone(), xg.grad.clone()))
    finally:
        _lib.check(lib.dvd_xconv_select(0), 'dvd_xconv_select')
    for cfg, (y, gx) in enumerate(outs[1:], start=1):
        assert torch.equal(y, outs[0][0]), 'forward differs for block shape %d' % cfg
        assert torch.equal(gx, outs[0][1]), 'backward-data differs for block shape %d' % cfg


GROUPED = [
    # N, C, groups, H, W, stride
    (2, 2048, 32, 6, 11, 1),         # ResNeXt-101 32x8d stage 4 (64 channels per group)
    (1, 2048, 32, 12, 21, 2),        # its stride-2 entry
    (1, 1024, 32, 13, 23, 2),        # stage 3's stride-2 entry (32 per group), odd image
    (2, 96, 3, 9, 14, 1),            # group counts / sizes that are multiples of nothing much
    (1, 64, 2, 24, 41, 2),           # stride 2 on the strided kernels (round 6): even x odd image, one tile
    (2, 128, 2, 50, 90, 2),          # ... several tiles per image (64 per group: 64-channel blocks), ragged last tile row
    (1, 64, 2, 1, 7, 2),             # ... a one-row image
    (1, 256, 1, 21, 30, 2),          # ... dense: 128-channel blocks, two per image
]


@pytest.mark.parametrize('N,Cc,G,H,W,stride', GROUPED)
def test_grouped_3x3(N, Cc, G, H, W, stride):
    """Grouped 3x3 convolutions of the ResNeXt encoder (torchvision resnet.py Bottleneck.conv2 as MiDaS.py:186-195 runs
    it): forward, input gradient and weight gradient against float64 autograd."""
    from dvd_hip import conv as C
    torch.manual_seed(Cc + G + stride)
    x, conv = torch.randn(N, Cc, H, W), torch.nn.Conv2d(Cc, Cc, 3, stride=stride, padding=1, groups=G, bias=False)
    xd = x.double().requires_grad_(True)
    wd = conv.weight.detach().double().requires_grad_(True)
    want = F.conv2d(xd, wd, None, stride=stride, padding=1, groups=G)
    gy = torch.randn_like(want, dtype=torch.float32)
    want.backward(gy.double())
    cg = C.XConv2d(Cc, Cc, 3, stride=stride, padding=1, groups=G, bias=False).cuda()
    cg.load_state_dict(conv.state_dict())
    xg = x.cuda().requires_grad_(True)
    y = cg(xg)
    assert y.shape == want.shape
    assert _err(y.detach(), want.detach()) < TOL, _where(y.detach(), want.detach(), 'n,co,y,x')
    y.backward(gy.cuda())
    assert _err(xg.grad, xd.grad) < TOL, 'dgrad: ' + _where(xg.grad, xd.grad, 'n,ci,y,x')
    assert _err(cg.weight.grad, wd.grad) < 2e-5, 'wgrad: ' + _where(cg.weight.grad, wd.grad, 'co,ci,ky,kx')


@pytest.mark.parametrize('stride', [1, 2])
def test_sixteen_per_group_module_incl_stride_two(stride):
    """ResNeXt stage 2's 3x3 convolutions (16 channels per group; the first one strided): conv.GroupedConv3x3C16 pairs the
    groups into block-diagonal 32-channel tiles; forward and both gradients against float64 autograd."""
    from dvd_hip import conv as C
    torch.manual_seed(7 + stride)
    N, Cc, H, W = 2, 64, 11, 18
    mod = C.GroupedConv3x3C16(Cc, stride=stride)
    x = torch.randn(N, Cc, H, W)
    xd = x.double().requires_grad_(True)
    wd = mod.weight.detach().double().requires_grad_(True)
    want = F.conv2d(xd, wd, None, stride=stride, padding=1, groups=Cc // 16)
    gy = torch.randn_like(want, dtype=torch.float32)
    want.backward(gy.double())
    mg = mod.cuda()
    xg = x.cuda().requires_grad_(True)
    y = mg(xg)
    assert y.shape == want.shape

    def on_hip_kernel(fn, depth=0):        # the convolution in y's autograd graph is the package's kernel, not ATen's
        if fn is None or depth > 4:
            return False
        return 'XConv' in type(fn).__name__ or any(on_hip_kernel(n, depth + 1) for n, _ in fn.next_functions)
    assert on_hip_kernel(y.grad_fn)
    y.backward(gy.cuda())
    assert _err(y.detach(), want.detach()) < TOL
    assert _err(xg.grad, xd.grad) < TOL
    assert _err(mg.weight.grad, wd.grad) < 2e-5


def test_stride_two_is_the_subsampled_stride_one_result():
    """The strided kernels (csrc/xconv.hip XArgs::S2 / ZI, conv._XConv with stride=2) against rounds 2-5's form of the same convolution:
    the stride-1 kernel's output sub-sampled, the gradient zero-interleaved in HBM.  Same products, same split operands (the
    tensor-wide scales are shared), another accumulation order per output: 2e-6 of the largest element; the module with a
    bias, in front of a BatchNorm+ReLU site's input (the mask hand-over of conv._Site)."""
    from dvd_hip import conv as C
    torch.manual_seed(5)
    N, Cc, G, H, W = 2, 128, 4, 26, 45
    mod = C.XConv2d(Cc, Cc, 3, stride=2, padding=1, groups=G, bias=True).cuda()
    x = torch.randn(N, Cc, H, W, device='cuda')
    gy = torch.randn(N, Cc, (H + 1) // 2, (W + 1) // 2, device='cuda')
    outs = []
    for off in (False, True):
        C.AB['no_s2'] = off
        try:
            xg = x.clone().requires_grad_(True)
            mod.zero_grad()
            y = mod(xg)
            names = set()

            def walk(fn, depth=0):
                if fn is None or depth > 4:
                    return
                names.add(type(fn).__name__)
                for n, _ in fn.next_functions:
                    walk(n, depth + 1)
            walk(y.grad_fn)
            # native: the strided kernel's own output; DVD_AB=no_s2: the stride-1 kernel's through _Subsample2
            assert C.xconv_s2_supported(mod, xg) == (not off)
            assert (type(y.grad_fn).__name__ == '_XConvBackward') == (not off) and any('Subsample2' in n for n in names) == off, names
            y.backward(gy)
            outs.append((y.detach().clone(), xg.grad.clone(), mod.weight.grad.clone(), mod.bias.grad.clone()))
        finally:
            C.AB['no_s2'] = False
    for name, a, b in zip(('y', 'gx', 'gw', 'gb'), outs[0], outs[1]):
        e = float((a - b).abs().max() / b.abs().max())
        print('%s: native vs sub-sampled stride 1: %.2e of max' % (name, e))
        assert e < 2e-6, name


def test_fused_input_relu_residual_and_its_backward():
    """ResidualConvUnit pieces (midas_blocks.py:121-135): conv(relu(x)) + relu(res), gradient masks included."""
    from dvd_hip import conv as C
    torch.manual_seed(5)
    N, Cc, H, W = 2, 64, 10, 18
    x, res, gy = torch.randn(N, Cc, H, W), torch.randn(N, Cc, H, W), torch.randn(N, Cc, H, W)
    conv = torch.nn.Conv2d(Cc, Cc, 3, padding=1)
    xd, rd = x.double().requires_grad_(True), res.double().requires_grad_(True)
    wd = conv.weight.detach().double().requires_grad_(True)
    want = F.conv2d(xd.relu(), wd, conv.bias.detach().double(), padding=1) + rd.relu()
    want.backward(gy.double())
    xg, rg = x.cuda().requires_grad_(True), res.cuda().requires_grad_(True)
    cg = conv.cuda()
    y = C.xconv2d(cg, xg, relu_in=True, residual=rg, res_relu=True)
    y.backward(gy.cuda())
    assert _err(y.detach(), want.detach()) < TOL
    assert _err(xg.grad, xd.grad) < TOL and _err(rg.grad, rd.grad) < 1e-7
    assert _err(cg.weight.grad, wd.grad) < 2e-5


def test_packed_weights_follow_weight_updates():
    from dvd_hip import conv as C, ops
    torch.manual_seed(6)
    conv = torch.nn.Conv2d(32, 32, 3, padding=1, bias=False).cuda()
    x = torch.randn(1, 32, 8, 12).cuda()
    y0 = C.xconv2d(conv, x)
    with torch.no_grad():
        conv.weight.mul_(2.0)                         # autograd-visible update
    assert _err(C.xconv2d(conv, x).detach(), 2 * y0.detach().double().cpu()) < 1e-6
    conv.weight.data.view(-1)[:] = conv.weight.data.view(-1) * 0.5      # update behind autograd's back ...
    ops.WEIGHT_EPOCH[0] += 1                          # ... announced the way the fused Adam step does
    assert _err(C.xconv2d(conv, x).detach(), y0.detach().double().cpu()) < 1e-6


def test_decoder_size_is_deterministic():
    """Same inputs, same bits (no atomics anywhere), at the size of the MiDaS decoder's largest level."""
    from dvd_hip import conv as C
    torch.manual_seed(7)
    conv = torch.nn.Conv2d(256, 256, 3, padding=1).cuda()
    x = torch.randn(2, 256, 96, 168, device='cuda').requires_grad_(True)
    outs = []
    for _ in range(2):
        conv.weight.grad = None
        x.grad = None
        y = C.xconv2d(conv, x)
        y.backward(torch.ones_like(y))
        outs.append((y.detach().clone(), x.grad.clone(), conv.weight.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


BN_CASES = [
    # Cin, Cout, k, groups, stride, affine, conv_bias, residual, relu, H, W
    (64, 256, 1, 1, 1, True, False, True, True, 12, 21),       # bottleneck conv3 + bn3 + skip + ReLU
    (256, 64, 1, 1, 1, True, False, False, True, 12, 21),      # conv1 + bn1 + ReLU
    (128, 128, 3, 4, 1, True, False, False, True, 9, 14),      # grouped conv2 (32 per group) + bn2 + ReLU
    (64, 128, 1, 1, 2, True, False, False, False, 12, 22),     # down-sampling shortcut: strided 1x1 + BN, no ReLU
    (48, 32, 5, 1, 1, False, True, False, True, 11, 13),       # hourglass inception branch: conv bias, BatchNorm2d(affine=False)
]


@pytest.mark.parametrize('Cin,Cout,k,groups,stride,affine,cbias,with_res,relu,H,W', BN_CASES)
def test_convolution_with_fused_batchnorm(Cin, Cout, k, groups, stride, affine, cbias, with_res, relu, H, W):
    """conv -> eval-mode BatchNorm (-> + residual) (-> ReLU) as one launch (conv.conv_bn_act; torchvision Bottleneck as
    third_party/midas_blocks.py:35-50 runs it, hourglass.py:21-57): output and ALL gradients (input, weight, conv bias,
    gamma, beta, residual) against float64 autograd of the unfused ops."""
    from dvd_hip import conv as C
    torch.manual_seed(Cin + Cout + k)
    N = 2
    conv = torch.nn.Conv2d(Cin, Cout, k, stride=stride, padding=0 if stride > 1 else k // 2, groups=groups, bias=cbias)
    bn = torch.nn.BatchNorm2d(Cout, affine=affine).eval()
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.5)
        bn.running_var.uniform_(0.3, 2.0)
        if affine:
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0, 0.3)
    x = torch.randn(N, Cin, H, W)
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    res = torch.randn(N, Cout, Ho, Wo) if with_res else None
    gy = torch.randn(N, Cout, Ho, Wo)
    # float64 reference
    xd = x.double().requires_grad_(True)
    gamma_d = bn.weight.detach().double().requires_grad_(True) if affine else None
    beta_d = bn.bias.detach().double().requires_grad_(True) if affine else None
    wd = conv.weight.detach().double().requires_grad_(True)
    cbd = conv.bias.detach().double().requires_grad_(True) if cbias else None
    z = F.conv2d(xd, wd, cbd, stride=stride, padding=conv.padding, groups=groups)
    yd = F.batch_norm(z, bn.running_mean.double(), bn.running_var.double(), gamma_d, beta_d, False, 0.0, bn.eps)
    rd = res.double().requires_grad_(True) if with_res else None
    if with_res:
        yd = yd + rd
    if relu:
        yd = yd.relu()
    yd.backward(gy.double())
    # fused path
    conv_g = (C.XConv2d(Cin, Cout, k, stride=stride, padding=conv.padding, groups=groups, bias=cbias)).cuda()
    conv_g.load_state_dict(conv.state_dict())
    bn_g = torch.nn.BatchNorm2d(Cout, affine=affine).cuda().eval()
    bn_g.load_state_dict(bn.state_dict())
    xg = x.cuda().requires_grad_(True)
    rg = res.cuda().requires_grad_(True) if with_res else None
    y = C.conv_bn_act(conv_g, bn_g, xg, residual=rg, relu=relu)
    assert y.grad_fn is not None and 'XConvBn' in type(y.grad_fn).__name__, 'the fused path must be taken'
    y.backward(gy.cuda())
    assert _err(y.detach(), yd.detach()) < 2 * TOL, _where(y.detach(), yd.detach(), 'n,c,y,x')
    assert _err(xg.grad, xd.grad) < 2 * TOL, 'dgrad: ' + _where(xg.grad, xd.grad, 'n,c,y,x')
    assert _err(conv_g.weight.grad, wd.grad) < 2e-5, 'wgrad'
    if cbias:
        assert _err(conv_g.bias.grad, cbd.grad) < 2e-5, 'conv bias grad'
    if affine:
        assert _err(bn_g.weight.grad, gamma_d.grad) < 2e-5, 'gamma grad'
        assert _err(bn_g.bias.grad, beta_d.grad) < 2e-5, 'beta grad'
    if with_res:
        assert _err(rg.grad, rd.grad) < 1e-7, 'residual grad'


@pytest.mark.parametrize('ratio', [1e3, 1e5, 1e7])
@pytest.mark.parametrize('KS', [1, 3])
def test_heavy_tailed_operands_dynamic_range(ratio, KS):
    """The split arithmetic scales a whole TENSOR by one power of two taken from max|x| (csrc/dvd_split.h): elements below
    2^-17 of the maximum keep fewer than 22 bits (absolute error <= 2^-38 of the maximum per element).  Gradients behind
    `10000 / clamp(out, 1e-2)` (third_party/MiDaS.py:240-242) are where a few elements can be 1e4 .. 1e6 x the rest, so: 0.01 %
    of the elements of x AND of gy are outliers at `ratio` x the rms; forward, backward-data and the weight gradient (3x3:
    xwgrad3; 1x1: the wide xwgrad1b workgroups) against float64.
    Bound that must hold at every ratio: max |err| <= 4e-6 max|y| (2e-5 for the weight gradient), the fp32-class bound of the
    well-scaled tests -- the outliers dominate max|y|, so this is what the scale is chosen for.
    What degrades, and is only MEASURED and logged (it is the cliff the design states): the error of the
    outputs that no outlier reaches, relative to THEIR largest value -- with the stated per-element bound it may reach
    2^-36 * max|x| * sum|w| / max|y_bulk|, i.e. ~ratio * 1.5e-11 * sqrt(K)."""
    from dvd_hip import conv as C
    from helpers import log_measured
    N, Cin, Cout, H, W = 2, 256, 256, 24, 40
    g = torch.Generator().manual_seed(int(ratio) % 9973 + KS)
    x, gy = torch.randn(N, Cin, H, W, generator=g), torch.randn(N, Cout, H, W, generator=g)
    mx = torch.rand(x.shape, generator=g) < 1e-4
    mg = torch.rand(gy.shape, generator=g) < 1e-4
    x[mx] *= ratio
    gy[mg] *= ratio
    conv = torch.nn.Conv2d(Cin, Cout, KS, padding=KS // 2, bias=False)
    xd = x.double().requires_grad_(True)
    wd = conv.weight.detach().double().requires_grad_(True)
    yd = F.conv2d(xd, wd, None, padding=KS // 2)
    yd.backward(gy.double())
    cg = torch.nn.Conv2d(Cin, Cout, KS, padding=KS // 2, bias=False).cuda()
    cg.load_state_dict(conv.state_dict())
    xg = x.cuda().requires_grad_(True)
    y = C.xconv2d(cg, xg)
    y.backward(gy.cuda())
    # outputs no outlier reaches: dilate the outlier masks by the kernel's support over all channels
    reach_x = F.max_pool2d(mx.any(1, keepdim=True).float(), KS, 1, KS // 2) > 0          # [N,1,H,W]
    reach_g = F.max_pool2d(mg.any(1, keepdim=True).float(), KS, 1, KS // 2) > 0
    for name, got, want, tol, bulk in (('fwd', y.detach(), yd.detach(), TOL, ~reach_x.expand_as(yd)),
                                       ('dgrad', xg.grad, xd.grad, TOL, ~reach_g.expand_as(xd)),
                                       ('wgrad', cg.weight.grad, wd.grad, 2e-5, None)):
        d = (got.double().cpu() - want).abs()
        e = float(d.max() / want.abs().max())
        log_measured('hdr %s ratio %.0e k%d: of max' % (name, ratio, KS), e, tol)
        assert e < tol, (name, e)
        if bulk is not None and bool(bulk.any()):
            eb = float(d[bulk].max() / want[bulk].abs().max())
            log_measured('hdr %s ratio %.0e k%d: bulk outputs, of their own max' % (name, ratio, KS), eb, ratio * 1.5e-11 * (Cin * KS * KS) ** 0.5 + 4e-6)
            print('%s ratio %.0e: %.2e of max, bulk %.2e of bulk max' % (name, ratio, e, eb))
            assert eb < ratio * 1.5e-11 * (Cin * KS * KS) ** 0.5 * 4 + 4e-6, (name, eb)


@pytest.mark.parametrize('N,Cc,H,W', [(5, 7, 9, 11), (48, 64, 12, 20), (3, 300, 8, 8), (1, 2, 1, 3)])
def test_bias_gradient_sums_and_amax_in_one_read(N, Cc, H, W):
    """dvd_chansum: the per-channel sums of gy (a convolution's bias gradient: what autograd's sum over (0, 2, 3) of
    torch.nn.Conv2d(bias=True) gives, third_party/midas_blocks.py:102-168) and max|gy| from the same read.
    Tolerance: fp32 summation of N*H*W terms against float64, 2e-6 of sum|x|; the maximum is exact; bitwise run to run."""
    from dvd_hip import ops
    torch.manual_seed(N * 1000 + Cc)
    x = (torch.randn(N, Cc, H, W) * 3).cuda()
    x[N // 2, Cc // 2, H // 2, W // 2] = -77.5
    got = ops.chansum(x, want_amax=True)
    want = x.double().sum((0, 2, 3)).cpu()
    scale = x.double().abs().sum((0, 2, 3)).cpu()
    assert float(((got.double().cpu() - want).abs() / scale).max()) < 2e-6
    assert float(ops.known_amax(x)) == 77.5
    assert torch.equal(got, ops.chansum(x)), 'summation order depends on scheduling'
    # a 4-byte aligned view (batch slice of odd planes) takes the scalar path
    if N > 1:
        v = x[1:]
        got_v = ops.chansum(v.contiguous() if not v.is_contiguous() else v)
        assert float(((got_v.double().cpu() - v.double().sum((0, 2, 3)).cpu()).abs() / scale).max()) < 2e-6


def test_pack_plan_gives_the_bytes_of_single_packings_and_follows_weight_updates():
    """dvd_xconv_pack_many (conv.PACK_PLAN: every packing of a network in two launches) against dvd_xconv_pack /
    dvd_xconv_pack_scaled tensor by tensor: byte-identical buffers (header maximum included) for dense, grouped, 1x1, 5x5,
    transposed, BatchNorm-scaled and 4-byte-aligned (odd row length: the stem's 27-element rows) weights; an in-place update
    of one weight is picked up by ensure_current() with ONE more launch pair, an unchanged plan launches nothing."""
    from dvd_hip import conv as C
    from dvd_hip import ops
    torch.manual_seed(5)
    plan = C._PackPlan()
    specs = [(64, 64, 3, 1), (256, 64, 1, 1), (48, 32, 5, 1), (64, 64, 3, 2), (32, 3, 3, 1), (40, 24, 1, 1), (128, 128, 3, 4)]
    flat = torch.randn(sum(co * (ci // g) * k * k for co, ci, k, g in specs) + 1, device='cuda')[1:]   # 4-byte aligned views
    weights, o = [], 0
    for co, ci, k, g in specs:
        n = co * (ci // g) * k * k
        weights.append(torch.nn.Parameter(flat[o:o + n].view(co, ci // g, k, k)))
        o += n
    gamma, var = torch.rand(64, device='cuda') + 0.5, torch.rand(64, device='cuda') + 0.1
    for w, (co, ci, k, g) in zip(weights, specs):
        plan.request(w, 'F', g)
        plan.request(w, 'T', g)
    plan.request(weights[0], 'Ts', 1, gamma, var, 1e-5)
    plan.extend()
    assert plan.launches == 1 and len(plan.entries) == 2 * len(specs) + 1

    def same(a, b):
        return torch.equal(a[:4], b[:4]) and torch.equal(a[256:], b[256:])

    def singles():
        out = []
        for w, (co, ci, k, g) in zip(weights, specs):
            for tr in (False, True):
                out.append((w, 'T' if tr else 'F', C.xconv_packed(w, tr, g).clone()))
        out.append((weights[0], 'Ts', C.xconv_packed_scaled(weights[0], 1, gamma, var, 1e-5).clone()))
        return out

    for w, kind, want in singles():
        got = plan.lookup(w, kind, gamma, var, 1e-5) if kind == 'Ts' else plan.lookup(w, kind)
        assert got is not None and same(got, want), (tuple(w.shape), kind)
    plan.ensure_current()
    assert plan.launches == 1
    with torch.no_grad():
        weights[2].mul_(3.0)
        weights[2][0, 0, 0, 0] = 1e3          # a new maximum: another power-of-two scale
    plan.ensure_current()
    assert plan.launches == 2
    for w, kind, want in singles():
        got = plan.lookup(w, kind, gamma, var, 1e-5) if kind == 'Ts' else plan.lookup(w, kind)
        assert same(got, want), (tuple(w.shape), kind)
    ops.WEIGHT_EPOCH[0] += 1                   # the fused Adam's step counter
    plan.ensure_current()
    assert plan.launches == 3
    del weights[:], w, got, want
