"""The nine ResNeXt `conv2` + BatchNorm + ReLU layers that the xconv family's stride-1 kernels do not cover, as fused sites inside
whole bottleneck blocks (third_party/MiDaS.py `_Bottleneck`, conv.conv_bn_act -> conv._conv2_site_kind): stage 1 (8 per group,
csrc/gconv.hip), stage 2 stride 1 (16 per group, groups paired on the grouped xconv kernels) and the stride-2 entries.

  * every parameter and input gradient against the float64 CPU module, with the tolerances of tests/test_09_fused_joins_gpu.py
    (2e-5 of max|.|, 1e-4 for 4-D weights: the convolution bounds of tests/test_06_xconv_gpu.py over a block's three convolutions);
  * the byte counters of the stand-alone BatchNorm kernels over the block's forward + backward: `bnrelu_fwd` moves nothing;
    `bnrelu_bwd` moves the block's outer site (bn3 masks for itself here: nothing consumes the block's output -- gy, y read and g
    written, 12 B per output element) plus, per inner site, at most a per-channel-sum pass (4 B per element) where the weight
    gradient kernel of that shape does not deliver the sums;
  * both inner sites find their mask pre-applied;
  * a captured HIP graph of the block follows gamma and the convolution weight changed in place between replays (the paired
    16-per-group weight is derived per call: its packings are launches of the graph)."""
import copy

import pytest
import torch

from helpers import seeded_fill_

pytestmark = pytest.mark.gpu

CONFIGS = [(256, 64, 1, False),      # stage 1: 8 per group
           (512, 128, 1, False),     # stage 2, stride 1: 16 per group
           (256, 128, 2, True),      # stage 2 entry: 16 per group, stride 2
           (512, 256, 2, True)]      # stage 3 entry: 32 per group, stride 2


def _block(c_in, planes, stride, down):
    from dvd_hip.third_party.MiDaS import _Bottleneck
    blk = seeded_fill_(_Bottleneck(c_in, planes, stride, 32, 8, down), 3).eval()
    g = torch.Generator().manual_seed(c_in + planes + stride)
    x = torch.randn(2, c_in, 12, 20, generator=g).relu()
    gy = torch.randn(2, planes * 4, 12 // stride, 20 // stride, generator=g)
    return blk, x, gy


def _grads(m, x, gy):
    xx = x.clone().requires_grad_(True)
    y = m(xx * 1.0)
    y.backward(gy)
    out = {'y': y.detach().double().cpu(), 'gx': xx.grad.double().cpu()}
    for k, p in m.named_parameters():
        out['g_' + k] = p.grad.double().cpu()
    return out


@pytest.mark.parametrize('c_in,planes,stride,down', CONFIGS)
def test_block_gradients_bytes_and_sites(c_in, planes, stride, down):
    from dvd_hip import conv as C, ops
    blk, x, gy = _block(c_in, planes, stride, down)
    want = _grads(copy.deepcopy(blk).double(), x.double(), gy.double())
    m = copy.deepcopy(blk).cuda()
    for k in C.STATS:
        C.STATS[k] = 0
    before = ops.flop_counters()
    got = _grads(m, x.cuda(), gy.cuda())
    after = ops.flop_counters()
    for k in want:
        err = float((got[k] - want[k]).abs().max() / max(float(want[k].abs().max()), 1e-30))
        tol = 1e-4 if (k.startswith('g_') and k.endswith('weight') and want[k].dim() == 4) else 2e-5
        assert err < tol, '%s: %.2e of max against float64' % (k, err)
    assert C.STATS['sites_premasked'] == 2 and C.STATS['sites_masked'] == 1, C.STATS
    assert after['bnrelu_fwd'] - before['bnrelu_fwd'] == 0.0
    width = planes * 2
    inner = max(2 * width * 12 * 20, 2 * width * (12 // stride) * (20 // stride))       # elements of the largest inner tensor
    outer = 12.0 * gy.numel()
    moved = after['bnrelu_bwd'] - before['bnrelu_bwd']
    # sum passes only: one 4-byte read of a tensor per inner site at most (none where the weight gradient kernel sums)
    assert moved - outer <= 2 * 4.0 * inner, (moved, outer, inner)


@pytest.mark.parametrize('c_in,planes,stride,down', CONFIGS)
def test_captured_block_follows_its_parameters(c_in, planes, stride, down):
    from dvd_hip import conv as C, ops
    blk, x, gy = _block(c_in, planes, stride, down)
    m = blk.cuda()
    params = list(m.parameters())
    x, gy = x.cuda(), gy.cuda()

    def run(xv):
        y = m(xv * 1.0)
        y.backward(gy)
        return y

    def change(scale):
        with torch.no_grad():
            m.bn2.weight.mul_(scale)
            m.bn2.weight[1::2].neg_()
            m.conv2.weight.mul_(scale)
            m.conv2.weight[::3].neg_()

    def eager():
        for p in params:
            p.grad = None
        xe = x.clone().requires_grad_(True)
        y = run(xe)
        return [y.detach().clone(), xe.grad.clone()] + [p.grad.clone() for p in params]

    # eager references for both parameter sets first (they are also the warm-up passes), then back to the first set
    saved = [p.detach().clone() for p in params]
    want0 = eager()
    change(1.25)
    want1 = eager()
    with torch.no_grad():
        for p, s in zip(params, saved):
            p.copy_(s)
    for p in params:
        p.grad = None
    x_static = x.clone().requires_grad_(True)
    torch.cuda.synchronize()
    C.PACK_PLAN.extend()
    ops.begin_capture()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        y_static = run(x_static)
    static = [y_static.detach(), x_static.grad] + [p.grad for p in params]
    for want, scale in ((want0, None), (want1, 1.25)):
        if scale is not None:
            change(scale)
        C.PACK_PLAN.ensure_current()
        graph.replay()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(static, want)):
            assert torch.equal(a, b), 'replay %s: result %d differs from the eager run' % ('after the change' if scale else 'as captured', i)
    assert not torch.equal(want0[0], want1[0])
    for p in params:
        p.grad = None
