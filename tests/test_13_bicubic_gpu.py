"""csrc/bicubic.hip (ops.bicubic_resize): the bicubic resize with which MidasNet works at a resolution of its own, forward,
normalising forward and backward, against torch's CPU F.interpolate(mode='bicubic', align_corners=True) in float64 and its
autograd gradient.

Tolerances are not fitted to the kernels: for every case torch's own CPU fp32 result is compared with the float64 one, and
the kernels may be off by four times that (a different but fixed summation order) plus one fp32 ulp of the largest reference
magnitude (cases torch happens to compute exactly, such as the identity).  Every measured value is logged next to its bound
(helpers.log_measured).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers

pytestmark = pytest.mark.gpu

# (N, C, H_in, W_in, H_out, W_out)
CASES = [(2, 3, 20, 36, 32, 64),        # upscaling
         (2, 3, 32, 64, 20, 36),        # downscaling
         (1, 1, 5, 7, 5, 7),            # identity: exact copy and exact gradient
         (2, 3, 1, 9, 4, 3),            # size-1 input dimension
         (2, 3, 6, 1, 3, 8),            # size-1 input dimension
         (2, 3, 7, 5, 1, 1),            # out == 1: scale 0
         (1, 1, 9, 70, 33, 130)]        # outputs cross a wavefront row and a block tile in both directions
IDS = ['%dx%d_%dx%d_to_%dx%d' % c for c in CASES]
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def _interp(x, size):
    return F.interpolate(x, size=size, mode='bicubic', align_corners=True)


_REF = {}


def _reference(case, normalise):
    """float64 forward and gradient for a random gy (computed once per case, shared, never modified), and the error of torch's
    own CPU fp32 arithmetic against them."""
    key = (case, normalise)
    if key in _REF:
        return _REF[key]
    N, C, H, W, Ho, Wo = case
    if normalise:
        C = 3                            # channels = 3 on every shape: c = plane % 3
    g = torch.Generator().manual_seed(1000 + CASES.index(case))
    x = torch.randn(N, C, H, W, generator=g)
    gy = torch.randn(N, C, Ho, Wo, generator=g)
    mean, std = torch.tensor(MEAN[:C]), torch.tensor(STD[:C])

    def run(dtype):
        xin = x.to(dtype).clone().requires_grad_(True)
        z = xin
        if normalise:
            z = (z - mean.to(dtype).view(1, C, 1, 1)) / std.to(dtype).view(1, C, 1, 1)
        y = _interp(z, (Ho, Wo))
        gx, = torch.autograd.grad(y, xin, gy.to(dtype))
        return y.detach(), gx
    y64, gx64 = run(torch.float64)
    y32, gx32 = run(torch.float32)

    def bound(a32, a64):
        own = float((a32.double() - a64).abs().max())
        return 4.0 * own + float(np.spacing(np.float32(a64.abs().max())))
    _REF[key] = dict(x=x, gy=gy, mean=mean, std=std, y=y64, gx=gx64, y_bound=bound(y32, y64), gx_bound=bound(gx32, gx64))
    return _REF[key]


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_forward_and_backward_match_float64(case):
    from dvd_hip import ops
    r = _reference(case, False)
    x = r['x'].cuda().requires_grad_(True)
    y = ops.bicubic_resize(x, case[4:])
    gx, = torch.autograd.grad(y, x, r['gy'].cuda())
    ey = float((y.detach().cpu().double() - r['y']).abs().max())
    eg = float((gx.cpu().double() - r['gx']).abs().max())
    helpers.log_measured('bicubic_fwd/' + IDS[CASES.index(case)], ey, r['y_bound'])
    helpers.log_measured('bicubic_bwd/' + IDS[CASES.index(case)], eg, r['gx_bound'])
    print('forward %.3e (bound %.3e), backward %.3e (bound %.3e)' % (ey, r['y_bound'], eg, r['gx_bound']))
    assert y.shape == r['y'].shape and gx.shape == r['x'].shape
    assert ey <= r['y_bound']
    assert eg <= r['gx_bound']
    if case[2:4] == case[4:]:            # identity: a copy, bit for bit, in both directions
        assert torch.equal(y.detach().cpu(), r['x']) and torch.equal(gx.cpu(), r['gy'])


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_normalising_forward_matches_float64(case):
    """mean / std set: (x - mean[c]) / std[c] on every tap, c = plane % channels, then the resize -- MidasNet's input side."""
    from dvd_hip import ops
    r = _reference(case, True)
    y = ops.bicubic_resize(r['x'].cuda(), case[4:], r['mean'].cuda(), r['std'].cuda())
    ey = float((y.cpu().double() - r['y']).abs().max())
    helpers.log_measured('bicubic_fwd_norm/' + IDS[CASES.index(case)], ey, r['y_bound'])
    print('normalising forward %.3e (bound %.3e)' % (ey, r['y_bound']))
    assert ey <= r['y_bound']


def test_normalising_form_has_no_backward_and_cpu_tensors_are_refused():
    from dvd_hip import ops
    x = torch.rand(1, 3, 8, 8, device='cuda', requires_grad=True)
    m, s = torch.tensor(MEAN, device='cuda'), torch.tensor(STD, device='cuda')
    with pytest.raises(RuntimeError, match='no backward'):
        ops.bicubic_resize(x, (4, 4), m, s)
    with pytest.raises(RuntimeError, match='go together'):
        ops.bicubic_resize(x.detach(), (4, 4), m, None)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.bicubic_resize(torch.rand(1, 3, 8, 8), (4, 4))
    with pytest.raises(RuntimeError, match='float32'):
        ops.bicubic_resize(x.detach().half(), (4, 4))


@pytest.mark.parametrize('case', CASES[:2], ids=IDS[:2])
def test_backward_is_the_adjoint_of_the_forward(case):
    """<A x, y> == <x, A^T y>, both sides summed in float64 from the kernels' fp32 results.  Bound: an element of A x is two
    stages of four products and three additions (<= 16 roundings of terms no larger than sum|w| max|x|, sum|w| <= 1.3 per axis,
    1.7 in two dimensions); an element of A^T y is two chains of at most 16 sequential additions over such terms.  Either side
    is therefore within (16 + 32) * 1.7 * eps * max|x| * sum|y| of the exact bilinear form; a tap credited to the wrong
    column (the border clamp) would be O(sqrt(rows)) times max|x| max|y|."""
    from dvd_hip import ops
    r = _reference(case, False)
    x = r['x'].cuda().requires_grad_(True)
    gy = r['gy'].cuda()
    y = ops.bicubic_resize(x, case[4:])
    gx, = torch.autograd.grad(y, x, gy)
    lhs = float((y.detach().double() * gy.double()).sum())
    rhs = float((x.detach().double() * gx.double()).sum())
    tol = 48 * 1.7 * float(np.finfo(np.float32).eps) * float(r['x'].abs().max()) * float(r['gy'].abs().sum())
    helpers.log_measured('bicubic_adjoint/' + IDS[CASES.index(case)], abs(lhs - rhs), tol)
    print('<Ax,y> %.9g  <x,A^T y> %.9g  diff %.3e (bound %.3e)' % (lhs, rhs, abs(lhs - rhs), tol))
    assert abs(lhs - rhs) <= tol


@pytest.mark.parametrize('case', [CASES[0], CASES[1], CASES[6]], ids=[IDS[0], IDS[1], IDS[6]])
def test_backward_is_reproducible_and_capturable(case):
    """No atomics: two backward calls are bit-identical; forward + backward captured in ONE graph and replayed twice with
    refilled static inputs equal eager execution bit for bit (no host-side state, no allocation outside the graph's pool)."""
    from dvd_hip import ops
    N, C, H, W, Ho, Wo = case
    g = torch.Generator().manual_seed(77)
    xs = [torch.randn(N, C, H, W, generator=g).cuda() for _ in range(2)]
    gys = [torch.randn(N, C, Ho, Wo, generator=g).cuda() for _ in range(2)]

    def eager(x, gy):
        x = x.clone().requires_grad_(True)
        y = ops.bicubic_resize(x, (Ho, Wo))
        gx, = torch.autograd.grad(y, x, gy)
        return y.detach(), gx
    want = [eager(x, gy) for x, gy in zip(xs, gys)]
    again = eager(xs[0], gys[0])
    assert torch.equal(again[0], want[0][0]) and torch.equal(again[1], want[0][1])

    sx = xs[0].clone().requires_grad_(True)
    sgy = gys[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.autograd.grad(ops.bicubic_resize(sx, (Ho, Wo)), sx, sgy)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sy = ops.bicubic_resize(sx, (Ho, Wo))
        sgx, = torch.autograd.grad(sy, sx, sgy)
    for i in (1, 0):
        with torch.no_grad():
            sx.copy_(xs[i])
            sgy.copy_(gys[i])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(sy.detach(), want[i][0]) and torch.equal(sgx, want[i][1])


def test_bytes_are_counted_under_the_upsample_classes():
    from dvd_hip import ops
    N, C, H, W, Ho, Wo = CASES[0]
    x = torch.randn(N, C, H, W, device='cuda', requires_grad=True)
    before = ops.flop_counters()
    y = ops.bicubic_resize(x, (Ho, Wo))
    torch.autograd.grad(y, x, torch.ones_like(y))
    since = ops.flops_since(before)
    nbytes = 4.0 * N * C * (H * W + Ho * Wo)
    assert since['upsample_fwd'] == nbytes and since['upsample_bwd'] == nbytes
    assert all(v == 0.0 for k, v in since.items() if k not in ('upsample_fwd', 'upsample_bwd'))


# -- MidasNet(resize=...) ------------------------------------------------------------------------------------------------------
def _midas(resize):
    from dvd_hip.third_party.MiDaS import MidasNet
    net = helpers.seeded_fill_(MidasNet(non_negative=True, normalize_input=True, resize=resize), 211)
    with torch.no_grad():        # calibrated head (as the full-step fixtures): depth of O(5) instead of the random-init 3e5
        net.scratch.output_conv[4].weight.mul_(30.0)
        net.scratch.output_conv[4].bias.fill_(2000.0)
    return net.eval()


def _run(net, x, gd):
    net.zero_grad()
    d = net(x)
    d.backward(gd)
    return d.detach(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


def test_midasnet_with_a_working_resolution_matches_its_cpu_branch():
    """MidasNet(resize=[64, 96]) on a 1x3x48x80 image: the GPU path (normalising bicubic resize in, plain bicubic resize out,
    no F.interpolate) against the same module on CPU tensors, which runs the reference's ATen ops.  Bounds: those
    tests/test_30_full_step_gpu.py applies to its MiDaS case at this working size (fullstep_midas_b1_64x96_train: per-parameter
    gradient norms 8e-3 relative) and, for the depth map element by element, the tighter of its two element-wise bounds (8e-3 of
    the largest magnitude).  Two GPU runs give bit-identical depth-net gradients."""
    import copy
    from torch.profiler import ProfilerActivity, profile
    cpu = _midas([64, 96])
    gpu = copy.deepcopy(cpu).cuda()
    g = torch.Generator().manual_seed(5)
    x = torch.rand(1, 3, 48, 80, generator=g)
    gd = torch.randn(1, 1, 48, 80, generator=g) * 1e-3
    d_ref, g_ref = _run(cpu, x, gd)
    d, grads = _run(gpu, x.cuda(), gd.cuda())
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        d2, grads2 = _run(gpu, x.cuda(), gd.cuda())
    names = {e.key for e in prof.key_averages()}
    assert not [n for n in names if 'upsample_bicubic' in n], names          # no F.interpolate on the GPU path
    assert d.shape == (1, 1, 48, 80)
    assert torch.equal(d, d2) and sorted(grads) == sorted(grads2) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    d_err = float((d.cpu() - d_ref).abs().max() / d_ref.abs().max())
    worst, worst_k = 0.0, None
    for k, want in g_ref.items():
        a, b = float(grads[k].double().norm()), float(want.double().norm())
        if b == 0.0:
            continue
        if abs(a - b) / b > worst:
            worst, worst_k = abs(a - b) / b, k
    helpers.log_measured('midas_resize_module/depth_rel', d_err, 8e-3)
    helpers.log_measured('midas_resize_module/grad_norm_worst_rel', worst, 8e-3)
    print('depth %.3e of max, worst gradient norm %.3e (%s)' % (d_err, worst, worst_k))
    assert sorted(grads) == sorted(g_ref)
    assert d_err <= 8e-3
    assert worst <= 8e-3
