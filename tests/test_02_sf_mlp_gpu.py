"""Parity of the fused scene-flow MLP kernels (through the C ABI) with the
golden fixture generated from the real reference network and with the oracle.
Arithmetic: two-term fp16-split MFMA products (three partial products, fp32 accumulation; csrc/sf_mlp.hip, csrc/dvd_split.h) against MKL sgemm on the CPU
(the golden fixture) and against the oracle with its 1x1 convolutions in float64 (the ragged sizes, _oracle_f64).
Tolerances = about 4x the worst value measured on MI355X (round 3, gpurun_out/r03a/parity.jsonl: every gradient tensor
agrees to 2.6e-6 of its largest element, median 2e-7; the values are appended to $DVD_PARITY_LOG on every run):
  forward           rtol 1e-4, atol 2e-6
  d/dx              1e-5 of max|g|   (at most 6 elements = 2 LeakyReLU'-sign-flip pixels beyond it, see _close)
  weight/bias grads 1e-5 of per-tensor max|g|
"""
import numpy as np
import pytest
import torch

from helpers import golden_mlp_sd, load_golden, mlp_oracle_f64, seeded_fill_, t
from oracle import sceneflow_mlp as M

pytestmark = pytest.mark.gpu


def _net_from_sd(sd, time_dependent=True, n_freq_xyz=16, n_freq_t=16):
    from dvd_hip.networks.sceneflow_field import SceneFlowFieldNet
    net = SceneFlowFieldNet(net_width=256, n_layers=4, time_dependent=time_dependent, N_freq_xyz=n_freq_xyz, N_freq_t=n_freq_t)
    missing = net.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return net.cuda()


_oracle_f64 = mlp_oracle_f64       # (tests/helpers.py: shared with tests/test_02b_sf_mlp_geometry_gpu.py)


def _close(got, want, rel, name, max_outliers=0):
    """max |got - want| <= rel * max|want|, except for at most `max_outliers` elements.

    Outliers are legitimate here: LeakyReLU' is discontinuous at 0, so a hidden
    pre-activation within fp32 noise of zero (about one per 2.5e6 units on these
    inputs) can take slope 1 on one device and 0.2 on the other; that perturbs the
    input gradient of that ONE pixel (3 elements) and, through it, every weight
    gradient by a fraction of a percent.  Verified with tests/debug_mlp_err.py."""
    want = np.asarray(want)
    got = np.asarray(got).reshape(want.shape)
    scale = max(np.abs(want).max(), 1e-30)
    err = np.abs(got - want) / scale
    bad = int((err > rel).sum())
    import json
    import os
    if os.environ.get('DVD_PARITY_LOG'):
        with open(os.environ['DVD_PARITY_LOG'], 'a') as f:
            f.write(json.dumps({'test': 'sf_mlp', 'name': name, 'tol': rel, 'worst': float(err.max()),
                                'median': float(np.median(err)), 'outliers': bad}) + '\n')
    if max_outliers < 0:           # only count
        return bad
    assert bad <= max_outliers, '%s: %d elements off by more than %.1e of max|ref| (worst %.3e)' % (
        name, bad, rel, err.max())


def test_state_dict_keys_match_reference():
    gd = load_golden('mlp_b2_8x16')
    from dvd_hip.networks.sceneflow_field import SceneFlowFieldNet
    net = SceneFlowFieldNet(net_width=256, n_layers=4, time_dependent=True, N_freq_xyz=16, N_freq_t=16)
    assert sorted(net.state_dict().keys()) == sorted(k[3:] for k in gd if k.startswith('sd_'))


@pytest.mark.parametrize('name', ['mlp_b2_8x16', 'mlp_b2_8x16_notime', 'mlp_b2_8x16_f4_2'])
def test_module_forward_backward_vs_golden(name):
    """The real reference network's outputs and gradients: the shipped input layer (weights stored in the fixture), the
    reference's default time-independent one and a (4, 2) embedding (weights from helpers.seeded_fill_; the gradients of
    convs.0 and convs.5 element by element, of every parameter by its norm)."""
    gd = load_golden(name)
    if 'geometry' in gd:
        nx, nt, td, seed = (int(v) for v in gd['geometry'])
        from dvd_hip.networks.sceneflow_field import SceneFlowFieldNet
        net = seeded_fill_(SceneFlowFieldNet(net_width=256, n_layers=4, time_dependent=bool(td), N_freq_xyz=nx, N_freq_t=nt),
                           seed).cuda()
    else:
        td, net = 1, _net_from_sd(golden_mlp_sd(gd))
    x = t(gd['in_x']).cuda().requires_grad_(True)
    y = net(x, t(gd['in_t']).cuda() if td else None)
    np.testing.assert_allclose(y.detach().cpu().numpy(), gd['out_y'], rtol=1e-4, atol=2e-6)
    (y * t(gd['up_y']).cuda()).sum().backward()
    _close(x.grad.cpu().numpy(), gd['g_x'], 1e-5, 'g_x')
    for k, p in net.named_parameters():
        if 'gsd_' + k in gd:
            _close(p.grad.cpu().numpy(), gd['gsd_' + k], 1e-5, k)
    if 'grad_norms' in gd:
        # | ||g|| - ||ref|| | <= ||g - ref|| <= 1e-5 max|g| sqrt(n): what the element-wise tolerance allows a norm
        params = dict(net.named_parameters())
        for k, want in zip(gd['param_names'], gd['grad_norms']):
            g = params[str(k)].grad.double()
            assert abs(float(g.norm()) - float(want)) <= 1e-5 * float(g.abs().max()) * g.numel() ** 0.5, k


@pytest.mark.parametrize('B,H,W', [(1, 8, 8), (2, 24, 40), (3, 17, 23)])
def test_forward_backward_vs_oracle_ragged(B, H, W):
    """Sizes that are not multiples of the 64-pixel tile, tiles straddling images."""
    sd = M.init_params(seed=3)
    g = torch.Generator().manual_seed(B * 100 + W)
    for k in sd:
        if k.endswith('bias'):
            sd[k] = 0.05 * torch.randn(sd[k].shape, generator=g)
    x = 3.0 * torch.randn(B, 3, H, W, generator=g)
    tt = torch.rand(B, 1, 1, 1, generator=g).expand(B, 1, H, W).contiguous()
    up = torch.randn(B, 3, H, W, generator=g)
    sdr = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    xr = x.clone().requires_grad_(True)
    yr = _oracle_f64(sdr, xr, tt)
    (yr * up.double()).sum().backward()
    net = _net_from_sd(sd)
    xg = x.cuda().requires_grad_(True)
    yg = net(xg, tt.cuda())
    (yg * up.cuda()).sum().backward()
    np.testing.assert_allclose(yg.detach().cpu().numpy(), yr.detach().numpy(), rtol=1e-4, atol=2e-6)
    # A pre-activation within fp32 noise of 0 may take the other LeakyReLU slope on the GPU than in the float64 oracle.
    # No such pixel (what MI355X boxes measured): everything to 1e-5.  Otherwise at
    # most 2 pixels of g_x are off and the weight gradients carry that pixel's share (a fraction of a percent).
    flips = _close(xg.grad.cpu().numpy(), xr.grad.numpy(), 1e-5, 'g_x', max_outliers=-1)
    assert flips <= 6, 'g_x: %d elements off' % flips
    for k, p in net.named_parameters():
        _close(p.grad.cpu().numpy(), sdr[k].grad.numpy(), 1e-5 if flips == 0 else 2e-2, k)


def test_euler_steps_fused_bookkeeping():
    """p_next / acc outputs of the forward kernel reproduce forward_sf_net_multi_step."""
    from dvd_hip import ops
    sd = M.init_params(seed=9)
    B, H, W, steps, dt, div = 2, 16, 24, 3, 0.01, 100.0
    g = torch.Generator().manual_seed(1)
    p = 2.0 * torch.randn(B, 3, H, W, generator=g)
    ts = torch.rand(B, 1, 1, 1, generator=g).expand(B, 1, H, W).contiguous()
    want = M.sf_multi_step(sd, p, ts, dt, steps, div)
    k = ops.SceneFlowMLPKernels('cuda', 16, 16, True)
    k.pack([sd['convs.%d.conv.weight' % i].cuda() for i in range(6)], [sd['convs.%d.conv.bias' % i].cuda() for i in range(6)])
    acc = torch.zeros(B, 3, H, W, device='cuda')
    cur = p.cuda()
    tg = ts.cuda()
    for i in range(steps):
        nxt = torch.empty_like(cur)
        k.forward(cur, tg, t_offset=i * dt, out_scale=1.0 / div, p_next=nxt, acc=acc)
        cur = nxt
    np.testing.assert_allclose(acc.cpu().numpy(), want.numpy(), rtol=1e-4, atol=1e-7)


def test_unsupported_configuration_is_refused():
    from dvd_hip.networks.sceneflow_field import SceneFlowFieldNet
    with pytest.raises(NotImplementedError):
        SceneFlowFieldNet(net_width=128, n_layers=4, N_freq_xyz=16, N_freq_t=16)


@pytest.mark.parametrize('stash_f16', [False, True])
@pytest.mark.parametrize('B,H,W', [(2, 24, 40), (3, 17, 23), (4, 96, 168)])
def test_workgroup_shapes_give_the_same_bits(B, H, W, stash_f16):
    """dvd_sf_mlp_select: two 4-wave workgroups per CU (the default since round 5) against one of 8 waves (rounds 2-4).  Who
    computes a 32-channel row tile changes, the products and their order do not: outputs, both stashes (activations, sign
    words, per-layer maxima) and the input gradient are bit-identical; the weight gradients are computed from identical
    stashes by the same kernel.  dW5 / db5 are per-workgroup shares summed in workgroup order, and the two shapes have
    different grids: equal to rounding only."""
    from dvd_hip import _lib, ops
    lib = _lib.load()
    sd = M.init_params(seed=11)
    g = torch.Generator().manual_seed(5)
    p = (3.0 * torch.randn(B, 3, H, W, generator=g)).cuda()
    ts = torch.rand(B, 1, H, W, generator=g).cuda()
    gout = torch.randn(B, 3, H, W, generator=g).cuda()
    n_pix = B * H * W
    res = {}
    try:
        for nw in (8, 4):
            _lib.check(lib.dvd_sf_mlp_select(nw), 'dvd_sf_mlp_select')
            k = ops.SceneFlowMLPKernels('cuda', 16, 16, True, stash_f16=stash_f16)
            k.pack([sd['convs.%d.conv.weight' % i].cuda() for i in range(6)], [sd['convs.%d.conv.bias' % i].cuda() for i in range(6)])
            st, gst = k.new_stash(n_pix).zero_(), k.new_gstash(n_pix).zero_()
            sf, sf2, gp = torch.empty_like(p), torch.empty_like(p), torch.empty_like(p)
            k.forward(p, ts, 0.25, 0.01, sf_out=sf, stash=st)
            k.forward(p, ts, 0.25, 0.01, sf_out=sf2)                 # the instantiation without a stash
            gW5, gb5 = torch.zeros(3, 256, device='cuda'), torch.zeros(3, device='cuda')
            k.backward_dx(st, 0.01, gout, gp, gst, gW5, gb5, (B, H, W))
            n_g = ((n_pix + 63) // 64) * 5 * 256 * 64      # the gradient tiles (the dW partials behind them are scratch)
            gW = [torch.zeros(256, k.c_in if i == 0 else 256, device='cuda') for i in range(5)]
            gb = [torch.zeros(256, device='cuda') for _ in range(5)]
            k.backward_dw(st, gst, n_pix, gW, gb)
            torch.cuda.synchronize()
            res[nw] = dict(sf=sf.cpu(), sf2=sf2.cpu(), st=st.cpu(), gst=gst[:n_g].cpu(), gp=gp.cpu(), gW5=gW5.cpu(), gb5=gb5.cpu(),
                           gW=[x.cpu() for x in gW], gb=[x.cpu() for x in gb])
    finally:
        _lib.check(lib.dvd_sf_mlp_select(0), 'dvd_sf_mlp_select')
    a, b = res[8], res[4]
    for key in ('sf', 'sf2', 'st', 'gst', 'gp'):
        assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), key
    for x, y in zip(a['gW'] + a['gb'], b['gW'] + b['gb']):
        assert torch.equal(x, y)
    assert torch.equal(a['sf'], a['sf2'])
    for key in ('gW5', 'gb5'):
        np.testing.assert_allclose(b[key].numpy(), a[key].numpy(), rtol=0, atol=2e-5 * float(a[key].abs().max()))
