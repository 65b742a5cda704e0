"""The scene-flow MLP kernels (csrc/sf_mlp.hip) away from the one input geometry every other test uses.

`make_geometry` derives the kernels' shape from (n_freq_xyz, n_freq_t, time_dependent): the K steps of layer 0, the row tiles
of W_0^T in the dX kernel, the channel of t / of x, the pack layout, the stash tile size, the live column tiles of the layer-0
weight gradient.  Here forward, dX and dW run against the float64 oracle of tests/test_02_sf_mlp_gpu.py
(helpers.mlp_oracle_f64) on eight geometries, each picked for an edge (GEOMETRIES), under both workgroup shapes; the backward
arguments of `dvd_sf_mlp_bwd_dx` that carry the Euler chain and the merged regulariser (gscale, scale_ptr, g_out2, g_p_add) are
checked at kernel level against float64 autograd and against the contract of include/dvd_hip.h; the persistent tile loops
(more tiles than resident workgroups, weight-gradient slices of uneven length) and pixels of 1e2 / 1e4 times the usual
magnitude sharing a tile with ordinary ones are compared with the same oracle.

Tolerances are those of tests/test_02_sf_mlp_gpu.py:
  forward            |y - ref| <= 1e-4 |ref| + 5e-7 max|ref|   (that file's atol 2e-6 was measured at max|y| = 4.2; the small
                     embeddings reach max|y| = 17, so the absolute term is stated relative -- the same number there)
  d/dx               1e-5 of max|g|, at most 6 elements (2 LeakyReLU'-sign-flip pixels) beyond it
  weight/bias grads  1e-5 of per-tensor max|g|  (2e-2 when g_x shows such a pixel: the float32 ATen evaluation of the oracle has
                     none on any new geometry with the seeds below, 3 elements on (16, 16, T) at (3, 17, 23))
  fp16 stash         sf and g_x bit-identical to the fp32 stash, dW_0 1e-6, dW_1..5 8e-4 of max|g|, biases as
                     tests/test_10_act_fp16_gpu.py::test_mlp_fp16_stash_changes_only_the_weight_gradients
Every comparison appends its worst value and its bound to $DVD_PARITY_LOG (helpers.log_measured); the values measured on
MI355X are kept in profiles/sf_mlp_geometry_measured.jsonl.  Bounds with less than 2x headroom over what was measured there:
in the 33 120-pixel case the forward's excess over the rtol term 1.83e-6 of 2.09e-6 allowed (the fp32 ATen evaluation of the
oracle: 2.10e-6) and db_0 at 5.0e-6 of 1e-5; dW_5 of the fp16 stash on (16, 16, F) at 2x24x40, 6.0e-4 of 8e-4; and the Euler
chain on (16, 16, T), whose 2 flipped pixels are the whole cap.  Everywhere else: forward <= 0.48 of its bound, g_x <= 0.08,
weight and bias gradients <= 0.17, the fp16 stash's weight gradients <= 0.42, p_next of the chain <= 0.39; db_5 of the two
stash modes is bit-identical.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

from helpers import log_measured, mlp_oracle_f64
from oracle import sceneflow_mlp as M
from test_02_sf_mlp_gpu import _net_from_sd

pytestmark = pytest.mark.gpu

# (n_freq_xyz, n_freq_t, time_dependent): c_in / c_in16 / K steps of layer 0 / row tiles of W_0^T
GEOMETRIES = [
    (16, 16, False),   # 99 / 112 / 7 / 4   the reference's default: t == nullptr, xyz_base = 0, no partial wave
    (0, 0, False),     # 3 / 16 / 1 / 1     one K step, both frequency tables null, empty embedding backward, 13 pad channels
    (2, 0, True),      # 16 / 16 / 1 / 1    no pad channels, time channel without frequencies
    (4, 2, True),      # 32 / 32 / 2 / 1    exactly one full row tile, even K step count
    (12, 10, True),    # 96 / 96 / 6 / 3    wave 1 owns one live row tile at 4 waves
    (16, 0, True),     # 100 / 112 / 7 / 4  the t channel alone in front of a full xyz embedding
    (20, 20, True),    # 164 / 176 / 11 / 6 the largest accepted: layer-0 dW column wave 1 has two live tiles
    (16, 16, True),    # 132 / 144 / 9 / 5  control: the shipped point through this file's code path
]
SHAPES = [(3, 17, 23), (2, 24, 40)]        # ragged last tile, tiles straddling images
STASH16 = [(16, 16, False), (0, 0, False), (20, 20, True)]
FWD_RTOL, FWD_ATOL_OF_MAX, GRAD_TOL, FLIP_CAP, GRAD_TOL_FLIPPED = 1e-4, 5e-7, 1e-5, 6, 2e-2


def _gid(g):
    return 'x%d_t%d_%s' % (g[0], g[1], 'T' if g[2] else 'F')


@contextlib.contextmanager
def _workgroup_shape(nw):
    from dvd_hip import _lib
    lib = _lib.load()
    try:
        _lib.check(lib.dvd_sf_mlp_select(nw), 'dvd_sf_mlp_select')
        yield
    finally:
        _lib.check(lib.dvd_sf_mlp_select(0), 'dvd_sf_mlp_select')


def make_inputs(geom, B, H, W, seed, far=False):
    """Weights (kaiming, seed 3), biases 0.05 randn, points 3 randn, one time per image, upstream gradient randn.
    far: about 1 % of the pixels times 1e2 and 1 % times 1e4 (far-depth pixels, as dvd_hip.synthetic produces them)."""
    nx, nt, td = geom
    sd = M.init_params(seed=3, n_freq_xyz=nx, n_freq_t=nt, time_dependent=td)
    g = torch.Generator().manual_seed(seed)
    for k in sd:
        if k.endswith('bias'):
            sd[k] = 0.05 * torch.randn(sd[k].shape, generator=g)
    x = 3.0 * torch.randn(B, 3, H, W, generator=g)
    tt = torch.rand(B, 1, 1, 1, generator=g).expand(B, 1, H, W).contiguous()
    up = torch.randn(B, 3, H, W, generator=g)
    near = None
    if far:
        r = torch.rand(B, 1, H, W, generator=g)
        x = x * torch.where(r < 0.01, 1e2, 1.0) * torch.where((r >= 0.01) & (r < 0.02), 1e4, 1.0)
        near = (r >= 0.02).expand(B, 3, H, W).numpy()
    return dict(geom=geom, sd=sd, x=x, t=tt if td else None, up=up, near=near, shape=(B, H, W))


def evaluate(inp, dtype=torch.float64):
    """The oracle and its autograd gradients: float64 = the reference of every comparison here; float32 = what the same
    criteria say about a plain fp32 evaluation (how the seeds were checked for LeakyReLU' sign flips)."""
    nx, nt, _ = inp['geom']
    sdr = {k: v.to(dtype).requires_grad_(True) for k, v in inp['sd'].items()}
    xr = inp['x'].clone().requires_grad_(True)
    if dtype == torch.float64:
        yr = mlp_oracle_f64(sdr, xr, inp['t'], nx, nt)
    else:
        yr = M.mlp_forward(sdr, xr, inp['t'], nx, nt)
    (yr * inp['up'].to(dtype)).sum().backward()
    return dict(y=yr.detach().numpy(), g_x=xr.grad.numpy(), g={k: v.grad.numpy() for k, v in sdr.items()})


@functools.lru_cache(maxsize=None)
def _case(geom, B, H, W, seed, far=False):
    inp = make_inputs(geom, B, H, W, seed, far)
    return inp, evaluate(inp)


def forward_excess(y, yr, sel=None):
    """max of |y - ref| - FWD_RTOL |ref| over the selected elements, and the absolute term it is held to."""
    y, yr = np.asarray(y, np.float64).reshape(yr.shape), np.asarray(yr, np.float64)
    if sel is not None:
        y, yr = y[sel], yr[sel]
    return float((np.abs(y - yr) - FWD_RTOL * np.abs(yr)).max()), FWD_ATOL_OF_MAX * float(np.abs(yr).max())


def rel_of_max(got, want, sel=None):
    got, want = np.asarray(got, np.float64).reshape(np.shape(want)), np.asarray(want, np.float64)
    if sel is not None:
        got, want = got[sel], want[sel]
    return np.abs(got - want) / max(float(np.abs(want).max()), 1e-30)


def check_against(got, ref, tag, near=None, weights=True):
    """The criteria of the module docstring; got / ref: dicts y, g_x, g (parameter gradients by state_dict key)."""
    exc, atol = forward_excess(got['y'], ref['y'], near)
    log_measured(tag + ' forward: |y - ref| - 1e-4 |ref|', exc, atol)
    assert exc <= atol, '%s forward: excess %.3e over the rtol term, allowed %.3e' % (tag, exc, atol)
    e = rel_of_max(got['g_x'], ref['g_x'], near)
    flips = int((e > GRAD_TOL).sum())
    log_measured(tag + ' g_x of max|g| (%d elements beyond)' % flips, float(np.where(e > GRAD_TOL, 0.0, e).max()), GRAD_TOL)
    assert flips <= FLIP_CAP, '%s g_x: %d elements off by more than %.0e of max|g| (worst %.3e)' % (tag, flips, GRAD_TOL, e.max())
    if not weights:
        return
    tol = GRAD_TOL if flips == 0 else GRAD_TOL_FLIPPED
    for k in sorted(ref['g']):
        ek = float(rel_of_max(got['g'][k], ref['g'][k]).max())
        log_measured('%s %s of max|g|' % (tag, k), ek, tol)
        assert ek <= tol, '%s %s: %.3e of max|g| (allowed %.0e, %d g_x elements flipped)' % (tag, k, ek, tol, flips)


def run_module(inp):
    """SceneFlowFieldNet.forward + autograd (the fp32 stash)."""
    nx, nt, td = inp['geom']
    net = _net_from_sd(inp['sd'], td, nx, nt)
    assert net.kernels(torch.device('cuda')).c_in == inp['sd']['convs.0.conv.weight'].shape[1]
    xg = inp['x'].cuda().requires_grad_(True)
    yg = net(xg, inp['t'].cuda() if td else None)
    (yg * inp['up'].cuda()).sum().backward()
    torch.cuda.synchronize()
    return dict(y=yg.detach().cpu().numpy(), g_x=xg.grad.cpu().numpy(),
                g={k: p.grad.cpu().numpy().reshape(inp['sd'][k].shape) for k, p in net.named_parameters()})


def _kernels(geom, sd, stash_f16=False):
    from dvd_hip import ops
    k = ops.SceneFlowMLPKernels('cuda', geom[0], geom[1], geom[2], stash_f16=stash_f16)
    assert k.c_in == sd['convs.0.conv.weight'].shape[1]
    k.pack([sd['convs.%d.conv.weight' % i].float().cuda() for i in range(6)],
           [sd['convs.%d.conv.bias' % i].float().cuda() for i in range(6)])
    return k


def _zero_grads(k):
    dims = [k.c_in] + [256] * 5
    return ([torch.zeros(256 if i < 5 else 3, dims[i], device='cuda') for i in range(6)],
            [torch.zeros(256 if i < 5 else 3, device='cuda') for i in range(6)])


def run_kernels(inp, stash_f16):
    """ops.SceneFlowMLPKernels: forward with a stash, dX, dW."""
    B, H, W = inp['shape']
    n_pix = B * H * W
    k = _kernels(inp['geom'], inp['sd'], stash_f16)
    p, up = inp['x'].cuda(), inp['up'].cuda()
    ts = inp['t'].cuda() if inp['t'] is not None else None
    st, gst = k.new_stash(n_pix), k.new_gstash(n_pix)
    sf, g_p = torch.empty_like(p), torch.empty_like(p)
    k.forward(p, ts, 0.0, 1.0, sf_out=sf, stash=st)
    gW, gb = _zero_grads(k)
    k.backward_dx(st, 1.0, up, g_p, gst, gW[5], gb[5], (B, H, W))
    k.backward_dw(st, gst, n_pix, gW[:5], gb[:5])
    torch.cuda.synchronize()
    g = {}
    for i in range(6):
        g['convs.%d.conv.weight' % i] = gW[i].cpu().numpy().reshape(inp['sd']['convs.%d.conv.weight' % i].shape)
        g['convs.%d.conv.bias' % i] = gb[i].cpu().numpy()
    return dict(y=sf.cpu().numpy(), g_x=g_p.cpu().numpy(), g=g)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the geometry sweep

@pytest.mark.parametrize('B,H,W', SHAPES)
@pytest.mark.parametrize('geom', GEOMETRIES, ids=_gid)
def test_geometry_forward_backward_vs_oracle(geom, B, H, W):
    inp, ref = _case(geom, B, H, W, 100 * B + W + geom[0])
    for nw in (8, 4):
        with _workgroup_shape(nw):
            got = run_module(inp)
        check_against(got, ref, 'geometry %s %dx%dx%d nw%d' % (_gid(geom), B, H, W, nw))


@functools.lru_cache(maxsize=None)
def _stash_pair(geom, B, H, W, nw):
    inp, _ = _case(geom, B, H, W, 100 * B + W + geom[0])
    with _workgroup_shape(nw):
        return run_kernels(inp, False), run_kernels(inp, True)


@pytest.mark.parametrize('B,H,W', SHAPES)
@pytest.mark.parametrize('geom', STASH16, ids=_gid)
def test_geometry_fp16_stash(geom, B, H, W):
    """The stash offsets depend on c_in16: with the hidden activations stored as fp16 the kernels still meet the oracle
    (weight gradients within the fp16 stash's own bounds of the fp32-stash kernels), sf and g_x to the bit.  (The bias of the
    last layer: the next test.)"""
    _, ref = _case(geom, B, H, W, 100 * B + W + geom[0])
    for nw in (8, 4):
        tag = 'geometry %s %dx%dx%d nw%d fp16 stash' % (_gid(geom), B, H, W, nw)
        a, b = _stash_pair(geom, B, H, W, nw)
        check_against(a, ref, tag + ' (its fp32 twin)')
        check_against(b, ref, tag, weights=False)
        assert np.array_equal(a['y'].view(np.int32), b['y'].view(np.int32)), tag
        assert np.array_equal(a['g_x'].view(np.int32), b['g_x'].view(np.int32)), tag
        for i in range(6):
            if i < 5:
                gb32, gb16 = a['g']['convs.%d.conv.bias' % i], b['g']['convs.%d.conv.bias' % i]
                np.testing.assert_allclose(gb16, gb32, rtol=1e-6, atol=1e-7 * float(np.abs(gb32).max()), err_msg=tag)
            e = float(rel_of_max(b['g']['convs.%d.conv.weight' % i], a['g']['convs.%d.conv.weight' % i]).max())
            bound = 1e-6 if i == 0 else 8e-4                 # layer 0 contracts against the fp32 embedding
            log_measured('%s dW_%d vs fp32 stash, of max|g|' % (tag, i), e, bound)
            assert e <= bound, (tag, i, e)


@pytest.mark.parametrize('B,H,W', SHAPES)
@pytest.mark.parametrize('geom', STASH16, ids=_gid)
def test_geometry_fp16_stash_last_layer_bias(geom, B, H, W):
    """db_5 of the fp16-stash run against the fp32-stash run, at the bound tests/test_10_act_fp16_gpu.py holds all six biases
    to (rtol 1e-6, atol 1e-7 max|db|).  db_5 does not depend on the stash at all, so this compares two runs of one sum: 1920
    addends of size 1 whose partial sums reach 30 (ulp 1.9e-6 .. 3.8e-6), i.e. a bound of 1 - 2 ulp of a partial sum.  While
    the dX kernel's workgroups added their shares to db_5 with float atomics, in the order they happened to finish, one
    element in 36 missed it ((16, 16, F) at 2x24x40, 8 waves: 6.7e-6 and 4.8e-6 in two runs where 3.7e-6 is allowed); the
    shares are now summed in workgroup order (mlp_dx5_reduce_kernel) and two runs give the same bits."""
    for nw in (8, 4):
        tag = 'geometry %s %dx%dx%d nw%d fp16 stash db_5' % (_gid(geom), B, H, W, nw)
        a, b = _stash_pair(geom, B, H, W, nw)
        gb32, gb16 = a['g']['convs.5.conv.bias'], b['g']['convs.5.conv.bias']
        atol = 1e-7 * float(np.abs(gb32).max())
        log_measured(tag + ': |db16 - db32| - 1e-6 |db32|', float((np.abs(gb16 - gb32) - 1e-6 * np.abs(gb32)).max()), atol)
        np.testing.assert_allclose(gb16, gb32, rtol=1e-6, atol=atol, err_msg=tag)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the backward arguments of the Euler chain

CHAIN = dict(B=2, H=16, W=24, steps=3, dt=0.01, inv_div=1.0 / 100.0)


@functools.lru_cache(maxsize=None)
def _chain_inputs(geom):
    nx, nt, td = geom
    B, H, W = CHAIN['B'], CHAIN['H'], CHAIN['W']
    sd = M.init_params(seed=9, n_freq_xyz=nx, n_freq_t=nt, time_dependent=td)
    g = torch.Generator().manual_seed(21 + nx + int(td))
    for k in sd:
        if k.endswith('bias'):
            sd[k] = 0.05 * torch.randn(sd[k].shape, generator=g)
    p = 2.0 * torch.randn(B, 3, H, W, generator=g)
    ts = torch.rand(B, 1, 1, 1, generator=g).expand(B, 1, H, W).contiguous()
    g_acc = torch.randn(B, 3, H, W, generator=g)
    return dict(geom=geom, sd=sd, p=p, t=ts if td else None, g_acc=g_acc)


def chain_reference(inp, points=None):
    """The float64 restatement of oracle.sceneflow_mlp.sf_multi_step (fp32 embedding, as helpers.mlp_oracle_f64) and its
    autograd gradients for the upstream gradient g_acc of the summed flow.

    points: the fp32 points p_1, p_2 the kernels stored (p_next).  The oracle's own p_i = p_{i-1} + sf_{i-1} rounds to fp32
    one ulp off the kernel's for about every fifth pixel (sf differs in its last bits), and the embedding multiplies that ulp
    by frequencies up to 17: the later evaluations' pre-activations would differ by 1e-5 for a reason that is no error of
    either side.  So the oracle evaluates step i AT the kernel's p_i -- value p_i^kernel, derivative of p_{i-1} + sf_{i-1} --
    and returns how far the two are apart; the caller holds that to the forward tolerance of sf plus one fp32 ulp of p.
    (Measured on MI355X: (16, 16, T) has 2 LeakyReLU'-flip pixels of 768 -- 6 elements of g_x, the whole cap -- with either
    form of the oracle, so they are the kernels' own rounding at a pre-activation next to zero; weight gradients then 6.1e-3
    of 2e-2.  (16, 16, F): none.)"""
    nx, nt, td = inp['geom']
    steps, dt, inv_div = CHAIN['steps'], CHAIN['dt'], CHAIN['inv_div']
    sdr = {k: v.double().requires_grad_(True) for k, v in inp['sd'].items()}
    pr = inp['p'].double().requires_grad_(True)
    cur, acc, gaps = pr, 0, []
    for i in range(steps):
        if i > 0 and points is not None:
            gaps.append((points[i - 1].double() - cur.detach(), cur.detach(), sf.detach()))
            cur = cur + (points[i - 1].double() - cur.detach())
        sf = mlp_oracle_f64(sdr, cur, (inp['t'] + i * dt) if td else None, nx, nt) * inv_div
        acc = acc + sf
        cur = cur + sf
    (acc * inp['g_acc'].double()).sum().backward()
    return dict(y=acc.detach().numpy(), g_x=pr.grad.numpy(), g={k: v.grad.numpy() for k, v in sdr.items()}), gaps


@pytest.mark.parametrize('geom', [(16, 16, True), (16, 16, False)], ids=_gid)
def test_euler_chain_backward_vs_float64_autograd(geom):
    """Forward with stashes, p_next and acc, then the backward exactly as Model.mlp_backward_chunk issues it
    (g_out1 = g_acc, g_out2 = g_p_add = g_p of the later step, reverse order, backward_dw after each): the summed flow, the
    gradient of the first points and all twelve parameter gradients against float64 autograd through the chain."""
    inp = _chain_inputs(geom)
    B, H, W, steps, dt, inv_div = (CHAIN[k] for k in ('B', 'H', 'W', 'steps', 'dt', 'inv_div'))
    n_pix = B * H * W
    for nw in (8, 4):
        tag = 'euler chain %s nw%d' % (_gid(geom), nw)
        with _workgroup_shape(nw):
            k = _kernels(geom, inp['sd'])
            ts = inp['t'].cuda() if inp['t'] is not None else None
            cur, acc, stashes, points = inp['p'].cuda(), torch.zeros(B, 3, H, W, device='cuda'), [], []
            for i in range(steps):
                st = k.new_stash(n_pix)
                nxt = torch.empty_like(cur) if i + 1 < steps else None
                k.forward(cur, ts, t_offset=i * dt, out_scale=inv_div, p_next=nxt, acc=acc, stash=st)
                stashes.append(st)
                if nxt is not None:
                    points.append(nxt)
                cur = nxt
            gW, gb = _zero_grads(k)
            gst, g_acc, g_p = k.new_gstash(n_pix), inp['g_acc'].cuda(), None
            for i in reversed(range(steps)):
                g_new = torch.empty(B, 3, H, W, device='cuda')
                k.backward_dx(stashes[i], inv_div, g_acc, g_new, gst, gW[5], gb[5], (B, H, W), g_out2=g_p, g_p_add=g_p)
                k.backward_dw(stashes[i], gst, n_pix, gW[:5], gb[:5])
                g_p = g_new
            torch.cuda.synchronize()
        ref, gaps = chain_reference(inp, [x.cpu() for x in points])
        for i, (gap, p_or, sf_or) in enumerate(gaps):       # p_next of step i: |p - ref| <= forward tolerance of sf + ulp(p)
            allowed = FWD_RTOL * sf_or.abs() + FWD_ATOL_OF_MAX * float(sf_or.abs().max()) + 2.0 ** -23 * p_or.abs()
            log_measured('%s p_next of step %d: |p - ref| / allowed' % (tag, i), float((gap.abs() / allowed).max()), 1.0)
            assert bool((gap.abs() <= allowed).all()), '%s: p_next of step %d' % (tag, i)
        g = {}
        for i in range(6):
            g['convs.%d.conv.weight' % i] = gW[i].cpu().numpy().reshape(inp['sd']['convs.%d.conv.weight' % i].shape)
            g['convs.%d.conv.bias' % i] = gb[i].cpu().numpy()
        check_against(dict(y=acc.cpu().numpy(), g_x=g_p.cpu().numpy(), g=g), ref, tag)


@pytest.mark.parametrize('geom', [(16, 16, True), (16, 16, False)], ids=_gid)
def test_backward_dx_contract_with_distinct_arguments(geom):
    """include/dvd_hip.h: g_out = gscale * *scale_ptr * g_out1 + g_out2, g_p = J^T(out_scale * g_out) + g_p_add -- one
    evaluation with gscale = -1, *scale_ptr = 0.37 and DIFFERENT tensors for g_out2 and g_p_add (every caller passes the same
    tensor for both, so a swapped pair would go unseen), against float64 autograd of one evaluation."""
    nx, nt, td = geom
    inp = _chain_inputs(geom)
    B, H, W, inv_div = CHAIN['B'], CHAIN['H'], CHAIN['W'], CHAIN['inv_div']
    n_pix = B * H * W
    g = torch.Generator().manual_seed(77)
    g1, g2, gadd = (torch.randn(B, 3, H, W, generator=g) for _ in range(3))
    gscale, scale = -1.0, 0.37
    sdr = {k: v.double().requires_grad_(True) for k, v in inp['sd'].items()}
    pr = inp['p'].double().requires_grad_(True)
    yr = mlp_oracle_f64(sdr, pr, inp['t'], nx, nt) * inv_div
    g_out = gscale * float(np.float32(scale)) * g1.double() + g2.double()
    (yr * g_out).sum().backward()
    ref = dict(y=yr.detach().numpy(), g_x=(pr.grad + gadd.double()).numpy(), g={k: v.grad.numpy() for k, v in sdr.items()})
    for nw in (8, 4):
        with _workgroup_shape(nw):
            k = _kernels(geom, inp['sd'])
            st, gst = k.new_stash(n_pix), k.new_gstash(n_pix)
            p = inp['p'].cuda()
            sf, g_p = torch.empty_like(p), torch.empty_like(p)
            k.forward(p, inp['t'].cuda() if td else None, 0.0, inv_div, sf_out=sf, stash=st)
            gW, gb = _zero_grads(k)
            k.backward_dx(st, inv_div, g1.cuda(), g_p, gst, gW[5], gb[5], (B, H, W), gscale=gscale,
                          scale_ptr=torch.full((1,), scale, device='cuda'), g_out2=g2.cuda(), g_p_add=gadd.cuda())
            k.backward_dw(st, gst, n_pix, gW[:5], gb[:5])
            torch.cuda.synchronize()
        gg = {}
        for i in range(6):
            gg['convs.%d.conv.weight' % i] = gW[i].cpu().numpy().reshape(inp['sd']['convs.%d.conv.weight' % i].shape)
            gg['convs.%d.conv.bias' % i] = gb[i].cpu().numpy()
        check_against(dict(y=sf.cpu().numpy(), g_x=g_p.cpu().numpy(), g=gg), ref, 'dx contract %s nw%d' % (_gid(geom), nw))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the persistent loops

PERSISTENT = dict(B=3, H=96, W=115, seed=4117, z_margin=2e-5)     # 33 120 pixels = 517.5 tiles


def persistent_batch(cu_count):
    """B such that the 4-wave grid (2 workgroups per CU, persistent_grid in csrc/sf_mlp.hip) is smaller than the tile count
    and the weight-gradient slices are of uneven length."""
    B, hw = PERSISTENT['B'], PERSISTENT['H'] * PERSISTENT['W']
    while (B * hw + 63) // 64 <= 2 * cu_count or ((B * hw + 63) // 64) % 51 == 0:
        B += 1
    return B


@functools.lru_cache(maxsize=None)
def persistent_case(B):
    """The inputs of part 1 at 33 120 pixels, with one change.  42 million hidden units hold, at one LeakyReLU' sign flip per
    2.5 - 8 million units (tests/test_02_sf_mlp_gpu.py::_close; the fp32 ATen evaluation of this very case: 5 pixels), more
    flipped pixels than the cap of part 1 allows ANY correct fp32 implementation.  A flip needs a pre-activation within the
    implementation's rounding noise (1e-7 .. 1e-6 of |z| ~ 1) of zero, so the upstream gradient is set to ZERO at the pixels
    where the float64 oracle has a hidden pre-activation with |z| < 2e-5 (about 2 % of the pixels, known from the oracle
    alone): a flip there changes no gradient, everywhere else none can happen, and every gradient is held to 1e-5 with no
    allowance.  Those pixels still run through every tile loop and their outputs are compared like all others."""
    geom = (16, 16, True)
    inp = make_inputs(geom, B, PERSISTENT['H'], PERSISTENT['W'], PERSISTENT['seed'])
    pre = []
    with torch.no_grad():
        mlp_oracle_f64({k: v.double() for k, v in inp['sd'].items()}, inp['x'], inp['t'], geom[0], geom[1], pre=pre)
    zmin = torch.stack([z.abs().amin(1, keepdim=True) for z in pre]).amin(0)
    live = zmin >= PERSISTENT['z_margin']
    assert 0.9 < float(live.float().mean()) < 0.999
    inp['up'] = inp['up'] * live
    return inp, evaluate(inp)


def test_persistent_tile_loops_vs_oracle():
    """More tiles than resident workgroups: some forward / dX workgroup takes a second tile (next-tile prefetch, X and `red`
    reused across tiles), and the weight-gradient slices hold uneven tile counts (kDwSlices = 51).  Every other oracle
    comparison of these kernels has at most 30 tiles."""
    from dvd_hip import _lib
    cus = int(_lib.load().dvd_device_cu_count())
    assert cus > 0
    B, H, W = persistent_batch(cus), PERSISTENT['H'], PERSISTENT['W']
    n_tiles = (B * H * W + 63) // 64
    assert n_tiles > 2 * cus and n_tiles > 51 and n_tiles % 51 != 0, (n_tiles, cus)
    inp, ref = persistent_case(B)
    for nw in (8, 4):
        with _workgroup_shape(nw):
            got = run_module(inp)
        check_against(got, ref, 'persistent loops %dx%dx%d (%d tiles, %d CUs) nw%d' % (B, H, W, n_tiles, cus, nw))


# ---------------------------------------------------------------------------------------------------------------------
# 4. wide dynamic range of the points

@pytest.mark.parametrize('geom', [(16, 16, True), (16, 16, False)], ids=_gid)
def test_far_pixels_do_not_cost_the_near_ones_their_precision(geom):
    """About 1 % of the pixels at 1e2 and 1 % at 1e4 times the usual magnitude.  The operand scale is per 64-pixel tile, so
    near pixels share a tile (and its scale) with far ones; by csrc/dvd_split.h a value keeps its 22 bits down to 2^-17 of the
    tile maximum, so the near pixels are held to the usual forward and g_x criteria, normalised by the NEAR pixels' own
    max|y| / max|g| (the global maxima are 100 to 10 000 times larger and would hide everything).  The weight gradients are
    dominated by the far pixels and not compared."""
    B, H, W = 3, 17, 23
    inp, ref = _case(geom, B, H, W, 100 * B + W + geom[0], True)
    near = inp['near']
    assert 0.9 < near.mean() < 0.995
    assert np.abs(inp['x'].numpy()[~near]).max() > 1e3 * np.abs(inp['x'].numpy()[near]).max()
    for nw in (8, 4):
        with _workgroup_shape(nw):
            got = run_module(inp)
        check_against(got, ref, 'far pixels %s nw%d (near pixels)' % (_gid(geom), nw), near=near, weights=False)
