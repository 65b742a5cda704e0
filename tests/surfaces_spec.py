"""Float64 specification of the warp-module surface (csrc/surfaces.hip, csrc/unproject.hip and their wrappers in
dvd_hip/ops.py), for tests/test_67_surfaces_kernel_gpu.py and tests/test_surfaces_spec_cpu.py.

oracle/geometry.py restates the reference's modules op for op; called with float64 inputs it is their float64 specification, and
its autograd is the float64 vector-Jacobian product.  This file adds

  * CASES / case(name): the named input sets, at the smallest shapes at which the kernels can still go wrong;
  * surfaces(name, dtype) / vjp(name, dtype, surface): the nine surfaces, the discrete decisions, and the gradients of
    <surface, upstream(surface)> w.r.t. depth_1, depth_2 and the scene flow;
  * decisions_agree(name): the fp32 and the float64 oracle take the same behind-camera and tap-cell decisions at every pixel
    (a condition on the inputs and the reference alone; a case that violates it gets another seed, nothing is masked);
  * rel_err and TOL: the error measure and the tolerances, measured on the reference -- not on the kernel;
  * flow_warp_spec: F.grid_sample through G.flow_sample in float64.
"""
import functools
import math
import os
import sys

import torch

if __name__ == '__main__':          # run as a script (prints the measured table): the paths tests/conftest.py sets for pytest
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, 'dynamic-video-depth_amd')]

from dvd_hip import synthetic
from oracle import geometry as G

CAM_KEYS = ('R_1', 'R_2', 'R_1_T', 'R_2_T', 't_1', 't_2', 'K', 'K_inv')
SURFACES = ('global_p1', 'warped_global_p2', 'sf_by_depth', 'staticflow_1_2', 'dflow_1_2', 'depth_image_1_2', 'depth_warp_1_2',
            'p1_camera_2', 'warped_p2_camera_2')
STATIC_SUBSET = ('staticflow_1_2', 'sf_by_depth', 'warped_global_p2', 'global_p1')                    # flow_by_depth
SLACK_SUBSET = ('dflow_1_2', 'depth_image_1_2', 'depth_warp_1_2', 'global_p1', 'staticflow_1_2', 'p1_camera_2',
                'warped_p2_camera_2')                                                                 # scene_flow_projection_slack
GRADS = ('g_depth_1', 'g_depth_2', 'g_sflow')
WARP_CHANNELS = (1, 2, 3, 5)

# name -> (B, H, W, seed)
CASES = {
    'b1_2x2': (1, 2, 2, 21),       # the minimum the entry points accept: every tap touches a border
    'b3_7x9': (3, 7, 9, 22),       # HW = 63 < one block, odd width, three cameras
    'b2_16x16': (2, 16, 16, 23),   # HW = 256: exactly one block, the tail test is never true
    'b2_16x17': (2, 16, 17, 24),   # HW = 272: the second block has 16 live threads
    'b3_17x23': (3, 17, 23, 25),   # odd in both dimensions, several rows per block
    'b2_17x33': (2, 17, 33, 26),   # (W-1)/2 = 16, (H-1)/2 = 8: the normalise / un-normalise round trip is exact
}


def _rot(ax, a):
    c, s = math.cos(a), math.sin(a)
    m = {'x': [[1, 0, 0], [0, c, -s], [0, s, c]], 'y': [[c, 0, s], [0, 1, 0], [-s, 0, c]]}[ax]
    return torch.tensor(m, dtype=torch.float64)


def cameras(B, H, W, seed, behind_camera_pairs=0):
    """(the synthetic batch, its eight camera tensors with a camera 1 and intrinsics of its own for every image)."""
    batch = synthetic.make_batch(B, H, W, gap=list(range(1, B + 1)), seed=seed, behind_camera_pairs=behind_camera_pairs,
                                 with_images=False)
    c = {k: batch[k].clone() for k in CAM_KEYS}
    for b in range(B):
        R1 = _rot('y', 0.02 * b + 0.01) @ _rot('x', 0.015 * b - 0.01)              # cam -> world of frame 1
        f = 0.9 * W * (1.0 + 0.1 * b)
        K = torch.tensor([[f, 0.0, (W - 1) / 2.0 + 0.25 * b], [0.0, 1.05 * f, (H - 1) / 2.0 - 0.125 * b], [0.0, 0.0, 1.0]],
                         dtype=torch.float64)
        c['R_1_T'][b, 0, 0] = R1.float()
        c['R_1'][b, 0, 0] = R1.float().T
        c['t_1'][b, 0, 0, 0] = torch.tensor([0.02 * b, -0.01 * b, 0.03 * b])
        c['K'][b, 0, 0] = K.T.float()
        c['K_inv'][b, 0, 0] = torch.linalg.inv(K).T.float()
    return batch, c


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of a case (fp32 CPU tensors; shared, never modified): depth_1, depth_2 [B,1,H,W], flow_1_2 [B,H,W,2],
    sflow_1_2 [B,H,W,1,3] and the eight camera tensors.  Built from dvd_hip.synthetic like tests/test_01; on top of it

      * every image has its own camera 1 and intrinsics (camera 2 differs per image through the per-pair frame gaps), so a
        per-image index slip in any camera load shows;
      * the last image of a batch of more than one is a behind-camera pair (all of it);
      * image 0 is behind camera 2 at part of its pixels: camera 2 sits 3.5 along z and depth_1 avoids [3, 4.5), so the
        reprojected z is below -0.5 or above 1 -- the 1e-3 threshold decides, and no pixel is close enough to it for its 1 / z
        to amplify rounding; at every fifth pixel the scene flow moves the point 4 across the camera plane, so the dynamic and
        the static flag differ there;
      * the flows of the first rows of image 0 are multiplied by 15 and the four corner pixels of the last image point far
        outside, one to each side pair (fractional targets: no tap cell rests on a rounding); three pixels of image 0 have
        fixed depths on either side of camera 2, so that every flag is taken both ways even at 2 x 2;
      * 1 % far depths (150).
    """
    B, H, W, seed = CASES[name]
    batch, c = cameras(B, H, W, seed, behind_camera_pairs=1 if B > 1 else 0)
    d1, d2 = synthetic.make_depths(B, H, W, seed=seed + 100, far_depth_frac=0.01)
    sf = 20.0 * synthetic.make_scene_flow(B, H, W, seed=seed + 200).permute(0, 2, 3, 1)[..., None, :].contiguous()
    # image 0: partly behind camera 2
    c['t_2'][0, 0, 0, 0, 2] = 3.5
    d = d1[0]
    d[(d >= 3.0) & (d < 4.5)] += 1.5
    d[0, 0, 0], d[0, 0, 1], d[0, 1, 0] = 5.0, 2.0, 5.5      # (in front / behind / in front: each flag both ways even at 2 x 2)
    every5 = (torch.arange(H * W) % 5 == 0).view(H, W)
    sf[0, :, :, 0, 2] = torch.where(every5, torch.where(d[0] >= 4.5, -4.0, 4.0), sf[0, :, :, 0, 2])
    flow = batch['flow_1_2'].clone()
    flow[0, :max(1, H // 4)] *= 15.0
    flow[B - 1, 0, 0] = torch.tensor([-W - 3.5, -H - 2.25])
    flow[B - 1, 0, W - 1] = torch.tensor([W + 5.5, -H - 7.75])
    flow[B - 1, H - 1, 0] = torch.tensor([-2.0 * W - 0.25, 2.0 * H + 0.5])
    flow[B - 1, H - 1, W - 1] = torch.tensor([3.0 * W + 0.25, H + 0.75])
    out = dict(c, depth_1=d1, depth_2=d2, flow_1_2=flow, sflow_1_2=sf)
    return {k: v.contiguous() for k, v in out.items()}


def _nine(cs, d1, d2, sf):
    cams = {k: cs[k] for k in CAM_KEYS}
    dy = G.dynamic_reprojection(d1, d2, cs['flow_1_2'], -cs['flow_1_2'], sflow_1_2=sf, sflow_2_1=sf, **cams)
    st = G.static_reprojection(d1, d2, cs['flow_1_2'], **cams)
    s = {k: dy[k] for k in SLACK_SUBSET}
    s.update(warped_global_p2=st['warped_global_p2'], sf_by_depth=st['sf_by_depth'])
    s.update(_behind=dy['_behind'][..., 0, 0], _behind_static=dy['_behind_static'][..., 0, 0])
    return s


@functools.lru_cache(maxsize=None)
def _graph(name, dtype, with_sflow):
    cs = {k: v.to(dtype) for k, v in case(name).items()}
    leaves = [cs[k].clone().requires_grad_(True) for k in ('depth_1', 'depth_2', 'sflow_1_2')]
    if not with_sflow:
        leaves[2] = torch.zeros_like(leaves[2]).requires_grad_(True)
    return leaves, _nine(cs, *leaves)


def surfaces(name, dtype=torch.float64, with_sflow=True):
    """The nine surfaces of a case in `dtype`, with the boolean [B,H,W] maps '_behind' and '_behind_static'."""
    return {k: v.detach() for k, v in _graph(name, dtype, with_sflow)[1].items()}


def upstream(name, surface):
    """The fixed random upstream gradient (fp32) of one surface of a case."""
    B, H, W, seed = CASES[name]
    g = torch.Generator().manual_seed(seed * 1000 + SURFACES.index(surface))
    shape = tuple(_graph(name, torch.float32, True)[1][surface].shape)
    return torch.randn(shape, generator=g)


@functools.lru_cache(maxsize=None)
def vjp(name, dtype, surface):
    """(g_depth_1, g_depth_2, g_sflow) of <surface, upstream(name, surface)> by the oracle's autograd in `dtype`."""
    leaves, s = _graph(name, dtype, True)
    gs = torch.autograd.grad((s[surface] * upstream(name, surface).to(dtype)).sum(), leaves, retain_graph=True, allow_unused=True)
    return tuple(torch.zeros_like(l) if g is None else g.detach() for g, l in zip(gs, leaves))


def decisions_agree(name):
    """Asserts that the fp32 and the float64 oracle decide alike at every pixel of a case: the behind-camera flags of the
    dynamic and the static reprojection, and the north-west tap cell.  Also that each decision is taken both ways."""
    B, H, W, _ = CASES[name]
    s32, s64 = surfaces(name, torch.float32), surfaces(name, torch.float64)
    for k in ('_behind', '_behind_static'):
        assert torch.equal(s32[k], s64[k]), '%s: %s differs between fp32 and float64' % (name, k)
        assert s32[k].any() and not s32[k].all(), '%s: %s is taken one way only' % (name, k)
    assert not torch.equal(s32['_behind'], s32['_behind_static']), name
    flow = case(name)['flow_1_2']
    for a, b in zip(G.tap_indices(flow, H, W), G.tap_indices(flow.double(), H, W)):
        assert torch.equal(a, b), '%s: a tap cell differs between fp32 and float64' % name


def rel_err(got, want, planar=None):
    """max|got - want| over max|want|, taken per image and per component (the largest such ratio), so that a 150-unit world
    coordinate of one image does not hide a wrong 0.2 px flow of another.  Layouts: [B,H,W,1,C]; with four dimensions [B,C,H,W]
    where planar, [B,H,W,C] where not (None: planar if C would be 1, as for the depth maps).  An image component whose
    specification is all zero must be matched exactly (else inf)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape and want.dim() in (4, 5), (got.shape, want.shape)
    if planar is None:
        planar = want.dim() == 4 and want.shape[1] == 1
    if planar:
        B, C = want.shape[:2]
        got, want = got.reshape(B, C, -1), want.reshape(B, C, -1)
    else:
        B, C = want.shape[0], want.shape[-1]
        got, want = got.reshape(B, -1, C).transpose(1, 2), want.reshape(B, -1, C).transpose(1, 2)
    err, mag = (got - want).abs().amax(-1), want.abs().amax(-1)
    if bool(torch.isnan(err).any()):
        return float('nan')
    ratio = torch.where(mag > 0, err / mag.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), err))
    return float(ratio.max())


def taps(flow, H, W):
    """The cells the four bilinear taps of every pixel read, as the kernels decide them: [B,H,W,4] linear indices y * W + x, -1
    for an east or south tap past the border (the kernels do not touch it)."""
    x0, y0 = (v.long() for v in G.tap_indices(flow, H, W))
    cells = []
    for dy in (0, 1):
        for dx in (0, 1):
            ok = (x0 + dx < W) & (y0 + dy < H)
            cells.append(torch.where(ok, (y0 + dy) * W + x0 + dx, torch.full_like(x0, -1)))
    return torch.stack(cells, -1)


def scatter_counts(flow, H, W):
    """[B,H,W]: how many taps land in each cell -- at most that many atomic adds build a scattered gradient there.  Up to two
    commute, so such a cell has the same bits in every launch; more are added in an order the hardware picks."""
    t = taps(flow, H, W)
    B = t.shape[0]
    n = torch.zeros(B, H * W + 1, dtype=torch.long)
    n.scatter_add_(1, (t.reshape(B, -1) + 1), torch.ones(B, H * W * 4, dtype=torch.long))
    return n[:, 1:].view(B, H, W)


def flow_warp_inputs(name, C):
    """(x [B,C,H,W], upstream g [B,C,H,W]) of the flow_warp checks of a case (fp32)."""
    B, H, W, seed = CASES[name]
    g = torch.Generator().manual_seed(seed * 77 + C)
    return torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)


def flow_warp_spec(x, flow, g=None):
    """G.flow_sample in the dtype of x; with an upstream gradient g also its VJP w.r.t. x, by autograd."""
    B, C, H, W = x.shape
    x = x.clone().requires_grad_(g is not None)
    out = G.flow_sample(x, flow.to(x.dtype), G.pixel_grid(H, W, dtype=x.dtype))
    if g is None:
        return out.detach()
    (gx,) = torch.autograd.grad((out * g.to(x.dtype)).sum(), x)
    return out.detach(), gx


def tol_key(surface, with_sflow=True):
    """The TOL entry a surface is held to: its own, but without a scene flow dflow_1_2 IS staticflow_1_2, bit for bit, and is
    held to that one's (the static flow is the smaller quantity, so the same rounding is more of it)."""
    return 'staticflow_1_2' if surface == 'dflow_1_2' and not with_sflow else surface


def measure():
    """The error of the fp32 oracle against the float64 oracle, per quantity: {key: {case: rel_err}}.  This is what TOL is
    derived from; tests/test_surfaces_spec_cpu.py holds TOL to it from both sides."""
    m = {k: {} for k in SURFACES + GRADS + ('flow_warp', 'flow_warp_bwd')}
    for name in CASES:
        for with_sflow in (True, False):
            s32, s64 = surfaces(name, torch.float32, with_sflow), surfaces(name, torch.float64, with_sflow)
            for k in SURFACES:
                key = tol_key(k, with_sflow)
                m[key][name] = max(m[key].get(name, 0.0), rel_err(s32[k], s64[k]))
        for i, gk in enumerate(GRADS):
            m[gk][name] = max(rel_err(vjp(name, torch.float32, k)[i], vjp(name, torch.float64, k)[i]) for k in SURFACES)
        flow, fw, bw = case(name)['flow_1_2'], 0.0, 0.0
        for C in WARP_CHANNELS:
            x, g = flow_warp_inputs(name, C)
            o32, g32 = flow_warp_spec(x, flow, g)
            o64, g64 = flow_warp_spec(x.double(), flow, g)
            fw, bw = max(fw, rel_err(o32, o64, planar=True)), max(bw, rel_err(g32, g64, planar=True))
        m['flow_warp'][name], m['flow_warp_bwd'][name] = fw, bw
    return m


# How much of the measured reference error a tolerance is: twice, because the kernels follow the reference's fp32 operation
# order and differ from ATen's CPU kernels by FMA contraction only; four times where the kernel scatters with fp32 atomics
# in arbitrary order and border cells collect many clamped targets.
TOL_FACTOR = {k: 2.0 for k in SURFACES + GRADS + ('flow_warp', 'flow_warp_bwd')}
TOL_FACTOR.update(g_depth_2=4.0, flow_warp_bwd=4.0)


def tol_from(worst, factor):
    """factor * worst, rounded up to one significant digit."""
    v = factor * worst
    e = math.floor(math.log10(v))
    return math.ceil(v / 10.0 ** e - 1e-9) * 10.0 ** e


# TOL[key] = tol_from(largest measured value over the cases, TOL_FACTOR[key]).  The comments hold what was measured: the fp32
# oracle against the float64 oracle with torch's CPU kernels on the x86-64 build host of this suite, the largest value first and
# then the six cases in the order of CASES, each the larger of the runs with and without a scene flow (python
# tests/surfaces_spec.py prints the table again).  Nothing here was measured on
# a kernel.
TOL = {
    'global_p1': 5e-7,            # 2.107e-07   7.1e-08 1.6e-07 1.7e-07 2.1e-07 1.4e-07 1.0e-07
    'warped_global_p2': 5e-6,     # 2.035e-06   6.7e-08 1.7e-07 1.4e-06 1.6e-06 9.6e-07 2.0e-06
    'sf_by_depth': 3e-6,          # 1.377e-06   1.6e-07 1.3e-07 4.4e-07 1.3e-06 9.0e-07 1.4e-06
    'staticflow_1_2': 8e-6,       # 3.808e-06   2.7e-07 3.7e-06 5.6e-07 6.6e-07 3.8e-06 7.2e-07
    'dflow_1_2': 2e-6,            # 8.698e-07   5.2e-07 4.2e-07 7.9e-07 4.9e-07 5.2e-07 8.7e-07
    'depth_image_1_2': 6e-7,      # 2.774e-07   2.8e-07 1.1e-07 1.3e-07 8.7e-08 1.3e-07 1.1e-07
    'depth_warp_1_2': 4e-6,       # 1.745e-06   0.0e+00 1.4e-07 6.3e-07 1.7e-06 9.5e-07 1.5e-06
    'p1_camera_2': 6e-7,          # 2.774e-07   2.8e-07 1.6e-07 1.9e-07 2.5e-07 1.5e-07 1.2e-07
    'warped_p2_camera_2': 5e-6,   # 2.035e-06   3.5e-08 1.6e-07 1.4e-06 1.7e-06 9.5e-07 2.0e-06
    'g_depth_1': 4e-6,            # 1.511e-06   8.6e-07 6.6e-07 1.2e-06 6.4e-07 1.2e-06 1.5e-06
    'g_depth_2': 5e-6,            # 1.089e-06   5.9e-08 3.8e-07 5.0e-07 7.5e-07 1.1e-06 8.6e-07     (four times)
    'g_sflow': 3e-6,              # 1.448e-06   7.2e-07 2.8e-07 9.8e-07 4.1e-07 6.9e-07 1.4e-06
    'flow_warp': 4e-6,            # 1.965e-06   0.0e+00 5.4e-07 9.0e-07 1.1e-06 2.0e-06 2.0e-06
    'flow_warp_bwd': 6e-6,        # 1.411e-06   0.0e+00 3.2e-07 7.4e-07 6.7e-07 1.4e-06 1.1e-06     (four times)
}


if __name__ == '__main__':
    meas = measure()
    for key, per in meas.items():
        worst = max(per.values())
        print("    %-22r %.3e,   # -> TOL %.0e   %s" % (key + ':', worst, tol_from(worst, TOL_FACTOR[key]),
                                                        ' '.join('%.1e' % per[n] for n in CASES)))
