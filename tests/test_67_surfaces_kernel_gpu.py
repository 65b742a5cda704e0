"""The warp-module kernels (csrc/surfaces.hip: dvd_warp_surfaces, dvd_warp_surfaces_bwd, dvd_flow_warp_fwd / _bwd;
csrc/unproject.hip: dvd_unproject_fwd), their wrappers in dvd_hip/ops.py and the modules of losses/scene_flow_projection.py,
one surface at a time against the float64 specification of tests/surfaces_spec.py.

Shapes, cases and tolerances are the specification's: every tolerance is a multiple of the fp32 reference's own error against
float64 (surfaces_spec.TOL, held to it from both sides by tests/test_surfaces_spec_cpu.py), measured per image and per component.
Discrete decisions (behind-camera flags, tap cells), output subsets, guard bytes, integer warps, the scalar / vector paths of
unproject and the reach of a NaN are bit-exact.  A gradient scattered with fp32 atomics is bit-exact between two launches only
where at most two taps land in a cell (two adds commute, the order of more is the hardware's): _same_scatter asserts the bits
there and the tolerance everywhere."""
import ctypes

import pytest
import torch

import surfaces_spec as S
from oracle import geometry as G

pytestmark = pytest.mark.gpu
F64 = torch.float64
PATTERN = 0xA5


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


_gpu = {}


def _case(name):
    """(depth_1, depth_2, flow_1_2, sflow_1_2, cams) of a case on the GPU; uploaded once, never modified."""
    if name not in _gpu:
        c = {k: v.cuda() for k, v in S.case(name).items()}
        _gpu[name] = (c['depth_1'], c['depth_2'], c['flow_1_2'], c['sflow_1_2'], {k: c[k] for k in S.CAM_KEYS})
    return _gpu[name]


def _check(figures):
    """figures: (label, measured, bound).  Prints every one, then asserts them all."""
    bad = []
    for label, e, tol in figures:
        print('%-60s %.3e  (bound %.0e)' % (label, e, tol))
        if not e <= tol:
            bad.append('%s: %.3e > %.0e' % (label, e, tol))
    assert not bad, '\n'.join(bad)


def _same_scatter(got, other, counts, label, tol):
    """Two launches of a scattered gradient [B,C,H,W]: the same bits where at most two taps land, `tol` everywhere."""
    sure = (counts <= 2)[:, None].expand(got.shape)
    assert torch.equal(_bits(got)[sure], _bits(other)[sure]), label
    _check([(label, S.rel_err(got, other, planar=True), tol)])


# -- a. each surface against float64 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_sflow', [True, False])
@pytest.mark.parametrize('name', list(S.CASES))
def test_each_surface_against_float64(name, with_sflow):
    from dvd_hip import ops
    d1, d2, flow, sf, cams = _case(name)
    got = ops.warp_surfaces(d1, d2, flow, cams, sflow_1_2=sf if with_sflow else None)
    assert tuple(got) == S.SURFACES
    spec = S.surfaces(name, F64, with_sflow)
    _check([('%s %s sflow=%s' % (name, k, with_sflow), S.rel_err(got[k], spec[k]), S.TOL[S.tol_key(k, with_sflow)])
            for k in S.SURFACES])
    # the decisions are exactly the oracle's
    behind, behind_static = spec['_behind'], spec['_behind_static']
    assert torch.equal((got['depth_image_1_2'][:, 0] < 1e-3).cpu(), behind)
    assert behind.any() and not behind.all() and behind_static.any() and not behind_static.all()
    assert (_bits(got['dflow_1_2'])[behind] == 0).all() and (_bits(got['staticflow_1_2'])[behind_static] == 0).all()
    assert ((got['dflow_1_2'].cpu() != 0).any(-1) | behind).all()          # ... and nowhere else is the flow exactly (0, 0)
    assert ((got['staticflow_1_2'].cpu() != 0).any(-1) | behind_static).all()
    if not with_sflow:
        zero = ops.warp_surfaces(d1, d2, flow, cams, sflow_1_2=torch.zeros_like(sf))
        for k in S.SURFACES:
            assert _same_bits(got[k], zero[k]), k
        assert _same_bits(got['dflow_1_2'], got['staticflow_1_2'])


# -- b. subsets, through the C ABI, into a guarded buffer --------------------------------------------------------------------
GUARD = 64          # bytes of pattern before, between and after the surfaces


@pytest.mark.parametrize('name', list(S.CASES))
def test_a_subset_has_the_bits_of_the_full_call_and_writes_nothing_else(name):
    from dvd_hip import _lib, ops
    d1, d2, flow, sf, cams = _case(name)
    B, H, W, _ = S.CASES[name]
    full = ops.warp_surfaces(d1, d2, flow, cams, sflow_1_2=sf)
    cst, keep = ops.pack_cameras(cams, B)
    lib = _lib.load()
    size = {k: full[k].numel() * 4 for k in S.SURFACES}
    offset, total = {}, GUARD
    for k in S.SURFACES:
        offset[k] = total
        total += size[k] + GUARD
    for subset in [(k,) for k in S.SURFACES] + [S.STATIC_SUBSET, S.SLACK_SUBSET]:
        buf = torch.full((total,), PATTERN, dtype=torch.uint8, device='cuda')
        assert buf.data_ptr() % 16 == 0
        st = _lib.Surfaces()
        for k in subset:
            setattr(st, k, buf.data_ptr() + offset[k])
        _lib.check(lib.dvd_warp_surfaces(ops._p(d1), ops._p(d2), ops._p(flow), ops._p(sf), ctypes.byref(cst), ctypes.byref(st),
                                         B, H, W, ops._stream()), 'dvd_warp_surfaces')
        host = buf.cpu()
        untouched = torch.ones(total, dtype=torch.bool)
        for k in subset:
            got = host[offset[k]:offset[k] + size[k]].view(torch.int32)
            assert torch.equal(got, _bits(full[k]).reshape(-1)), (subset, k)
            untouched[offset[k]:offset[k] + size[k]] = False
        assert (host[untouched] == PATTERN).all(), subset
    del keep


# -- c. integer flows at (2, 17, 33): weights exactly 0 and 1 ----------------------------------------------------------------
def _integer_flow(B, H, W):
    g = torch.Generator().manual_seed(67)
    flow = torch.randint(-5, 6, (B, H, W, 2), generator=g).float()
    ys, xs = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing='ij')
    flow[0, 3] = torch.stack([W - 1 - xs[3], torch.zeros(W)], -1)                     # exactly on the last column
    flow[0, :, 5] = torch.stack([torch.zeros(H), H - 1 - ys[:, 5]], -1)               # exactly on the last row
    flow[0, 0, 0] = torch.tensor([W - 1.0, H - 1.0])                                  # the last cell itself
    flow[1, 2, 0:4] = torch.tensor([[100.0, 0.0], [-100.0, 0.0], [0.0, 100.0], [0.0, -100.0]])      # far outside, each side
    flow[1, 4, 0:4] = torch.tensor([[100.0, 100.0], [-100.0, -100.0], [100.0, -100.0], [-100.0, 100.0]])
    flow[1, 6] = torch.stack([-xs[6], -ys[6]], -1)                                    # exactly on the first cell
    tx = (xs + flow[..., 0]).clamp(0, W - 1).long()
    ty = (ys + flow[..., 1]).clamp(0, H - 1).long()
    return flow, tx, ty


def test_integer_flows_shift_and_clamp_bit_for_bit():
    from dvd_hip import ops
    name = 'b2_17x33'
    B, H, W, _ = S.CASES[name]
    assert (W - 1) / 2 == 16 and (H - 1) / 2 == 8
    d1, d2, _, sf, cams = _case(name)
    flow, tx, ty = _integer_flow(B, H, W)
    assert (tx == W - 1).any() and (ty == H - 1).any() and (tx == 0).any() and (ty == 0).any()
    bi = torch.arange(B)[:, None, None]
    for C in S.WARP_CHANNELS:
        x, _ = S.flow_warp_inputs(name, C)
        got = ops.flow_warp(x.cuda(), flow.cuda())
        want = x.permute(0, 2, 3, 1)[bi, ty, tx].permute(0, 3, 1, 2)
        assert _same_bits(got, want), C
    got = ops.warp_surfaces(d1, d2, flow.cuda(), cams, sflow_1_2=sf, want=('depth_warp_1_2',))['depth_warp_1_2']
    assert _same_bits(got, d2.cpu()[bi, 0, ty, tx][:, None])


# -- d. the VJP, one surface at a time ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(S.CASES))
def test_vjp_one_surface_at_a_time(name):
    from dvd_hip import ops
    d1, d2, flow, sf, cams = _case(name)
    B, H, W, _ = S.CASES[name]
    spec = S.surfaces(name, F64)
    behind = {'dflow_1_2': spec['_behind'], 'staticflow_1_2': spec['_behind_static']}
    counts = S.scatter_counts(S.case(name)['flow_1_2'], H, W)
    ups = {k: S.upstream(name, k).cuda() for k in S.SURFACES}
    figures, single = [], {}
    for k in S.SURFACES:
        got = ops.warp_surfaces_backward(d1, d2, flow, cams, {k: ups[k]}, sflow_1_2=sf, want_sflow_grad=True)
        single[k] = [g.double().cpu() for g in got]
        for gname, g, want in zip(S.GRADS, got, S.vjp(name, F64, k)):
            figures.append(('%s %s <- %s' % (name, gname, k), S.rel_err(g, want), S.TOL[gname]))
    # the gradient cut at behind-camera pixels, pixel by pixel
    for k, mask in behind.items():
        assert (single[k][0][:, 0][mask] == 0).all() and (single[k][2][:, :, :, 0][mask] == 0).all(), k
    assert (single['dflow_1_2'][0][:, 0][~behind['dflow_1_2']] != 0).all()
    assert (single['depth_image_1_2'][0][:, 0][behind['dflow_1_2']] != 0).all()
    assert (single['depth_image_1_2'][2][:, :, :, 0][behind['dflow_1_2']] != 0).any(-1).all()
    # all nine at once: linear
    g_all = ops.warp_surfaces_backward(d1, d2, flow, cams, ups, sflow_1_2=sf, want_sflow_grad=True)
    for i, gname in enumerate(S.GRADS):
        figures.append(('%s %s: all nine vs the sum of nine' % (name, gname),
                        S.rel_err(g_all[i], sum(single[k][i] for k in S.SURFACES)), S.TOL[gname]))
    _check(figures)
    # without the scene-flow gradient the other two are the same
    g1, g2, gs = ops.warp_surfaces_backward(d1, d2, flow, cams, ups, sflow_1_2=sf, want_sflow_grad=False)
    assert gs is None and _same_bits(g1, g_all[0])
    _same_scatter(g2, g_all[1], counts, name + ' g_depth_2 without g_sflow', S.TOL['g_depth_2'])
    # ... and a null scene flow is a zero scene flow
    z1 = ops.warp_surfaces_backward(d1, d2, flow, cams, ups, sflow_1_2=None, want_sflow_grad=True)
    z2 = ops.warp_surfaces_backward(d1, d2, flow, cams, ups, sflow_1_2=torch.zeros_like(sf), want_sflow_grad=True)
    assert _same_bits(z1[0], z2[0]) and _same_bits(z1[2], z2[2])
    _same_scatter(z1[1], z2[1], counts, name + ' g_depth_2, null vs zero scene flow', S.TOL['g_depth_2'])


# -- e. flow_warp and its backward -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(S.CASES))
def test_flow_warp_backward_against_float64_and_adjoint(name):
    from dvd_hip import ops
    from dvd_hip.losses.scene_flow_projection import BackwardWarp
    B, H, W, _ = S.CASES[name]
    flow_h = S.case(name)['flow_1_2']
    flow = _case(name)[2]
    counts = S.scatter_counts(flow_h, H, W)
    figures = []
    for C in S.WARP_CHANNELS:
        x, g = S.flow_warp_inputs(name, C)
        want, gwant = S.flow_warp_spec(x.double(), flow_h, g)
        out = ops.flow_warp(x.cuda(), flow)
        gx = ops.flow_warp_backward(g.cuda(), flow)
        figures.append(('%s flow_warp C=%d' % (name, C), S.rel_err(out, want, planar=True), S.TOL['flow_warp']))
        figures.append(('%s flow_warp_backward C=%d' % (name, C), S.rel_err(gx, gwant, planar=True), S.TOL['flow_warp_bwd']))
        lhs = float((out.double().cpu() * g.double()).sum())
        rhs = float((x.double() * gx.double().cpu()).sum())
        scale = float((x.double().abs() * g.double().abs()).sum())
        figures.append(('%s <warp(x), g> - <x, warp^T(g)> C=%d (of sum|x||g|)' % (name, C), abs(lhs - rhs) / scale, S.TOL['flow_warp']))
        leaf = x.cuda().requires_grad_(True)
        res = BackwardWarp()(leaf, flow)
        res.backward(g.cuda())
        assert _same_bits(res, out)
        _same_scatter(leaf.grad, gx, counts, '%s BackwardWarp.grad vs flow_warp_backward C=%d' % (name, C), S.TOL['flow_warp_bwd'])
    _check(figures)


# -- f. unproject forward ----------------------------------------------------------------------------------------------------
UNPROJECT_SHAPES = [(2, 6, 20), (1, 33, 32), (2, 7, 37), (1, 1, 1), (2, 1, 5)]


def _offset(t, off=1):
    """A contiguous copy of t that starts `off` floats into a 256-byte aligned buffer."""
    buf = torch.zeros(t.numel() + off + 4, device='cuda')
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off and v.is_contiguous()
    return v


@pytest.mark.parametrize('B,H,W', UNPROJECT_SHAPES)
def test_unproject_forward_against_float64_on_both_paths(B, H, W):
    from dvd_hip import ops, synthetic
    from dvd_hip.losses.scene_flow_projection import unproject_ptcld
    _, cams = S.cameras(B, H, W, seed=B * 100 + W)
    R, t, Kinv = cams['R_1'], cams['t_1'], cams['K_inv']
    depth, _ = synthetic.make_depths(B, H, W, seed=H * W, far_depth_frac=0.01)
    want = G.unproject(depth.double(), R.double(), t.double(), Kinv.double())         # [B,H,W,1,3]
    dg, Rg, tg, Kg = depth.cuda(), R.cuda(), t.cuda(), Kinv.cuda()
    assert dg.data_ptr() % 16 == 0
    planar = ops.unproject(dg, Rg, tg, Kg, planar=True)
    inter = ops.unproject(dg, Rg, tg, Kg, planar=False)
    assert tuple(planar.shape) == (B, 3, H, W) and tuple(inter.shape) == (B, H, W, 1, 3)
    _check([('unproject planar %dx%dx%d' % (B, H, W), S.rel_err(planar, want[:, :, :, 0].permute(0, 3, 1, 2), planar=True), S.TOL['global_p1']),
            ('unproject interleaved %dx%dx%d' % (B, H, W), S.rel_err(inter, want), S.TOL['global_p1'])])
    assert _same_bits(planar.permute(0, 2, 3, 1)[:, :, :, None], inter)
    assert _same_bits(unproject_ptcld()(dg, Rg, tg, Kg), inter)
    # a depth or an output one float into a line takes the scalar path whatever W is: the same bits as the vector path
    for pl, ref in ((True, planar), (False, inter)):
        assert _same_bits(ops.unproject(_offset(dg), Rg, tg, Kg, planar=pl), ref)
        out = _offset(torch.full_like(ref, float('nan')))
        assert ops.unproject(dg, Rg, tg, Kg, planar=pl, out=out) is out and _same_bits(out, ref)


# -- g. hostile values stay local --------------------------------------------------------------------------------------------
def test_nan_and_inf_in_depth_1_stay_in_their_pixel():
    from dvd_hip import ops
    name = 'b2_16x17'
    d1, d2, flow, sf, cams = _case(name)
    B, H, W, _ = S.CASES[name]
    ups = {k: S.upstream(name, k).cuda() for k in S.SURFACES}
    clean = ops.warp_surfaces(d1, d2, flow, cams, sflow_1_2=sf)
    g_clean = ops.warp_surfaces_backward(d1, d2, flow, cams, ups, sflow_1_2=sf, want_sflow_grad=True)
    bad = d1.clone()
    bad[0, 0, 3, 4], bad[1, 0, 15, 16] = float('nan'), float('inf')
    hit = torch.zeros(B, H, W, dtype=torch.bool)
    hit[0, 3, 4] = hit[1, 15, 16] = True
    got = ops.warp_surfaces(bad, d2, flow, cams, sflow_1_2=sf)
    g_got = ops.warp_surfaces_backward(bad, d2, flow, cams, ups, sflow_1_2=sf, want_sflow_grad=True)

    def per_pixel(t):            # [B,H,W,C] view of any layout
        t = t.cpu()
        return t.permute(0, 2, 3, 1) if t.shape[1] == 1 and t.dim() == 4 else t.reshape(B, H, W, -1)

    for k in S.SURFACES:
        a, b = per_pixel(got[k]), per_pixel(clean[k])
        assert torch.isfinite(a[~hit]).all() and torch.equal(_bits(a[~hit]), _bits(b[~hit])), k
    for k in ('global_p1', 'p1_camera_2', 'depth_image_1_2', 'sf_by_depth'):
        assert (~torch.isfinite(per_pixel(got[k])[hit])).any(-1).all(), k
    for i in (0, 2):
        a, b = per_pixel(g_got[i]), per_pixel(g_clean[i])
        assert torch.isfinite(a[~hit]).all() and torch.equal(_bits(a[~hit]), _bits(b[~hit])), S.GRADS[i]
    # depth_2's gradient does not read depth_1 at all
    assert torch.isfinite(g_got[1]).all()
    _same_scatter(g_got[1], g_clean[1], S.scatter_counts(S.case(name)['flow_1_2'], H, W), 'g_depth_2 under a NaN depth_1',
                  S.TOL['g_depth_2'])


def test_nan_in_depth_2_reaches_exactly_the_pixels_that_tap_it():
    from dvd_hip import ops
    name = 'b3_17x23'
    d1, d2, flow, sf, cams = _case(name)
    B, H, W, _ = S.CASES[name]
    b0, y0, x0 = 1, 8, 11
    bad = d2.clone()
    bad[b0, 0, y0, x0] = float('nan')
    reach = (S.taps(S.case(name)['flow_1_2'], H, W) == y0 * W + x0).any(-1)
    reach[:b0], reach[b0 + 1:] = False, False
    assert 1 <= int(reach.sum()) < H * W
    clean = ops.warp_surfaces(d1, d2, flow, cams, sflow_1_2=sf)
    got = ops.warp_surfaces(d1, bad, flow, cams, sflow_1_2=sf)
    reads_d2 = ('depth_warp_1_2', 'warped_p2_camera_2', 'warped_global_p2', 'sf_by_depth')
    for k in S.SURFACES:
        a, b = got[k].cpu(), clean[k].cpu()
        a, b = (a[:, 0][..., None], b[:, 0][..., None]) if a.shape[1] == 1 and a.dim() == 4 else (a.reshape(B, H, W, -1), b.reshape(B, H, W, -1))
        if k in reads_d2:
            assert torch.isnan(a[reach]).all(), k
            assert torch.equal(_bits(a[~reach]), _bits(b[~reach])), k
        else:
            assert torch.equal(_bits(a), _bits(b)), k


# -- h. refusals, before any launch ------------------------------------------------------------------------------------------
@pytest.fixture
def no_launch(monkeypatch):
    from dvd_hip import ops

    def load():
        raise AssertionError('a call that must be refused reached the library')
    monkeypatch.setattr(ops._lib, 'load', load)


def _refused(match, fn, *args, **kw):
    with pytest.raises(RuntimeError, match=match):
        fn(*args, **kw)


def _other_sizes(t, dims):
    """t with one more / one fewer entry along each of dims, one at a time."""
    out = []
    for d in dims:
        out.append(torch.cat([t, t.narrow(d, 0, 1)], d))
        if t.shape[d] > 1:
            out.append(t.narrow(d, 0, t.shape[d] - 1).contiguous())
    return out


def test_surface_wrappers_refuse_before_they_launch(no_launch):
    from dvd_hip import ops
    from dvd_hip.losses.scene_flow_projection import flow_by_depth, scene_flow_projection_slack
    name = 'b3_7x9'
    d1, d2, flow, sf, cams = _case(name)
    B, H, W, _ = S.CASES[name]
    ups = {k: S.upstream(name, k).cuda() for k in S.SURFACES}
    fwd = lambda **kw: ops.warp_surfaces(**dict(dict(depth_1=d1, depth_2=d2, flow_1_2=flow, cams=cams, sflow_1_2=sf), **kw))
    bwd = lambda **kw: ops.warp_surfaces_backward(**dict(dict(depth_1=d1, depth_2=d2, flow_1_2=flow, cams=cams, grads=ups,
                                                              sflow_1_2=sf), **kw))
    static = lambda **kw: flow_by_depth()(**dict(dict(cams, depth_1=d1, depth_2=d2, flow_1_2=flow), **kw))
    slack = lambda **kw: scene_flow_projection_slack()(**dict(dict(cams, depth_1=d1, depth_2=d2, flow_1_2=flow, flow_2_1=None,
                                                                   sflow_1_2=sf, sflow_2_1=None), **kw))
    for what, fn in (('warp_surfaces', fwd), ('warp_surfaces_backward', bwd), ('warp_surfaces', static), ('warp_surfaces', slack)):
        for arg, t, dims in (('depth_2', d2, (0, 2, 3)), ('flow_1_2', flow, (0, 1, 2, 3)), ('sflow_1_2', sf, (0, 1, 2, 4))):
            if arg == 'sflow_1_2' and fn is static:
                continue
            for other in _other_sizes(t, dims):
                _refused('%s: %s must be a tensor' % (what, arg), fn, **{arg: other})
            _refused('%s must be a GPU tensor' % arg, fn, **{arg: t.cpu()})
            _refused('%s must be float32' % arg, fn, **{arg: t.double()})
            _refused('%s must be float32' % arg, fn, **{arg: t.half()})
        for other in _other_sizes(d1, (0, 2, 3)):                      # depth_1 sets B, H, W: now everything else disagrees
            _refused('%s: \\w+ must be a tensor' % what, fn, depth_1=other)
        _refused('%s: depth_1 must be a tensor \\[B,1,H,W\\]' % what, fn, depth_1=d1[:, 0])
        for k in S.CAM_KEYS:
            c = cams[k]
            wrong = _other_sizes(c, (0,)) + [c[..., :2].contiguous(), c.reshape(-1)]
            for other in wrong:
                kw = {k: other} if fn in (static, slack) else {'cams': dict(cams, **{k: other})}
                _refused('%s: %s must be a tensor' % (what, k), fn, **kw)
            for other, msg in ((c.cpu(), 'a GPU tensor'), (c.double(), 'float32')):
                kw = {k: other} if fn in (static, slack) else {'cams': dict(cams, **{k: other})}
                _refused('%s must be %s' % (k, msg), fn, **kw)
    _refused('warp_surfaces: want holds', fwd, want=('global_p1', 'global_p3'))
    _refused('warp_surfaces: want holds', fwd, want=('_behind',))
    _refused('warp_surfaces_backward: grads holds', bwd, grads=dict(ups, flow=ups['dflow_1_2']))
    for k in S.SURFACES:
        dims = tuple(d for d in range(ups[k].dim()) if ups[k].shape[d] != 1 or d == 0)
        for other in _other_sizes(ups[k], dims):
            _refused('warp_surfaces_backward: the gradient of %s must be a tensor' % k, bwd, grads={k: other})
        _refused('the gradient of %s must be a GPU tensor' % k, bwd, grads={k: ups[k].cpu()})
        _refused('the gradient of %s must be float32' % k, bwd, grads={k: ups[k].double()})


def test_warp_and_unproject_wrappers_refuse_before_they_launch(no_launch):
    from dvd_hip import ops
    from dvd_hip.losses.scene_flow_projection import BackwardWarp, unproject_ptcld
    name = 'b3_7x9'
    d1, _, flow, _, cams = _case(name)
    B, H, W, _ = S.CASES[name]
    x = torch.randn(B, 2, H, W, device='cuda')
    for what, arg, fn in (('flow_warp', 'buffer', ops.flow_warp), ('flow_warp_backward', 'g_out', ops.flow_warp_backward),
                          ('flow_warp', 'buffer', BackwardWarp())):
        for other in _other_sizes(flow, (0, 1, 2, 3)):
            _refused('%s: flow_1_2 must be a tensor' % what, fn, x, other)
        for other in _other_sizes(x, (0, 2, 3)):
            _refused('%s: flow_1_2 must be a tensor' % what, fn, other, flow)
        _refused('%s: %s must be a tensor \\[B,C,H,W\\]' % (what, arg), fn, x[:, 0], flow)
        _refused('flow_1_2 must be a GPU tensor', fn, x, flow.cpu())
        _refused('%s must be a GPU tensor' % arg, fn, x.cpu(), flow)
        _refused('flow_1_2 must be float32', fn, x, flow.double())
        _refused('%s must be float32' % arg, fn, x.half(), flow)
    R, t, Kinv = cams['R_1'], cams['t_1'], cams['K_inv']
    for fn in (ops.unproject, unproject_ptcld()):
        for arg, c, pos in (('R', R, 1), ('t', t, 2), ('K_inv', Kinv, 3)):
            for other in _other_sizes(c, (0,)) + [c[..., :2].contiguous(), c.reshape(-1)]:
                args = [d1, R, t, Kinv]
                args[pos] = other
                _refused('unproject: %s must be a tensor' % arg, fn, *args)
            for other, msg in ((c.cpu(), '%s must be a GPU tensor'), (c.double(), '%s must be float32')):
                args = [d1, R, t, Kinv]
                args[pos] = other
                _refused(msg % arg, fn, *args)
        _refused('unproject: depth must be a tensor \\[B,1,H,W\\]', fn, d1[:, 0], R, t, Kinv)
        _refused('depth must be float32', fn, d1.double(), R, t, Kinv)
    for planar, shape in ((True, (B, 3, H, W)), (False, (B, H, W, 1, 3))):
        for bad in (torch.empty(shape, device='cuda', dtype=F64), torch.empty(shape), torch.empty((B + 1,) + shape[1:], device='cuda'),
                    torch.empty((B, 3, W, H) if planar else (B, W, H, 1, 3), device='cuda'),
                    torch.empty((B, H, W, 3) if planar else (B, H, W, 3), device='cuda'),
                    torch.empty(shape[:-1] + (2 * shape[-1],), device='cuda')[..., ::2]):
            _refused('unproject: out must be a contiguous', ops.unproject, d1, R, t, Kinv, planar=planar, out=bad)
        g = torch.randn(shape, device='cuda')
        for bad in (torch.empty(B, 1, H, W, device='cuda', dtype=F64), torch.empty(B, 1, H, W), torch.empty(B + 1, 1, H, W, device='cuda'),
                    torch.empty(B, 1, W, H, device='cuda'), torch.empty(B, H, W, device='cuda'),
                    torch.empty(B, 1, H, 2 * W, device='cuda')[..., ::2], torch.empty(B, 1, W, H, device='cuda').transpose(2, 3)):
            _refused('unproject_backward: out must be a contiguous', ops.unproject_backward, g, planar, R, Kinv, out=bad)
        for arg, kw in (('R', dict(R=R[:1], K_inv=Kinv)), ('K_inv', dict(R=R, K_inv=Kinv[..., :2].contiguous())),
                        ('scale', dict(R=R, K_inv=Kinv, scale=torch.ones(2, device='cuda')))):
            _refused('unproject_backward: %s must be a tensor' % arg, ops.unproject_backward, g, planar, **kw)
        _refused('g_points must be a GPU tensor', ops.unproject_backward, g.cpu(), planar, R, Kinv)
        _refused('g_points must be float32', ops.unproject_backward, g.double(), planar, R, Kinv)
        _refused('unproject_backward: g_points must be a tensor', ops.unproject_backward, g[:, :2] if planar else g[..., :2],
                 planar, R, Kinv)
    _refused('accumulate=True needs an output tensor', ops.unproject_backward, torch.randn(B, 3, H, W, device='cuda'), True, R, Kinv,
             accumulate=True)


def test_unproject_backward_writes_into_the_callers_tensor():
    """out is written in place (a view included, as long as it is contiguous); the result is never put into a copy."""
    from dvd_hip import ops
    B, H, W = 2, 5, 8
    _, cams = S.cameras(B, H, W, seed=3)
    R, Kinv = cams['R_1'].cuda(), cams['K_inv'].cuda()
    g = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(1)).cuda()
    want = ops.unproject_backward(g, True, R, Kinv)
    whole = torch.full((B + 2, 1, H, W), float('nan'), device='cuda')
    res = ops.unproject_backward(g, True, R, Kinv, out=whole[1:B + 1])
    assert res.data_ptr() == whole[1:B + 1].data_ptr() and _same_bits(whole[1:B + 1], want)
    assert torch.isnan(whole[0]).all() and torch.isnan(whole[B + 1]).all()
    strided = torch.full((B, 1, H, 2 * W), float('nan'), device='cuda')
    with pytest.raises(RuntimeError, match='unproject_backward: out must be a contiguous'):
        ops.unproject_backward(g, True, R, Kinv, out=strided[..., ::2])
    assert torch.isnan(strided).all()


def test_one_row_or_one_column_is_refused_by_the_library():
    from dvd_hip import ops
    for B, H, W in ((1, 1, 5), (2, 4, 1), (1, 1, 1)):
        _, cams = S.cameras(B, H, W, seed=5)
        cams = {k: v.cuda() for k, v in cams.items()}
        d = torch.ones(B, 1, H, W, device='cuda')
        flow, sf = torch.zeros(B, H, W, 2, device='cuda'), torch.zeros(B, H, W, 1, 3, device='cuda')
        shape = 'bad shape B=%d H=%d W=%d' % (B, H, W)
        _refused('dvd_warp_surfaces failed.*warp_surfaces: ' + shape, ops.warp_surfaces, d, d, flow, cams, sflow_1_2=sf)
        _refused('dvd_warp_surfaces_bwd failed.*warp_surfaces_bwd: ' + shape, ops.warp_surfaces_backward, d, d, flow, cams,
                 {'depth_warp_1_2': d}, sflow_1_2=sf)
        _refused('dvd_flow_warp_fwd failed.*flow_warp_fwd: bad shape', ops.flow_warp, d, flow)
        _refused('dvd_flow_warp_bwd failed.*flow_warp_bwd: bad shape', ops.flow_warp_backward, d, flow)
