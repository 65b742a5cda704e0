"""The fp16 / fp32 boundary kernels of csrc/a16.hip across their parameter space, at single-trip shapes: the 1x1 and 3x3 depth
heads (every channel count that selects another code path, fp16 and fp32 storage, with and without the input ReLU and the
bias), and the loss-scale rules dvd_gscale_begin / dvd_gscale_end at their branches and clamps.

Heads: random fp16-valued / fp32 inputs against float64 computed from the same values (tests/boundary_spec.py).  Every bound is
a rounding-error bound derived from the kernel's operation count (boundary_spec.head1x1_bounds / head3x3_bounds say how), not a
tuned tolerance; `measured / bound` of every quantity goes to helpers.log_measured.  The loss-scale kernels are compared with
small Python models of the rule in csrc/a16.hip's header comment, exactly."""
import numpy as np
import pytest
import torch

import boundary_spec as S
from helpers import log_measured

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda')
FRESH = [1.0, 1.0, 4.0] + [0.0] * 13


@pytest.fixture
def state():
    from dvd_hip import conv as C, ops
    st = ops.gscale_new(DEV)
    C.set_grad_scale_state(st)
    yield st
    C.set_grad_scale_state(None)


def _ratio(got, ref, bound):
    """max |got - ref| / bound; where the bound is 0 (no terms at all) the result must be exact."""
    err = (got.detach().double().cpu().reshape(ref.shape) - ref).abs()
    assert bool((err[bound == 0] == 0).all())
    return float((err / bound.clamp(min=1e-300)).max())


def _inputs(shape, f16, wshape, bias, seed):
    """x (fp16-valued when the storage is fp16, every fifth element 0: the ReLU mask's edge), w, b, gy as fp32 CPU tensors;
    gy is tiny (unscaled it would underflow fp16)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g)
    x.view(-1)[::5] = 0.0
    x.view(-1)[3::10] = -0.0
    if f16:
        x = x.half().float()
    w = torch.randn(*wshape, generator=g) * float(1.0 / np.sqrt(np.prod(wshape)))
    b = 0.3 * torch.randn(1, generator=g) if bias else None
    gy = 3e-6 * torch.randn(shape[0], 1, shape[2], shape[3], generator=g)
    return x, w, b, gy


def _run_head(conv, run, x, gy, dtype):
    xg = x.to(dtype).to(DEV).requires_grad_(True)
    y = run(xg)
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    return y.detach(), xg.grad, conv.weight.grad, None if conv.bias is None else conv.bias.grad


def _scale_state_checks(st, f16, w, gy, y, gx, gx32_amax):
    """fp16 features: S is the power of two of the rule, [1] its reciprocal, [3] the largest |S gx| in fp32 BEFORE it was
    stored (so also, rounded to fp16 -- rounding is monotone -- the largest stored element), [6] the largest |y| stored."""
    s = st.tolist()
    if not f16:
        assert s == FRESH
        return 1.0
    scale = s[0]
    assert scale == S.gscale_begin_ref(float(gy.abs().max()), float(w.abs().max()), 4.0)
    assert np.frexp(scale)[0] == 0.5 and s[1] == 1.0 / scale and s[2] == 4.0
    assert s[3] == gx32_amax(scale)
    assert float(torch.tensor(s[3]).half()) == float(gx.abs().max())
    assert s[6] == float(y.abs().max())
    return scale


HEAD1X1_SHAPES = [(1, 2, 2), (3, 13, 20), (2, 24, 44)]          # one item; 195 items: a partly filled block; several blocks


@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('relu_in', [True, False], ids=['relu', 'norelu'])
@pytest.mark.parametrize('dtype', [torch.float16, torch.float32], ids=['f16', 'f32'])
@pytest.mark.parametrize('Cc', [1, 5, 32, 33, 64])
def test_head1x1_against_float64_within_rounding_bounds(Cc, dtype, relu_in, bias, state):
    """conv.head1x1 for C = 1, 5, 32 (head1x1_bwd_kernel<T, 32>) and 33, 64 (<T, 64>).  Bounds (u = 2^-24):
      y   (C + 2) u (|b| + sum_c |w_c| |act(x_c)|) per pixel;
      gx  one fp32 product v = S w_c g [x > 0]: u |v|; stored as fp16: (2^-11 + 2 u) |v| + 2^-25;
      gw  16 u sum |g act(x_c)| (a 4-term FMA chain, 6 wave steps, 2 adds; the rest in double);  gb  16 u sum |g|."""
    from dvd_hip import conv as C
    f16 = dtype == torch.float16
    worst = dict(y=0.0, gx=0.0, gw=0.0, gb=0.0)
    for i, (N, H, W) in enumerate(HEAD1X1_SHAPES):
        x, w, b, gy = _inputs((N, Cc, H, W), f16, (Cc,), bias, 100 * Cc + i)
        conv = torch.nn.Conv2d(Cc, 1, 1, bias=bias).to(DEV)
        with torch.no_grad():
            conv.weight.copy_(w.view(1, Cc, 1, 1))
            if bias:
                conv.bias.copy_(b)
        state.copy_(torch.tensor(FRESH))
        y, gx, gw, gb = _run_head(conv, lambda t: C.head1x1(conv, t, relu_in=relu_in), x, gy, dtype)
        assert y.dtype == torch.float32 and gx.dtype == dtype and (gb is None) == (not bias)
        mask = (x > 0).float() if relu_in else torch.ones_like(x)

        def gx32_amax(scale):                        # the kernel's own fp32 product: fl(fl(w S) g), S a power of two
            return float(((w * scale).view(1, Cc, 1, 1) * gy * mask).abs().max())
        scale = _scale_state_checks(state, f16, w, gy, y, gx, gx32_amax)
        ref = S.head1x1_ref(x, w, b, gy, relu_in, scale)
        bound = S.head1x1_bounds(ref, Cc, f16)
        worst['y'] = max(worst['y'], _ratio(y, ref['y'], bound['y']))
        worst['gx'] = max(worst['gx'], _ratio(gx, ref['gx'], bound['gx']))
        worst['gw'] = max(worst['gw'], _ratio(gw, ref['gw'], bound['gw']))
        if bias:
            worst['gb'] = max(worst['gb'], _ratio(gb, ref['gb'], bound['gb']))
    for k, v in worst.items():
        log_measured('head1x1 C=%d %s relu=%d bias=%d: %s measured / bound' % (Cc, 'f16' if f16 else 'f32', relu_in, bias, k), v, 1.0)
    assert all(v <= 1.0 for v in worst.values()), worst


def test_head1x1_refuses_what_it_does_not_cover_by_shape(state):
    from dvd_hip import conv as C
    conv = torch.nn.Conv2d(65, 1, 1).to(DEV)
    with pytest.raises(RuntimeError, match=r'dvd_head1x1_fwd failed.*bad shape N=1 C=65 HW=4'):
        C.head1x1(conv, torch.zeros(1, 65, 2, 2, device=DEV, dtype=torch.float16))
    conv = torch.nn.Conv2d(4, 1, 1).to(DEV)
    with pytest.raises(RuntimeError, match=r'dvd_head1x1_fwd failed.*bad shape N=2 C=4 HW=9'):
        C.head1x1(conv, torch.zeros(2, 4, 3, 3, device=DEV))


HEAD3X3_SHAPES = [(2, 19, 27), (1, 1, 9), (1, 7, 1), (2, 3, 3), (1, 33, 40)]


@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('Cc', [1, 5, 8, 12, 64])
def test_head3x3_against_float64_within_rounding_bounds(Cc, bias, state):
    """conv.head3x3 (fp16 features) against F.conv2d(..., padding=1) in float64, C below, at and above one channel group
    of the weight gradient (8), images of one row, one column and 3 x 3.  Bounds (u = 2^-24):
      y   (9 C + 2) u (|b| + sum |w| |x|) per pixel;
      gx  2^-11 |v| + 10 u (1 + 2^-11) sum_t |S w_t g_t| + 2^-25 (a 9-FMA chain rounded once more to fp16);
      gw  (ceil(chunk / 256) + 10) u sum |x g|, chunk = ceil(total / min(256, ceil(total / 1024)));  gb  the same with sum |g|."""
    from dvd_hip import conv as C
    worst = dict(y=0.0, gx=0.0, gw=0.0, gb=0.0)
    for i, (N, H, W) in enumerate(HEAD3X3_SHAPES):
        x, w, b, gy = _inputs((N, Cc, H, W), True, (1, Cc, 3, 3), bias, 1000 + 100 * Cc + i)
        conv = torch.nn.Conv2d(Cc, 1, 3, padding=1, bias=bias).to(DEV)
        with torch.no_grad():
            conv.weight.copy_(w)
            if bias:
                conv.bias.copy_(b)
        state.copy_(torch.tensor(FRESH))
        y, gx, gw, gb = _run_head(conv, lambda t: C.head3x3(conv, t), x, gy, torch.float16)
        assert y.dtype == torch.float32 and gx.dtype == torch.float16 and (gb is None) == (not bias)
        s = state.tolist()
        scale = s[0]
        assert scale == S.gscale_begin_ref(float(gy.abs().max()), float(w.abs().max()), 4.0)
        assert np.frexp(scale)[0] == 0.5 and s[1] == 1.0 / scale and s[6] == float(y.abs().max())
        assert float(torch.tensor(s[3]).half()) == float(gx.abs().max())       # [3]: max |S gx| in fp32, before the store
        ref = S.head3x3_ref(x, w, b, gy, scale)
        bound = S.head3x3_bounds(ref, Cc, N * H * W)
        worst['y'] = max(worst['y'], _ratio(y, ref['y'], bound['y']))
        worst['gx'] = max(worst['gx'], _ratio(gx, ref['gx'], bound['gx']))
        worst['gw'] = max(worst['gw'], _ratio(gw, ref['gw'], bound['gw']))
        if bias:
            worst['gb'] = max(worst['gb'], _ratio(gb, ref['gb'], bound['gb']))
        assert abs(s[3] - float(ref['gx'].abs().max())) <= float((10 * S.U32 * ref['gx_abs']).max())
    for k, v in worst.items():
        log_measured('head3x3 C=%d bias=%d: %s measured / bound' % (Cc, bias, k), v, 1.0)
    assert all(v <= 1.0 for v in worst.values()), worst


def test_head3x3_refuses_what_it_does_not_cover(state):
    from dvd_hip import conv as C
    x = torch.zeros(1, 8, 6, 6, device=DEV, dtype=torch.float16)
    assert C.head3x3_supported(torch.nn.Conv2d(8, 1, 3, padding=1).to(DEV), x)
    for kw in (dict(stride=2, padding=1), dict(padding=0), dict(padding=1, dilation=2), dict(padding=1, padding_mode='reflect')):
        assert not C.head3x3_supported(torch.nn.Conv2d(8, 1, 3, **kw).to(DEV), x), kw
    assert not C.head3x3_supported(torch.nn.Conv2d(8, 1, 3, padding=1).to(DEV), x.float())
    conv = torch.nn.Conv2d(65, 1, 3, padding=1).to(DEV)
    x65 = torch.zeros(1, 65, 4, 4, device=DEV, dtype=torch.float16)
    assert not C.head3x3_supported(conv, x65)
    with pytest.raises(RuntimeError, match='not the fp16 depth head'):
        C.head3x3(conv, x65)
    with pytest.raises(RuntimeError, match=r'dvd_head3x3_fwd failed.*bad shape N=1 C=65 H=4 W=4'):
        C._Head3x3.apply(x65, conv.weight, conv.bias)


# ---- dvd_gscale_begin ---------------------------------------------------------------------------------------------------
W2 = [0.25, -2.0, 1.0]                       # max |w| = 2
BEGIN_CASES = [(f * 2.0 ** k / 2.0, W2, 4.0) for k in (-20, 0, 10) for f in (1.0, 1.5)] + [
    (1e-38, [1.0], 14.0),                    # 14 + 126 octaves: the upper clamp, S = 2^120
    (1e38, [1.0], -24.0),                    # -24 - 127 octaves: the lower clamp, S = 2^-120
    (3.0, None, 4.0),                        # no weights (null pointer, n_w = 0): max |w| taken as 1
    (1.0, [0.01] * 64 + [-8.0], 4.0),        # 65 weights, the largest last: lane 0's second turn
    (1.0, [0.01] * 575 + [8.0], 4.0),        # 576 = 9 x 64 weights, the largest last: lane 63's ninth turn
    (0.0, W2, 4.0), (float('inf'), W2, 4.0), (float('nan'), W2, 4.0), (3.2e38, [1.0], 4.0),     # S = 1
    (1.0, [0.0, -0.0], 4.0), (1e30, [1e30], 4.0), (1.0, [float('inf')], 4.0)]                   # S = 1


@pytest.mark.parametrize('g_amax,w,target', BEGIN_CASES)
def test_gscale_begin_matches_the_rule_exactly(g_amax, w, target):
    """dvd_gscale_begin on a fresh state against boundary_spec.gscale_begin_ref: S = 2^clamp(int(target) - e, -120, 120) with
    max|g| * max|w| = f 2^e (np.frexp of the fp32 product); 1 for a product of 0, Inf, NaN or >= 3e38.  [0] = S, [1] = 1 / S
    exactly, nothing else moves."""
    from dvd_hip import _lib, ops
    from dvd_hip.ops import _p, _stream
    st = ops.gscale_new(DEV, target)
    g = torch.tensor([g_amax], dtype=torch.float32, device=DEV)
    wt = None if w is None else torch.tensor(w, dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().dvd_gscale_begin(_p(st), _p(g), _p(wt), 0 if w is None else len(w), _stream()), 'dvd_gscale_begin')
    want = S.gscale_begin_ref(g_amax, 1.0 if w is None else max(abs(v) for v in w), target)
    assert st.tolist() == [want, 1.0 / want, target] + [0.0] * 13


# ---- dvd_gscale_end -----------------------------------------------------------------------------------------------------
K = S.GS_OVERFLOW                            # 2^15.5 in fp32: the overflow threshold
END_CASES = [
    # (target, observed max |S g|, forward monitor) -> what must happen
    (4.0, 0.0, 0.0),                                         # nothing observed: nothing moves
    (4.0, 2.0 ** 13, 0.0),                                   # centred exactly
    (4.0, float(np.nextafter(K, np.float32(0))), 0.0),       # just representable: no skip, 2.5 octaves too high -> -2
    (4.0, float(K), 0.0),                                    # the threshold itself: skip, back off 3
    (4.0, float(np.nextafter(K, np.float32(1e9))), 0.0),     # just beyond: skip
    (12.0, 1.0, 0.0),                                        # +4 would pass 14: clamped at 14
    (13.0, 2.0 ** 11, 0.0),                                  # +2 would pass 14
    (14.0, 1000.0, 0.0),                                     # already at the clamp
    (-20.0, float('inf'), 0.0),                              # -8 would pass -24: clamped at -24
    (-22.0, 2.0 ** 20, 0.0),                                 # -7 would pass -24
    (-24.0, 2.0 ** 16, 0.0),                                 # already at the clamp
    (4.0, float('nan'), 0.0),                                # NaN counts as an overflow: -8
    (4.0, 2.0 ** 13, 65504.0),                               # an activation AT fp16's maximum: skipped for both networks
    (4.0, 2.0 ** 13, float(np.nextafter(np.float32(65504.0), np.float32(0)))),     # just below it: a normal step
]


@pytest.mark.parametrize('target,obs,fwd', END_CASES)
def test_gscale_end_edges_match_the_model(target, obs, fwd):
    """dvd_gscale_end at the edges tests/test_10_act_fp16_gpu.py does not reach, against boundary_spec.gscale_end_model: all 16
    floats afterwards -- the target with its clamps to [-24, 14], the cleared monitors [3] and [6], the step's flags [4], [8]
    and the counters [5], [9], [10], which start from non-zero values here."""
    from dvd_hip import ops
    before = [2.0, 0.5, target, obs, 1.0, 3.0, fwd, 0.0, 1.0, 2.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    st = torch.tensor(before, dtype=torch.float32).to(DEV)
    ops.gscale_end(st)
    want = S.gscale_end_model(before)
    got = st.tolist()
    assert got == want, (got, want)
    assert got[3] == 0.0 and got[6] == 0.0 and -24.0 <= got[2] <= 14.0 and got[:2] == [2.0, 0.5]
